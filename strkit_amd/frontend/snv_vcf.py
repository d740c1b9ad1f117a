"""The candidate SNVs of `--incorporate-snvs`.  A BGZF file with a tabix index next to it (<path>.tbi) is read region by
region, by the library (IndexedSnvVcf, DESIGN.md §18: inflated and parsed on the device or on the host cores); any other file
(plain, gzip, BGZF without .tbi) is read once, whole, through Python's `gzip` (read_snv_vcf).  Stands where the reference opens its SNV VCF (strkit/call/call_sample.py:133-157, strkit_rust_ext's
STRkitVCFReader): only records whose REF and every ALT are single bases count (no indels, no symbolic or multi-base
alleles); what comes back per contig is what frontend/phase_inputs.py's locus_candidates takes."""
from __future__ import annotations

import ctypes as C
import gzip
import os
import time
from dataclasses import dataclass

import numpy as np

from .loci import resolve_contig
from .tabix_text import TabixText

__all__ = ["SnvCandidates", "read_snv_vcf", "IndexedSnvVcf", "open_snv_candidates"]

_BASES = frozenset("ACGTN")


@dataclass
class ContigSnvs:
    pos: np.ndarray          # int64, 0-based, ascending, distinct
    ids: list[str]           # the ID column; "" where it is "."
    ref: list[str]           # the reference base


class SnvCandidates:
    """Per contig the sorted positions, ids and reference bases of the file's SNV records."""

    def __init__(self, by_contig: dict[str, ContigSnvs]):
        self.by_contig = by_contig

    def contig(self, name: str) -> ContigSnvs | None:
        """The records of a contig, named with or without the "chr" prefix (as n_alleles_of and the readers do)."""
        found = resolve_contig(self.by_contig, name)
        return None if found is None else self.by_contig[found]

    def window(self, contig: str, beg: int, end: int) -> ContigSnvs | None:
        """What a block of loci asks for: here the whole contig's records (the file was read whole)."""
        return self.contig(contig)

    def snv_id(self, contig: str, k: int) -> str:
        """The id of record k of a contig as the report names it: the ID column, or <contig>_<1-based position>."""
        c = self.contig(contig)
        return c.ids[k] or f"{contig}_{int(c.pos[k]) + 1}"


def read_snv_vcf(path: str) -> SnvCandidates:
    with open(path, "rb") as fh:
        gz = fh.read(2) == b"\x1f\x8b"
    rows: dict[str, list[tuple[int, str, str]]] = {}
    with (gzip.open(path, "rt") if gz else open(path, "rt")) as fh:
        for line in fh:
            if not line or line[0] == "#":
                continue
            f = line.rstrip("\r\n").split("\t")
            if len(f) < 5:
                continue
            ref, alts = f[3].upper(), f[4].upper().split(",")
            if len(ref) != 1 or ref not in _BASES or not alts or any(len(a) != 1 or a not in _BASES for a in alts):
                continue
            rows.setdefault(f[0], []).append((int(f[1]) - 1, "" if f[2] == "." else f[2], ref))
    out = {}
    for contig, rs in rows.items():
        rs.sort(key=lambda r: r[0])                       # stable: of two records at one position the first one stays
        keep = [r for k, r in enumerate(rs) if k == 0 or r[0] != rs[k - 1][0]]
        out[contig] = ContigSnvs(np.array([r[0] for r in keep], np.int64), [r[1] for r in keep], [r[2] for r in keep])
    return SnvCandidates(out)


class _Column:
    """One text column of a window's records, decoded on access: `ids` (slices of the concatenated ID bytes) or `ref` (one byte
    each).  Behaves as the list of str that ContigSnvs holds for a file read whole, without a Python object per record."""

    def __init__(self, data: np.ndarray, off: np.ndarray):
        self._data, self._off = data, off

    def __len__(self) -> int:
        return len(self._off) - 1

    def __getitem__(self, k):
        if isinstance(k, slice):
            return [self[i] for i in range(*k.indices(len(self)))]
        k = int(k)
        if k < 0:
            k += len(self)
        if not 0 <= k < len(self):
            raise IndexError(k)
        return self._data[int(self._off[k]):int(self._off[k + 1])].tobytes().decode()

    def __iter__(self):
        return (self[k] for k in range(len(self)))

    def __eq__(self, other):
        return list(self) == list(other)


class IndexedSnvVcf(TabixText):
    """Region access to a BGZF-compressed VCF through its tabix index, the reference's per-block query (call_sample.py:124):
    `window` inflates the BGZF blocks the index names for [beg, end) and has the library turn their text into candidate arrays
    — on the device (front_end="device": a strk_dbam object of its own holds the inflated piece in HBM; strk_dbam_vcf_snvs) or
    on the host cores (strk_bgzf_inflate_range + strk_vcf_snvs).  The range is walked in pieces (TabixText.walk)."""

    def __init__(self, path: str, index: str | None = None, front_end: str = "host", device: int = 0, piece_bytes: int = 32 << 20,
                 tile_bytes: int = 0):
        super().__init__(path, index or path + ".tbi", front_end, device, piece_bytes, tile_bytes, "vcf")

    def _parse(self, L, buf, n, start, name, beg, end, final, prev, seen):
        """One library call over a piece, with the arrays grown to what it asks for -> (pos, ref, id_off, ids, end_off, past)."""
        cap, ids_cap = max(64, (n - start) // 128), max(256, (n - start) // 16)
        while True:
            pos, ref, id_off, ids = np.empty(cap, np.int64), np.empty(cap, np.uint8), np.empty(cap + 1, np.int64), np.empty(ids_cap, np.uint8)
            id_bytes, end_off, past = C.c_int64(0), C.c_int64(0), C.c_int32(0)
            tail = (cap, pos.ctypes.data, ref.ctypes.data, id_off.ctypes.data, ids.ctypes.data, ids_cap, C.byref(id_bytes), C.byref(end_off), C.byref(past))
            if self._h is not None:
                k = L.strk_dbam_vcf_snvs(self._h, start, name, beg, end, final, prev, seen, self.tile_bytes, *tail)
            else:
                k = L.strk_vcf_snvs(buf.ctypes.data, n, start, name, beg, end, final, prev, seen, *tail)
            if k < 0 and id_bytes.value > ids_cap:           # the ID bytes did not fit (the count did)
                ids_cap = int(id_bytes.value)
                continue
            if k < 0:
                from .. import _lib
                _lib.check(int(k))
            if k > cap:
                cap, ids_cap = int(k), max(ids_cap, int(id_bytes.value))
                continue
            k = int(k)
            return pos[:k], ref[:k], id_off[:k + 1], ids[:int(id_bytes.value)], int(end_off.value), bool(past.value)

    def window(self, contig: str, beg: int, end: int) -> ContigSnvs | None:
        """The single-base records of `contig` (named with or without "chr") inside [beg, end), or None when the index does not
        have the contig."""
        from .. import _lib
        L = _lib.load()
        t0 = time.perf_counter()
        name = self.index.resolve(contig)
        if name is None:
            return None
        self.n_queries += 1
        beg, end = max(0, int(beg)), max(0, int(end))
        parts = []
        state = [-1, 0]     # the last position reported; whether a record of the contig was seen

        def consume(buf, n, start, final):
            pos, ref, id_off, ids, end_off, past = self._parse(L, buf, n, start, name.encode(), beg, end, final, state[0], state[1])
            if len(pos):
                parts.append((pos, ref, id_off, ids))
                state[0] = int(pos[-1])
            # (a record of the contig seen: only through one that was kept or lies past the window; one in front of it keeps
            # the walk going, which is all `seen` is for)
            state[1] = int(state[1] or len(pos) > 0)
            return end_off, past

        rng = self.index.block_range(name, beg, end)
        if rng is not None:
            self.walk(rng, consume)
        self.seconds += time.perf_counter() - t0
        if not parts:
            z = np.zeros(0, np.int64)
            return ContigSnvs(z, _Column(np.zeros(0, np.uint8), np.zeros(1, np.int64)), _Column(np.zeros(0, np.uint8), np.zeros(1, np.int64)))
        pos = np.concatenate([p[0] for p in parts])
        ref = np.concatenate([p[1] for p in parts])
        ids = np.concatenate([p[3] for p in parts])
        base = np.cumsum([0] + [len(p[3]) for p in parts])
        id_off = np.concatenate([p[2][:-1] + base[i] for i, p in enumerate(parts)] + [base[-1:]]).astype(np.int64)
        return ContigSnvs(pos, _Column(ids, id_off), _Column(ref, np.arange(len(ref) + 1, dtype=np.int64)))


def open_snv_candidates(path: str, front_end: str = "host", device: int = 0):
    """An IndexedSnvVcf when the file is BGZF and <path>.tbi exists; otherwise the whole file, read once (read_snv_vcf)."""
    if os.path.exists(path + ".tbi"):
        with open(path, "rb") as fh:
            head = fh.read(18)
        if len(head) == 18 and head[:4] == b"\x1f\x8b\x08\x04" and head[12:14] == b"BC":
            return IndexedSnvVcf(path, path + ".tbi", front_end, device)
    return read_snv_vcf(path)
