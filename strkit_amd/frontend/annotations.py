"""The annotations of `--gff` / `--annotation-file`: per catalog locus the ids of the genome features it overlaps, from a
tabix-indexed GFF3 or GTF file.  Stands where the reference fetches the features of every locus (strkit/call/loci.py:158-166,
209-214, 250-253: one TabixFile.fetch per locus through pysam's asGFF3 / asGTF).  Here a contig's part of the file is read once
and all its loci are joined against it by the library (IndexedAnnotations; DESIGN.md §19: on the device or on the host cores).

The rule is written once, below, in plain Python (parse_line, attributes, feature_id, read_annotations, annotate); the tests hold
the library against it.  It is UNPINNED: pysam is not available, so nothing here was compared against asGFF3 / asGTF, and the
index layout is unpinned against htslib (frontend/tabix.py).  Stated choices: attribute values are not percent-decoded; GTF
values stay text (pysam turns unquoted numbers into numbers, whose str() would drop leading zeros); a GFF3 piece without '=' is a
key with an empty value; `exon` is not among the types that use exon_id (as in the reference)."""
from __future__ import annotations

import ctypes as C
import gzip
import os
import time
from dataclasses import dataclass

import numpy as np

from .loci import resolve_contig
from .tabix_text import TabixText

__all__ = ["Feature", "Annotations", "AnnotationError", "parse_line", "attributes", "feature_id", "read_annotations", "annotate",
           "is_gtf", "IndexedAnnotations", "annotate_rows", "EXON_FEATURE_TYPES"]

EXON_FEATURE_TYPES = frozenset(("5UTR", "3UTR", "CDS", "start_codon", "stop_codon"))   # loci.py:155
_DIGITS = frozenset("0123456789")


class AnnotationError(ValueError):
    """A line that breaks the rule; `offset` = the byte offset of the line in the text."""

    def __init__(self, offset: int, why: str):
        super().__init__(f"line at byte {offset}: {why}")
        self.offset = offset


@dataclass
class Feature:
    contig: str
    type: str
    beg: int           # 0-based
    end: int           # exclusive
    id: str


def is_gtf(path: str) -> bool:
    """As the reference decides (loci.py:213)."""
    return ".gtf" in path


def attributes(column: str, gtf: bool) -> dict[str, str]:
    out: dict[str, str] = {}
    if not gtf:
        for piece in column.split(";"):
            key, _, value = piece.lstrip(" ").partition("=")
            out[key] = value
        return out
    pieces, cur, quoted = [], [], False
    for ch in column:
        if ch == '"':
            quoted = not quoted
        if ch == ";" and not quoted:
            pieces.append("".join(cur))
            cur = []
        else:
            cur.append(ch)
    pieces.append("".join(cur))
    for piece in pieces:
        key, _, value = piece.strip(" ").partition(" ")
        value = value.strip(" ")
        if len(value) >= 2 and value[0] == '"' and value[-1] == '"':
            value = value[1:-1]
        out[key] = value
    return out


def feature_id(contig: str, type_: str, beg: int, end: int, attrs: dict[str, str]) -> str:
    """get_feature_id (loci.py:158-166)."""
    if "ID" in attrs:
        return attrs["ID"]
    if type_ in EXON_FEATURE_TYPES and "exon_id" in attrs:
        return f"{type_}:{attrs['exon_id']}"
    return f"{type_}:{contig}-{beg}-{end}"


def parse_line(line: str, offset: int, gtf: bool) -> Feature | None:
    """One line without its '\\n' -> the feature, None for an empty or comment line, AnnotationError for anything else."""
    line = line.rstrip("\r")
    if not line or line[0] == "#":
        return None
    f = line.split("\t")
    if len(f) < 9:
        raise AnnotationError(offset, f"{len(f)} tab-separated fields, a feature line has nine")
    for v in (f[3], f[4]):
        if not 1 <= len(v) <= 18 or not set(v) <= _DIGITS:
            raise AnnotationError(offset, f"start / end {v!r} is not 1 to 18 decimal digits")
    start, end = int(f[3]), int(f[4])
    if not 1 <= start <= end:
        raise AnnotationError(offset, f"start {start} and end {end} do not satisfy 1 <= start <= end")
    return Feature(f[0], f[2], start - 1, end, feature_id(f[0], f[2], start - 1, end, attributes(f[8], gtf)))


class Annotations:
    """The features of a file read whole, per contig in file order."""

    def __init__(self, by_contig: dict[str, list[Feature]]):
        self.by_contig = by_contig

    def contig_overlaps(self, contig: str, starts, ends) -> list[list[str]]:
        name = resolve_contig(self.by_contig, contig)
        feats = self.by_contig[name] if name is not None else []
        return [[ft.id for ft in feats if ft.beg < e and ft.end > s] for s, e in zip(starts, ends)]


def parse_text(text: bytes, gtf: bool) -> Annotations:
    by_contig: dict[str, list[Feature]] = {}
    off = 0
    for raw in text.split(b"\n"):
        ft = parse_line(raw.decode("latin-1"), off, gtf)
        if ft is not None:
            feats = by_contig.setdefault(ft.contig, [])
            if feats and ft.beg < feats[-1].beg:
                raise AnnotationError(off, f"start {ft.beg + 1} after {feats[-1].beg + 1}: not coordinate-sorted")
            feats.append(ft)
        off += len(raw) + 1
    return Annotations(by_contig)


def read_annotations(path: str, gtf: bool | None = None) -> Annotations:
    """The whole file, plain or gzip: the restatement the tests hold the library against."""
    with open(path, "rb") as fh:
        text = fh.read()
    if text[:2] == b"\x1f\x8b":
        text = gzip.decompress(text)
    return parse_text(text, is_gtf(path) if gtf is None else gtf)


def annotate(loci, source) -> list[list[str]]:
    """Per locus (anything with .contig, .start, .end; or (contig, start, end)), in the order given, the ids of the features it
    overlaps, in file order.  `source`: an Annotations or an IndexedAnnotations.  One contig_overlaps call per contig."""
    loci = [(l.contig, l.start, l.end) if hasattr(l, "contig") else tuple(l) for l in loci]
    out: list[list[str]] = [[] for _ in loci]
    by_contig: dict[str, list[int]] = {}
    for i, l in enumerate(loci):
        by_contig.setdefault(l[0], []).append(i)
    for contig, idx in by_contig.items():
        idx.sort(key=lambda i: (loci[i][1], loci[i][2]))
        got = source.contig_overlaps(contig, [loci[i][1] for i in idx], [loci[i][2] for i in idx])
        for i, ids in zip(idx, got):
            out[i] = ids
    return out


class IndexedAnnotations(TabixText):
    """A BGZF-compressed GFF3 / GTF file with its tabix index: `contig_overlaps` walks the contig's byte range once, in pieces
    (TabixText.walk), and has the library join every piece against all of the contig's loci — on the device (front_end="device": a
    strk_dbam object of its own holds the inflated piece in HBM; strk_dbam_gff_overlaps) or on the host cores
    (strk_bgzf_inflate_range + strk_gff_overlaps).  Counters as IndexedSnvVcf's."""

    def __init__(self, path: str, index: str | None = None, front_end: str = "host", device: int = 0, piece_bytes: int = 32 << 20,
                 tile_bytes: int = 0, gtf: bool | None = None):
        super().__init__(path, index or path + ".tbi", front_end, device, piece_bytes, tile_bytes, "gff")
        self.gtf = is_gtf(path) if gtf is None else bool(gtf)

    def _precondition(self, path: str, index: str) -> None:
        with open(path, "rb") as fh:
            head = fh.read(18)
        if not (len(head) == 18 and head[:4] == b"\x1f\x8b\x08\x04" and head[12:14] == b"BC") or not os.path.exists(index):
            raise ValueError(f"{path}: an annotation file must be BGZF-compressed with a tabix index next to it ({index}); "
                             f"bgzip the sorted file and run `tabix -p gff` on it")

    def _join(self, L, buf, n, start, name, final, prev, ls, le):
        """One library call over a piece, with the arrays grown to what it asks for -> (pair_locus, pair_feat, ids of the hit
        features, last f_beg, end_off, past)."""
        n_loci = len(ls)
        caps = [max(64, 4 * n_loci), max(64, n_loci), 4096]
        while True:
            pl, pf = np.empty(caps[0], np.int32), np.empty(caps[0], np.int32)
            fb, fe, fk, fo = np.empty(caps[1], np.int64), np.empty(caps[1], np.int64), np.empty(caps[1], np.int32), np.empty(2 * caps[1] + 1, np.int64)
            text = np.empty(caps[2], np.uint8)
            sizes, end_off, past = np.zeros(4, np.int64), C.c_int64(0), C.c_int32(0)
            tail = (n_loci, ls.ctypes.data, le.ctypes.data, caps[0], pl.ctypes.data, pf.ctypes.data, caps[1], fb.ctypes.data, fe.ctypes.data, fk.ctypes.data,
                    fo.ctypes.data, caps[2], text.ctypes.data, sizes.ctypes.data, C.byref(end_off), C.byref(past))
            if self._h is not None:
                k = L.strk_dbam_gff_overlaps(self._h, start, name, int(self.gtf), final, prev, self.tile_bytes, *tail)
            else:
                k = L.strk_gff_overlaps(buf.ctypes.data, n, start, name, int(self.gtf), final, prev, *tail)
            if k < 0:
                from .. import _lib
                _lib.check(int(k))
            if any(int(sizes[i]) > caps[i] for i in range(3)):
                caps = [max(caps[i], int(sizes[i])) for i in range(3)]
                continue
            n_pairs, n_feat = int(sizes[0]), int(sizes[1])
            raw = text[:int(sizes[2])].tobytes().decode("latin-1")      # (one decode; plain lists: no numpy scalar per feature)
            contig = name.decode()
            off, kinds, begs, ends = fo[:2 * n_feat + 1].tolist(), fk[:n_feat].tolist(), fb[:n_feat].tolist(), fe[:n_feat].tolist()
            ids = []
            for j in range(n_feat):
                a, b, c = off[2 * j], off[2 * j + 1], off[2 * j + 2]
                ids.append(raw[b:c] if kinds[j] == 0 else f"{raw[a:b]}:{raw[b:c]}" if kinds[j] == 1 else f"{raw[a:b]}:{contig}-{begs[j]}-{ends[j]}")
            return pl[:n_pairs], pf[:n_pairs], ids, int(sizes[3]), int(end_off.value), bool(past.value)

    def locus_overlaps(self, contig: str, start: int, end: int) -> list[str]:
        """One locus through one index query of its own, the way the reference fetches (loci.py:252): the linear index names where
        to begin, which a contig-long feature pulls back to the contig's start.  For comparison (tools/bench_annot.py); `call`
        does not use it."""
        name = self.index.resolve(contig)
        rng = self.index.block_range(name, int(start), max(int(end), int(start) + 1)) if name is not None else None
        return self.contig_overlaps(contig, [start], [end], _range=rng)[0] if rng is not None else []

    def contig_overlaps(self, contig: str, starts, ends, _range=None) -> list[list[str]]:
        """Per locus [starts[i], ends[i]) of `contig` (named with or without "chr"), in the order given, the ids of the features it
        overlaps, in file order; empty lists when the index does not have the contig."""
        from .. import _lib
        L = _lib.load()
        t0 = time.perf_counter()
        starts, ends = np.asarray(starts, np.int64), np.asarray(ends, np.int64)
        out: list[list[str]] = [[] for _ in range(len(starts))]
        name = self.index.resolve(contig)
        rng = (_range or self.index.contig_range(name)) if name is not None and len(starts) else None
        if rng is None:
            return out
        self.n_queries += 1
        order = np.argsort(starts, kind="stable")
        ls, le = np.ascontiguousarray(starts[order]), np.ascontiguousarray(ends[order])
        prev = [-1]         # the last f_beg of the contig so far

        def consume(buf, n, start, final):
            pl, pf, ids, prev[0], end_off, past = self._join(L, buf, n, start, name.encode(), final, prev[0], ls, le)
            for l, j in zip(order[pl].tolist(), pf.tolist()):      # pieces come in file order, so do a locus's ids
                out[l].append(ids[j])
            return end_off, past

        self.walk(rng, consume)
        self.seconds += time.perf_counter() - t0
        return out


def annotate_rows(rows: list[dict], path: str, front_end: str = "host", device: int = 0) -> dict:
    """Fills row["annotations"] of every row of a report (contig / start / end are the catalog's) from the annotation file: one
    walk per contig of the rows.  Returns the reader's counters for stage_times."""
    src = IndexedAnnotations(path, front_end=front_end, device=device)
    try:
        for row, ids in zip(rows, annotate([(r["contig"], r["start"], r["end"]) for r in rows], src)):
            row["annotations"] = ids
        tm = {"annotate_s": src.seconds, "annotate_compressed_mb": round(src.compressed_bytes / 1e6, 4)}
        if front_end == "device":
            tm["annotate_device_s"] = src.kernel_s()
        return tm
    finally:
        src.close()
