"""A tabix index (.tbi) of a BGZF-compressed VCF (or, with preset="gff", of a GFF3 / GTF file): which compressed bytes hold the records of a region.  Stands where the
reference's reader hands a locus block to htslib's tabix access (call_sample.py:124); the layout is the one of the tabix
specification (samtools.github.io/hts-specs/tabix.pdf), the binning scheme the one of `synth_large._reg2bin` and `write_bai`.
Unpinned against htslib: the only writer on hand is `synth_snvs.write_tbi`, which comes from the same reading of the format.

The index file is itself BGZF and small (kilobytes to a few megabytes): it is inflated on the host."""
from __future__ import annotations

import gzip
import os
import struct
import warnings

import numpy as np

from .loci import resolve_contig

__all__ = ["TabixIndex", "reg2bins"]

_META_BIN = 37450
_LEVELS = ((26, 1), (23, 9), (20, 73), (17, 585), (14, 4681))


def reg2bins(beg: int, end: int) -> list[int]:
    """The bins that may hold records overlapping [beg, end): bin 0 and the region's bins on the five levels below it."""
    end = min(end, 1 << 29) - 1
    out = [0]
    for shift, base in _LEVELS:
        out.extend(range(base + (beg >> shift), base + (end >> shift) + 1))
    return out


class TabixIndex:
    """`names`: the contigs in the index's order; per contig the bins with their chunks and the 16 kb linear index."""

    def __init__(self, path: str, vcf_path: str | None = None, preset: str = "vcf"):
        """`preset`: "vcf" (format 2, columns 1 / 2) or, by request only, "gff" (the generic format 0 with columns 1 / 4 / 5 and
        the comment character '#': what `tabix -p gff` writes); an index of any other layout is refused."""
        if preset not in ("vcf", "gff"):
            raise ValueError(f"preset must be 'vcf' or 'gff', not {preset!r}")
        self.path, self.preset = path, preset
        if vcf_path is not None and os.path.getmtime(path) + 1.0 < os.path.getmtime(vcf_path):
            warnings.warn(f"{path} is older than {vcf_path}: the index may be stale (re-index the file if records go missing)",
                          RuntimeWarning, stacklevel=3)
        try:
            with gzip.open(path, "rb") as fh:
                raw = fh.read()
        except (OSError, EOFError) as e:
            raise ValueError(f"{path}: not a tabix index (it does not inflate: {e})") from None
        if raw[:4] != b"TBI\x01":
            raise ValueError(f"{path}: not a tabix index (bad magic)")
        try:
            self._parse(raw)
        except (struct.error, IndexError):
            raise ValueError(f"{path}: truncated tabix index") from None

    def _parse(self, raw: bytes) -> None:
        n_ref, fmt, col_seq, col_beg, col_end, meta, _skip, l_nm = struct.unpack_from("<8i", raw, 4)
        if self.preset == "gff":
            if fmt != 0 or (col_seq, col_beg, col_end) != (1, 4, 5) or meta != ord("#"):
                raise ValueError(f"{self.path}: not the index of a GFF3 / GTF file (format {fmt}, columns {col_seq} / {col_beg} / {col_end}, "
                                 f"comment character {meta}; expected 0, 1 / 4 / 5, {ord('#')})")
        elif fmt != 2 or col_seq != 1 or col_beg != 2:
            raise ValueError(f"{self.path}: not the index of a VCF (format {fmt}, columns {col_seq} / {col_beg}; expected 2, 1 / 2)")
        if n_ref < 0 or l_nm < 0 or 36 + l_nm > len(raw):
            raise IndexError
        names = raw[36:36 + l_nm].split(b"\0")[:-1]
        if len(names) != n_ref:
            raise ValueError(f"{self.path}: {len(names)} contig names for {n_ref} contigs")
        self.names = [n.decode() for n in names]
        off = 36 + l_nm
        self.bins: list[dict[int, np.ndarray]] = []
        self.linear: list[np.ndarray] = []
        for _ in range(n_ref):
            n_bin, = struct.unpack_from("<i", raw, off)
            off += 4
            bins = {}
            for _b in range(n_bin):
                b, n_chunk = struct.unpack_from("<Ii", raw, off)
                off += 8
                if n_chunk < 0 or off + 16 * n_chunk > len(raw):
                    raise IndexError
                if b != _META_BIN:
                    bins[b] = np.frombuffer(raw, "<u8", 2 * n_chunk, off).reshape(n_chunk, 2)
                off += 16 * n_chunk
            n_intv, = struct.unpack_from("<i", raw, off)
            off += 4
            if n_intv < 0 or off + 8 * n_intv > len(raw):
                raise IndexError
            self.bins.append(bins)
            self.linear.append(np.frombuffer(raw, "<u8", n_intv, off))
            off += 8 * n_intv
        # (an optional uint64, the number of unplaced records, may follow)

    def resolve(self, contig: str) -> str | None:
        """The contig as the file spells it (with or without "chr"), or None."""
        return resolve_contig(self.names, contig)

    def contig_range(self, contig: str) -> tuple[int, int] | None:
        """(virtual offset of the contig's first record, compressed offset of the last BGZF block that holds one of its records), from
        the chunks of all its bins (a first record at virtual offset 0, which the linear index cannot tell from "none", is found
        too), or None when the index knows of none."""
        name = self.resolve(contig)
        if name is None:
            return None
        chunks = [c for c in self.bins[self.names.index(name)].values() if len(c)]
        if not chunks:
            return None
        both = np.concatenate(chunks)
        start, stop = int(both[:, 0].min()), int(both[:, 1].max())
        return (start, stop >> 16) if stop > start else None

    def block_range(self, contig: str, beg: int, end: int) -> tuple[int, int] | None:
        """(virtual offset to start reading at, compressed offset of the last BGZF block that has to be read) for the records of
        `contig` inside [beg, end), or None when the index knows of none.  Records in front of `beg` may come first (the linear
        index's entry of a window without records is its neighbour's): the reader filters by position."""
        name = self.resolve(contig)
        if name is None or end <= beg:
            return None
        tid = self.names.index(name)
        lin = self.linear[tid]
        w = max(0, int(beg)) >> 14
        nz = np.flatnonzero(lin[w:]) if w < len(lin) else np.zeros(0, np.int64)
        if nz.size == 0:
            return None
        start = int(lin[w + int(nz[0])])
        # the stop comes from the bins, never from the linear index: a record with a long REF that begins windows earlier pulls a
        # later window's entry back in front of records that are still wanted
        bins = self.bins[tid]
        stop = max((int(bins[b][:, 1].max()) for b in reg2bins(max(0, int(beg)), int(end)) if b in bins and len(bins[b])), default=None)
        if stop is None or stop <= start:
            return None
        return start, stop >> 16
