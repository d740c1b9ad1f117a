"""The candidate SNVs of `--incorporate-snvs`: a VCF (plain, gzip or BGZF text) read once, through Python's `gzip`; no .tbi
region queries.  Stands where the reference opens its SNV VCF (strkit/call/call_sample.py:133-157, strkit_rust_ext's
STRkitVCFReader): only records whose REF and every ALT are single bases count (no indels, no symbolic or multi-base
alleles); what comes back per contig is what frontend/phase_inputs.py's locus_candidates takes."""
from __future__ import annotations

import gzip
from dataclasses import dataclass

import numpy as np

from .loci import resolve_contig

__all__ = ["SnvCandidates", "read_snv_vcf"]

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
