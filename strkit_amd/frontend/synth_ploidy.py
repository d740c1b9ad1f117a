"""Synthetic data for ploidy configurations: contigs chr1, chrX, chrY and chrM with a chosen number of
haplotypes each, loci whose haplotypes carry copy numbers at least 5 apart, error-free reads.  synth_dataset.make_dataset and
its random stream are untouched; this generator has a stream of its own."""
from __future__ import annotations

import os

import numpy as np

from .bam import write_bam
from .fasta import write_fasta
from .synth_dataset import _motif, _rand

__all__ = ["make_ploidy_dataset", "XY_HAPLOTYPES"]

XY_HAPLOTYPES = {"chr1": 2, "chrX": 1, "chrY": 1, "chrM": 1}      # a male sample


def make_ploidy_dataset(out_dir: str, haplotypes: dict | int | None = None, loci_per_contig: int = 3, reads_per_haplotype: int = 12,
                        read_len: int = 2000, seed: int = 19, spacing: int = 4000) -> dict:
    """Writes ref.fa, loci.bed and reads.bam under out_dir.  `haplotypes`: per contig (chr1, chrX, chrY, chrM) the number of
    haplotypes that carry reads, one number for all four, or XY_HAPLOTYPES when None; a contig with 0 is in the reference and
    the catalog but has no reads.  Every haplotype of a locus has a copy number of its own, neighbours 5 to 9 apart; its
    reads_per_haplotype reads of read_len bases span the tract.  Returns paths and the truth: per locus `contig` and `alleles`
    (the haplotypes' copy numbers in ascending order), in catalog order."""
    rng = np.random.default_rng(seed)
    os.makedirs(out_dir, exist_ok=True)
    contigs = ("chr1", "chrX", "chrY", "chrM")
    if haplotypes is None:
        haplotypes = XY_HAPLOTYPES
    if not isinstance(haplotypes, dict):
        haplotypes = {c: int(haplotypes) for c in contigs}
    genomes, loci, records = {}, [], []
    for contig in contigs:
        pieces, pos, here = [], 0, []
        for _ in range(loci_per_contig):
            gap = _rand(rng, spacing)
            motif = _motif(rng, 3, 6)
            while gap.endswith(motif[-1]):
                gap = gap[:-1] + "ACGT".replace(motif[-1], "")[int(rng.integers(3))]
            ref_cn = int(rng.integers(10, 30))
            pieces.append(gap)
            pos += len(gap)
            here.append({"contig": contig, "start": pos, "end": pos + ref_cn * len(motif), "motif": motif, "ref_cn": ref_cn})
            pieces.append(motif * ref_cn)
            pos += ref_cn * len(motif)
        pieces.append(_rand(rng, spacing))
        g = list("".join(pieces))
        for L in here:
            if g[L["end"]] == L["motif"][0]:
                g[L["end"]] = "ACGT".replace(L["motif"][0], "")[int(rng.integers(3))]
        genome = genomes[contig] = "".join(g)
        for L in here:
            k = len(L["motif"])
            n_hap = int(haplotypes.get(contig, 0))
            first = max(3, L["ref_cn"] - int(rng.integers(0, 6)))
            alleles = (first + np.concatenate(([0], np.cumsum(rng.integers(5, 10, max(n_hap - 1, 0)))))).tolist()[:n_hap]
            L["alleles"] = alleles
            for h, cn in enumerate(alleles):
                for ri in range(reads_per_haplotype):
                    left_len = int(rng.integers(600, read_len - 600 - cn * k))
                    start = L["start"] - left_len
                    right_len = read_len - left_len - cn * k
                    seq = genome[start:L["start"]] + L["motif"] * cn + genome[L["end"]:L["end"] + right_len]
                    d = cn - L["ref_cn"]
                    ops = [(left_len, "M")]
                    ops += ([(L["ref_cn"] * k, "M")] + ([(d * k, "I")] if d else [])) if d >= 0 else [(cn * k, "M"), (-d * k, "D")]
                    ops += [(right_len, "M")]
                    records.append({"name": f"{contig}_l{len(loci)}_h{h}_r{ri}", "flag": 0 if ri % 3 else 16, "contig": contig,
                                    "pos": start, "mapq": 60, "cigar": ops, "seq": seq, "qual": np.full(len(seq), 40, np.uint8)})
            loci.append(L)
    write_fasta(os.path.join(out_dir, "ref.fa"), genomes)
    with open(os.path.join(out_dir, "loci.bed"), "w") as fh:
        for i, L in enumerate(loci):
            fh.write(f"{L['contig']}\t{L['start']}\t{L['end']}\tID=pl{i};MOTIF={L['motif']}\n")
    order = {c: i for i, c in enumerate(contigs)}
    records.sort(key=lambda r: (order[r["contig"]], r["pos"]))
    write_bam(os.path.join(out_dir, "reads.bam"), [(c, len(genomes[c])) for c in contigs], records)
    return {"paths": {k: os.path.join(out_dir, v) for k, v in (("ref", "ref.fa"), ("loci", "loci.bed"), ("bam", "reads.bam"))},
            "loci": [{"contig": L["contig"], "alleles": L["alleles"]} for L in loci]}
