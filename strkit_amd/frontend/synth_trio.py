"""Synthetic data for `mi`: a child / mother / father trio over one reference and one catalog, three alignment
files.  The parents are diploid with copy numbers of their own; the child inherits one haplotype of each parent at every locus;
a named subset of loci carries a de novo change of +1 to +3 copies on one child allele.  Error-free reads, in the manner of
synth_ploidy.py; a random stream of its own."""
from __future__ import annotations

import os

import numpy as np

from .bam import write_bam
from .fasta import write_fasta
from .synth_dataset import _motif, _rand

__all__ = ["make_trio_dataset", "MEMBERS"]

MEMBERS = ("child", "mother", "father")


def make_trio_dataset(out_dir: str, n_loci: int = 12, de_novo: tuple = (2, 7), reads_per_haplotype: int = 12, read_len: int = 2000,
                      seed: int = 22, spacing: int = 4000, contigs: tuple = ("chr1", "chr2"), allele_gap: tuple = (2, 7),
                      apart: bool = False) -> dict:
    """Writes ref.fa, loci.bed and child.bam, mother.bam, father.bam under out_dir.  Locus i lies on contigs[i % len(contigs)].
    Each parent has two copy numbers allele_gap[0] .. allele_gap[1] - 1 apart (apart = True: the father's lie above the
    mother's by as much, so that all four differ); the child takes one of the mother's and one of the father's; the loci whose
    index is in `de_novo` get +1 .. +3 copies on one of the child's two alleles.  Every haplotype has reads_per_haplotype reads
    of read_len bases that span the tract.  Returns paths and the truth per locus in catalog order: contig, start, end, motif,
    ref_cn, the three members' alleles as (maternal or first, paternal or second), `inherited` = (index of the mother's allele,
    index of the father's) and `de_novo` = None or (which child allele: 0 from the mother / 1 from the father, copies added)."""
    rng = np.random.default_rng(seed)
    os.makedirs(out_dir, exist_ok=True)
    per_contig: dict[str, list] = {c: [] for c in contigs}
    for i in range(n_loci):
        per_contig[contigs[i % len(contigs)]].append(i)
    genomes, loci = {}, [None] * n_loci
    records = {m: [] for m in MEMBERS}
    for contig in contigs:
        pieces, pos, here = [], 0, []
        for i in per_contig[contig]:
            gap = _rand(rng, spacing)
            motif = _motif(rng, 3, 6)
            while gap.endswith(motif[-1]):
                gap = gap[:-1] + "ACGT".replace(motif[-1], "")[int(rng.integers(3))]
            ref_cn = int(rng.integers(10, 30))
            pieces.append(gap)
            pos += len(gap)
            here.append({"index": i, "contig": contig, "start": pos, "end": pos + ref_cn * len(motif), "motif": motif, "ref_cn": ref_cn})
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
            mother = [max(3, L["ref_cn"] - int(rng.integers(0, 5)))]
            mother.append(mother[0] + int(rng.integers(*allele_gap)))
            father = [mother[1] + int(rng.integers(*allele_gap)) if apart else max(3, L["ref_cn"] - int(rng.integers(0, 5)) + 1)]
            father.append(father[0] + int(rng.integers(*allele_gap)))
            inherited = (int(rng.integers(2)), int(rng.integers(2)))
            child = [mother[inherited[0]], father[inherited[1]]]
            L["de_novo"] = None
            if L["index"] in de_novo:
                L["de_novo"] = (int(rng.integers(2)), int(rng.integers(1, 4)))
                child[L["de_novo"][0]] += L["de_novo"][1]
            L.update(child=tuple(child), mother=tuple(mother), father=tuple(father), inherited=inherited)
            for member in MEMBERS:
                for h, cn in enumerate(L[member]):
                    for ri in range(reads_per_haplotype):
                        left_len = int(rng.integers(600, read_len - 600 - cn * k))
                        start = L["start"] - left_len
                        right_len = read_len - left_len - cn * k
                        seq = genome[start:L["start"]] + L["motif"] * cn + genome[L["end"]:L["end"] + right_len]
                        d = cn - L["ref_cn"]
                        ops = [(left_len, "M")]
                        ops += ([(L["ref_cn"] * k, "M")] + ([(d * k, "I")] if d else [])) if d >= 0 else [(cn * k, "M"), (-d * k, "D")]
                        ops += [(right_len, "M")]
                        records[member].append({"name": f"{member}_l{L['index']}_h{h}_r{ri}", "flag": 0 if ri % 3 else 16, "contig": contig,
                                                "pos": start, "mapq": 60, "cigar": ops, "seq": seq, "qual": np.full(len(seq), 40, np.uint8)})
            loci[L["index"]] = L
    # the catalog in contig order, as the alignment files are sorted
    catalog = sorted(loci, key=lambda L: (contigs.index(L["contig"]), L["start"]))
    write_fasta(os.path.join(out_dir, "ref.fa"), genomes)
    with open(os.path.join(out_dir, "loci.bed"), "w") as fh:
        for L in catalog:
            fh.write(f"{L['contig']}\t{L['start']}\t{L['end']}\tID=trio{L['index']};MOTIF={L['motif']}\n")
    order = {c: i for i, c in enumerate(contigs)}
    for member in MEMBERS:
        records[member].sort(key=lambda r: (order[r["contig"]], r["pos"]))
        write_bam(os.path.join(out_dir, member + ".bam"), [(c, len(genomes[c])) for c in contigs], records[member])
    names = (("ref", "ref.fa"), ("loci", "loci.bed")) + tuple((m, m + ".bam") for m in MEMBERS)
    keep = ("index", "contig", "start", "end", "motif", "ref_cn", "child", "mother", "father", "inherited", "de_novo")
    return {"paths": {k: os.path.join(out_dir, v) for k, v in names}, "loci": [{k: L[k] for k in keep} for L in catalog]}
