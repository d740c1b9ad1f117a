"""Synthetic data for phasing from files: diploid loci whose two haplotypes differ at 1-6 heterozygous flank
positions, reads with HP / PS tags of mixed integer types, and a candidate VCF with the heterozygous sites plus decoys.
synth_dataset.make_dataset and its random stream are untouched; this generator has a stream of its own."""
from __future__ import annotations

import os
import struct

import numpy as np

from .bam import write_bam
from .fasta import write_fasta
from .synth_dataset import _motif, _rand

__all__ = ["make_phased_dataset"]

_OTHER = {"A": "C", "C": "G", "G": "T", "T": "A"}


def _int_tag(tag: bytes, ty: str, val: int) -> bytes:
    return tag + ty.encode() + struct.pack({"c": "<b", "C": "<B", "s": "<h", "S": "<H", "i": "<i", "I": "<I"}[ty], val)


def make_phased_dataset(out_dir: str, n_loci: int = 12, reads_per_locus: int = 24, read_len: int = 3000, seed: int = 11,
                        equal_cn: bool = True, tags: bool = True, untagged: float = 0.0, flank_size: int = 70,
                        spacing: int = 6000, soft_clipped: int = 0) -> dict:
    """Writes ref.fa, loci.bed, reads.bam and snvs.vcf under out_dir.  Haplotype 0 is the reference outside the tract,
    haplotype 1 carries the ALT base at the locus's heterozygous sites; reads alternate between the two and are error-free.
    `equal_cn`: both haplotypes have the same copy number (only phasing can tell them apart).  `tags`: every read (but a share
    `untagged`) carries HP = haplotype + 1 and PS = one value per four loci, in integer types that vary from read to read.
    `soft_clipped`: that many reads of every locus are aligned up to the middle of the tract and soft-clipped from there (what
    `--realign` picks up).  The VCF holds the heterozygous sites and decoys: homozygous sites (both haplotypes carry the ALT), positions inside the
    tract, an indel record and a record with a multi-base ALT.  Returns paths and the truth: per locus `het` / `decoys`
    (0-based positions), `alleles`, `ps`, and per read name its haplotype."""
    rng = np.random.default_rng(seed)
    os.makedirs(out_dir, exist_ok=True)
    pieces, loci, pos = [], [], 0
    for li in range(n_loci):
        gap = _rand(rng, spacing)
        motif = _motif(rng, 3, 6)
        while gap.endswith(motif[-1]):
            gap = gap[:-1] + "ACGT".replace(motif[-1], "")[int(rng.integers(3))]
        ref_cn = int(rng.integers(10, 30))
        pieces.append(gap)
        pos += len(gap)
        loci.append({"contig": "chr1", "start": pos, "end": pos + ref_cn * len(motif), "motif": motif, "ref_cn": ref_cn})
        pieces.append(motif * ref_cn)
        pos += ref_cn * len(motif)
    pieces.append(_rand(rng, spacing))
    g = list("".join(pieces))
    for L in loci:
        if g[L["end"]] == L["motif"][0]:
            g[L["end"]] = "ACGT".replace(L["motif"][0], "")[int(rng.integers(3))]
    genome = "".join(g)
    write_fasta(os.path.join(out_dir, "ref.fa"), {"chr1": genome})
    with open(os.path.join(out_dir, "loci.bed"), "w") as fh:
        for i, L in enumerate(loci):
            fh.write(f"{L['contig']}\t{L['start']}\t{L['end']}\tID=ph{i};MOTIF={L['motif']}\n")
    records, vcf, truth_loci, read_hap = [], [], [], {}
    types = "cCsSiI"
    for li, L in enumerate(loci):
        k = len(L["motif"])
        a0 = max(2, L["ref_cn"] + int(rng.integers(-3, 4)))
        a1 = a0 if equal_cn else max(2, a0 + int(rng.integers(3, 7)))
        # sites within reach of every read: 100 .. 700 bases outside the flanked locus, on either side
        left = np.arange(L["start"] - flank_size - 700, L["start"] - flank_size - 100)
        right = np.arange(L["end"] + flank_size + 100, L["end"] + flank_size + 700)
        sites = rng.choice(np.concatenate((left, right)), int(rng.integers(1, 7)) + 2, replace=False)
        het, hom = np.sort(sites[:-2]), np.sort(sites[-2:])
        inside = [L["start"] + 1, L["start"] + k + 1]
        ps = 50000 + 7 * (li // 4)
        haps = []
        for h in (0, 1):
            s = list(genome)
            for p in hom:
                s[p] = _OTHER[genome[p]]
            if h == 1:
                for p in het:
                    s[p] = _OTHER[genome[p]]
            haps.append(s)
        for p in het:
            vcf.append((int(p), f"het{li}_{p}", genome[p], _OTHER[genome[p]]))
        for p in list(hom) + inside:
            vcf.append((int(p), f"decoy{li}_{p}", genome[p], _OTHER[genome[p]]))
        vcf.append((int(left[0]) - 20, f"indel{li}", genome[left[0] - 20:left[0] - 18], genome[left[0] - 20]))
        vcf.append((int(left[0]) - 40, f"multi{li}", genome[left[0] - 40], "GT"))
        for ri in range(reads_per_locus):
            h = ri % 2
            cn = (a0, a1)[h]
            left_len = int(rng.integers(1000, read_len - 1000 - cn * k))
            start = L["start"] - left_len
            right_len = read_len - left_len - cn * k
            seq = "".join(haps[h][start:L["start"]]) + L["motif"] * cn + "".join(haps[h][L["end"]:L["end"] + right_len])
            d = cn - L["ref_cn"]
            ops = [(left_len, "M")]
            ops += ([(L["ref_cn"] * k, "M")] + ([(d * k, "I")] if d else [])) if d >= 0 else [(cn * k, "M"), (-d * k, "D")]
            ops += [(right_len, "M")]
            if ri < soft_clipped:              # the aligner gave up inside the tract: the left part stays, the rest is clipped
                keep = left_len + min(cn, L["ref_cn"]) * k // 2
                ops = [(keep, "M"), (len(seq) - keep, "S")]
            name = f"ph{li}_r{ri}"
            aux = b""
            if tags and rng.random() >= untagged:
                aux = _int_tag(b"HP", types[int(rng.integers(0, 4))], h + 1) + b"RGZgrp\0" + _int_tag(b"PS", types[int(rng.integers(3, 6))], ps)
            records.append({"name": name, "flag": 0 if ri % 3 else 16, "contig": "chr1", "pos": start, "mapq": 60, "cigar": ops, "seq": seq,
                            "qual": np.full(len(seq), 40, np.uint8), "tags": aux})
            read_hap[name] = h
        truth_loci.append({"het": [int(p) for p in het], "decoys": [int(p) for p in list(hom) + inside], "alleles": (a0, a1), "ps": ps})
    records.sort(key=lambda r: r["pos"])
    write_bam(os.path.join(out_dir, "reads.bam"), [("chr1", len(genome))], records)
    with open(os.path.join(out_dir, "snvs.vcf"), "w") as fh:
        fh.write("##fileformat=VCFv4.2\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\n")
        for p, i, r, a in sorted(vcf):
            fh.write(f"chr1\t{p + 1}\t{i}\t{r}\t{a}\t.\t.\t.\n")
    return {"paths": {k: os.path.join(out_dir, v) for k, v in (("ref", "ref.fa"), ("loci", "loci.bed"), ("bam", "reads.bam"), ("snvs", "snvs.vcf"))},
            "loci": truth_loci, "read_hap": read_hap}
