"""Synthetic data for methylation from MM / ML tags: diploid loci with CpG-rich tracts (CGG, CCG) and a CG-free
control (CAG), two haplotypes of different copy number and different methylation level, reads of both strands whose MM / ML
tags are written from a per-read truth in all three modes ('', '.', '?'), a share of reads with a decoy entry in front of
the taken one, and a share without tags.  synth_dataset.make_dataset and its random stream are untouched; this generator has
a stream of its own."""
from __future__ import annotations

import os
import struct

import numpy as np

from .bam import write_bam
from .fasta import write_fasta
from .synth_dataset import _rand

__all__ = ["make_methyl_dataset", "encode_mm", "mm_tags", "MOTIFS"]

MOTIFS = ("CGG", "CCG", "CAG")     # the last has no CG: the control
LEVELS = (0.15, 0.85)              # share of methylated tract sites of haplotype 0 / 1


def encode_mm(seq: str, reverse: bool, calls: dict[int, int]) -> tuple[list[int], list[int]]:
    """(skips, probabilities) of a C+m entry for calls at stored positions `calls` (position of the call base -> 0 .. 255):
    stored Cs of a forward read, stored Gs of a reverse one (the Cs of the read as sequenced).  The t-th skip is the number of
    uncalled target bases between call t - 1 and call t, counted along the read as sequenced."""
    n = len(seq)
    order = [p for p in range(n - 1, -1, -1) if seq[p] == "G"] if reverse else [p for p in range(n) if seq[p] == "C"]
    ordinal = {p: o for o, p in enumerate(order)}
    skips, probs, last = [], [], -1
    for o, p in sorted((ordinal[p], p) for p in calls):
        skips.append(o - last - 1)
        probs.append(int(calls[p]))
        last = o
    return skips, probs


def mm_tags(entries: list[tuple[str, list[int], list[int]]], final_semicolon: bool = True, lower: bool = False) -> bytes:
    """Auxiliary bytes MM:Z + ML:B,C of entries (head such as "C+m?", skips, the entry's ML bytes in order)."""
    text = ";".join(head + "".join(f",{d}" for d in skips) for head, skips, _ in entries) + (";" if final_semicolon and entries else "")
    ml = [x for _, _, probs in entries for x in probs]
    mm, mlt = (b"Mm", b"Ml") if lower else (b"MM", b"ML")
    return mm + b"Z" + text.encode() + b"\0" + mlt + b"BC" + struct.pack("<I", len(ml)) + bytes(ml)


def make_methyl_dataset(out_dir: str, n_loci: int = 12, reads_per_locus: int = 24, read_len: int = 3000, seed: int = 17,
                        untagged: float = 0.15, decoy: float = 0.3, spacing: int = 6000, flank_call_rate: float = 0.5,
                        soft_clipped: int = 0) -> dict:
    """Writes ref.fa, loci.bed and reads.bam under out_dir.  Locus i has the motif MOTIFS[i % 3]; haplotype 0 has the smaller
    copy number and methylation level LEVELS[0], haplotype 1 the larger and LEVELS[1]; reads alternate between the two, every
    third read is reverse-strand, and all are error-free.  A tagged read calls every CpG site of its tract but a tenth (left to
    the entry's mode) and a share `flank_call_rate` of its other targets; a methylated site gets a probability of 128 .. 255,
    an unmethylated one 0 .. 127.  `soft_clipped`: that many reads of every locus are aligned up to the middle of the
    tract and soft-clipped from there (what `--realign` picks up; their tags and truth are those of the whole read).  Returns paths and the truth: per read name `reads[name]` = {"hap", "locus", "tagged",
    "mode", "known", "mc", "m"} (m = mc / known, None without a known site), per locus its motif and alleles."""
    rng = np.random.default_rng(seed)
    os.makedirs(out_dir, exist_ok=True)
    pieces, loci, pos = [], [], 0
    for li in range(n_loci):
        motif = MOTIFS[li % 3]
        gap = _rand(rng, spacing)
        while gap.endswith(motif[-1]):
            gap = gap[:-1] + "ACGT".replace(motif[-1], "")[int(rng.integers(3))]
        ref_cn = int(rng.integers(12, 30))
        pieces.append(gap)
        pos += len(gap)
        loci.append({"contig": "chr1", "start": pos, "end": pos + ref_cn * 3, "motif": motif, "ref_cn": ref_cn})
        pieces.append(motif * ref_cn)
        pos += ref_cn * 3
    pieces.append(_rand(rng, spacing))
    g = list("".join(pieces))
    for L in loci:
        if g[L["end"]] == L["motif"][0]:
            g[L["end"]] = "AT"[int(rng.integers(2))]
    genome = "".join(g)
    write_fasta(os.path.join(out_dir, "ref.fa"), {"chr1": genome})
    with open(os.path.join(out_dir, "loci.bed"), "w") as fh:
        for i, L in enumerate(loci):
            fh.write(f"{L['contig']}\t{L['start']}\t{L['end']}\tID=me{i};MOTIF={L['motif']}\n")
    records, truth_loci, reads = [], [], {}
    for li, L in enumerate(loci):
        a0 = max(4, L["ref_cn"] - int(rng.integers(0, 4)))
        a1 = a0 + int(rng.integers(5, 9))
        truth_loci.append({"motif": L["motif"], "alleles": (a0, a1), "control": "CG" not in L["motif"] * 2})
        for ri in range(reads_per_locus):
            h = ri % 2
            cn = (a0, a1)[h]
            left_len = int(rng.integers(1000, read_len - 1000 - cn * 3))
            start = L["start"] - left_len
            right_len = read_len - left_len - cn * 3
            seq = genome[start:L["start"]] + L["motif"] * cn + genome[L["end"]:L["end"] + right_len]
            d = cn - L["ref_cn"]
            ops = [(left_len, "M")]
            ops += ([(L["ref_cn"] * 3, "M")] + ([(d * 3, "I")] if d else [])) if d >= 0 else [(cn * 3, "M"), (-d * 3, "D")]
            ops += [(right_len, "M")]
            if ri < soft_clipped:              # the aligner gave up inside the tract: the left part stays, the rest is clipped
                keep = left_len + min(cn, L["ref_cn"]) * 3 // 2
                ops = [(keep, "M"), (len(seq) - keep, "S")]
            reverse = ri % 3 == 0
            name = f"me{li}_r{ri}"
            q_l, q_r = left_len, left_len + cn * 3
            t = {"hap": h, "locus": li, "tagged": bool(rng.random() >= untagged), "mode": ("", ".", "?")[int(rng.integers(3))],
                 "known": 0, "mc": 0, "m": None}
            aux = b"RGZgrp\0"
            if t["tagged"]:
                calls: dict[int, int] = {}
                target = "G" if reverse else "C"
                for p in range(len(seq) - 1):
                    site = seq[p] == "C" and seq[p + 1] == "G"
                    if site and q_l <= p < q_r:
                        listed = rng.random() >= 0.1
                        methylated = rng.random() < LEVELS[h]
                        prob = int(rng.integers(128, 256)) if methylated else int(rng.integers(0, 128))
                        if listed:
                            calls[p + 1 if reverse else p] = prob
                            t["known"] += 1
                            t["mc"] += prob > 127
                        elif t["mode"] != "?":
                            t["known"] += 1
                for p in range(len(seq)):     # the other targets of the read, CpG or not
                    if seq[p] == target and p not in calls and not (q_l <= p <= q_r) and rng.random() < flank_call_rate:
                        calls[p] = int(rng.integers(0, 256))
                skips, probs = encode_mm(seq, reverse, calls)
                entries = [("C+m" + t["mode"], skips, probs)]
                if rng.random() < decoy:
                    n_dec = int(rng.integers(0, 5))
                    dec = (("A+a", 1), ("C+h.", 1), ("G-m?", 1), ("C+76792", 1), ("T+gc", 2))[int(rng.integers(5))]
                    entries.insert(0, (dec[0], [int(x) for x in rng.integers(0, 9, n_dec)], [int(x) for x in rng.integers(0, 256, n_dec * dec[1])]))
                aux += mm_tags(entries, final_semicolon=bool(rng.random() < 0.8))
                t["m"] = t["mc"] / t["known"] if t["known"] else None
            reads[name] = t
            records.append({"name": name, "flag": 16 if reverse else 0, "contig": "chr1", "pos": start, "mapq": 60, "cigar": ops, "seq": seq,
                            "qual": np.full(len(seq), 40, np.uint8), "tags": aux})
    records.sort(key=lambda r: r["pos"])
    write_bam(os.path.join(out_dir, "reads.bam"), [("chr1", len(genome))], records)
    return {"paths": {k: os.path.join(out_dir, v) for k, v in (("ref", "ref.fa"), ("loci", "loci.bed"), ("bam", "reads.bam"))},
            "loci": truth_loci, "reads": reads}
