#!/usr/bin/env python3
"""Writes tests/golden/mi/{child,mother,father}.{json,vcf}: three small reports of one catalog, built row by row here and written
by this project's own writers (frontend.call.write_json, frontend.output.write_vcf), for tests/test_mi_frontend.py.  Needs no
GPU:  python tests/golden/make_mi_golden.py.  The rows (key -> per member the call, or what is wrong with it):

  chr1:1000-1040 CAG   all called, two peaks each, inherited; the child alone carries a phase set
  chr1:2000-2030 AT    all called; the child's second allele is the father's 12 copies + 3 (de novo); 16 reads per allele
  chr1:3000-3024 GGC   all called; the child is homozygous with ONE peak called by distance (split in two by `mi`)
  chr1:4000-4020 A     not in the father's file
  chr1:5000-5030 TTA   the mother's call failed
  chr2:100-160 CA      the father is haploid here (one allele): skipped and counted
  chr2:500-548 AAG     all called, all three phased
  chr2:700-730 TG      the child is homozygous with two peaks assigned by SNVs (not split)
  chrX:900-930 CGG     all called, on a sex chromosome: dropped"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from strkit_amd.frontend.call import write_json  # noqa: E402
from strkit_amd.frontend.output import write_vcf  # noqa: E402

ANCHOR = "GATTACAGATTACAGA"


def row(contig, start, end, motif, ref_cn, alleles, depth=6, method="dist", ps=None, one_peak=False, failed=False):
    """alleles: the called copy numbers; reads: `depth` per allele around it (cn, cn, cn + 1, cn, cn - 1, cn ...)."""
    r = {"locus_index": start, "locus_id": f"{contig}_{start}", "contig": contig, "start": start, "end": end, "motif": motif,
         "ref_cn": ref_cn, "ref_start_anchor": ANCHOR, "ref_seq": motif * ref_cn, "reads": {}}
    if failed:
        r.update(call=None, call_95_cis=None, peaks=None)
        for i in range(depth):
            r["reads"][f"{contig}_{start}_r{i}"] = {"s": "+", "cn": ref_cn + i % 2, "w": 1.0, "sl": len(motif) * (ref_cn + i % 2)}
        return r
    wobble = (0, 0, 1, 0, -1, 0, 0, 1)
    for a, cn in enumerate(alleles):
        for i in range(depth):
            v = cn + wobble[i % len(wobble)]
            r["reads"][f"{contig}_{start}_a{a}_r{i}"] = {"s": "+-"[i % 2], "cn": v, "w": 1.0, "sl": len(motif) * v, "p": 0 if one_peak else a}
    calls = list(alleles)
    r.update(call=calls, call_95_cis=[[c - 1, c + 1] for c in calls], assign_method=method, mean_model_align_score=1.9,
             peaks={"means": [float(c) for c in (calls[:1] if one_peak else calls)], "weights": [1.0 / len(calls)] * (1 if one_peak else len(calls)),
                    "stdevs": [0.5] * (1 if one_peak else len(calls)), "modal_n": 1 if one_peak else len(calls),
                    "n_reads": [depth * len(calls)] if one_peak else [depth] * len(calls),
                    "seqs": [[motif * c, "single"] for c in calls], "start_anchor_seqs": [[ANCHOR, "single"] for _ in calls]})
    if ps is not None:
        r["ps"] = ps
    return r


def reports():
    child = [row("chr1", 1000, 1040, "CAG", 13, (12, 15), ps=1000), row("chr1", 2000, 2030, "AT", 15, (10, 15), depth=16),
             row("chr1", 3000, 3024, "GGC", 8, (8, 8), one_peak=True), row("chr1", 4000, 4020, "A", 20, (19, 21)),
             row("chr1", 5000, 5030, "TTA", 10, (10, 11)), row("chr2", 100, 160, "CA", 30, (28, 31)),
             row("chr2", 500, 548, "AAG", 16, (16, 18), method="snv", ps=500), row("chr2", 700, 730, "TG", 15, (14, 14), method="snv"),
             row("chrX", 900, 930, "CGG", 10, (10, 12))]
    mother = [row("chr1", 1000, 1040, "CAG", 13, (12, 13)), row("chr1", 2000, 2030, "AT", 15, (10, 11), depth=16),
              row("chr1", 3000, 3024, "GGC", 8, (8, 9)), row("chr1", 4000, 4020, "A", 20, (19, 20)),
              row("chr1", 5000, 5030, "TTA", 10, (), failed=True), row("chr2", 100, 160, "CA", 30, (28, 30)),
              row("chr2", 500, 548, "AAG", 16, (16, 17), method="snv", ps=480), row("chr2", 700, 730, "TG", 15, (14, 16)),
              row("chrX", 900, 930, "CGG", 10, (10, 11))]
    father = [row("chr1", 1000, 1040, "CAG", 13, (14, 15)), row("chr1", 2000, 2030, "AT", 15, (12, 13), depth=16),
              row("chr1", 3000, 3024, "GGC", 8, (7, 8)),
              row("chr1", 5000, 5030, "TTA", 10, (11, 12)), row("chr2", 100, 160, "CA", 30, (31,)),
              row("chr2", 500, 548, "AAG", 16, (18, 20), method="snv", ps=500), row("chr2", 700, 730, "TG", 15, (13, 14)),
              row("chrX", 900, 930, "CGG", 10, (12, 12))]
    out = {}
    for name, rows in (("child", child), ("mother", mother), ("father", father)):
        out[name] = {"sample_id": name, "caller": {"name": "strkit_amd"}, "parameters": {"n_alleles": 2},
                     "contigs": sorted({r["contig"] for r in rows}), "results": rows}
    return out


if __name__ == "__main__":
    d = os.path.join(ROOT, "tests", "golden", "mi")
    os.makedirs(d, exist_ok=True)
    for name, rep in reports().items():
        write_json(rep, os.path.join(d, name + ".json"))
        print(name, write_vcf(rep, os.path.join(d, name + ".vcf"), date="20261020"), "VCF records")
