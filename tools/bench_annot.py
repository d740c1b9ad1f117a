#!/usr/bin/env python
"""Times the annotation readers on a synthetic GFF3 of `--lines` feature lines on `--contigs` contigs, each with one
contig-long `region` as its first line (the habit of NCBI's files), against `--loci` catalog loci on the same contigs.  Records:
  (1) the per-contig walk on the device (IndexedAnnotations, front_end="device"): seconds for all loci, of which the HIP-event time
      of the inflation kernel and of the line / join / id kernels; the remainder is reading, upload, download and the Python strings;
  (2) the per-contig walk on the host, the library's threads held to `--threads` CPUs;
  (3) a loop of one index query plus parse per locus through the same host reader (IndexedAnnotations.locus_overlaps) over a
      sample of `--sample` loci, scaled to all loci.  THIS STANDS IN for the reference's per-locus TabixFile.fetch (loci.py:252):
      pysam is not available, so the reference itself is not measured.
The device's and the host's lists are checked against each other, and on a sample of loci against the per-locus loop, first.
Prints one JSON line, then the claims in words."""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from strkit_amd.frontend.annotations import IndexedAnnotations, annotate  # noqa: E402
from strkit_amd.frontend.synth_annot import index_annotations  # noqa: E402


def make_text(n_lines: int, contigs: int, length: int, seed: int = 1) -> bytes:
    rng = np.random.default_rng(seed)
    per = n_lines // contigs
    out = ["##gff-version 3"]
    kinds = ("gene", "mRNA", "exon", "CDS")
    for c in range(contigs):
        name = f"chr{c + 1}"
        out.append(f"{name}\tRefSeq\tregion\t1\t{length}\t.\t+\t.\tID={name}:1..{length};Dbxref=taxon:9606;Name={c + 1};gbkey=Src;genome=chromosome;mol_type=genomic DNA")
        starts = np.sort(rng.integers(1, length - 40000, size=per)).tolist()
        lens = (2 ** rng.uniform(4, 15, size=per)).astype(np.int64).tolist()
        for i, (s, w) in enumerate(zip(starts, lens)):
            k = i & 3
            attrs = (f"ID=gene-{c}.{i};Dbxref=GeneID:{100000 + i},HGNC:HGNC:{i};Name=G{i};gbkey=Gene;gene=G{i};gene_biotype=protein_coding",
                     f"ID=rna-{c}.{i};Parent=gene-{c}.{i - 1};Dbxref=GeneID:{100000 + i};Name=NM_{i}.1;gbkey=mRNA;gene=G{i};product=protein {i}",
                     f"Parent=rna-{c}.{i - 1};Dbxref=GeneID:{100000 + i};gbkey=mRNA;gene=G{i};product=protein {i};transcript_id=NM_{i}.1",
                     f"Parent=rna-{c}.{i - 2};Dbxref=GeneID:{100000 + i};gbkey=CDS;gene=G{i};product=protein {i};exon_id=E{c}.{i};protein_id=NP_{i}.1")[k]
            out.append(f"{name}\tRefSeq\t{kinds[k]}\t{s}\t{s + w}\t.\t+\t.\t{attrs}")
    return ("\n".join(out) + "\n").encode()


def walk(path, front_end, loci, piece_bytes):
    t0 = time.perf_counter()
    r = IndexedAnnotations(path, front_end=front_end, piece_bytes=piece_bytes)
    got = annotate(loci, r)
    dt = time.perf_counter() - t0
    out = {"seconds": round(dt, 4), "walks": r.n_queries, "compressed_mb": round(r.compressed_bytes / 1e6, 2), "text_mb": round(r.text_bytes / 1e6, 2),
           "ids": int(sum(map(len, got)))}
    if front_end == "device":
        out["inflate_kernel_ms"], out["gff_kernels_ms"] = round(r.kernel_ms[0], 3), round(r.kernel_ms[1], 3)
        out["other_ms"] = round(1e3 * dt - r.kernel_ms[0] - r.kernel_ms[1], 3)
        out["gff_kernels_text_gb_per_s"] = round(r.text_bytes / 1e9 / max(r.kernel_ms[1] / 1e3, 1e-9), 2)
    r.close()
    return out, got


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--lines", type=int, default=1_000_000)
    ap.add_argument("--contigs", type=int, default=4)
    ap.add_argument("--contig-length", type=int, default=200_000_000)
    ap.add_argument("--loci", type=int, default=100_000)
    ap.add_argument("--sample", type=int, default=40, help="loci of the per-locus loop")
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--piece-bytes", type=int, default=32 << 20)
    ap.add_argument("--front-ends", default="device,host")
    ap.add_argument("--dir", default=None)
    a = ap.parse_args()
    cpus = sorted(os.sched_getaffinity(0))[:a.threads]
    os.sched_setaffinity(0, cpus)                 # the library sizes its threads by the CPUs it may run on
    work = a.dir or tempfile.mkdtemp(prefix="bench_annot_")
    t0 = time.perf_counter()
    text = make_text(a.lines, a.contigs, a.contig_length)
    path = index_annotations(text, os.path.join(work, "genes.gff3.gz"))
    rng = np.random.default_rng(2)
    loci = []
    for c in range(a.contigs):
        s = np.sort(rng.integers(1000, a.contig_length - 50000, size=a.loci // a.contigs))
        loci += [(f"chr{c + 1}", int(x), int(x) + int(w)) for x, w in zip(s, rng.integers(10, 300, size=len(s)))]
    res = {"shape": {"lines": a.lines, "contigs": a.contigs, "loci": len(loci), "threads": len(cpus), "piece_bytes": a.piece_bytes, "text_mb": round(len(text) / 1e6, 1),
                     "bgzf_mb": round(os.path.getsize(path) / 1e6, 1)}, "make_files_s": round(time.perf_counter() - t0, 1)}
    del text
    lists = {}
    for fe in a.front_ends.split(","):
        walk(path, fe, loci[:64], a.piece_bytes)           # warm-up: the library, the device, the page cache
        runs = []
        for _ in range(a.repeats):
            one, lists[fe] = walk(path, fe, loci, a.piece_bytes)
            runs.append(one)
        s = [r["seconds"] for r in runs]
        res[f"walk_{fe}"] = {**runs[int(np.argsort(s)[len(s) // 2])], "seconds_all": s}
    fes = list(lists)
    assert all(lists[fe] == lists[fes[0]] for fe in fes), "the front ends disagree"
    # the per-locus loop, on a sample spread over the catalog
    pick = [int(i) for i in np.linspace(0, len(loci) - 1, a.sample)]
    r = IndexedAnnotations(path, front_end="host", piece_bytes=a.piece_bytes)
    t0 = time.perf_counter()
    single = [r.locus_overlaps(*loci[i]) for i in pick]
    dt = time.perf_counter() - t0
    assert single == [lists[fes[0]][i] for i in pick], "the per-locus loop disagrees with the walk"
    res["per_locus_loop_host"] = {"sample": len(pick), "seconds_sample": round(dt, 3), "per_locus_ms": round(1e3 * dt / len(pick), 2),
                                  "text_mb_per_locus": round(r.text_bytes / 1e6 / len(pick), 2), "seconds_scaled_to_all_loci": round(dt / len(pick) * len(loci), 1)}
    print(json.dumps(res))
    loop = res["per_locus_loop_host"]["seconds_scaled_to_all_loci"]
    for fe in fes:
        w = res[f"walk_{fe}"]
        print(f"per-contig walk, {fe}: {w['seconds_all']} s for {len(loci)} loci ({w['ids']} ids, {w['text_mb']} MB of text in {w['walks']} walks); the per-locus loop "
              f"(stand-in for the reference's per-locus fetch; {loop} s scaled from {len(pick)} loci) takes {loop / w['seconds']:.0f} times as long")


if __name__ == "__main__":
    main()
