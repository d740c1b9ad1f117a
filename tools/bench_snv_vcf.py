#!/usr/bin/env python
"""Times the candidate-SNV readers on a dbSNP-like file (frontend/synth_snvs.make_dbsnp_like: single-base records
with INFO fields of 100 - 400 bytes, a share of indels and multi-allelic lines) and on a file of 8x its records, the extra ones
behind every window.  The windows are those of a panel of `--loci` loci `--spacing` bases apart with reads of `--read-len`
bases: one query per locus over [start - read_len, start + read_len), the per-block query of a run whose blocks hold one locus
(loci more than 20 kb apart are blocks of their own, loci.py).  Records:
  (1) read_snv_vcf on both files, each in a process of its own: seconds and peak resident memory (the parent commit's path);
  (2) IndexedSnvVcf, device and host, `--repeats` times on each file: open + all queries (what a run reports as
      snv_candidates_s), seconds per query, compressed bytes read, on the device the HIP-event time of the inflation kernel and of
      the VCF kernels and the decompressed bytes per second of the latter.
The device's and the host's windows are checked against read_snv_vcf's first.  Prints one JSON line, then the claims in words."""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from strkit_amd.frontend.snv_vcf import IndexedSnvVcf, read_snv_vcf  # noqa: E402
from strkit_amd.frontend.synth_snvs import index_snv_vcf, make_dbsnp_like  # noqa: E402

WHOLE_FILE = """
import resource, sys, time
sys.path.insert(0, %r)
from strkit_amd.frontend.snv_vcf import read_snv_vcf
t0 = time.perf_counter()
c = read_snv_vcf(sys.argv[1])
print(time.perf_counter() - t0, resource.getrusage(resource.RUSAGE_SELF).ru_maxrss / 1024.0, sum(len(v.pos) for v in c.by_contig.values()))
"""


def whole_file(path: str) -> dict:
    out = subprocess.run([sys.executable, "-c", WHOLE_FILE % ROOT, path], check=True, capture_output=True, text=True).stdout.split()
    return {"seconds": round(float(out[0]), 3), "peak_rss_mb": round(float(out[1]), 1), "records_kept": int(out[2])}


def indexed(path: str, front_end: str, windows, piece_bytes: int) -> tuple[dict, list]:
    t0 = time.perf_counter()
    r = IndexedSnvVcf(path, front_end=front_end, piece_bytes=piece_bytes)
    got = [r.window("chr1", a, b) for a, b in windows]
    dt = time.perf_counter() - t0
    out = {"snv_candidates_s": round(dt, 4), "per_query_ms": round(1e3 * r.seconds / max(1, r.n_queries), 4), "queries": r.n_queries,
           "compressed_mb": round(r.compressed_bytes / 1e6, 3), "text_mb": round(r.text_bytes / 1e6, 3), "records": int(sum(len(g.pos) for g in got))}
    if front_end == "device":
        out["inflate_kernel_ms"], out["vcf_kernels_ms"] = round(r.kernel_ms[0], 3), round(r.kernel_ms[1], 3)
        out["vcf_kernels_text_gb_per_s"] = round(r.text_bytes / 1e9 / max(r.kernel_ms[1] / 1e3, 1e-9), 2)
    r.close()
    return out, got


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--loci", type=int, default=500)
    ap.add_argument("--spacing", type=int, default=20000)
    ap.add_argument("--read-len", type=int, default=1500)
    ap.add_argument("--step", type=int, default=100, help="mean distance of two records")
    ap.add_argument("--times", type=int, default=8, help="records of the larger file, in multiples of the smaller one's")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--piece-bytes", type=int, default=32 << 20)
    ap.add_argument("--front-ends", default="device,host")
    ap.add_argument("--dir", default=None)
    a = ap.parse_args()
    work = a.dir or tempfile.mkdtemp(prefix="bench_snv_vcf_")
    span = (a.loci + 1) * a.spacing
    n1 = span // a.step
    windows = [(a.spacing * (l + 1) - a.read_len, a.spacing * (l + 1) + a.read_len) for l in range(a.loci)]
    t0 = time.perf_counter()
    files = {}
    plain = os.path.join(work, "snvs_1x.vcf")
    text = make_dbsnp_like(plain, n1, first=1, step=a.step)
    files["1x"] = (plain, index_snv_vcf(plain), n1)
    # the larger file: the same records, then (times - 1) x as many behind the last window
    last = int(text[text.rstrip(b"\n").rindex(b"\n") + 1:].split(b"\t")[1])
    more = make_dbsnp_like(os.path.join(work, "more.vcf"), n1 * (a.times - 1), first=max(last, windows[-1][1]) + 1000, step=a.step, seed=2)
    plain = os.path.join(work, f"snvs_{a.times}x.vcf")
    with open(plain, "wb") as fh:
        fh.write(text + b"".join(ln + b"\n" for ln in more.split(b"\n") if ln and ln[:1] != b"#"))
    os.remove(os.path.join(work, "more.vcf"))
    files[f"{a.times}x"] = (plain, index_snv_vcf(plain), n1 * a.times)
    res = {"shape": {"loci": a.loci, "spacing": a.spacing, "read_len": a.read_len, "records_1x": n1, "times": a.times, "piece_bytes": a.piece_bytes,
                     "plain_mb": {k: round(os.path.getsize(v[0]) / 1e6, 1) for k, v in files.items()},
                     "bgzf_mb": {k: round(os.path.getsize(v[1]) / 1e6, 1) for k, v in files.items()}}, "make_files_s": round(time.perf_counter() - t0, 1)}
    res["read_snv_vcf"] = {k: whole_file(v[1]) for k, v in files.items()}
    oracle = read_snv_vcf(files["1x"][0]).contig("chr1")
    want = [oracle.pos[(oracle.pos >= lo) & (oracle.pos < hi)] for lo, hi in windows]
    for fe in a.front_ends.split(","):
        indexed(files["1x"][1], fe, windows[:4], a.piece_bytes)         # warm-up: the library, the device, the page cache
        for label, (_plain, gz, _n) in files.items():
            runs = []
            for _ in range(a.repeats):
                one, got = indexed(gz, fe, windows, a.piece_bytes)
                assert all(np.array_equal(g.pos, w) for g, w in zip(got, want)), (fe, label)
                runs.append(one)
            s = [r["snv_candidates_s"] for r in runs]
            res[f"indexed_{fe}_{label}"] = {**runs[int(np.argsort(s)[len(s) // 2])], "snv_candidates_s_all": s, "spread_s": round(max(s) - min(s), 4)}
    print(json.dumps(res))
    big = f"{a.times}x"
    w1, w8 = res["read_snv_vcf"]["1x"], res["read_snv_vcf"][big]
    print(f"read_snv_vcf: 1x {w1['seconds']} s, {w1['peak_rss_mb']} MB; {big} {w8['seconds']} s, {w8['peak_rss_mb']} MB (x {w8['seconds'] / w1['seconds']:.1f})")
    for fe in a.front_ends.split(","):
        r1, r8 = res[f"indexed_{fe}_1x"], res[f"indexed_{fe}_{big}"]
        lo, hi = min(r1["snv_candidates_s_all"]), max(r1["snv_candidates_s_all"])
        inside = lo - r1["spread_s"] <= r8["snv_candidates_s"] <= hi + r1["spread_s"]
        print(f"indexed, {fe}: 1x {r1['snv_candidates_s_all']} s (spread {r1['spread_s']} s), {big} {r8['snv_candidates_s_all']} s: "
              f"{'within' if inside else 'OUTSIDE'} the 1x runs' range widened by their spread; "
              f"against read_snv_vcf on the 1x file: {w1['seconds'] / r1['snv_candidates_s']:.1f} times faster")


if __name__ == "__main__":
    main()
