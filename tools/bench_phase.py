"""Throughput of strk_call_alleles_phased on HiFi-shaped diploid loci of 30 reads (B = 100, defaults), against
strk_call_alleles on the same loci in the same session.

usage: python tools/bench_phase.py [N_LOCI ...] [--reps R] [--only tagged|snv]
Two workloads per size: every read haplotagged (one phase set, HP by haplotype), and untagged reads that carry 4 SNVs with
2 % base errors.  Prints, per workload, loci/s by the device time (HIP events around the four kernels) and by the wall time
of the whole library call (input checks, copies, launches, read-back), and the same for strk_call_alleles (the yardstick).
Last, 64 loci of 1 024 reads x 64 SNVs (the limits of the call): what the serial and quadratic stretches of k_phase_group and
k_phase_finish cost where they are largest.  Under rocprofv3, run it with a single size, --reps 1 and --only.
"""
from __future__ import annotations

import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from strkit_amd import _lib  # noqa: E402
from strkit_amd.alleles import AlleleParams, call_alleles_batch  # noqa: E402
from strkit_amd.phasing import call_alleles_phased_batch  # noqa: E402

N_READS, N_SNVS = 30, 4


def make_loci(n_loci: int, seed: int = 1, N_READS: int = N_READS, N_SNVS: int = N_SNVS):
    rng = np.random.default_rng(seed)
    a1 = rng.integers(5, 80, n_loci)
    a2 = a1 + rng.integers(1, 20, n_loci)
    hap = rng.random((n_loci, N_READS)) < 0.5
    cn = np.where(hap, a2[:, None], a1[:, None]) + rng.choice([0, 0, 0, 0, 0, 0, 1, -1, 2, -2], (n_loci, N_READS))
    read_off = (np.arange(n_loci + 1) * N_READS).astype(np.int32)
    seeds = rng.integers(0, 1 << 63, n_loci, dtype=np.uint64)
    base_args = (read_off, cn.ravel().astype(np.int32), np.ones(n_loci * N_READS), np.full(n_loci, 2, np.int32), seeds)
    hp = (1 + hap).astype(np.int32).ravel()
    ps = np.repeat(np.arange(n_loci, dtype=np.int32), N_READS)
    acgt = np.frombuffer(b"ACGT", np.uint8)
    ref = rng.integers(0, 4, (n_loci, 1, N_SNVS))
    alt = (ref + rng.integers(1, 4, (n_loci, 1, N_SNVS))) % 4
    cell = np.where(hap[:, :, None], alt, ref)
    err = rng.random(cell.shape) < 0.02
    cell = np.where(err, rng.integers(0, 4, cell.shape), cell)
    snv = dict(snv_off=(np.arange(n_loci + 1) * N_SNVS).astype(np.int32), snv_base=acgt[cell].ravel(),
               snv_qual=np.full(cell.size, 40, np.uint8))
    return base_args, dict(hp=hp, ps=ps), snv


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("sizes", nargs="*", type=int, default=[10000, 170000])
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--only", choices=["tagged", "snv", "large"])
    args = ap.parse_args()
    ctx = _lib.default_context(0)
    p = AlleleParams()
    wb, wt, ws = make_loci(256, seed=99)
    call_alleles_batch(*wb, p, ctx)
    call_alleles_phased_batch(*wb, **wt, fallback=False, ctx=ctx)
    call_alleles_phased_batch(*wb, **ws, fallback=False, ctx=ctx)

    def timed(fn):
        dev, wall, out = [], [], None
        for _ in range(args.reps):
            t0 = time.perf_counter()
            out, st = fn()
            wall.append(time.perf_counter() - t0)
            dev.append(st["kernel_ms"] / 1e3)
        return min(dev), min(wall), out

    if args.only in (None, "large"):
        n = 64
        base, tags, snvs = make_loci(n, seed=5, N_READS=1024, N_SNVS=64)
        for name, kw in (("phased, tagged", tags), ("phased, 64 SNVs", snvs)):
            dev, wall, out = timed(lambda: call_alleles_phased_batch(*base, **kw, fallback=False, ctx=ctx, with_stats=True))
            print(f"{n:>7} loci x 1024 reads, B=100, {name:<18}: device {dev * 1e3:9.2f} ms = {dev / n * 1e3:8.3f} ms per locus | "
                  f"with host {wall * 1e3:9.2f} ms | methods none/hp/snv/snv+dist {np.bincount(out['method'], minlength=4).tolist()}", flush=True)
    for n in ([] if args.only == "large" else args.sizes):
        base, tags, snvs = make_loci(n)
        rows = []
        if args.only != "snv":
            rows.append(("phased, tagged", lambda: call_alleles_phased_batch(*base, **tags, fallback=False, ctx=ctx, with_stats=True)))
        if args.only != "tagged":
            rows.append(("phased, 4 SNVs", lambda: call_alleles_phased_batch(*base, **snvs, fallback=False, ctx=ctx, with_stats=True)))
        rows.append(("strk_call_alleles", lambda: call_alleles_batch(*base, p, ctx, with_stats=True)))
        for name, fn in rows:
            dev, wall, out = timed(fn)
            note = f"called {int((out['status'] == 0).sum())}"
            if "method" in out:
                note += f", methods none/hp/snv/snv+dist {np.bincount(out['method'], minlength=4).tolist()}"
            print(f"{n:>7} loci x {N_READS} reads, B=100, {name:<18}: device {dev * 1e3:9.2f} ms = {n / dev:12,.0f} loci/s | "
                  f"with host {wall * 1e3:9.2f} ms = {n / wall:12,.0f} loci/s | {note}", flush=True)


if __name__ == "__main__":
    main()
