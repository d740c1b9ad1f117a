"""Throughput of strk_call_alleles (k_alleles) on HiFi-shaped diploid loci: 30 reads each, B = 100 (defaults).

usage: python tools/bench_alleles.py [N_LOCI ...] [--reps R]
Prints, per size, loci/s by the device time (HIP events around the kernel) and by the wall time of the whole library
call (input checks, copies, launch, read-back).  Under rocprofv3, run it with a single size and --reps 1.
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


def make_loci(n_loci: int, n_reads: int = 30, seed: int = 1):
    rng = np.random.default_rng(seed)
    a1 = rng.integers(5, 80, n_loci)
    a2 = a1 + rng.integers(0, 20, n_loci)
    pick = rng.random((n_loci, n_reads)) < 0.5
    cn = np.where(pick, a1[:, None], a2[:, None]) + rng.choice([0, 0, 0, 0, 0, 0, 1, -1, 2, -2], (n_loci, n_reads))
    read_off = (np.arange(n_loci + 1) * n_reads).astype(np.int32)
    seeds = rng.integers(0, 1 << 63, n_loci, dtype=np.uint64)
    return read_off, cn.ravel().astype(np.int32), np.ones(n_loci * n_reads), np.full(n_loci, 2, np.int32), seeds


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("sizes", nargs="*", type=int, default=[10000, 170000])
    ap.add_argument("--reps", type=int, default=3)
    args = ap.parse_args()
    ctx = _lib.default_context(0)
    p = AlleleParams()
    warm = make_loci(256, seed=99)
    call_alleles_batch(*warm, p, ctx)
    for n in args.sizes:
        data = make_loci(n)
        dev, wall = [], []
        for _ in range(args.reps):
            t0 = time.perf_counter()
            out, st = call_alleles_batch(*data, p, ctx, with_stats=True)
            wall.append(time.perf_counter() - t0)
            dev.append(st["kernel_ms"] / 1e3)
        called = int((out["status"] == 0).sum())
        print(f"{n:>7} loci x 30 reads, B=100: device {min(dev) * 1e3:9.2f} ms = {n / min(dev):12,.0f} loci/s | "
              f"with host {min(wall) * 1e3:9.2f} ms = {n / min(wall):12,.0f} loci/s | called {called}, "
              f"modal_n=2 {int((out['modal_n'] == 2).sum())}", flush=True)


if __name__ == "__main__":
    main()
