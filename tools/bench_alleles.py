"""Throughput of strk_call_alleles (k_alleles = k_alleles_w<2>) on HiFi-shaped diploid loci: 30 reads each, B = 100
(defaults), and of strk_call_alleles_n (k_alleles_n = k_alleles_w<6>, the same kernel template) on loci of `--n-alleles` alleles.

usage: python tools/bench_alleles.py [N_LOCI ...] [--reps R] [--n-alleles A] [--entry two|n]
`--n-alleles A`: loci with A alleles (neighbours 5 to 19 apart), called with n_alleles = A; above 2 through strk_call_alleles_n.
`--entry n`: strk_call_alleles_n also for A <= 2 (the same results as strk_call_alleles; what the wider kernel costs).
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
from strkit_amd.alleles import AlleleParams, call_alleles_batch, call_alleles_n_batch  # noqa: E402


def make_loci(n_loci: int, n_reads: int = 30, seed: int = 1):
    rng = np.random.default_rng(seed)
    a1 = rng.integers(5, 80, n_loci)
    a2 = a1 + rng.integers(0, 20, n_loci)
    pick = rng.random((n_loci, n_reads)) < 0.5
    cn = np.where(pick, a1[:, None], a2[:, None]) + rng.choice([0, 0, 0, 0, 0, 0, 1, -1, 2, -2], (n_loci, n_reads))
    read_off = (np.arange(n_loci + 1) * n_reads).astype(np.int32)
    seeds = rng.integers(0, 1 << 63, n_loci, dtype=np.uint64)
    return read_off, cn.ravel().astype(np.int32), np.ones(n_loci * n_reads), np.full(n_loci, 2, np.int32), seeds


def make_loci_n(n_loci: int, n_alleles: int, n_reads: int = 30, seed: int = 1):
    """As make_loci with n_alleles alleles per locus, every read from one of them at random."""
    rng = np.random.default_rng(seed)
    alleles = rng.integers(5, 80, (n_loci, 1)) + np.cumsum(rng.integers(5, 20, (n_loci, n_alleles)), axis=1)
    cn = np.take_along_axis(alleles, rng.integers(0, n_alleles, (n_loci, n_reads)), axis=1)
    cn = cn + rng.choice([0, 0, 0, 0, 0, 0, 1, -1, 2, -2], (n_loci, n_reads))
    read_off = (np.arange(n_loci + 1) * n_reads).astype(np.int32)
    seeds = rng.integers(0, 1 << 63, n_loci, dtype=np.uint64)
    return read_off, cn.ravel().astype(np.int32), np.ones(n_loci * n_reads), np.full(n_loci, n_alleles, np.int32), seeds


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("sizes", nargs="*", type=int, default=[10000, 170000])
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--n-alleles", type=int, default=None, choices=range(1, 7))
    ap.add_argument("--entry", choices=("two", "n"), default=None)
    args = ap.parse_args()
    ctx = _lib.default_context(0)
    p = AlleleParams()
    make = make_loci if args.n_alleles is None else (lambda n, seed=1: make_loci_n(n, args.n_alleles, seed=seed))
    wide = (args.entry or ("n" if (args.n_alleles or 2) > 2 else "two")) == "n"
    if (args.n_alleles or 2) > 2 and not wide:
        ap.error("--entry two takes at most 2 alleles")
    call_alleles_batch = globals()["call_alleles_n_batch" if wide else "call_alleles_batch"]
    print(f"strk_call_alleles{'_n' if wide else ''}, loci of {args.n_alleles or 2} alleles", flush=True)
    warm = make(256, seed=99)
    call_alleles_batch(*warm, p, ctx)
    for n in args.sizes:
        data = make(n)
        dev, wall = [], []
        for _ in range(args.reps):
            t0 = time.perf_counter()
            out, st = call_alleles_batch(*data, p, ctx, with_stats=True)
            wall.append(time.perf_counter() - t0)
            dev.append(st["kernel_ms"] / 1e3)
        called = int((out["status"] == 0).sum())
        print(f"{n:>7} loci x 30 reads, B=100: device {min(dev) * 1e3:9.2f} ms = {n / min(dev):12,.0f} loci/s | "
              f"with host {min(wall) * 1e3:9.2f} ms = {n / min(wall):12,.0f} loci/s | called {called}, "
              f"modal_n={args.n_alleles or 2} {int((out['modal_n'] == (args.n_alleles or 2)).sum())}", flush=True)


if __name__ == "__main__":
    main()
