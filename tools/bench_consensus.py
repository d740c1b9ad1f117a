"""Throughput of strk_best_representatives (k_best_rep) on the two shapes of the flagship configs.

usage: python tools/bench_consensus.py [--short-groups N] [--long-groups N] [--reps R]
(a) N groups of 15 HiFi-like reads of 40-80 bases (config 2's shape: one haplotype, 0.5 % errors, most reads identical);
(b) N groups of 20 reads of 6-12 kb with 1 % errors (config 5's shape: every read distinct).
Prints groups/s and DP cell updates/s by the device time (HIP events around the kernel) and by the wall time of the whole
library call.  Cells are those of the distinct pairs the kernel really aligns (|a| * |b| each); the count before duplicates
are collapsed, m (m - 1) / 2 pairs per group, is printed next to it.  Duplicate collapsing cannot be switched off.
"""
from __future__ import annotations

import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from strkit_amd import _lib  # noqa: E402
from strkit_amd._groups import pack_groups  # noqa: E402
from strkit_amd.consensus import best_representatives_packed  # noqa: E402

_A = np.frombuffer(b"ACGT", np.uint8)


def _read(rng, hap: np.ndarray, rate: float) -> np.ndarray:
    """hap with substitutions (half of the errors), deletions and insertions (a quarter each)."""
    x = rng.random(hap.shape[0])
    out = hap.copy()
    sub = x < rate / 2
    out[sub] = _A[rng.integers(0, 4, int(sub.sum()))]
    ins = np.flatnonzero((x >= rate / 2) & (x < rate * 3 / 4))
    out = np.delete(out, np.flatnonzero((x >= rate * 3 / 4) & (x < rate)))
    ins = ins[ins <= out.shape[0]]
    return np.insert(out, ins, _A[rng.integers(0, 4, ins.shape[0])])


def make_groups(n_groups: int, n_reads: int, lo: int, hi: int, rate: float, seed: int = 1):
    rng = np.random.default_rng(seed)
    groups = []
    for _ in range(n_groups):
        hap = _A[rng.integers(0, 4, int(rng.integers(lo, hi + 1)))]
        groups.append([_read(rng, hap, rate) for _ in range(n_reads)])
    # cells: all pairs, and the pairs of distinct strings
    all_cells = distinct_cells = 0
    for g in groups:
        ln = np.array([x.shape[0] for x in g], np.int64)
        all_cells += int((ln.sum() ** 2 - (ln ** 2).sum()) // 2)
        seen = {}
        for x in g:
            seen.setdefault(x.tobytes(), x.shape[0])
        u = np.array(list(seen.values()), np.int64)
        distinct_cells += int((u.sum() ** 2 - (u ** 2).sum()) // 2)
    return pack_groups(groups), all_cells, distinct_cells


def run(label: str, data, all_cells: int, distinct_cells: int, reps: int, ctx) -> None:
    off = data[0]
    n = off.shape[0] - 1
    dev, wall = [], []
    for _ in range(reps):
        t0 = time.perf_counter()
        out, st = best_representatives_packed(data[0], data[1], data[2], seqs=data[3], ctx=ctx, with_stats=True)
        wall.append(time.perf_counter() - t0)
        dev.append(st["kernel_ms"] / 1e3)
    print(f"{label}: {n} groups, cells {distinct_cells:.3e} (before collapsing {all_cells:.3e}) | device {min(dev) * 1e3:9.2f} ms = "
          f"{n / min(dev):12,.0f} groups/s, {distinct_cells / min(dev):.3e} cells/s | with host {min(wall) * 1e3:9.2f} ms = "
          f"{n / min(wall):12,.0f} groups/s | single {int((out['method'] == 1).sum())}, best_rep {int((out['method'] == 2).sum())}",
          flush=True)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--short-groups", type=int, default=20000)
    ap.add_argument("--long-groups", type=int, default=500)
    ap.add_argument("--reps", type=int, default=3)
    args = ap.parse_args()
    ctx = _lib.default_context(0)
    warm, _, _ = make_groups(64, 15, 40, 80, 0.005, seed=99)
    best_representatives_packed(warm[0], warm[1], warm[2], seqs=warm[3], ctx=ctx)
    if args.short_groups:
        run("(a) 15 reads of 40-80 bases", *make_groups(args.short_groups, 15, 40, 80, 0.005), args.reps, ctx)
    if args.long_groups:
        run("(b) 20 reads of 6-12 kb", *make_groups(args.long_groups, 20, 6000, 12000, 0.01), args.reps, ctx)


if __name__ == "__main__":
    main()
