"""Throughput of strk_count_kmers (k_kmers_hash, k_kmers_sort) on the shapes the front end and long-read catalogs give it.

usage: python tools/bench_kmers.py [--scale F] [--reps R] [--cpu-windows N]
(a) 300 000 singleton groups of HiFi-like tracts of 30-300 bases, k 3-6 (count_kmers="read" on a 10 000-locus x 30x file);
(b) 20 000 groups of 15 such reads (the peak groups of the same file);
(c) 500 groups of 20 reads of 6-12 kb, HiFi-like, k 1-6;
(d) the same with ONT-like noise and k = 20: nearly every window is distinct, the on-chip table spills;
(e) 2 000 groups of 15 tracts of 100-300 bases with k = 40: windows that do not pack into 64 bits (the general path).
--scale multiplies the group counts.  Per case: windows, entries written, groups that spilled / took the general path, device
time (HIP events around the kernels) and windows/s by it, wall time of the whole library call; and, for comparison only, the
rate of the CPU restatement (tests/kmers_restatement.py, one core) on the first groups of the same input (--cpu-windows).
"""
from __future__ import annotations

import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import kmers_restatement as R  # noqa: E402
from strkit_amd import _lib  # noqa: E402
from strkit_amd._groups import pack_groups  # noqa: E402
from strkit_amd.kmers import count_kmers_packed  # noqa: E402

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


def make_groups(n_groups: int, n_reads: int, lo: int, hi: int, rate: float, k_lo: int, k_hi: int, motif_len=None, seed: int = 1):
    """Groups of n_reads reads of one tract (a random motif of k bases, or of motif_len, repeated to lo..hi bases) each."""
    rng = np.random.default_rng(seed)
    groups = []
    ks = rng.integers(k_lo, k_hi + 1, n_groups).astype(np.int32)
    for g in range(n_groups):
        m = int(motif_len or ks[g])
        length = int(rng.integers(lo, hi + 1))
        hap = np.tile(_A[rng.integers(0, 4, m)], length // m + 1)[:length]
        groups.append([_read(rng, hap, rate) for _ in range(n_reads)])
    off, starts, lens, buf = pack_groups(groups)
    return off, starts, lens, ks, buf


def run(label: str, data, reps: int, cpu_windows: int, ctx) -> None:
    off, starts, lens, ks, buf = data
    n = off.shape[0] - 1
    windows = int(np.maximum(lens.astype(np.int64) - np.repeat(ks, np.diff(off)) + 1, 0).sum())
    dev, wall = [], []
    for _ in range(reps):
        t0 = time.perf_counter()
        out, st = count_kmers_packed(off, starts, lens, ks, seqs=buf, ctx=ctx, with_stats=True)
        wall.append(time.perf_counter() - t0)
        dev.append(st["kernel_ms"] / 1e3)
    # the restatement on the first groups, up to cpu_windows windows
    per_group = np.add.reduceat(np.maximum(lens.astype(np.int64) - np.repeat(ks, np.diff(off)) + 1, 0), off[:-1])
    n_cpu = max(1, int(np.searchsorted(np.cumsum(per_group), cpu_windows)))
    text = buf.tobytes()
    t0 = time.perf_counter()
    eo, pos, cnt = R.count_packed(off[:n_cpu + 1], starts, lens, ks, text)
    t_cpu = time.perf_counter() - t0
    e_cpu = int(out["entry_off"][n_cpu])
    same = eo == out["entry_off"][:n_cpu + 1].tolist() and pos == out["pos"][:e_cpu].tolist() and cnt == out["count"][:e_cpu].tolist()
    w_cpu = int(per_group[:n_cpu].sum())
    print(f"{label}: {n} groups, {windows:.3e} windows, {out['pos'].shape[0]} entries, spilled {st['n_fallback']}, general "
          f"{st['n_miss_reads']}, launches {st['n_dp_launches']} | device {min(dev) * 1e3:9.2f} ms = {windows / min(dev):.3e} windows/s | "
          f"with host {min(wall) * 1e3:9.2f} ms = {windows / min(wall):.3e} windows/s | restatement, one core, first {n_cpu} groups: "
          f"{w_cpu / t_cpu:.3e} windows/s ({'equal' if same else 'DIFFERENT'})", flush=True)
    if not same:
        sys.exit(1)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--cpu-windows", type=int, default=2_000_000)
    args = ap.parse_args()
    ctx = _lib.default_context(0)
    warm = make_groups(64, 15, 30, 300, 0.002, 3, 6, seed=99)
    count_kmers_packed(*warm[:4], seqs=warm[4], ctx=ctx)
    n = lambda x: max(1, int(x * args.scale))      # noqa: E731
    run("(a) singletons of 30-300 bases, k 3-6", make_groups(n(300000), 1, 30, 300, 0.002, 3, 6), args.reps, args.cpu_windows, ctx)
    run("(b) 15 reads of 30-300 bases, k 3-6", make_groups(n(20000), 15, 30, 300, 0.002, 3, 6, seed=2), args.reps, args.cpu_windows, ctx)
    run("(c) 20 reads of 6-12 kb, k 1-6", make_groups(n(500), 20, 6000, 12000, 0.002, 1, 6, seed=3), args.reps, args.cpu_windows, ctx)
    run("(d) 20 noisy reads of 6-12 kb, k 20", make_groups(n(500), 20, 6000, 12000, 0.08, 20, 20, motif_len=6, seed=4), args.reps,
        args.cpu_windows, ctx)
    run("(e) 15 reads of 100-300 bases, k 40", make_groups(n(2000), 15, 100, 300, 0.002, 40, 40, motif_len=5, seed=5), args.reps,
        args.cpu_windows, ctx)


if __name__ == "__main__":
    main()
