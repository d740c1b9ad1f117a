"""Throughput of strk_consensus (k_poa) on the shapes of tools/bench_consensus.py and on an ONT-like one.

usage: python tools/bench_poa.py [--short-groups N] [--long-groups N] [--ont-groups N] [--reps R] [--check K]
(a) N groups of 15 HiFi-like reads of 40-80 bases (0.5 % errors, most reads identical);
(b) N groups of 20 reads of 6-12 kb with 1 % errors: their median length is above max_mdn_poa_length = 5000, so every one of
    them takes the best-representative path (what the front end's call does with such alleles);
(c) N groups of 15 reads of 40-300 bases with 6 % errors (ONT-like: every read distinct).
Prints groups/s and DP cells/s by the device time (HIP events around every kernel of the call, stats.kernel_ms) and by the
wall time of the whole library call, the methods chosen, and the CPU restatement's one-core rate on the first K groups of
the same input, whose answers must equal the library's.  A DP cell is one (graph node, string byte) pair of an alignment.
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
sys.path.insert(0, os.path.join(ROOT, "tools"))

import poa_restatement as P  # noqa: E402
from bench_consensus import make_groups  # noqa: E402
from strkit_amd import _lib  # noqa: E402
from strkit_amd.consensus import METHOD_NAMES, consensus_packed  # noqa: E402


def run(label: str, data, reps: int, check: int, ctx) -> None:
    off, starts, lens, buf = data
    n = off.shape[0] - 1
    dev, wall = [], []
    for _ in range(reps):
        t0 = time.perf_counter()
        out, st = consensus_packed(off, starts, lens, seqs=buf, ctx=ctx, with_stats=True)
        wall.append(time.perf_counter() - t0)
        dev.append(st["kernel_ms"] / 1e3)
    methods = ", ".join(f"{METHOD_NAMES[m]} {int((out['method'] == m).sum())}" for m in range(4) if (out["method"] == m).any())
    print(f"{label}: {n} groups, {st['dp_cells']:.3e} DP cells, {st['n_sub_batches']} POA launches | device {min(dev) * 1e3:9.2f} ms = "
          f"{n / min(dev):12,.0f} groups/s, {st['dp_cells'] / min(dev):.3e} cells/s | with host {min(wall) * 1e3:9.2f} ms = "
          f"{n / min(wall):12,.0f} groups/s | {methods}, fallback {st['n_fallback']}", flush=True)
    k = min(check, n)
    if k:
        text = buf.tobytes()
        t0 = time.perf_counter()
        cells = 0
        for g in range(k):
            group = [text[int(starts[i]):int(starts[i]) + int(lens[i])] for i in range(int(off[g]), int(off[g + 1]))]
            idx, method, seq, _lim = P.consensus(group)
            got = out["seqs"][int(out["seq_off"][g]):int(out["seq_off"][g + 1])].tobytes()
            assert (idx, method, seq or b"") == (int(out["index"][g]), METHOD_NAMES[int(out["method"][g])], got), (label, g)
            if method == "poa":
                cells += P.build(group).cells
        dt = time.perf_counter() - t0
        print(f"    restatement, one core, first {k} groups (answers equal): {k / dt:10,.2f} groups/s, {cells / dt:.3e} cells/s "
              f"(both passes over a poa group counted in the time, one in the cells)", flush=True)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--short-groups", type=int, default=20000)
    ap.add_argument("--long-groups", type=int, default=500)
    ap.add_argument("--ont-groups", type=int, default=5000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--check", type=int, default=20)
    args = ap.parse_args()
    ctx = _lib.default_context(0)
    warm = make_groups(64, 15, 40, 80, 0.005, seed=99)[0]
    consensus_packed(warm[0], warm[1], warm[2], seqs=warm[3], ctx=ctx)
    if args.short_groups:
        run("(a) 15 reads of 40-80 bases, 0.5 %", make_groups(args.short_groups, 15, 40, 80, 0.005)[0], args.reps, args.check, ctx)
    if args.long_groups:
        run("(b) 20 reads of 6-12 kb, 1 %", make_groups(args.long_groups, 20, 6000, 12000, 0.01)[0], args.reps, min(args.check, 2), ctx)
    if args.ont_groups:
        run("(c) 15 reads of 40-300 bases, 6 %", make_groups(args.ont_groups, 15, 40, 300, 0.06, seed=3)[0], args.reps, args.check, ctx)


if __name__ == "__main__":
    main()
