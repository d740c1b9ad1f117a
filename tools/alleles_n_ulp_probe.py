#!/usr/bin/env python
"""How far the allele-calling restatement moves when exp / log / sqrt move by one ulp (CPU only).

tests/test_gpu_alleles_n.py holds the device to tests/alleles_n_restatement.py on a seeded corpus and allows 1 % of the
loci to part for that reason.  This script runs the restatement against itself, with the three functions answering one ulp
up, down or exactly at random, through that test's own comparison, and prints the loci that part: a corpus seed whose
count stays within the cap here is one the device can be expected to meet.

    python tools/alleles_n_ulp_probe.py [--corpus-seed S] [--perturbations 5]
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import alleles_n_restatement as N   # noqa: E402
import alleles_restatement as R   # noqa: E402
import test_gpu_alleles_n as T   # noqa: E402


class OneUlpNumpy:
    """numpy, except that exp, log and sqrt answer one ulp off at random."""

    def __init__(self, seed):
        self._rng = np.random.default_rng(seed)

    def __getattr__(self, name):
        f = getattr(np, name)
        if name not in ("exp", "log", "sqrt"):
            return f

        def moved(x, *a, **k):
            y = np.asarray(f(x, *a, **k), dtype=np.float64)
            step = self._rng.integers(-1, 2, y.shape)
            out = np.where(step == 0, y, np.nextafter(y, np.where(step > 0, np.inf, -np.inf)))
            return out if out.shape else float(out)
        return moved


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--corpus-seed", type=int, default=T.CORPUS_SEED)
    ap.add_argument("--perturbations", type=int, default=5)
    args = ap.parse_args()
    groups = T.corpus(args.corpus_seed)
    exact = T.expected(args.corpus_seed)
    worst = worst_broken = 0
    for ps in range(args.perturbations):
        R.np = N.np = OneUlpNumpy(ps)
        try:
            moved = [[N.call_locus_n(cn, w, A, int(s), p) for (cn, w, A), s in zip(loci, seeds)] for p, loci, seeds in groups]
        finally:
            R.np = N.np = np

        def got_of(gi, p, loci, seeds):
            rows = moved[gi]
            read_off = np.concatenate([[0], np.cumsum([c.shape[0] for c, _, _ in loci])])
            got = {k: np.array([r[k] for r in rows]) for k in rows[0] if k not in ("read_peak", "median_tie", "median_cands")}
            got["read_peak"] = np.concatenate([r["read_peak"] for r in rows])
            return read_off, got
        checked, exempt, tied, resolved, drift, broken = T.compare(groups, exact, got_of)
        print(f"perturbation {ps}: {checked} loci, {exempt} exempt at a half-point, {tied} tied at the median ({resolved} resolved), "
              f"{len(drift)} parted: {[d[:2] for d in drift]}; of these {len(broken)} beyond calls within 1 and equal status: {broken}")
        worst, worst_broken = max(worst, len(drift)), max(worst_broken, len(broken))
    print(f"corpus seed {args.corpus_seed}: at most {worst} loci part (the cap is {T.MAX_DRIFT_FRACTION * checked:.1f}), "
          f"at most {worst_broken} beyond calls within 1 and equal status (none may)")


if __name__ == "__main__":
    main()
