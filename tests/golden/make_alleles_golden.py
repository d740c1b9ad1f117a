#!/usr/bin/env python3
"""Writes tests/golden/alleles_parent.npz: fixed inputs of the three allele entry points (strk_call_alleles,
strk_call_alleles_n, strk_call_alleles_phased) and every output array that the library returned for them, at 100 and 300
bootstraps.  tests/test_gpu_alleles_golden.py holds later builds to these bytes.  Needs the GPU:
    python tests/golden/make_alleles_golden.py [DIR]      (writes DIR/alleles_parent.npz, DIR = out/golden by default; copy from there)
The file in the tree was recorded with the commit before the two allele kernels became one; record it anew only with a build
whose results are meant to become the new reference.  These are outputs of THIS backend, not STRkit outputs."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

BOOTSTRAPS = (100, 300)   # at 300 a lane of the 256-lane block owns more than one bootstrap
KINDS = 7                 # x 6 values of n_alleles: 210 loci carry every pair five times
INPUT_KEYS = ("read_off", "cns", "weights", "seeds")
PHASE_KEYS = ("read_off", "cns", "weights", "n_alleles", "seeds", "hp", "ps", "snv_off", "snv_base", "snv_qual")


def _locus(rng, kind: int):
    """Copy numbers of one locus (5..60)."""
    if kind == 0:    # two alleles, 0 to 40 reads
        n = int(rng.integers(0, 41))
        a, b = rng.integers(8, 58, 2)
        return np.where(rng.random(n) < 0.5, a, b) + rng.choice([0, 0, 0, 1, -1, 2, -2], n)
    if kind == 1:    # one allele
        n = int(rng.integers(4, 41))
        return int(rng.integers(7, 58)) + rng.choice([0, 0, 0, 1, -1, 2, -2], n)
    if kind == 2:    # below min_reads
        return rng.integers(5, 61, int(rng.integers(0, 4)))
    if kind == 3:    # one distinct value
        return np.full(int(rng.integers(4, 31)), int(rng.integers(5, 61)))
    if kind == 4:    # two distinct values
        n = int(rng.integers(4, 31))
        cn = rng.choice(rng.choice(np.arange(5, 61), 2, replace=False), n)
        cn[:2] = cn.min(), cn.max()
        return cn
    if kind == 5:    # 4 or 5 reads of more than one value: fewer than n_alleles = 5 or 6
        n = int(rng.integers(4, 6))
        return rng.choice(np.arange(5, 61), n, replace=False)
    n = int(rng.integers(20, 41))   # three to six alleles
    centres = 5 + np.cumsum(rng.integers(3, 10, int(rng.integers(3, 7))))
    return centres[rng.integers(0, centres.shape[0], n)] + rng.choice([0, 0, 0, 1, -1], n)


def make_inputs(seed: int = 20261020) -> dict:
    """The plain inputs (211 loci: 210 small ones and one of 300 reads; n_alleles comes with the entry point) and a handful
    of phased loci of tests/phase_cases.py, as `phase_*`."""
    import phase_cases as PC
    rng = np.random.default_rng(seed)
    cns = [np.clip(_locus(rng, l % KINDS), 5, 60).astype(np.int32) for l in range(KINDS * 6 * 5)]
    cns.append((np.where(rng.random(300) < 0.45, 21, 47) + rng.integers(-2, 3, 300)).astype(np.int32))
    n = sum(c.shape[0] for c in cns)
    inp = dict(read_off=np.concatenate(([0], np.cumsum([c.shape[0] for c in cns]))).astype(np.int32), cns=np.concatenate(cns),
               weights=np.where(rng.random(n) < 0.5, 1.0, rng.uniform(0.2, 2.0, n)),
               seeds=rng.integers(0, 1 << 63, len(cns), dtype=np.uint64))
    loci = [PC.make_locus(rng, size, 4 if i % 4 else 0, 1 if i % 5 == 3 else 2, PC.TAG_KINDS[i % len(PC.TAG_KINDS)],
                          PC.CELL_KINDS[i % len(PC.CELL_KINDS)])
            for i, size in enumerate((3, 8, 9, 16, 17, 30, 30, 30, 63, 65, PC.LDS_CUT, PC.LDS_CUT + 1, 30, 30, 16, 250))]
    packed = PC.pack(loci, rng.integers(0, 1 << 63, len(loci), dtype=np.uint64))
    inp.update({"phase_" + k: packed[k] for k in PHASE_KEYS})
    return inp


def n_alleles_of(entry: str, n_loci: int) -> np.ndarray:
    """n_alleles per plain locus: 1, 2 in turn for strk_call_alleles, 1 .. 6 in turn for strk_call_alleles_n (the kinds turn
    with period 7); the locus of 300 reads has 2 and 4."""
    nal = 1 + np.arange(n_loci, dtype=np.int32) % (2 if entry == "plain" else 6)
    nal[-1] = 2 if entry == "plain" else 4
    return nal


def run_all(inp: dict, ctx=None) -> dict:
    """Every output array of the three entry points on `inp`, keyed `<entry>_B<bootstraps>_<array>`."""
    from strkit_amd.alleles import AlleleParams, call_alleles_batch, call_alleles_n_batch
    from strkit_amd.phasing import call_alleles_phased_batch
    plain = [inp[k] for k in INPUT_KEYS]
    n_loci = plain[0].shape[0] - 1
    out = {}
    for B in BOOTSTRAPS:
        p = AlleleParams(num_bootstrap=B)
        res = dict(plain=call_alleles_batch(*plain[:3], n_alleles_of("plain", n_loci), plain[3], p, ctx),
                   n=call_alleles_n_batch(*plain[:3], n_alleles_of("n", n_loci), plain[3], p, ctx),
                   phased=call_alleles_phased_batch(*[inp["phase_" + k] for k in PHASE_KEYS], params=p, fallback=False, ctx=ctx))
        for entry, arrays in res.items():
            out.update({f"{entry}_B{B}_{k}": v for k, v in arrays.items()})
    return out


if __name__ == "__main__":
    dst = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "out", "golden")
    os.makedirs(dst, exist_ok=True)
    inp = make_inputs()
    out = run_all(inp)
    np.savez_compressed(os.path.join(dst, "alleles_parent.npz"), **inp, **out)
    for entry in ("plain", "n", "phased"):
        o = {k: out[f"{entry}_B100_{k}"] for k in ("status", "modal_n")}
        print(entry, "status", np.bincount(o["status"]).tolist(), "modal_n", np.bincount(o["modal_n"]).tolist())
    print(len(inp["read_off"]) - 1, "loci,", inp["cns"].shape[0], "reads,", len(out), "output arrays")
