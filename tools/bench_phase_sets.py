#!/usr/bin/env python3
"""How long the phase-set rule takes (frontend/phase_sets.py).

    python tools/bench_phase_sets.py                 # the rule alone, on the CPU: 100 000 synthetic loci with 4 SNVs each
    python tools/bench_phase_sets.py --linked        # and `call` on the linked data set (needs the GPU): phase_sets_s of the run

The synthetic loci lie on one contig; locus i holds the sites i .. i + 3 of a row of heterozygous sites, in an orientation of its
own, so that nearly every locus joins the set before it or opens one, and one locus in eight bridges two sets.  Blocks of 200 loci
take a snapshot each, as call_blocks does; the contig's rows get the fix-up at the end."""
from __future__ import annotations

import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from strkit_amd.frontend.phase_inputs import PhaseSetRemap  # noqa: E402
from strkit_amd.frontend.phase_sets import PhaseSets  # noqa: E402


def rule_alone(n_loci: int, n_snvs: int, seed: int) -> dict:
    rng = np.random.default_rng(seed)
    truth = [("ACGT"[a], "ACGT"[(a + 1 + b) % 4]) for a, b in zip(rng.integers(4, size=n_loci * 2 + n_snvs), rng.integers(3, size=n_loci * 2 + n_snvs))]
    swapped = rng.integers(2, size=n_loci).astype(bool)
    step = rng.choice([1, 2, 5], size=n_loci, p=[0.5, 0.375, 0.125])      # 5: past every site of the locus before -> a new set
    # (a start that wanders by up to 3 sites: a later locus can reach back over the gap between two sets and join them)
    first = np.maximum(np.cumsum(step) + rng.integers(-3, 4, size=n_loci), 0) % (n_loci * 2)
    loci = [[(f"s{k}", truth[k][::-1] if sw else truth[k]) for k in range(f, f + n_snvs)] for f, sw in zip(first.tolist(), swapped.tolist())]
    sets = PhaseSets()
    sets.remap = PhaseSetRemap(sets)
    rows = []
    t0 = time.perf_counter()
    for i, snvs in enumerate(loci):
        if i % 200 == 0:
            sets.snapshot()
        sets.enter("chr1", i + 1)
        r = sets.resolve(snvs)
        if r.ps is not None:
            rows.append({"locus_index": i + 1, "ps": r.ps, "call": [1, 2], "reads": {}})
    t_rule = time.perf_counter() - t0
    n_syn = len(sets.syn)
    t0 = time.perf_counter()
    sets.finish_contig(rows)
    t_fix = time.perf_counter() - t0
    return {"n_loci": n_loci, "n_snvs": n_snvs, "rule_s": round(t_rule, 4), "fix_up_s": round(t_fix, 4),
            "us_per_locus": round((t_rule + t_fix) / n_loci * 1e6, 3), "rows_with_ps": len(rows), "synonyms": n_syn,
            "final_sets": len({r["ps"] for r in rows})}


def linked_call() -> dict:
    from strkit_amd.frontend import call_sample
    from strkit_amd.frontend.synth_linked import make_linked_dataset
    with tempfile.TemporaryDirectory() as d:
        t = make_linked_dataset(d)
        out = {}
        for name, kw in (("off", {}), ("on", {"snv_phase_sets": True})):
            best = None
            for _ in range(5):      # (the first run pays for the library's set-up)
                rep = call_sample(t["paths"]["bam"], t["paths"]["ref"], t["paths"]["loci"], call_alleles=True, seed=1, consensus=True,
                                  count_kmers="peak", snv_vcf=t["paths"]["snvs"], front_end="device", **kw)
                if best is None or rep["runtime"] < best["runtime"]:
                    best = rep
            out[name] = {"runtime_s": round(best["runtime"], 4), "alleles_s": best["stage_times"].get("alleles_s"),
                         "phase_sets_s": best["stage_times"].get("phase_sets_s")}
        return out


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--loci", type=int, default=100_000)
    ap.add_argument("--snvs", type=int, default=4)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--linked", action="store_true", help="also run `call` on the linked data set (GPU)")
    a = ap.parse_args()
    res = {"rule": rule_alone(a.loci, a.snvs, a.seed)}
    if a.linked:
        res["linked"] = linked_call()
    print(json.dumps(res))
    return 0


if __name__ == "__main__":
    sys.exit(main())
