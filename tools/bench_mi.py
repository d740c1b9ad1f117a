#!/usr/bin/env python3
"""Times the trio inheritance rule (strkit_amd.mi.mi_trio_batch) on synthetic trios and writes profiles/r22_mi.txt:

  per (loci, depth per sample, test), medians of --reps runs: strk_mi_trio's kernel milliseconds and the time of the whole call
  over packed arrays, strk_mi_trio_host's time on 16 threads (OMP_NUM_THREADS where set), and the scipy restatement (tests/mi_restatement.py) on one core over the first --scipy-loci loci, which is
  the number the speed is judged against (scipy is the reference's arithmetic);
  registers, LDS and scratch of k_mi_small and k_mi_large from the library's gfx950 code object;
  the agreement lines of the corpus of tests/mi_cases.py (device against the oracle) and its share of lenient loci per cell.

  python tools/bench_mi.py [--loci 10000,1000000] [--depths 15,30,250] [--scipy-loci 10000] [--reps 5] [--max-reads 800000000] [--out PATH]

A cell whose reads exceed --max-reads is skipped and said so.  No rate is asserted anywhere."""
import argparse
import os
import re
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from strkit_amd import _build, mi  # noqa: E402


def synth(n_loci, depth, seed=22, chunk=100_000):
    """synth_chunk over chunks of loci (the noise of a million deep loci would not fit the memory at once)."""
    parts = [synth_chunk(min(chunk, n_loci - l0), depth, seed + l0 // chunk) for l0 in range(0, n_loci, chunk)]
    gt, ci95 = np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])
    cn = np.concatenate([p[3] for p in parts])
    grp_off = np.zeros(6 * n_loci + 1, np.int64)
    np.cumsum(np.concatenate([np.diff(p[2]) for p in parts]), out=grp_off[1:])
    return gt, ci95, grp_off, cn


def synth_chunk(n_loci, depth, seed):
    """Trios of `depth` reads per sample (two groups of depth // 2 and the rest): parents' alleles 5 .. 40, the child inherits one
    of each, every tenth locus carries +1 .. +3 copies on one child allele; reads = allele + rounded normal noise."""
    rng = np.random.default_rng(seed)
    par = rng.integers(5, 41, (n_loci, 4))
    pick_m, pick_f = rng.integers(0, 2, n_loci), rng.integers(0, 2, n_loci)
    child = np.stack([par[np.arange(n_loci), pick_m], par[np.arange(n_loci), 2 + pick_f]], axis=1)
    step = np.where(np.arange(n_loci) % 10 == 0, rng.integers(1, 4, n_loci), 0)
    child[np.arange(n_loci), rng.integers(0, 2, n_loci)] += step
    gt = np.concatenate([child, par], axis=1).astype(np.int32)
    sizes = np.tile(np.array([depth // 2, depth - depth // 2] * 3, np.int64), n_loci)
    grp_off = np.zeros(6 * n_loci + 1, np.int64)
    np.cumsum(sizes, out=grp_off[1:])
    alleles = np.repeat(gt.reshape(-1), sizes)
    cn = np.maximum(0, np.rint(alleles + rng.normal(0.0, 0.35, alleles.size) * (1 + 0.05 * alleles))).astype(np.int32)
    ci95 = np.stack([gt - 1, gt + 1], axis=2).reshape(n_loci, 12).astype(np.int32)
    return gt, ci95, grp_off, cn


def loci_dicts(gt, ci95, grp_off, cn, n):
    return [{"gt": gt[i].tolist(), "ci95": ci95[i].reshape(6, 2).tolist(), "ci99": None, "seqs": None,
             "reads": [cn[grp_off[6 * i + g]:grp_off[6 * i + g + 1]].tolist() for g in range(6)]} for i in range(n)]


def resources():
    """vgprs, sgprs, LDS and scratch bytes per mi kernel from the gfx950 code object inside the library."""
    llvm = os.path.join(os.path.dirname(os.path.dirname(_build._hipcc())), "llvm", "bin")
    with tempfile.TemporaryDirectory() as d:
        fat, co = os.path.join(d, "fat.bin"), os.path.join(d, "co.elf")
        subprocess.run(["objcopy", "-O", "binary", "--only-section=.hip_fatbin", _build.LIB_PATH, fat], check=True)
        subprocess.run([os.path.join(llvm, "clang-offload-bundler"), "--unbundle", "--type=o", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950",
                        "--input=" + fat, "--output=" + co], check=True)
        notes = subprocess.run([os.path.join(llvm, "llvm-readelf"), "--notes", co], check=True, capture_output=True, text=True).stdout
    lines = []
    for block in re.split(r"\n\s+- \.agpr_count:", notes)[1:]:
        name = re.search(r"\.name:\s+(\S+)", block)
        if not name or "k_mi_" not in name.group(1):
            continue
        f = {k: int(re.search(r"\.%s:\s+(\d+)" % k, block).group(1)) for k in
             ("vgpr_count", "sgpr_count", "group_segment_fixed_size", "private_segment_fixed_size", "vgpr_spill_count", "sgpr_spill_count")}
        short = re.sub(r"^_ZN7strk_mi\d+|ENS_.*$", "", name.group(1))
        lines.append(f"{short}: {f['vgpr_count']} VGPRs, {f['sgpr_count']} SGPRs, "
                     f"{f['group_segment_fixed_size']} B LDS, {f['private_segment_fixed_size']} B scratch per lane, "
                     f"spills {f['vgpr_spill_count']} VGPR / {f['sgpr_spill_count']} SGPR")
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--loci", default="10000,1000000")
    ap.add_argument("--depths", default="15,30,250")
    ap.add_argument("--tests", default="x2,wmw,wmw-gt")
    ap.add_argument("--scipy-loci", type=int, default=10000)
    ap.add_argument("--max-reads", type=int, default=800_000_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-corpus", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r22_mi.txt"))
    a = ap.parse_args()
    import mi_restatement as R
    out = ["# tools/bench_mi.py: trio inheritance rule, synthetic trios (sizes, depth per sample, test)", f"# threshold of k_mi_small: {mi.small_threshold()} reads per locus", ""]
    out += ["resources (gfx950 code object):"] + ["  " + x for x in resources()] + [""]
    host_threads = min(len(os.sched_getaffinity(0)), int(os.environ.get("OMP_NUM_THREADS", "16") or 16))
    out += [f"every figure is the median of {a.reps} runs after a warm-up call.  'call' = one mi_trio_batch over packed arrays: check, pieces, copies up,",
            "kernels, copies down.  It does not cover reading the three files and packing them, which is per-locus Python (see the last line).", ""]
    scipy_rate = {}
    for n_loci in [int(x) for x in a.loci.split(",")]:
        for depth in [int(x) for x in a.depths.split(",")]:
            if n_loci * depth * 3 > a.max_reads:
                out.append(f"loci {n_loci} depth {depth}: skipped, {n_loci * depth * 3} reads are more than --max-reads {a.max_reads}")
                continue
            gt, ci95, grp_off, cn = synth(n_loci, depth)
            for test in a.tests.split(","):
                mi.mi_trio_batch(gt[:64], ci95[:64], grp_off[:385], cn[:grp_off[384]], test=test)      # warm-up: context, buffers
                t_devs, t_hosts, k_ms = [], [], []
                for _ in range(a.reps):
                    t0 = time.perf_counter()
                    dev = mi.mi_trio_batch(gt, ci95, grp_off, cn, test=test)
                    t_devs.append(time.perf_counter() - t0)
                    k_ms.append(dev["stats"]["kernel_ms"])
                    t0 = time.perf_counter()
                    host = mi.mi_trio_batch(gt, ci95, grp_off, cn, test=test, device="host")
                    t_hosts.append(time.perf_counter() - t0)
                t_dev, t_host, kernel_ms = float(np.median(t_devs)), float(np.median(t_hosts)), float(np.median(k_ms))
                same = all(dev[k].tobytes() == host[k].tobytes() for k in ("respects", "p", "config", "mutation_from", "status"))
                key = (depth, test)
                if key not in scipy_rate:
                    ns = min(a.scipy_loci, n_loci)
                    ls = loci_dicts(gt, ci95, grp_off, cn, ns)
                    t0 = time.perf_counter()
                    for l in ls:
                        R.respects_mi(l)
                        R.de_novo(l, test)
                    scipy_rate[key] = ns / (time.perf_counter() - t0)
                out.append(f"loci {n_loci} depth {depth} test {test}: device kernels {kernel_ms:.2f} ms, call {t_dev * 1e3:.2f} ms "
                           f"({n_loci / t_dev:.0f} loci/s), {dev['stats']['n_fallback']} loci on k_mi_large, {dev['stats']['n_sub_batches']} pieces; "
                           f"host {t_host * 1e3:.2f} ms ({n_loci / t_host:.0f} loci/s, {host_threads} threads); scipy restatement on one core "
                           f"{scipy_rate[key]:.0f} loci/s; device = host bit for bit: {same}; below the level: {int((dev['p'] < 0.05).sum())}")
                print(out[-1], flush=True)
    # what a run from files adds in front of the call: packing loci that are Python objects (assemble_trio ends in pack_loci)
    gt, ci95, grp_off, cn = synth(10000, 30)
    ls = loci_dicts(gt, ci95, grp_off, cn, 10000)
    t_pack = []
    for _ in range(a.reps):
        t0 = time.perf_counter()
        mi.pack_loci(ls)
        t_pack.append(time.perf_counter() - t0)
    out += ["", f"pack_loci (Python, one core) on 10000 loci of depth 30: {np.median(t_pack) * 1e3:.1f} ms ({10000 / np.median(t_pack):.0f} loci/s): a run from files is bound by "
            "reading and packing, not by the rule"]
    if not a.no_corpus:
        import mi_cases as cases
        pk = mi.pack_loci(cases.all_loci()[0])
        out.append("")
        for test in ("none",) + cases.TESTS:
            got = mi.mi_trio_batch(pk["gt"], pk["ci95"], pk["grp_off"], pk["cn"], None, pk["seq_id"], pk["seq_len"], test=test, sig_level=cases.SIG)
            out.append("corpus: " + cases.compare(got, test))
            if test != "none":
                out.append("corpus: lenient share per cell " + ", ".join(f"{k} {v:.3f}" for k, v in cases.lenient_share(test).items()))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write("\n".join(out) + "\n")
    print("\n".join(out[:8]))


if __name__ == "__main__":
    main()
