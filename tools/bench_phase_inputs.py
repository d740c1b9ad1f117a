#!/usr/bin/env python
"""Times the inputs of the phased call read from an alignment file: k_dbam_phase_cells and k_snv_useful (+ k_snv_gather) by HIP
events (strk_dbam_kernel_ms around each call; medians of repeated calls after a warm-up) and their host twins strk_phase_cells /
strk_useful_snvs (wall clock, the library's own threads) as the yardstick, on a synthetic file: `--loci` loci x `--reads` reads
of `--read-len` bases with about `--candidates` candidate positions per locus; half of the reads carry a HiFi-like CIGAR (tens of
operations), half an ONT-like one (thousands).  The issue's shape is 10 000 x 30 x 15 000 with 100 candidates; a smaller
--loci keeps the same per-item work.  Prints one JSON line; the device results are checked against the host's first.

--call-loci N also runs a phased `call` on N synthetic loci (frontend/synth_phased.py) and reports the share of its wall time
that the two stages take (wall clock of the calls inside the block path, their uploads and downloads included)."""
import argparse
import json
import os
import struct
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from strkit_amd.frontend import DeviceBam, NativeBam  # noqa: E402
from strkit_amd.frontend import phase_inputs as pi  # noqa: E402
from strkit_amd.frontend.bam import _BGZF_EOF, bgzf_block  # noqa: E402


def _cigar(rng, read_len: int, ont: bool) -> np.ndarray:
    """M runs separated by single-base I / D / X, soft clips of 120 at both ends; about read_len query bases."""
    n_runs = max(2, read_len // (12 if ont else 600))
    runs = np.maximum(rng.multinomial(read_len - 240, np.ones(n_runs) / n_runs), 1)
    ops = [(120 << 4) | 4]
    for k, ln in enumerate(runs):
        ops.append((int(ln) << 4) | 0)
        if k + 1 < n_runs:
            ops.append((1 << 4) | int(rng.choice([1, 2, 8])))
    ops.append((120 << 4) | 4)
    return np.array(ops, np.uint32)


def _template(rng, cigar: np.ndarray, tags: bytes) -> tuple[bytes, int]:
    ops, lens = cigar & 15, cigar >> 4
    n_q = int(lens[np.isin(ops, (0, 1, 4, 7, 8))].sum())
    ref_len = int(lens[np.isin(ops, (0, 2, 3, 7, 8))].sum())
    nib = rng.choice(np.array([1, 2, 4, 8], np.uint8), n_q + (n_q & 1))
    body = struct.pack("<iiBBHHHIiii", 0, 0, 2, 60, 4680, len(cigar), 0, n_q, -1, -1, 0) + b"r\0" + cigar.tobytes()
    body += ((nib[0::2] << 4) | nib[1::2]).astype(np.uint8).tobytes() + rng.integers(5, 50, n_q).astype(np.uint8).tobytes() + tags
    return struct.pack("<i", len(body)) + body, ref_len


def make_file(path: str, n_loci: int, n_reads: int, read_len: int, n_cand: int, seed: int = 1) -> dict:
    rng = np.random.default_rng(seed)
    temps = []
    for k in range(64):
        tags = b"" if k % 4 == 0 else b"HPC" + bytes([1 + k % 2]) + b"PSi" + struct.pack("<i", 1000 + k // 8)
        temps.append(_template(rng, _cigar(rng, read_len, ont=bool(k & 1)), tags))
    contig_len = (n_loci + 2) * (read_len + 1000)
    head = b"BAM\x01" + struct.pack("<i", 0) + struct.pack("<i", 1) + struct.pack("<i", 5) + b"chr1\0" + struct.pack("<i", contig_len)
    import zlib
    item_locus, cand, cand_off = [], [], [0]
    buf = bytearray(head)
    with open(path, "wb") as fh:          # stored deflate blocks, written as the records come: the file is made to be read, not to be small
        def flush(everything: bool) -> None:
            n = len(buf) if everything else len(buf) // 0xFF00 * 0xFF00
            for i in range(0, n, 0xFF00):
                chunk = bytes(buf[i:min(i + 0xFF00, n)])
                comp = zlib.compressobj(0, zlib.DEFLATED, -15)
                fh.write(bgzf_block(chunk, comp.compress(chunk) + comp.flush()))
            del buf[:n]

        for l in range(n_loci):
            at = 1000 + l * (read_len + 1000)
            # (records in locus order with positions jittered inside a locus: the readers scan the chain, they do not need them sorted)
            for r in range(n_reads):
                rec, _ = temps[int(rng.integers(0, 64))]
                buf += rec[:8] + struct.pack("<i", at + int(rng.integers(0, 200))) + rec[12:]
                item_locus.append(l)
            c = np.unique(at + rng.integers(0, read_len, n_cand))
            cand.append(c)
            cand_off.append(cand_off[-1] + c.size)
            flush(False)
        flush(True)
        fh.write(_BGZF_EOF)
    return {"item_locus": np.array(item_locus, np.int32), "cand_off": np.array(cand_off, np.int32), "cand_pos": np.concatenate(cand).astype(np.int64)}


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--loci", type=int, default=10000)
    ap.add_argument("--reads", type=int, default=30)
    ap.add_argument("--read-len", type=int, default=15000)
    ap.add_argument("--candidates", type=int, default=100)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--host-repeats", type=int, default=3)
    ap.add_argument("--host-threads", type=int, default=16, help="CPUs the host twins may use (the process's affinity while they run)")
    ap.add_argument("--call-loci", type=int, default=0,
                    help="also run a phased `call` (SNVs and haplotags) on this many synthetic loci of --reads reads of --read-len bases and "
                         "report the share of its wall time that the two stages take")
    a = ap.parse_args()
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "bench.bam")
        t0 = time.perf_counter()
        d = make_file(path, a.loci, a.reads, a.read_len, a.candidates)
        t_make = time.perf_counter() - t0
        nb, db = NativeBam(path), DeviceBam(path)
    n_items = int(d["item_locus"].size)
    rec_idx = np.arange(n_items)
    kept_off = np.arange(0, n_items + 1, a.reads, dtype=np.int32)
    kept_item = np.arange(n_items, dtype=np.int32)
    args = (rec_idx, d["item_locus"], d["cand_off"], d["cand_pos"])

    cpus = sorted(os.sched_getaffinity(0))
    os.sched_setaffinity(0, cpus[:max(1, a.host_threads)])      # the library sizes its thread pool by the CPUs it may run on
    host_cells_s, host_useful_s = [], []
    for _ in range(a.host_repeats):
        t0 = time.perf_counter()
        hc = pi.phase_cells(nb, *args)
        host_cells_s.append(time.perf_counter() - t0)
        t0 = time.perf_counter()
        hu = pi.library_useful_snvs(hc, kept_off, kept_item, 2)
        host_useful_s.append(time.perf_counter() - t0)

    os.sched_setaffinity(0, cpus)
    dc = pi.phase_cells(db, *args, download=True)             # warm-up, and the check
    du = pi.library_useful_snvs(dc, kept_off, kept_item, 2)
    same = all(np.array_equal(dc[k], hc[k]) for k in ("hp", "ps", "base", "qual")) and all(np.array_equal(du[k], hu[k]) for k in du)
    cells_ms, useful_ms, cells_wall, useful_wall = [], [], [], []
    for _ in range(a.repeats):
        k0, t0 = db.kernel_s(), time.perf_counter()
        dc = pi.phase_cells(db, *args)
        k1, t1 = db.kernel_s(), time.perf_counter()
        pi.library_useful_snvs(dc, kept_off, kept_item, 2)
        k2, t2 = db.kernel_s(), time.perf_counter()
        cells_ms.append((k1 - k0) * 1e3)
        useful_ms.append((k2 - k1) * 1e3)
        cells_wall.append((t1 - t0) * 1e3)
        useful_wall.append((t2 - t1) * 1e3)
    db.close()
    med = lambda xs: round(float(np.median(xs)), 4)  # noqa: E731
    share = None
    if a.call_loci:
        from strkit_amd.frontend import call_sample
        from strkit_amd.frontend.synth_phased import make_phased_dataset
        with tempfile.TemporaryDirectory() as tmp:
            t = make_phased_dataset(tmp, n_loci=a.call_loci, reads_per_locus=a.reads, read_len=a.read_len, spacing=a.read_len + 5000)
            runs = [call_sample(t["paths"]["bam"], t["paths"]["ref"], t["paths"]["loci"], call_alleles=True, seed=1, use_hp=True,
                                snv_vcf=t["paths"]["snvs"], front_end="device") for _ in range(3)]
        rep = sorted(runs, key=lambda r: r["runtime"])[1]
        st = rep["stage_times"]
        share = {"loci": a.call_loci, "runtime_s": round(rep["runtime"], 4), "phase_cells_s": st.get("phase_cells_s"), "useful_snvs_s": st.get("useful_snvs_s"),
                 "phase_cells_share": round(st.get("phase_cells_s", 0.0) / rep["runtime"], 4), "useful_snvs_share": round(st.get("useful_snvs_s", 0.0) / rep["runtime"], 4),
                 "methods": sorted({str(r["assign_method"]) for r in rep["results"]})}
    print(json.dumps({
        "shape": {"loci": a.loci, "reads": a.reads, "read_len": a.read_len, "items": n_items, "candidates": int(d["cand_pos"].size),
                  "cells": int(dc["n_cells"]), "useful_snvs": int(hu["snv_off"][-1])},
        "device_equals_host": bool(same), "make_file_s": round(t_make, 2), "repeats": a.repeats,
        "k_dbam_phase_cells_ms": {"median": med(cells_ms), "min": round(min(cells_ms), 4), "max": round(max(cells_ms), 4)},
        "k_snv_useful_and_gather_ms": {"median": med(useful_ms), "min": round(min(useful_ms), 4), "max": round(max(useful_ms), 4)},
        "device_call_wall_ms": {"cells": med(cells_wall), "useful": med(useful_wall)},
        "every_repeat_ms": {k: [round(x, 4) for x in v] for k, v in (("cells_kernel", cells_ms), ("useful_kernel", useful_ms),
                                                                     ("cells_wall", cells_wall), ("useful_wall", useful_wall))},
        "host_threads": min(len(cpus), max(1, a.host_threads)), "phased_call": share,
        "host_phase_cells_ms": med([x * 1e3 for x in host_cells_s]), "host_useful_snvs_ms": med([x * 1e3 for x in host_useful_s]),
    }))
    if not same:
        raise SystemExit("the device results differ from the host's")


if __name__ == "__main__":
    main()
