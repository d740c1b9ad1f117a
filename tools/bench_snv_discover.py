#!/usr/bin/env python
"""Times the discovery of candidate SNVs from the reads: k_snv_span + k_snv_pileup + k_snv_pick by HIP events
(strk_dbam_kernel_ms around each call; medians of repeated calls after a warm-up) and the whole device call by the wall clock,
and the host twin strk_discover_snvs on `--host-threads` CPUs (wall clock, the library's own threads) as the yardstick, on a
synthetic file: `--loci` loci x `--reads` reads of `--read-len` bases around a locus in their middle; half of the reads carry a
HiFi-like CIGAR (tens of operations of hundreds of bases), half an ONT-like one (thousands of short operations); the two
haplotypes differ at `--het` positions a locus, and every X operation is a sequencing error.  The issue's shape is
10 000 x 30 x 15 000; a smaller --loci keeps the same work per locus.  Prints one JSON line; the device result is checked
against the host's first.

--call-loci N also runs `call` on N synthetic loci (frontend/synth_phased.py) twice, with --discover-snvs and with the same
sites from a tabix-indexed VCF (--incorporate-snvs), and reports the stage times of both routes for scale: snv_discover_s on the
one side, snv_candidates_s + phase_cells_s on the other."""
import argparse
import json
import os
import struct
import sys
import tempfile
import time
import zlib

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from strkit_amd.frontend import DeviceBam, NativeBam  # noqa: E402
from strkit_amd.frontend import snv_discovery as sd  # noqa: E402
from strkit_amd.frontend.bam import _BGZF_EOF, bgzf_block  # noqa: E402

_OTHER = {1: 2, 2: 4, 4: 8, 8: 1}      # 4-bit codes: A -> C -> G -> T -> A


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


def _template(rng, cigar: np.ndarray, ref: np.ndarray, start: int, alt_at: dict) -> bytes:
    """A record (position left to the caller) that reads `ref` from `start` along `cigar`: the reference's bases under M, another
    base under X, alt_at[p] at a heterozygous position p; inserted and clipped bases are random."""
    nib, r = [], start
    for c in cigar:
        op, ln = int(c) & 15, int(c) >> 4
        if op in (0, 8):
            part = ref[r:r + ln].copy()
            if op == 8:
                part = np.array([_OTHER[int(b)] for b in part], np.uint8)
            for p, b in alt_at.items():
                if r <= p < r + ln:
                    part[p - r] = b
            nib.append(part)
        elif op in (1, 4):
            nib.append(rng.choice(np.array([1, 2, 4, 8], np.uint8), ln))
        if op in (0, 2, 8):
            r += ln
    nib = np.concatenate(nib)
    n_q = int(nib.size)
    pad = np.concatenate((nib, np.zeros(n_q & 1, np.uint8)))
    body = struct.pack("<iiBBHHHIiii", 0, 0, 2, 60, 4680, len(cigar), 0, n_q, -1, -1, 0) + b"r\0" + cigar.tobytes()
    body += ((pad[0::2] << 4) | pad[1::2]).astype(np.uint8).tobytes() + rng.integers(15, 50, n_q).astype(np.uint8).tobytes()
    return struct.pack("<i", len(body)) + body


def make_file(path: str, n_loci: int, n_reads: int, read_len: int, n_het: int, seed: int = 1) -> dict:
    """Every locus repeats one stretch of `read_len + 200` reference bases; 64 record templates (a jitter of 0 .. 199, a haplotype,
    a CIGAR each) are copied to every locus with their positions moved."""
    rng = np.random.default_rng(seed)
    stretch = read_len + 1200
    ref = rng.choice(np.array([1, 2, 4, 8], np.uint8), stretch)
    mid = read_len // 2
    het = np.sort(rng.choice(np.concatenate((np.arange(400, mid - 100), np.arange(mid + 200, read_len - 400))), n_het, replace=False))
    alt_at = {int(p): _OTHER[int(ref[p])] for p in het}
    temps = []
    for k in range(64):
        jitter = int(rng.integers(0, 200))
        temps.append((_template(rng, _cigar(rng, read_len, ont=bool(k & 1)), ref, jitter, alt_at if (k >> 1) & 1 else {}), jitter))
    head = b"BAM\x01" + struct.pack("<i", 0) + struct.pack("<i", 1) + struct.pack("<i", 5) + b"chr1\0" + struct.pack("<i", (n_loci + 2) * stretch)
    item_locus, left = [], []
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
            at = 1000 + l * stretch
            for r in range(n_reads):
                rec, jitter = temps[int(rng.integers(0, 64))]
                buf += rec[:8] + struct.pack("<i", at + jitter) + rec[12:]
                item_locus.append(l)
            left.append(at + mid)
            flush(False)
        flush(True)
        fh.write(_BGZF_EOF)
    left = np.array(left, np.int64)
    return {"item_locus": np.array(item_locus, np.int32), "left": left, "right": left + 60, "het_per_locus": int(n_het)}


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--loci", type=int, default=10000)
    ap.add_argument("--reads", type=int, default=30)
    ap.add_argument("--read-len", type=int, default=15000)
    ap.add_argument("--het", type=int, default=12, help="heterozygous positions a locus")
    ap.add_argument("--window", type=int, default=sd.DEFAULT_WINDOW)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--host-repeats", type=int, default=3)
    ap.add_argument("--host-threads", type=int, default=16, help="CPUs the host twin may use (the process's affinity while it runs)")
    ap.add_argument("--call-loci", type=int, default=0, help="also run `call` on this many synthetic loci with discovered SNVs and with a candidate VCF")
    a = ap.parse_args()
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "bench.bam")
        t0 = time.perf_counter()
        d = make_file(path, a.loci, a.reads, a.read_len, a.het)
        t_make = time.perf_counter() - t0
        nb, db = NativeBam(path), DeviceBam(path)
    n_items = int(d["item_locus"].size)
    args = (np.arange(n_items), d["item_locus"], d["left"], d["right"], np.arange(0, n_items + 1, a.reads, dtype=np.int32), np.arange(n_items, dtype=np.int32))
    kw = {"window": a.window}

    cpus = sorted(os.sched_getaffinity(0))
    os.sched_setaffinity(0, cpus[:max(1, a.host_threads)])      # the library sizes its thread pool by the CPUs it may run on
    host_s = []
    for _ in range(a.host_repeats):
        t0 = time.perf_counter()
        h_off, h_pos = sd.library_discover_snvs(nb, *args, **kw)
        host_s.append(time.perf_counter() - t0)
    os.sched_setaffinity(0, cpus)

    d_off, d_pos = sd.library_discover_snvs(db, *args, **kw)             # warm-up, and the check
    same = np.array_equal(d_off, h_off) and np.array_equal(d_pos, h_pos)
    kernel_ms, wall_ms = [], []
    for _ in range(a.repeats):
        k0, t0 = db.kernel_s(), time.perf_counter()
        sd.library_discover_snvs(db, *args, **kw)
        kernel_ms.append((db.kernel_s() - k0) * 1e3)
        wall_ms.append((time.perf_counter() - t0) * 1e3)
    db.close()
    med = lambda xs: round(float(np.median(xs)), 4)  # noqa: E731
    routes = None
    if a.call_loci:
        from strkit_amd.frontend import call_sample
        from strkit_amd.frontend.synth_phased import make_phased_dataset
        from strkit_amd.frontend.synth_snvs import index_snv_vcf
        keys = ("snv_discover_s", "snv_discover_device_s", "snv_candidates_s", "snv_vcf_device_s", "phase_cells_s", "useful_snvs_s", "phase_inputs_s")
        with tempfile.TemporaryDirectory() as tmp:
            t = make_phased_dataset(tmp, n_loci=a.call_loci, reads_per_locus=a.reads, read_len=a.read_len, spacing=a.read_len + 5000)
            gz = index_snv_vcf(t["paths"]["snvs"])
            routes = {}
            for name, how in (("discover_snvs", {"discover_snvs": True, "snv_discover_window": a.window}), ("snv_vcf", {"snv_vcf": gz})):
                runs = [call_sample(t["paths"]["bam"], t["paths"]["ref"], t["paths"]["loci"], call_alleles=True, seed=1, front_end="device", **how)
                        for _ in range(3)]
                rep = sorted(runs, key=lambda r: r["runtime"])[1]
                routes[name] = {"loci": a.call_loci, "runtime_s": round(rep["runtime"], 4), **{k: rep["stage_times"][k] for k in keys if k in rep["stage_times"]},
                                "methods": sorted({str(r.get("assign_method")) for r in rep["results"]}),
                                "snvs_called": sum(len(r.get("snvs", [])) for r in rep["results"])}
    print(json.dumps({
        "shape": {"loci": a.loci, "reads": a.reads, "read_len": a.read_len, "items": n_items, "window": a.window, "het_per_locus": d["het_per_locus"],
                  "tiles": int(a.loci) * 2 * ((a.window + 4095) // 4096), "candidates": int(h_off[-1]), "max_candidates_of_a_locus": int(np.diff(h_off).max())},
        "device_equals_host": bool(same), "make_file_s": round(t_make, 2), "repeats": a.repeats,
        "kernels_ms": {"median": med(kernel_ms), "min": round(min(kernel_ms), 4), "max": round(max(kernel_ms), 4)},
        "device_call_wall_ms": {"median": med(wall_ms), "min": round(min(wall_ms), 4), "max": round(max(wall_ms), 4)},
        "every_repeat_ms": {"kernels": [round(x, 4) for x in kernel_ms], "wall": [round(x, 4) for x in wall_ms]},
        "host_threads": min(len(cpus), max(1, a.host_threads)), "host_discover_snvs_ms": med([x * 1e3 for x in host_s]),
        "host_every_repeat_ms": [round(x * 1e3, 2) for x in host_s], "call_routes": routes,
    }))
    if not same:
        raise SystemExit("the device result differs from the host's")


if __name__ == "__main__":
    main()
