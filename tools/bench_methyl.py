#!/usr/bin/env python
"""Times methylation from MM / ML tags: k_dbam_methyl by HIP events (strk_dbam_kernel_ms around each call; median of repeated
calls after a warm-up) and its host twin strk_methyl (wall clock, the library's own threads, the process held to --host-threads
CPUs) as the yardstick, on a synthetic file: `--loci` loci x `--reads` reads of `--read-len` bases, half of them reverse-strand,
each with a CGG tract of 20-200 copies in its middle, an =/X CIGAR of some forty operations and a C+m entry that calls every
CpG of the tract and about one target per 50 bases elsewhere.  The issue's shape is 10 000 x 30 x 15 000; a smaller --loci keeps
the same per-item work.  Prints one JSON line; the device results are checked against the host's first.

`call` is then run on --call-loci synthetic loci (frontend/synth_methyl.py) with and without the switch and reports the share
of the run that the switch takes."""
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
from strkit_amd.frontend import methyl as me  # noqa: E402
from strkit_amd.frontend.bam import _BGZF_EOF, bgzf_block  # noqa: E402
from strkit_amd.frontend.synth_methyl import encode_mm, mm_tags  # noqa: E402

CLIP = 120


def _template(rng, read_len: int, reverse: bool) -> tuple[bytes, int, int]:
    """(record, q_l, q_r): the tract [q_l, q_r) of the read; reference offset = read position - CLIP."""
    cn = int(rng.integers(20, 201))
    left = (read_len - 3 * cn) // 2
    seq = "".join(rng.choice(list("ACGT"), left)) + "CGG" * cn
    seq += "".join(rng.choice(list("ACGT"), read_len - len(seq)))
    q_l, q_r = left, left + 3 * cn
    target = "G" if reverse else "C"
    calls = {(p + 1 if reverse else p): int(rng.integers(0, 256)) for p in range(q_l, q_r) if seq[p] == "C" and seq[p + 1] == "G"}
    for p in range(read_len):
        if seq[p] == target and p not in calls and not q_l <= p <= q_r and rng.random() < 0.08:      # a quarter of the bases are targets: one call per ~50 bases
            calls[p] = int(rng.integers(0, 256))
    skips, probs = encode_mm(seq, reverse, calls)
    tags = b"RGZgrp\0" + mm_tags([("C+m" + ("?" if rng.integers(0, 2) else ""), skips, probs)])
    n_runs = 20
    runs = np.maximum(rng.multinomial(read_len - 2 * CLIP - (n_runs - 1), np.ones(n_runs) / n_runs), 1)
    ops = [(CLIP << 4) | 4]
    for k, ln in enumerate(runs):
        ops.append((int(ln) << 4) | 7)
        if k + 1 < n_runs:
            ops.append((1 << 4) | 8)
    ops.append(((read_len - CLIP - int(runs.sum()) - (n_runs - 1)) << 4) | 4)
    cigar = np.array(ops, np.uint32)
    nib = np.array(["=ACMGRSVTWYHKDBN".index(ch) for ch in seq] + [0] * (read_len & 1), np.uint8)
    body = struct.pack("<iiBBHHHIiii", 0, 0, 2, 60, 4680, len(cigar), 16 if reverse else 0, read_len, -1, -1, 0) + b"r\0" + cigar.tobytes()
    body += ((nib[0::2] << 4) | nib[1::2]).astype(np.uint8).tobytes() + rng.integers(20, 50, read_len).astype(np.uint8).tobytes() + tags
    return struct.pack("<i", len(body)) + body, q_l, q_r


def make_file(path: str, n_loci: int, n_reads: int, read_len: int, seed: int = 1) -> np.ndarray:
    """Writes the file; returns the four locus boundaries of every item [n, 4] (items in file order)."""
    rng = np.random.default_rng(seed)
    temps = [_template(rng, read_len, reverse=bool(k & 1)) for k in range(64)]
    contig_len = (n_loci + 2) * (read_len + 1000)
    head = b"BAM\x01" + struct.pack("<i", 0) + struct.pack("<i", 1) + struct.pack("<i", 5) + b"chr1\0" + struct.pack("<i", contig_len)
    coords = []
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
            for r in range(n_reads):
                rec, q_l, q_r = temps[int(rng.integers(0, 64))]
                pos = at + int(rng.integers(0, 200))
                buf += rec[:8] + struct.pack("<i", pos) + rec[12:]
                lc, rc = pos + q_l - CLIP, pos + q_r - CLIP
                coords.append((lc - 70, lc, rc, rc + 70))
            flush(False)
        flush(True)
        fh.write(_BGZF_EOF)
    return np.array(coords, np.int64)


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--loci", type=int, default=10000)
    ap.add_argument("--reads", type=int, default=30)
    ap.add_argument("--read-len", type=int, default=15000)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--host-repeats", type=int, default=3)
    ap.add_argument("--host-threads", type=int, default=16, help="CPUs the host twin may use (the process's affinity while it runs)")
    ap.add_argument("--call-loci", type=int, default=100, help="`call` with and without --use-methyl runs on this many synthetic loci (0: not run)")
    a = ap.parse_args()
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "bench.bam")
        t0 = time.perf_counter()
        coords = make_file(path, a.loci, a.reads, a.read_len)
        t_make = time.perf_counter() - t0
        nb, db = NativeBam(path), DeviceBam(path)
    n_items = int(coords.shape[0])
    rec_idx = np.arange(n_items)

    cpus = sorted(os.sched_getaffinity(0))
    os.sched_setaffinity(0, cpus[:max(1, a.host_threads)])      # the library sizes its thread pool by the CPUs it may run on
    host_s = []
    for _ in range(a.host_repeats):
        t0 = time.perf_counter()
        h = me.methyl(nb, rec_idx, coords)
        host_s.append(time.perf_counter() - t0)
    os.sched_setaffinity(0, cpus)

    d = me.methyl(db, rec_idx, coords)                          # warm-up, and the check
    same = all(np.array_equal(d[k], h[k]) for k in ("status", "sites", "known", "mc"))
    kernel_ms, wall_ms = [], []
    for _ in range(a.repeats):
        k0, t0 = db.kernel_s(), time.perf_counter()
        me.methyl(db, rec_idx, coords)
        kernel_ms.append((db.kernel_s() - k0) * 1e3)
        wall_ms.append((time.perf_counter() - t0) * 1e3)
    db.close()
    med = lambda xs: round(float(np.median(xs)), 4)  # noqa: E731
    share = None
    if a.call_loci:
        from strkit_amd.frontend import call_sample
        from strkit_amd.frontend.synth_methyl import make_methyl_dataset
        with tempfile.TemporaryDirectory() as tmp:
            t = make_methyl_dataset(tmp, n_loci=a.call_loci, reads_per_locus=a.reads, read_len=a.read_len, spacing=a.read_len + 5000)
            run = lambda **kw: sorted((call_sample(t["paths"]["bam"], t["paths"]["ref"], t["paths"]["loci"], call_alleles=True, seed=1,  # noqa: E731
                                                   front_end="device", **kw) for _ in range(3)), key=lambda r: r["runtime"])[1]
            off, on = run(), run(use_methyl=True)
        share = {"loci": a.call_loci, "runtime_s_without": round(off["runtime"], 4), "runtime_s_with": round(on["runtime"], 4),
                 "methyl_s": round(on["stage_times"].get("methyl_s", 0.0), 4),
                 "methyl_share": round(on["stage_times"].get("methyl_s", 0.0) / on["runtime"], 4)}
    print(json.dumps({
        "shape": {"loci": a.loci, "reads": a.reads, "read_len": a.read_len, "items": n_items, "sites": int(h["sites"].sum()),
                  "statuses": np.bincount(h["status"], minlength=6).tolist()},
        "device_equals_host": bool(same), "make_file_s": round(t_make, 2), "repeats": a.repeats,
        "k_dbam_methyl_ms": {"median": med(kernel_ms), "min": round(min(kernel_ms), 4), "max": round(max(kernel_ms), 4)},
        "device_call_wall_ms": med(wall_ms), "every_repeat_ms": {"kernel": [round(x, 4) for x in kernel_ms], "wall": [round(x, 4) for x in wall_ms]},
        "host_threads": min(len(cpus), max(1, a.host_threads)),
        "host_strk_methyl_ms": med([x * 1e3 for x in host_s]), "call": share,
    }))
    if not same:
        raise SystemExit("the device results differ from the host's")


if __name__ == "__main__":
    main()
