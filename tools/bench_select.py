#!/usr/bin/env python
"""Times read selection on a synthetic file of `--loci` loci x `--reads` reads of `--read-len` bases with read
names of 36 characters, one read in ten with a supplementary record of its name right behind it (the README's e2e shape is
10 000 x 30 x 15 000; a shorter --read-len keeps the records' count and names and shrinks the bases between them).  Three
variants, alternating in one run after a warm-up, with the spread over the repeats:
  (a) strk_dbam_select_reads: its kernels by HIP events (strk_dbam_kernel_ms around the call) and the whole call by wall clock;
  (b) strk_select_reads on the host cores over the same records (wall clock, the process held to --host-threads CPUs);
  (c) what the device stage replaces: DeviceBam.names of all fetched items plus the rule in Python (tests/select_restatement.py).
Prints one JSON line; the device results are checked against the host's and the restatement's first."""
import argparse
import json
import os
import struct
import sys
import tempfile
import time
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from select_restatement import select  # noqa: E402
from strkit_amd.frontend import DeviceBam, NativeBam  # noqa: E402
from strkit_amd.frontend.bam import _BGZF_EOF, bgzf_block  # noqa: E402
from strkit_amd.frontend.select import select_items  # noqa: E402


def make_file(path: str, n_loci: int, n_reads: int, read_len: int, seed: int = 1) -> np.ndarray:
    """Writes the file; returns item_off (the records of a locus are consecutive in the file)."""
    rng = np.random.default_rng(seed)
    tails = []
    for _ in range(16):                       # CIGAR, bases and qualities of sixteen reads; every record has its own name
        tails.append(struct.pack("<I", read_len << 4) + rng.integers(17, 137, (read_len + 1) // 2).astype(np.uint8).tobytes()
                     + rng.integers(20, 50, read_len).astype(np.uint8).tobytes())
    contig_len = (n_loci + 2) * (read_len + 1000)
    head = b"BAM\x01" + struct.pack("<i", 0) + struct.pack("<i", 1) + struct.pack("<i", 5) + b"chr1\0" + struct.pack("<i", contig_len)
    counts = []
    buf = bytearray(head)
    hexd = np.frombuffer(b"0123456789abcdef", np.uint8)
    with open(path, "wb") as fh:              # stored deflate blocks: the file is made to be read, not to be small
        def flush(everything: bool) -> None:
            n = len(buf) if everything else len(buf) // 0xFF00 * 0xFF00
            for i in range(0, n, 0xFF00):
                chunk = bytes(buf[i:min(i + 0xFF00, n)])
                comp = zlib.compressobj(0, zlib.DEFLATED, -15)
                fh.write(bgzf_block(chunk, comp.compress(chunk) + comp.flush()))
            del buf[:n]

        for l in range(n_loci):
            at = 1000 + l * (read_len + 1000)
            pos = np.sort(rng.integers(0, 200, n_reads)) + at
            names = hexd[rng.integers(0, 16, (n_reads, 36))]
            supp = rng.random(n_reads) < 0.1
            n = 0
            for r in range(n_reads):
                name = names[r].tobytes() + b"\0"
                tail = tails[int(rng.integers(0, 16))]
                for flag in (0, 0x800)[:2 if supp[r] else 1]:
                    body = struct.pack("<iiBBHHHIiii", 0, int(pos[r]), 37, 60, 4680, 1, flag, read_len, -1, -1, 0) + name + tail
                    buf += struct.pack("<i", len(body)) + body
                    n += 1
            counts.append(n)
            flush(False)
        flush(True)
        fh.write(_BGZF_EOF)
    return np.concatenate(([0], np.cumsum(counts))).astype(np.int64)


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--loci", type=int, default=10000)
    ap.add_argument("--reads", type=int, default=30)
    ap.add_argument("--read-len", type=int, default=15000)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--rules", type=int, default=7)
    ap.add_argument("--max-reads", type=int, default=250)
    ap.add_argument("--host-threads", type=int, default=16, help="CPUs the host entry may use (the process's affinity while it runs)")
    a = ap.parse_args()
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "bench.bam")
        t0 = time.perf_counter()
        item_off = make_file(path, a.loci, a.reads, a.read_len)
        t_make = time.perf_counter() - t0
        nb, db = NativeBam(path), DeviceBam(path)
    n_items = int(item_off[-1])
    assert nb.n_records == db.n_records == n_items
    rec = np.arange(n_items)
    cpus = sorted(os.sched_getaffinity(0))

    def device():
        k0, t0 = db.kernel_s(), time.perf_counter()
        out = select_items(db, db.rec_off, item_off, a.rules, a.max_reads)
        return out, (db.kernel_s() - k0) * 1e3, (time.perf_counter() - t0) * 1e3

    def host():
        os.sched_setaffinity(0, cpus[:max(1, a.host_threads)])      # the library sizes its thread pool by the CPUs it may run on
        t0 = time.perf_counter()
        out = select_items(nb, nb.rec_off, item_off, a.rules, a.max_reads)
        dt = (time.perf_counter() - t0) * 1e3
        os.sched_setaffinity(0, cpus)
        return out, dt

    def replaced():
        t0 = time.perf_counter()
        names = db.names(rec)
        t1 = time.perf_counter()
        flags = db.flag.tolist()
        off = item_off.tolist()
        reason, status, kept = [], [], []
        for l in range(len(off) - 1):
            r, s, n = select(list(zip(names[off[l]:off[l + 1]], flags[off[l]:off[l + 1]])), a.rules, a.max_reads)
            reason += r
            status += s
            kept.append(n)
        return (np.array(reason, np.uint8), np.array(status, np.uint8), np.array(kept, np.int32)), (t1 - t0) * 1e3, (time.perf_counter() - t0) * 1e3

    d, h, p = device()[0], host()[0], replaced()[0]                 # warm-up, and the check
    same = all(np.array_equal(x, y) and np.array_equal(x, z) for x, y, z in zip(d, h, p))
    t = {k: [] for k in ("device_kernel_ms", "device_call_ms", "host_ms", "names_ms", "names_plus_python_ms")}
    for _ in range(a.repeats):
        _, k, w = device()
        t["device_kernel_ms"].append(k)
        t["device_call_ms"].append(w)
        t["host_ms"].append(host()[1])
        _, n_ms, all_ms = replaced()
        t["names_ms"].append(n_ms)
        t["names_plus_python_ms"].append(all_ms)
    db.close()
    stat = lambda xs: {"median": round(float(np.median(xs)), 4), "min": round(min(xs), 4), "max": round(max(xs), 4),  # noqa: E731
                       "every_repeat": [round(x, 4) for x in xs]}
    rate = lambda xs: round(n_items / (float(np.median(xs)) / 1e3) / 1e6, 3)  # noqa: E731
    print(json.dumps({
        "shape": {"loci": a.loci, "reads": a.reads, "read_len": a.read_len, "items": n_items, "kept": int(d[2].sum()),
                  "reasons": np.bincount(d[0], minlength=5).tolist(), "chimeric_kept": int(((d[1] == 3) & (d[0] == 0)).sum())},
        "rules": a.rules, "max_reads": a.max_reads, "all_equal": bool(same), "make_file_s": round(t_make, 2), "repeats": a.repeats,
        "host_threads": min(len(cpus), max(1, a.host_threads)),
        "a_strk_dbam_select_reads_kernels_ms": stat(t["device_kernel_ms"]), "a_strk_dbam_select_reads_call_ms": stat(t["device_call_ms"]),
        "b_strk_select_reads_host_ms": stat(t["host_ms"]),
        "c_names_download_ms": stat(t["names_ms"]), "c_names_plus_python_rule_ms": stat(t["names_plus_python_ms"]),
        "million_items_per_s": {"a_kernels": rate(t["device_kernel_ms"]), "a_call": rate(t["device_call_ms"]), "b_host": rate(t["host_ms"]),
                                "c_replaced": rate(t["names_plus_python_ms"])},
    }))
    if not same:
        raise SystemExit("the three variants disagree")


if __name__ == "__main__":
    main()
