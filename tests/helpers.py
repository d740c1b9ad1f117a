"""Shared generators for the parity tests (seeded; no reference code involved)."""
from __future__ import annotations

import numpy as np

import oracle
from strkit_amd.synth import LocusBatch

ALPHA_ACGT = "ACGT"
ALPHA_WC = "ACGTXN"
ALPHA_IUPAC = "ACGTRYSWKMBDHVNX"


def rand_seq(rng, n, alpha=ALPHA_ACGT):
    return "".join(alpha[i] for i in rng.integers(len(alpha), size=n))


def noisy_tract(rng, motif, cn, n_edits, alpha):
    tr = list(motif * cn)
    for _ in range(n_edits):
        x = rng.random()
        if tr and x < 0.4:
            tr[rng.integers(len(tr))] = alpha[rng.integers(len(alpha))]
        elif tr and x < 0.7:
            del tr[rng.integers(len(tr))]
        else:
            tr.insert(int(rng.integers(len(tr) + 1)), alpha[rng.integers(len(alpha))])
    return "".join(tr)


def random_locus(rng, n_reads, motif_len=(1, 6), cn=(0, 40), flank=(1, 80), alpha=ALPHA_ACGT, motif_alpha=None,
                 edits=(0, 4)):
    m = int(rng.integers(motif_len[0], motif_len[1] + 1))
    motif = rand_seq(rng, m, motif_alpha or alpha)
    fl0 = rand_seq(rng, int(rng.integers(flank[0], flank[1] + 1)), alpha)
    fr0 = rand_seq(rng, int(rng.integers(flank[0], flank[1] + 1)), alpha)
    base_cn = int(rng.integers(cn[0], cn[1] + 1))
    reads = []
    for _ in range(n_reads):
        c = max(0, base_cn + int(rng.integers(-2, 3)))
        tr = noisy_tract(rng, motif, c, int(rng.integers(edits[0], edits[1] + 1)), alpha)
        fl = noisy_tract(rng, fl0, 1, int(rng.integers(0, 2)), alpha) or fl0
        fr = noisy_tract(rng, fr0, 1, int(rng.integers(0, 2)), alpha) or fr0
        reads.append((fl, tr, fr))
    return motif, reads


def oracle_table(b: LocusBatch, lo, n, flags=15):
    out = []
    for l in range(b.n_loci):
        motif = b.motif(l)
        for r in range(int(b.read_off[l]), int(b.read_off[l + 1])):
            fl, tr, fr = b.read(r)
            out.append(np.array([oracle.candidate_score(tr, fl, fr, motif, int(lo[r]) + k, flags)
                                 for k in range(int(n[r]))], np.int32))
    return out


def oracle_count(b: LocusBatch, max_iters=50, lsr=3, step=1, tie_rule=0, flags=15, feedback=True, narrowing=0):
    res = {k: np.zeros(b.n_reads, np.int32) for k in ("cn", "score", "n_iters", "start")}
    for l in range(b.n_loci):
        r0, r1 = int(b.read_off[l]), int(b.read_off[l + 1])
        if r1 == r0:
            continue
        s0 = int(b.seq_off[r0])
        o = oracle.count_locus(b.seqs[s0:int(b.seq_off[r1])], b.seq_off[r0:r1 + 1] - s0, b.nfl[r0:r1], b.ntr[r0:r1],
                               b.nfr[r0:r1], b.est_cn[r0:r1], b.motif(l), max_iters, lsr, step, tie_rule, flags,
                               feedback, narrowing=narrowing)
        for k in res:
            res[k][r0:r1] = o[k]
    return res


def oracle_count_pool(b: LocusBatch, threads=16, **kw):
    """oracle_count with the loci spread over a thread pool (the oracle is a C library that keeps no state between calls and
    runs without the interpreter lock): for batches of a few deep loci, where one core would take several seconds."""
    from concurrent.futures import ThreadPoolExecutor
    oracle.lib()
    order = sorted(range(b.n_loci), key=lambda l: int(b.read_off[l]) - int(b.read_off[l + 1]))     # deepest first
    with ThreadPoolExecutor(max(1, min(threads, 16, b.n_loci))) as pool:
        parts = dict(zip(order, pool.map(lambda l: oracle_count(b.locus_slice(l, l + 1), **kw), order)))
    return {k: np.concatenate([parts[l][k] for l in range(b.n_loci)]) if b.n_loci else np.zeros(0, np.int32) for k in ("cn", "score", "n_iters", "start")}


def py_search(start, step, lsr, max_iters, tie_last, narrow, table):
    """The read-side search as a plain Python loop over a {size: score} table (control flow of repeats.py:100-151 as
    strk_search.h states it), with the schedules of local_search_range the library offers (strk_search.h: LsrSchedule).
    Written from the description, not from the C++: (cn, score, n_explored), or "miss" when a size outside the table is needed,
    "empty" when nothing was scored."""
    to_explore = [(start - step, -1, True), (start + step, 1, True), (start, 0, True)]
    seen = {}
    floor1 = min(lsr, 1)
    cur = lsr
    n = 0
    while to_explore and n < max_iters:
        size, direction, seed = to_explore.pop()
        if size < 0:
            continue
        use = (lsr if seed else floor1) if narrow == 3 else cur
        if narrow == 1:
            cur = max(floor1, cur - 1)
        elif narrow == 2:
            cur = max(floor1, cur // 2)
        both = step > use
        w_lo = max(0, size - (use if (direction < 1 or both) else 0))
        w_hi = size + (use if (direction > -1 or both) else 0)
        szs = []
        for i in range(w_lo, w_hi + 1):
            if i not in table:
                return "miss"
            if i not in seen:
                seen[i] = table[i]
                n += 1
            szs.append((i, table[i]))
        mv = szs[0]
        for x in szs[1:]:
            if x[1] > mv[1] or (tie_last and x[1] == mv[1]):
                mv = x
        if mv[0] > size and (mv[0] + step) not in seen and mv[0] + step >= 0:
            to_explore.append((mv[0] + step, 1, False))
        if mv[0] < size and (mv[0] - step) not in seen and mv[0] - step >= 0:
            to_explore.append((mv[0] - step, -1, False))
    if not seen:
        return "empty"
    best = None
    for i, s in seen.items():                                  # insertion order: first (or last) maximum
        if best is None or s > best[1] or (tie_last and s == best[1]):
            best = (i, s)
    return best[0], best[1], n


# ---- realignment (strkit/call/realign.py) ---------------------------------------------------
def mutate(rng, seq, sub=0.01, indel=0.01, alpha=ALPHA_ACGT):
    out = []
    for ch in seq:
        x = rng.random()
        if x < sub:
            out.append(alpha[rng.integers(len(alpha))])
        elif x < sub + indel / 2:
            continue
        elif x < sub + indel:
            out.append(ch)
            out.append(alpha[rng.integers(len(alpha))])
        else:
            out.append(ch)
    return "".join(out)


def realign_pair(rng, n_ref, n_read, ins=0, dele=0, sub=0.01, indel=0.01, alpha=ALPHA_ACGT, wc=0.0):
    """A reference window of n_ref bases and a read of about n_read bases that contains a mutated copy of it
    (optionally with one large insertion / deletion in the middle, the soft-clip case of call_locus.py:860-865)."""
    ref = rand_seq(rng, n_ref, alpha)
    mid = n_ref // 2
    body = ref[:mid] + rand_seq(rng, ins, alpha) + ref[mid + dele:]
    body = mutate(rng, body, sub, indel, alpha)
    left = int(rng.integers(0, max(1, n_read - len(body)) + 1)) if n_read > len(body) else 0
    right = max(0, n_read - len(body) - left)
    read = rand_seq(rng, left, alpha) + body + rand_seq(rng, right, alpha)
    if wc > 0:
        read = "".join("X" if rng.random() < wc else ch for ch in read)
    return ref, read or "A"


def cigar_tuples(cig):
    return [(int(x) >> 4, "MIDNSHP=X"[int(x) & 15]) for x in cig]


_RESCORE = None   # (score matrix, byte -> symbol), from the oracle, once


def rescore_cigar(ref, read, cig, open_=7, ext=0):
    """Score of the alignment a CIGAR describes (s1 = ref window, s2 = read; leading D run is free)."""
    global _RESCORE
    if _RESCORE is None:
        _RESCORE = (oracle.matrix().astype(np.int64), np.array([oracle.lib().strk_o_encode(b) for b in range(256)], np.int64))
    M, enc = _RESCORE
    as_sym = lambda s: enc[np.frombuffer(s.encode("latin-1") if isinstance(s, str) else bytes(s), np.uint8)]   # noqa: E731
    a, b = as_sym(ref), as_sym(read)
    i = j = 0
    score = 0
    first = True
    for ln, op in cigar_tuples(cig):
        if op in "=X":
            if i + ln > len(a) or j + ln > len(b):
                raise IndexError("the CIGAR runs past a sequence")
            score += int(M[a[i:i + ln], b[j:j + ln]].sum())
            i += ln
            j += ln
        elif op == "I":
            score -= open_ + (ln - 1) * ext
            i += ln
        elif op == "D":
            if not (first and i == 0):
                score -= open_ + (ln - 1) * ext
            j += ln
        first = False
    return score, i, j


# rows of the call driver's shape without a device: the two-rank gather test and the codec test share them
def fake_rows(mine, ref):
    """Stands in for the device path in the CPU test: rows of the real shape with made-up read records."""
    from strkit_amd.frontend.call import CallOptions, _locus_dict, _locus_row
    rows, errors = [], []
    for blk in mine:
        for l in blk:
            if l.t_idx % 7 == 3:
                rows.append(_locus_dict(l))                    # a skipped locus (no reference data)
                continue
            if l.t_idx % 11 == 5:
                errors.append({"locus_index": l.t_idx, "error": "boom"})
                continue
            s_adj, e_adj = l.left_coord - (l.t_idx % 3), l.right_coord + (l.t_idx % 2)
            rd = {"ref_cn": 5 + l.t_idx, "left_coord_adj": s_adj, "right_coord_adj": e_adj, "ref_seq": ref.fetch(l.contig, s_adj, e_adj),
                  "ref_left_flank_seq": ref.fetch(l.contig, s_adj - 5, s_adj)}
            n = l.t_idx % 4
            reads = {f"read_{l.t_idx}_{k}" + "x" * (70 if k == 2 else 0): {"s": "+-"[k % 2], "cn": l.t_idx + k, "w": 1.0 / n,
                                                                       "sc": None if k == 1 else 1.5 + 0.125 * k, "sl": 30 + k,
                                                                       **({"realn": True} if k == 2 else {})} for k in range(n)}
            rows.append(_locus_row(l, rd, reads, CallOptions()))
    return rows, sum(len(r.get("reads") or {}) for r in rows), {"count_s": 0.1, "errors": errors}


def gloo_blocks():
    from strkit_amd.frontend.loci import Locus
    return [[Locus(10 * k + i + 1, f"l{10 * k + i}", "chr1", 200 + 100 * (10 * k + i), 200 + 100 * (10 * k + i) + 6 * (1 + (k * 7 + i) % 9), "CAG")
             for i in range(1 + k % 4)] for k in range(11)]


class FakeRef:
    seq = "ACGTTGCA" * 2000

    def fetch(self, contig, a, b):
        return self.seq[a:b]


def hip_runtime():
    """The HIP runtime the library itself is linked against (for a device buffer of a test's own)."""
    import ctypes
    import os

    import pytest

    from strkit_amd import _lib
    _lib.load()
    for name in ("libamdhip64.so", "libamdhip64.so.7", "libamdhip64.so.6", os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib", "libamdhip64.so")):
        try:
            return ctypes.CDLL(name)
        except OSError:
            continue
    pytest.fail("the HIP runtime library was not found")


# ---- HiFi-like loci, the resident-buffer entry point and the end of a context's band probation (shared by the band tests) ----
def hifi_seq(rng, n):
    return "".join(ALPHA_ACGT[i] for i in rng.integers(4, size=n))


def hifi_motif(rng, m):
    while True:
        s = hifi_seq(rng, m)
        if all(s != s[:p] * (m // p) for p in range(1, m) if m % p == 0):
            return s


def hifi_locus(rng, motif, nfl, ntr, nfr, n_reads):
    """Reads of exactly nfl + ntr + nfr bases: the tract is the motif repeated and cut at ntr bases, now and then with one
    substitution (a HiFi read's error rate); the flanks differ from read to read, so every read is an item of its own."""
    m = len(motif)
    reads = []
    for k in range(n_reads):
        tr = list((motif * (ntr // m + 1))[:ntr])
        if tr and k % 3 == 1:
            i = int(rng.integers(len(tr)))
            tr[i] = ALPHA_ACGT[(ALPHA_ACGT.index(tr[i]) + 1) % 4]
        reads.append((hifi_seq(rng, nfl), "".join(tr), hifi_seq(rng, nfr)))
    return motif, reads


def device_count(b, ctx, flags=15, **kw):
    """strk_count_loci_device on resident copies of the batch (device buffers of the test's own, through the HIP runtime)."""
    import ctypes as C

    from strkit_amd import _lib
    from strkit_amd.batch import make_params
    hip = hip_runtime()
    hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    hip.hipFree.argtypes = [C.c_void_p]
    assert hip.hipSetDevice(ctx.device) == 0
    held = []

    def dev(arr):
        arr = np.ascontiguousarray(arr)
        d = C.c_void_p()
        assert hip.hipMalloc(C.byref(d), max(arr.nbytes, 16)) == 0
        held.append(d)
        if arr.nbytes:
            assert hip.hipMemcpy(d, arr.ctypes.data, arr.nbytes, 1) == 0   # hipMemcpyHostToDevice
        return d.value
    try:
        dt = dict(seqs=np.uint8, seq_off=np.int64, nfl=np.int32, ntr=np.int32, nfr=np.int32, est_cn=np.int32, read_off=np.int32,
                  motifs=np.uint8, motif_off=np.int32)
        sb = _lib.StrkBatch(n_reads=b.n_reads, n_loci=b.n_loci, **{k: dev(np.asarray(getattr(b, k), t)) for k, t in dt.items()})
        host = np.zeros((4, b.n_reads), np.int32)
        d_out = dev(host)
        p = make_params(end_flags=flags, **kw)
        st = _lib.StrkStats()
        _lib.check(_lib.load().strk_count_loci_device(ctx.handle, C.byref(sb), C.byref(p), *[C.c_void_p(d_out + 4 * k * b.n_reads) for k in range(4)],
                                                      None, C.byref(st)))
        assert hip.hipMemcpy(host.ctypes.data, d_out, host.nbytes, 2) == 0   # hipMemcpyDeviceToHost
    finally:
        for d in held:
            hip.hipFree(d)
    return {k: host[j] for j, k in enumerate(("cn", "score", "n_iters", "start"))}, st.as_dict()


def end_probation(ctx):
    """A context's first calls band only their first 2 048 reads: one clean call of 90 reads ends that."""
    from strkit_amd.batch import count_loci
    rng = np.random.default_rng(1900)
    _, st = count_loci(LocusBatch.from_reads([hifi_locus(rng, hifi_motif(rng, 4), 60, 80, 60, 30) for _ in range(3)]), ctx=ctx, with_stats=True)
    assert st["n_band_reads"] == 90 and st["n_band_fallback"] < 45
