"""GPU: strk_best_representatives (k_best_rep) against the CPU restatement (tests/consensus_restatement.py), exactly:
index, method and distance sum of every group are integers, so there is no tolerance."""
import ctypes as C

import numpy as np
import pytest

import consensus_restatement as R
from helpers import hip_runtime
from strkit_amd import _lib
from strkit_amd import consensus as CS
from strkit_amd._groups import pack_groups

pytestmark = pytest.mark.gpu

METHOD = {"none": CS.NONE, "single": CS.SINGLE, "best_rep": CS.BEST_REP}
ALPHABETS = (b"A", b"AC", b"ACGT", b"ACGTN")


def _rand(rng, alpha, n):
    return bytes(alpha[int(k)] for k in rng.integers(0, len(alpha), n))


def _mutate(rng, s, rate, alpha=b"ACGT", indel=0.5):
    """Every position is hit with probability `rate`: a substitution, or (share `indel`) an insertion or a deletion."""
    out = bytearray()
    hit = rng.random(len(s)) < rate
    for i, ch in enumerate(s):
        if hit[i]:
            r = rng.random()
            if r < indel / 2:
                continue
            if r < indel:
                out.append(alpha[int(rng.integers(0, len(alpha)))])
                out.append(ch)
                continue
            out.append(alpha[int(rng.integers(0, len(alpha)))])
        else:
            out.append(ch)
    return bytes(out)


def _hifi(rng, n_reads, length, rate, alpha=b"ACGT"):
    hap = _rand(rng, alpha, length)
    return [_mutate(rng, hap, rate, alpha) for _ in range(n_reads)]


def _corpus():
    rng = np.random.default_rng(20261016)
    groups = []
    # every size 0 .. 250 once: HiFi-like, many exact duplicates
    for n in range(0, 251):
        groups.append(_hifi(rng, n, int(rng.integers(20, 90)), float(rng.uniform(0.001, 0.01)) * 20 / max(n, 20)))
    # the word crossings by construction, in every alphabet
    for L in (0, 1, 2, 31, 32, 33, 63, 64, 65, 66, 127, 128, 129, 191, 192, 193, 255, 256, 257, 300):
        for alpha in ALPHABETS:
            base = _rand(rng, alpha, L)
            g = [base, _mutate(rng, base, 0.05, alpha), _mutate(rng, base, 0.2, alpha), _rand(rng, alpha, L)]
            if L:
                g.append(base[:-1])
                g.append(base + alpha[:1])
            groups.append(g)
    # unrelated strings of random lengths 0 .. 300 (all pairs are real work), small alphabets included
    for _ in range(500):
        alpha = ALPHABETS[int(rng.integers(0, 4))]
        groups.append([_rand(rng, alpha, int(rng.integers(0, 301))) for _ in range(int(rng.integers(2, 7)))])
    # HiFi-like groups of the usual depth
    for _ in range(1100):
        groups.append(_hifi(rng, int(rng.integers(2, 30)), int(rng.integers(10, 300)), float(rng.uniform(0.001, 0.003))))
    # two haplotypes mixed
    for _ in range(300):
        L = int(rng.integers(10, 250))
        h1 = _rand(rng, b"ACGT", L)
        h2 = _mutate(rng, h1, 0.1)
        n = int(rng.integers(4, 30))
        groups.append([_mutate(rng, h1 if rng.random() < 0.5 else h2, 0.002) for _ in range(n)])
    # all identical, groups holding empty strings, raw bytes beyond eight values (the wide alphabet path), case
    for _ in range(60):
        groups.append([_rand(rng, b"ACGT", int(rng.integers(0, 200)))] * int(rng.integers(1, 30)))
    for _ in range(60):
        g = _hifi(rng, int(rng.integers(2, 12)), int(rng.integers(1, 30)), 0.05)
        g.insert(int(rng.integers(0, len(g) + 1)), b"")
        if rng.random() < 0.5:
            g.append(b"")
        groups.append(g)
    groups.append([b"", b"", b""])
    groups.append([b"", b"A"])
    for _ in range(60):
        alpha = bytes(range(256)) if rng.random() < 0.5 else b"ACGTNacgtn-*"
        base = _rand(rng, alpha, int(rng.integers(1, 300)))
        groups.append([_mutate(rng, base, 0.05, alpha) for _ in range(int(rng.integers(2, 10)))])
    # two large groups of distinct strings: thousands of pairs in one workgroup
    groups.append([_rand(rng, b"ACGT", int(rng.integers(0, 24))) for _ in range(250)])
    groups.append(_hifi(rng, 100, 40, 0.1))
    # ties that must go to the first index
    groups.append([b"AAAA", b"AAAT"])
    groups.append([b"AAAT", b"AAAA", b"AAAT", b"AAAA"])
    return groups


def _expect(groups):
    exp = [R.best_representative(g) for g in groups]
    return (np.array([e[0] for e in exp], np.int32), np.array([METHOD[e[1]] for e in exp], np.int32),
            np.array([e[2] for e in exp], np.int64))


def _assert_equal(out, exp, what):
    idx, meth, dist = exp
    bad = np.flatnonzero((out["index"] != idx) | (out["method"] != meth) | (out["dist_sum"] != dist))
    assert bad.size == 0, (what, bad[:10].tolist(), [(int(out["index"][b]), int(out["method"][b]), int(out["dist_sum"][b]),
                                                     int(idx[b]), int(meth[b]), int(dist[b])) for b in bad[:10]])


def test_corpus_equals_restatement(gpu_ctx):
    groups = _corpus()
    assert len(groups) > 2000 and {len(g) for g in groups} >= set(range(251))
    off, starts, lens, buf = pack_groups(groups)
    out, stats = CS.best_representatives_packed(off, starts, lens, seqs=buf, ctx=gpu_ctx, with_stats=True)
    _assert_equal(out, _expect(groups), "corpus")
    assert stats["kernel_ms"] > 0
    # the list interface on a part of it
    part = [g for g in groups[:400] if all(max(s, default=0) < 128 for s in g)]
    got = CS.best_representatives(part, ctx=gpu_ctx)
    for g, (seq, method) in zip(part, got):
        i, m, _ = R.best_representative(g)
        assert (seq, method) == ((None, "none") if i < 0 else (g[i].decode("ascii"), m))
    assert CS.consensus_seq([], ctx=gpu_ctx) is None
    assert CS.consensus_seq(["CAGCAG", "CAGCAG"], ctx=gpu_ctx) == ("CAGCAG", "single")
    assert CS.consensus_seq(["CAGCAG", "CAGCAT", "CAGCAT"], max_mdn_poa_length=500, poa=True, ctx=gpu_ctx) == ("CAGCAT", "best_rep")


def _long_groups():
    rng = np.random.default_rng(5)
    groups = []
    base = _rand(rng, b"ACGT", 2048)
    groups.append([_mutate(rng, base, 0.02) for _ in range(20)])                  # 20 strings of about 2 kb
    for L, n, rate in ((4096, 5, 0.03), (8192, 6, 0.02), (12288, 5, 0.03)):      # around multiples of 4 096: several passes
        base = _rand(rng, b"ACGT", L + 65)
        g = [base[:L - 1], base[:L], base[:L + 1], base[:L + 64]][:n - 1]
        g = [bytes(_mutate(rng, s, rate, indel=0.0)) for s in g]                  # substitutions keep the exact lengths
        while len(g) < n:
            g.append(_mutate(rng, base[:L], rate))                                # indels: lengths near L
        groups.append(g)
    base = _rand(rng, b"ACGTN", 12000)
    groups.append([_mutate(rng, base[:k], 0.02, b"ACGTN") for k in (4031, 4160, 6400, 8191, 10000, 12000)])
    return groups


def test_long_groups_equal_restatement(gpu_ctx):
    groups = _long_groups()
    lens = sorted(len(s) for g in groups for s in g)
    assert lens[-1] > 3 * 4096 - 200 and any(4096 < n for n in lens)
    off, starts, ln, buf = pack_groups(groups)
    out = CS.best_representatives_packed(off, starts, ln, seqs=buf, ctx=gpu_ctx)
    _assert_equal(out, _expect(groups), "long")
    assert (out["method"] == CS.BEST_REP).all()


def test_slices_host_and_device(gpu_ctx):
    """The same strings addressed through (seq_start, seq_len) into a buffer with other bytes around them."""
    rng = np.random.default_rng(9)
    groups = _corpus()[230:330] + [_hifi(rng, 6, 5000, 0.01)]
    exp = _expect(groups)
    parts, starts, lens = [], [], []
    pos = 0
    for g in groups:
        for s in g:
            pad = _rand(rng, b"ACGTX", int(rng.integers(0, 40)))
            parts += [pad, s]
            starts.append(pos + len(pad))
            lens.append(len(s))
            pos += len(pad) + len(s)
    parts.append(b"TAIL")
    buf = np.frombuffer(b"".join(parts), dtype=np.uint8)
    off = np.zeros(len(groups) + 1, np.int32)
    np.cumsum([len(g) for g in groups], out=off[1:])
    out = CS.best_representatives_packed(off, starts, lens, seqs=buf, ctx=gpu_ctx)
    _assert_equal(out, exp, "host slices")
    hip = hip_runtime()
    dev = C.c_void_p()
    assert hip.hipSetDevice(gpu_ctx.device) == 0 and hip.hipMalloc(C.byref(dev), C.c_size_t(buf.shape[0])) == 0
    try:
        assert hip.hipMemcpy(dev, C.c_void_p(buf.ctypes.data), C.c_size_t(buf.shape[0]), 1) == 0   # hipMemcpyHostToDevice
        out = CS.best_representatives_packed(off, starts, lens, d_seqs=dev.value, n_seq_bytes=buf.shape[0], ctx=gpu_ctx)
        _assert_equal(out, exp, "device slices")
        with pytest.raises(_lib.StrkError):     # a host address is not device memory
            CS.best_representatives_packed(off, starts, lens, d_seqs=buf.ctypes.data, n_seq_bytes=buf.shape[0], ctx=gpu_ctx)
    finally:
        hip.hipFree(dev)
    # overlapping slices of one string: prefixes of a tract
    s = _rand(rng, b"ACGT", 200)
    pre = [200, 199, 150, 200, 64, 0]
    out = CS.best_representatives_packed([0, len(pre)], [0] * len(pre), pre, seqs=np.frombuffer(s, dtype=np.uint8), ctx=gpu_ctx)
    _assert_equal(out, _expect([[s[:k] for k in pre]]), "prefixes")


def test_invalid_input_is_refused_and_the_context_stays_usable(fresh_ctx):
    ctx = fresh_ctx
    good = ([0, 2], [0, 3], [3, 3], np.frombuffer(b"CAGCAT", dtype=np.uint8))

    def refused(off, starts, lens, buf, **kw):
        with pytest.raises(_lib.StrkError) as e:
            CS.best_representatives_packed(off, starts, lens, seqs=buf, ctx=ctx, **kw)
        assert e.value.code == _lib.STRK_E_INVALID and len(str(e.value)) > 30
        out = CS.best_representatives_packed(*good[:3], seqs=good[3], ctx=ctx)   # the context still works
        assert out["index"].tolist() == [0] and out["method"].tolist() == [CS.BEST_REP] and out["dist_sum"].tolist() == [1]

    buf = np.frombuffer(b"A" * 300, dtype=np.uint8)
    refused([0, 251], [0] * 251, [1] * 251, buf)                       # group size > 250
    refused([0, 1], [0], [65536], np.zeros(70000, np.uint8))          # sequence length > 65 535
    refused([0, 1], [0], [-1], buf)                                    # negative length
    refused([0, 2], [0, 298], [3, 3], buf)                             # a slice past the end of the buffer
    refused([0, 1], [-1], [3], buf)                                    # a slice before its start
    refused([0, 2], [0, 0], [3, 3], buf, n_seq_bytes=2)                # ... of the bytes declared
    refused([0, 2, 1, 3], [0, 1, 2], [1, 1, 1], buf)                   # group_off not ascending
    refused([1, 2], [0, 0], [1, 1], buf)                               # group_off[0] != 0
    # 250 sequences of 65 535 bytes are legal limits (not run: the limits are checked, the work is not the point)
    out = CS.best_representatives_packed([0, 250], [0] * 250, [7] * 250, seqs=buf, ctx=ctx)
    assert out["index"].tolist() == [0] and out["method"].tolist() == [CS.SINGLE]
    out = CS.best_representatives_packed([0], [], [], seqs=buf, ctx=ctx)
    assert out["index"].shape == (0,)
