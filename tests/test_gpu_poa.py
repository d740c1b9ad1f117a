"""GPU: strk_consensus (k_poa) against the CPU restatement (tests/poa_restatement.py), exactly: method, index, offsets and
bytes of every group are integers and bytes, so there is no tolerance."""
import ctypes as C
import functools

import numpy as np
import pytest

import consensus_restatement as BR
import poa_restatement as P
from helpers import hip_runtime
from strkit_amd import _lib
from strkit_amd import consensus as CS
from strkit_amd._groups import pack_groups

pytestmark = pytest.mark.gpu

VECTORS, EMPTY_VECTORS, mutate = P.VECTORS, P.EMPTY_VECTORS, P.mutate

METHOD = {"none": CS.NONE, "single": CS.SINGLE, "best_rep": CS.BEST_REP, "poa": CS.POA}
ALPHABETS = (b"A", b"AC", b"ACGT", b"ACGTN", bytes(range(256)))
SPAN = 256   # columns one pass of the workgroup covers (kPoaThreads); a string of L bytes has L + 1 columns


def _rand(rng, alpha, n):
    return bytes(alpha[int(k)] for k in rng.integers(0, len(alpha), n))


def _expect(groups, **kw):
    return [P.consensus(g, **kw) for g in groups]


def _assert_equal(out, exp, what):
    assert out["seqs"] is not None, what
    text = out["seqs"].tobytes()
    off = out["seq_off"].tolist()
    assert off[0] == 0 and len(off) == len(exp) + 1
    for g, (idx, method, seq, _limited) in enumerate(exp):
        got = (int(out["index"][g]), int(out["method"][g]), text[off[g]:off[g + 1]])
        assert got == (idx, METHOD[method], seq or b""), (what, g, got, (idx, method, seq))
    assert off[-1] == len(text)


@functools.lru_cache(maxsize=None)
def _corpus():
    rng = np.random.default_rng(20261017)
    groups = [g.split() for g, _e, _n in VECTORS] + [list(g) for g, _e in EMPTY_VECTORS]
    groups = [[s.encode() if isinstance(s, str) else s for s in g] for g in groups]
    for k in range(60):          # unrelated strings: sizes 0 .. 30, lengths 0 .. 130, every alphabet
        alpha = ALPHABETS[k % 5]
        n = 30 if k in (7, 22) else int(rng.integers(0, 9))
        groups.append([_rand(rng, alpha, int(rng.integers(0, 131))) for _ in range(n)])
    for k in range(40):          # HiFi-like: many exact duplicates
        alpha = ALPHABETS[(k % 4) + 1]
        hap = _rand(rng, alpha, int(rng.integers(5, 131)))
        groups.append([mutate(rng, hap, 0.005, 0.7, alpha) for _ in range(int(rng.integers(2, 31)))])
    for k in range(30):          # noisy reads of one haplotype
        hap = _rand(rng, b"ACGT", int(rng.integers(5, 120)))
        groups.append([mutate(rng, hap, 0.06, 0.7) for _ in range(int(rng.integers(2, 31)))])
    for _ in range(20):          # two haplotypes mixed
        h1 = _rand(rng, b"ACGT", int(rng.integers(10, 120)))
        h2 = mutate(rng, h1, 0.1)
        groups.append([mutate(rng, h1 if rng.random() < 0.5 else h2, 0.01) for _ in range(int(rng.integers(4, 31)))])
    for _ in range(12):          # groups holding empty strings
        g = [mutate(rng, _rand(rng, b"ACGT", int(rng.integers(1, 20))), 0.1) for _ in range(int(rng.integers(1, 8)))]
        for _ in range(int(rng.integers(1, 6))):
            g.insert(int(rng.integers(0, len(g) + 1)), b"")
        groups.append(g)
    groups += [[], [b""], [b"", b""], [b"A"], [b"ACGT"] * 7]
    return tuple(tuple(g) for g in groups)


@functools.lru_cache(maxsize=None)
def _corpus_expect():
    return _expect(_corpus())


def test_hand_vectors(gpu_ctx):
    groups = [[s.encode() for s in g.split()] for g, _e, _n in VECTORS] + [list(g) for g, _e in EMPTY_VECTORS]
    want = [e.encode() for _g, e, _n in VECTORS] + [e for _g, e in EMPTY_VECTORS]
    out = CS.consensus_packed(*pack_groups(groups)[:3], seqs=pack_groups(groups)[3], ctx=gpu_ctx)
    off = out["seq_off"].tolist()
    text = out["seqs"].tobytes()
    assert [text[off[g]:off[g + 1]] for g in range(len(groups))] == want
    assert (out["method"] == CS.POA).all() and (out["index"] == -1).all()
    assert CS.consensus([g.split() for g, _e, _n in VECTORS], ctx=gpu_ctx) == [(e, "poa") for _g, e, _n in VECTORS]
    assert CS.consensus_seq(["CAGCAG", "CAGCAT", "CAGCAT"], ctx=gpu_ctx, method="poa") == ("CAGCAT", "poa")
    assert CS.consensus_seq(["CAGCAG", "CAGCAT", "CAGCAT"], poa=True, ctx=gpu_ctx) == ("CAGCAT", "best_rep")
    assert CS.consensus_seq([], ctx=gpu_ctx, method="poa") is None
    assert CS.consensus_seq(["CAG", "CAG"], ctx=gpu_ctx, method="poa") == ("CAG", "single")
    assert CS.METHOD_NAMES[CS.POA] == "poa"


def test_corpus_equals_restatement(gpu_ctx):
    groups = _corpus()
    assert len(groups) >= 150 and max(len(g) for g in groups) == 30
    off, starts, lens, buf = pack_groups(groups)
    out, stats = CS.consensus_packed(off, starts, lens, seqs=buf, ctx=gpu_ctx, with_stats=True)
    exp = _corpus_expect()
    _assert_equal(out, exp, "corpus")
    assert {e[1] for e in exp} == {"none", "single", "poa"}
    assert stats["kernel_ms"] > 0 and stats["n_fallback"] == 0 and stats["n_sub_batches"] == 1 and stats["n_dp_launches"] >= 2
    cells = sum(P.build(g).cells for g, e in zip(groups, exp) if e[1] == "poa")
    assert stats["dp_cells"] == cells


def test_lengths_around_the_wave_and_the_workgroup_span(gpu_ctx):
    rng = np.random.default_rng(4)
    groups = []
    for L in (62, 63, 64, 65, SPAN - 2, SPAN - 1, SPAN, SPAN + 1, 2 * SPAN - 1, 2 * SPAN, 2 * SPAN + 1):
        hap = _rand(rng, b"ACGT", L + 3)
        groups.append([hap[:L], mutate(rng, hap[:L], 0.05, 0.0), hap[:L - 1], hap[:L + 1], mutate(rng, hap[:L], 0.05)])
        groups.append([bytes(s) for s in (hap[:L], bytes(reversed(hap[:L])), mutate(rng, hap[:L], 0.03, 0.0))])
    lens = {len(s) for g in groups for s in g}
    assert {63, 64, 65, SPAN - 2, SPAN - 1, SPAN, 2 * SPAN - 1, 2 * SPAN} <= lens   # SPAN - 1 bytes fill one pass exactly
    _assert_equal(CS.consensus_packed(*pack_groups(groups)[:3], seqs=pack_groups(groups)[3], ctx=gpu_ctx), _expect(groups), "spans")


def test_graph_shapes(gpu_ctx):
    """A node with three and more predecessors, a column of four nodes, several sources and several sinks, 250 distinct strings,
    and strings of about 2 100 bases."""
    rng = np.random.default_rng(6)
    fan = [b"AXB", b"AYB", b"AZB", b"AWB", b"AWB"]
    ends = [b"ACGTAC", b"GCGTAC", b"ACGTAG", b"TCGTAT", b"TCGTAT"]
    gr = P.build(fan)
    assert max(len(p) for p in gr.pred) >= 4 and max(len(a) for a in gr.aligned) == 3
    gr = P.build(ends)
    assert sum(1 for p in gr.pred if not p) >= 3 and sum(1 for n in gr.n_succ if n == 0) >= 3
    many = []
    while len(many) < 250:
        s = _rand(rng, b"ACGT", int(rng.integers(0, 25)))
        if s not in many:
            many.append(s)
    hap = _rand(rng, b"ACGT", 2100)
    long_group = [mutate(rng, hap, 0.02) for _ in range(6)]
    assert all(2000 < len(s) < 2200 for s in long_group)
    groups = [fan, ends, many, long_group]
    out, stats = CS.consensus_packed(*pack_groups(groups)[:3], seqs=pack_groups(groups)[3], ctx=gpu_ctx, with_stats=True)
    exp = _expect(groups)
    _assert_equal(out, exp, "shapes")
    assert [e[1] for e in exp] == ["poa"] * 4 and stats["n_fallback"] == 0


def test_median_rule(gpu_ctx):
    g = [b"CAGCAG", b"CAGCAT", b"CAGCAT", b"CAG", b"CAGCAGCAGC"]      # ascending 3 6 6 6 10: the median is 6
    same = [b"CAGCAGCAG"] * 3
    for mdn, method in ((6, "poa"), (5, "best_rep"), (0, "best_rep"), (5000, "poa")):
        out, stats = CS.consensus_packed(*pack_groups([g, same, []])[:3], seqs=pack_groups([g, same, []])[3], max_mdn_poa_length=mdn,
                                         ctx=gpu_ctx, with_stats=True)
        exp = _expect([g, same, []], max_mdn_poa_length=mdn)
        assert [e[1] for e in exp] == [method, "single", "none"]
        _assert_equal(out, exp, f"median {mdn}")
        assert stats["n_fallback"] == 0


def test_node_limit_and_launch_cutting(gpu_ctx):
    groups = list(_corpus()[:70])
    off, starts, lens, buf = pack_groups(groups)
    ref = CS.consensus_packed(off, starts, lens, seqs=buf, ctx=gpu_ctx)
    limit = 60
    exp = _expect(groups, node_limit=limit)
    n_limited = sum(e[3] for e in exp)
    n_poa = sum(e[1] == "poa" for e in exp)
    assert n_limited >= 5 and n_poa >= 10
    out, stats = CS.consensus_packed(off, starts, lens, seqs=buf, ctx=gpu_ctx, node_limit=limit, with_stats=True)
    _assert_equal(out, exp, "node limit")
    assert stats["n_fallback"] == n_limited
    rep = CS.best_representatives_packed(off, starts, lens, seqs=buf, ctx=gpu_ctx)
    for g, e in enumerate(exp):
        if e[3]:
            assert out["method"][g] == CS.BEST_REP and out["index"][g] == rep["index"][g] == BR.best_representative(groups[g])[0]
    # a string beyond the kernel's rows: the same rule
    rng = np.random.default_rng(8)
    hap = _rand(rng, b"ACGT", CS.MAX_POA_LEN + 1)
    edge = [[hap, hap[:-1], hap[:-1]], [hap[:-1], hap[:-2], hap[:40]], [hap, hap]]
    o2, s2 = CS.consensus_packed(*pack_groups(edge)[:3], seqs=pack_groups(edge)[3], ctx=gpu_ctx, with_stats=True)
    e2 = _expect(edge)
    assert [e[1] for e in e2] == ["best_rep", "poa", "single"] and e2[0][3]
    _assert_equal(o2, e2, "row limit")
    assert s2["n_fallback"] == 1
    # the same call with a workspace that holds one group: one launch per group the kernel takes, the same answers
    cut, st_cut = CS.consensus_packed(off, starts, lens, seqs=buf, ctx=gpu_ctx, workspace_bytes=1, with_stats=True)
    n_kernel = sum(1 for g in groups if len(g) > 0)
    assert st_cut["n_sub_batches"] == n_kernel
    for key in ("index", "method", "seq_off", "seqs"):
        assert np.array_equal(cut[key], ref[key]), key


def test_slices_host_and_device_and_the_size_query(gpu_ctx):
    rng = np.random.default_rng(9)
    groups = list(_corpus()[40:100])
    exp = _corpus_expect()[40:100]
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
    out = CS.consensus_packed(off, starts, lens, seqs=buf, ctx=gpu_ctx)
    _assert_equal(out, exp, "host slices")
    total = int(out["seq_off"][-1])
    assert total > 100
    hip = hip_runtime()
    dev = C.c_void_p()
    assert hip.hipSetDevice(gpu_ctx.device) == 0 and hip.hipMalloc(C.byref(dev), C.c_size_t(buf.shape[0])) == 0
    try:
        assert hip.hipMemcpy(dev, C.c_void_p(buf.ctypes.data), C.c_size_t(buf.shape[0]), 1) == 0   # hipMemcpyHostToDevice
        o2 = CS.consensus_packed(off, starts, lens, d_seqs=dev.value, n_seq_bytes=buf.shape[0], ctx=gpu_ctx)
        _assert_equal(o2, exp, "device slices")
        with pytest.raises(_lib.StrkError):     # a host address is not device memory
            CS.consensus_packed(off, starts, lens, d_seqs=buf.ctypes.data, n_seq_bytes=buf.shape[0], ctx=gpu_ctx)
    finally:
        hip.hipFree(dev)
    # the size query, a buffer one byte short, the exact size
    q = CS.consensus_packed(off, starts, lens, seqs=buf, ctx=gpu_ctx, cap=0)
    assert q["seqs"] is None and np.array_equal(q["seq_off"], out["seq_off"]) and np.array_equal(q["method"], out["method"])
    short = CS.consensus_packed(off, starts, lens, seqs=buf, ctx=gpu_ctx, cap=total - 1)
    assert short["seqs"] is None and np.array_equal(short["seq_off"], out["seq_off"]) and np.array_equal(short["index"], out["index"])
    exact = CS.consensus_packed(off, starts, lens, seqs=buf, ctx=gpu_ctx, cap=total)
    assert np.array_equal(exact["seqs"], out["seqs"])
    # overlapping slices of one string: prefixes of a tract
    s = _rand(rng, b"ACGT", 200)
    pre = [200, 199, 150, 200, 64, 0, 199]
    o3 = CS.consensus_packed([0, len(pre)], [0] * len(pre), pre, seqs=np.frombuffer(s, dtype=np.uint8), ctx=gpu_ctx)
    _assert_equal(o3, _expect([[s[:k] for k in pre]]), "prefixes")


def test_invalid_input_is_refused_and_the_context_stays_usable(fresh_ctx):
    ctx = fresh_ctx
    good = ([0, 3], [0, 3, 6], [3, 3, 3], np.frombuffer(b"CAGCATCAT", dtype=np.uint8))

    def refused(off, starts, lens, buf, **kw):
        with pytest.raises(_lib.StrkError) as e:
            CS.consensus_packed(off, starts, lens, seqs=buf, ctx=ctx, **kw)
        assert e.value.code == _lib.STRK_E_INVALID and "strk_consensus" in str(e.value)
        out = CS.consensus_packed(*good[:3], seqs=good[3], ctx=ctx)   # the context still works
        assert out["method"].tolist() == [CS.POA] and out["seqs"].tobytes() == b"CAT"

    buf = np.frombuffer(b"A" * 300, dtype=np.uint8)
    refused([0, 251], [0] * 251, [1] * 251, buf)                       # group size > 250
    refused([0, 1], [0], [65536], np.zeros(70000, np.uint8))          # sequence length > 65 535
    refused([0, 1], [0], [-1], buf)                                    # negative length
    refused([0, 2], [0, 298], [3, 3], buf)                             # a slice past the end of the buffer
    refused([0, 1], [-1], [3], buf)                                    # a slice before its start
    refused([0, 2], [0, 0], [3, 3], buf, n_seq_bytes=2)                # ... of the bytes declared
    refused([0, 2, 1, 3], [0, 1, 2], [1, 1, 1], buf)                   # group_off not ascending
    refused([1, 2], [0, 0], [1, 1], buf)                               # group_off[0] != 0
    refused([0, 1], [0], [3], buf, max_mdn_poa_length=-1)
    refused([0, 1], [0], [3], buf, node_limit=CS.MAX_POA_NODES + 1)
    refused([0, 1], [0], [3], buf, cap=-1)
    out = CS.consensus_packed([0, 250], [0] * 250, [7] * 250, seqs=buf, ctx=ctx)
    assert out["index"].tolist() == [0] and out["method"].tolist() == [CS.SINGLE] and out["seqs"].tobytes() == b"A" * 7
    out = CS.consensus_packed([0], [], [], seqs=buf, ctx=ctx)
    assert out["index"].shape == (0,) and out["seq_off"].tolist() == [0]
