"""GPU: strk_count_kmers (k_kmers_hash, k_kmers_sort) against the CPU restatement (tests/kmers_restatement.py), exactly: every
entry's offset, count and order are integers, so there is no tolerance."""
import ctypes as C

import numpy as np
import pytest

import kmers_restatement as R
from helpers import hip_runtime
from strkit_amd import _lib
from strkit_amd import kmers as KM
from strkit_amd._groups import pack_groups

pytestmark = pytest.mark.gpu

ALPHABETS = {1: b"A", 2: b"AC", 4: b"ACGT", 5: b"ACGTN", 16: bytes(range(0x70, 0x80)) , 256: bytes(range(256))}


def _rand(rng, alpha, n):
    return np.frombuffer(alpha, np.uint8)[rng.integers(0, len(alpha), n)].tobytes()


def _mutate(rng, s, rate, alpha=b"ACGT", indel=0.5):
    out = bytearray()
    hit = rng.random(len(s)) < rate
    for i, ch in enumerate(s):
        if hit[i]:
            r = rng.random()
            if r < indel / 2:
                continue
            out.append(alpha[int(rng.integers(0, len(alpha)))])
            if r < indel:
                out.append(ch)
        else:
            out.append(ch)
    return bytes(out)


def _tract(rng, motif, copies, rate):
    return _mutate(rng, motif * copies, rate)


def _check(groups, ks, ctx, **kw):
    """Library == restatement for every group: entry offsets, first-occurrence offsets, counts, in order."""
    group_off, starts, lens, buf = pack_groups(groups)
    ks = np.asarray(ks, np.int32)
    out, st = KM.count_kmers_packed(group_off, starts, lens, ks, seqs=buf, ctx=ctx, with_stats=True, **kw)
    eo, pos, cnt = R.count_packed(group_off, starts, lens, ks, buf.tobytes())
    assert out["entry_off"].tolist() == eo
    assert out["pos"].tolist() == pos
    assert out["count"].tolist() == cnt
    for g, grp in enumerate(groups):      # conservation
        assert int(out["count"][eo[g]:eo[g + 1]].sum()) == R.n_windows(grp, int(ks[g]))
    return out, st


def test_hand_worked(gpu_ctx):
    assert KM.count_kmers([["CAG" * 5]], 3, ctx=gpu_ctx) == [{b"AGC": 4, b"CAG": 5, b"GCA": 4}]
    got = KM.count_kmers([["CAG" * 5], [], ["ACCA"], ["ACCA"], ["ACCA"], ["", "A", ""], ["aAaA"], [b"\xffA\x00\x7f\x80"]],
                         [3, 3, 1, 4, 5, 1, 1, 1], ctx=gpu_ctx)
    assert [list(d.items()) for d in got] == [
        [(b"AGC", 4), (b"CAG", 5), (b"GCA", 4)], [], [(b"A", 2), (b"C", 2)], [(b"ACCA", 1)], [], [(b"A", 1)],
        [(b"A", 2), (b"a", 2)], [(b"\x00", 1), (b"A", 1), (b"\x7f", 1), (b"\x80", 1), (b"\xff", 1)]]
    assert KM.count_kmers([], 3, ctx=gpu_ctx) == []


def test_group_sizes_0_to_250(gpu_ctx):
    rng = np.random.default_rng(20261017)
    groups, ks = [], []
    for n in range(0, 251):
        motif = _rand(rng, b"ACGT", int(rng.integers(2, 7)))
        groups.append([_tract(rng, motif, int(rng.integers(0, 40)), 0.01) for _ in range(n)])
        ks.append(len(motif))
    _, st = _check(groups, ks, gpu_ctx)
    assert st["dp_cells"] == sum(R.n_windows(g, k) for g, k in zip(groups, ks))


def test_lengths_window_lengths_and_alphabets(gpu_ctx):
    """Lengths 0 .. 300 with lengths around k, k 1 .. 40, every alphabet: one 64-bit key where k * bits <= 64 (bits = 1, 1, 2, 3,
    4, 8 for the six alphabets), the general path beyond; both sides of the threshold for every alphabet."""
    rng = np.random.default_rng(7)
    groups, ks = [], []
    for sigma, alpha in ALPHABETS.items():
        bits = max(1, (sigma - 1).bit_length())
        edge = 64 // bits
        for k in sorted(set(list(range(1, 41)) + [edge - 1, edge, edge + 1, edge + 2])):
            if k < 1:
                continue
            lens = [0, 1, k - 1, k, k + 1, 2 * k, int(rng.integers(0, 301)), int(rng.integers(0, 301)), 300]
            g = [_rand(rng, alpha, max(n, 0)) for n in lens]
            # make sure the whole alphabet is in the group (the bits per code are those of the set of byte values present)
            g.append(alpha)
            g.append(g[3])                                        # a duplicate string
            groups.append(g)
            ks.append(k)
    out, st = _check(groups, ks, gpu_ctx)
    assert st["n_miss_reads"] > 0                                 # groups on the general path ...
    assert st["n_miss_reads"] < len(groups)                       # ... and groups with packed keys


def test_key_of_all_ones(gpu_ctx):
    """k * bits = 64 exactly and a window that packs to 64 one-bits: 16 letters, k = 16, a run of the largest letter; 2 letters, k = 64."""
    alpha = ALPHABETS[16]
    top = alpha[-1:]
    rng = np.random.default_rng(3)
    g16 = [alpha, top * 40, _rand(rng, alpha, 100) + top * 20, top * 16]
    g2 = [b"AC", b"C" * 70, b"C" * 64 + b"A" + b"C" * 64, b"A" * 64]
    _, st = _check([g16, g2, g16 + g16], [16, 64, 16], gpu_ctx)
    assert st["n_miss_reads"] == 0


def test_one_long_window(gpu_ctx):
    rng = np.random.default_rng(5)
    base = _rand(rng, b"ACGT", 300)
    g = [base, base, _rand(rng, b"ACGT", 300), base[:299], base + b"A", b"A" + base]
    _, st = _check([g, [b"CAG" * 200], [b"A" * 299]], [300, 300, 300], gpu_ctx)
    assert st["n_miss_reads"] == 2


def test_read_shapes(gpu_ctx):
    """HiFi-like (0.1-0.3 % errors) and ONT-like (5-10 %) tracts at the depth of a locus, k = the motif's length."""
    rng = np.random.default_rng(99)
    groups, ks = [], []
    for i in range(600):
        motif = _rand(rng, b"ACGT", int(rng.integers(1, 7)))
        rate = float(rng.uniform(0.001, 0.003)) if i % 2 == 0 else float(rng.uniform(0.05, 0.1))
        hap = [int(rng.integers(3, 100)) for _ in range(2)]
        groups.append([_tract(rng, motif, hap[int(rng.integers(0, 2))], rate) for _ in range(int(rng.integers(1, 40)))])
        ks.append(len(motif))
    _check(groups, ks, gpu_ctx)


def _long_groups(rng, n_groups, rate):
    groups = []
    for _ in range(n_groups):
        motif = _rand(rng, b"ACGT", 6)
        groups.append([_tract(rng, motif, int(rng.integers(4000, 12000)) // 6, rate) for _ in range(20)])
    return groups


def test_long_reads_spill_and_launch_cuts(gpu_ctx):
    """Groups of 20 reads of 4-12 kb, k = 6 and k = 20, HiFi-like and ONT-like: the noisy groups have more distinct windows than
    the on-chip table holds (the library reports how many groups spilled).  The same call cut into several launches by a small
    workspace bound gives the same arrays."""
    rng = np.random.default_rng(12)
    groups = _long_groups(rng, 2, 0.002) + _long_groups(rng, 3, 0.08)
    groups, ks = groups + groups, [6] * 5 + [20] * 5
    out, st = _check(groups, ks, gpu_ctx)
    assert st["n_fallback"] >= 3 and st["n_miss_reads"] == 0      # k = 20 with 8 % errors: nearly every window is distinct
    assert st["n_sub_batches"] == 1
    cut, st2 = _check(groups, ks, gpu_ctx, workspace_bytes=1 << 22)      # 2^18 elements: every spilled group alone
    assert st2["n_sub_batches"] == st2["n_fallback"] == st["n_fallback"] and st2["n_sub_batches"] > 1
    for key in ("entry_off", "pos", "count"):
        assert np.array_equal(out[key], cut[key])


def test_host_and_device_buffers_and_overlapping_slices(gpu_ctx):
    rng = np.random.default_rng(21)
    buf = np.frombuffer(_tract(rng, b"CAG", 400, 0.02) + _rand(rng, bytes(range(256)), 600), np.uint8)
    n = 300
    starts = rng.integers(0, buf.shape[0] - 10, n).astype(np.int64)
    lens = np.minimum(rng.integers(0, 400, n), buf.shape[0] - starts).astype(np.int32)       # overlapping slices of one buffer
    sizes = []
    while sum(sizes) < n:
        sizes.append(min(int(rng.integers(0, 12)), n - sum(sizes)))
    group_off = np.concatenate(([0], np.cumsum(sizes))).astype(np.int32)
    ks = rng.integers(1, 30, len(sizes)).astype(np.int32)
    host = KM.count_kmers_packed(group_off, starts, lens, ks, seqs=buf, ctx=gpu_ctx)
    eo, pos, cnt = R.count_packed(group_off, starts, lens, ks, buf.tobytes())
    assert (host["entry_off"].tolist(), host["pos"].tolist(), host["count"].tolist()) == (eo, pos, cnt)
    hip = hip_runtime()
    d = C.c_void_p()
    assert hip.hipSetDevice(gpu_ctx.device) == 0 and hip.hipMalloc(C.byref(d), C.c_size_t(buf.shape[0])) == 0
    try:
        assert hip.hipMemcpy(d, C.c_void_p(buf.ctypes.data), C.c_size_t(buf.shape[0]), 1) == 0   # hipMemcpyHostToDevice
        dev = KM.count_kmers_packed(group_off, starts, lens, ks, d_seqs=d.value, n_seq_bytes=buf.shape[0], ctx=gpu_ctx)
    finally:
        hip.hipFree(d)
    for key in ("entry_off", "pos", "count"):
        assert np.array_equal(host[key], dev[key])


def _raw(ctx, group_off, starts, lens, ks, buf, cap, pos, cnt, fn="strk_count_kmers"):
    L = _lib.load()
    eo = np.full(len(group_off), -7, np.int64)
    p = lambda a: C.c_void_p(a.ctypes.data) if a is not None else None      # noqa: E731
    rc = getattr(L, fn)(ctx.handle, len(group_off) - 1, p(group_off), p(buf), buf.shape[0], p(starts), p(lens), p(ks), cap, p(eo),
                        p(pos), p(cnt), None)
    return rc, eo


def test_size_query_and_retry(gpu_ctx):
    rng = np.random.default_rng(8)
    groups = [[_tract(rng, b"CAG", 30, 0.02) for _ in range(5)], [], [_rand(rng, b"ACGT", 50)]]
    group_off, starts, lens, buf = pack_groups(groups)
    ks = np.array([3, 3, 4], np.int32)
    eo_ref, pos_ref, cnt_ref = R.count_packed(group_off, starts, lens, ks, buf.tobytes())
    E = eo_ref[-1]
    rc, eo = _raw(gpu_ctx, group_off, starts, lens, ks, buf, 0, None, None)       # cap = 0, NULL arrays: a size query
    assert rc == E and eo.tolist() == eo_ref
    pos, cnt = np.full(E, -1, np.int64), np.full(E, -1, np.int32)
    rc, eo = _raw(gpu_ctx, group_off, starts, lens, ks, buf, E - 1, pos, cnt)     # one short: nothing written
    assert rc == E and eo.tolist() == eo_ref
    assert (pos == -1).all() and (cnt == -1).all()
    rc, eo = _raw(gpu_ctx, group_off, starts, lens, ks, buf, E, pos, cnt)
    assert rc == E and pos.tolist() == pos_ref and cnt.tolist() == cnt_ref


def test_bad_input_is_rejected_before_any_launch(gpu_ctx):
    L = _lib.load()
    group_off, starts, lens, buf = pack_groups([[b"CAGCAG", b"CAG"], [b"ACGT"]])
    ks = np.array([3, 2], np.int32)
    pos, cnt = np.zeros(16, np.int64), np.zeros(16, np.int32)

    def bad(**kw):
        a = dict(group_off=group_off, starts=starts, lens=lens, ks=ks, buf=buf, cap=16, pos=pos, cnt=cnt)
        a.update(kw)
        rc, _ = _raw(gpu_ctx, a["group_off"], a["starts"], a["lens"], a["ks"], a["buf"], a["cap"], a["pos"], a["cnt"])
        assert rc == _lib.STRK_E_INVALID, kw
        assert b"strk_count_kmers" in L.strk_last_error()

    bad(ks=np.array([3, 0], np.int32))                            # k < 1
    bad(ks=np.array([-1, 2], np.int32))
    bad(group_off=np.array([1, 2, 3], np.int32))                  # does not start at 0
    bad(group_off=np.array([0, 3, 2], np.int32))                  # decreasing
    bad(lens=np.array([6, 3, 70000], np.int32))                   # too long
    bad(lens=np.array([6, 3, -1], np.int32))
    bad(starts=np.array([0, 6, 10], np.int64))                    # slice beyond the buffer
    bad(starts=np.array([-1, 6, 9], np.int64))
    bad(cap=-1)
    bad(pos=None)                                                 # cap > 0 without arrays
    g251 = np.array([0, 251], np.int32)
    bad(group_off=g251, starts=np.zeros(251, np.int64), lens=np.ones(251, np.int32), ks=np.array([1], np.int32))
    # a host pointer where device memory is expected
    rc = L.strk_count_kmers_dseqs(gpu_ctx.handle, 2, C.c_void_p(group_off.ctypes.data), C.c_void_p(buf.ctypes.data), buf.shape[0],
                                  C.c_void_p(starts.ctypes.data), C.c_void_p(lens.ctypes.data), C.c_void_p(ks.ctypes.data), 16,
                                  C.c_void_p(np.zeros(3, np.int64).ctypes.data), C.c_void_p(pos.ctypes.data),
                                  C.c_void_p(cnt.ctypes.data), None)
    assert rc == _lib.STRK_E_INVALID and b"strk_count_kmers_dseqs" in L.strk_last_error()
