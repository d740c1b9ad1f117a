"""GPU half of the group kernels' seam corpus (tests/group_cases.py): strk_count_kmers, strk_best_representatives and
strk_consensus against kmers_restatement, consensus_restatement and poa_restatement on every case, exactly (integers and
bytes: no tolerance), and the k-mer call's statistics against the Python model of the routing, which is what ties the model
to the kernels.  CPU half: test_group_cases.py."""
import ctypes as C
import functools
import time

import numpy as np
import pytest

import consensus_restatement as BR
import group_cases as G
import kmers_restatement as KR
import poa_restatement as P
from strkit_amd import _lib
from strkit_amd import consensus as CS
from strkit_amd import kmers as KM
from strkit_amd._groups import pack_groups

pytestmark = pytest.mark.gpu

METHOD = {"none": CS.NONE, "single": CS.SINGLE, "best_rep": CS.BEST_REP, "poa": CS.POA}


@functools.lru_cache(None)
def _kmer_call(names=None):
    """(cases, packed arrays, ks, the restatement's three arrays) of a call over the named cases (None: the k-mer corpus)."""
    cs = G.kmer_cases() if names is None else [G.by_name(n) for n in names]
    packed = pack_groups([c.group for c in cs])
    ks = np.array([c.k for c in cs], np.int32)
    group_off, starts, lens, buf = packed
    return cs, packed, ks, KR.count_packed(group_off, starts, lens, ks, buf.tobytes())


def _model(cs):
    r = [G.routes()[c.name] for c in cs]
    return dict(n_fallback=sum(x.state == G.SPILLED for x in r), n_miss_reads=sum(x.state == G.GENERAL for x in r),
                dp_cells=sum(x.windows for x in r), pow2=[G.pow2_above(x.windows) for x in r if x.sorted])


def _assert_kmers(out, exp, cs):
    eo, pos, cnt = exp
    assert out["entry_off"].tolist() == eo
    got_pos, got_cnt = out["pos"].tolist(), out["count"].tolist()
    for g, c in enumerate(cs):                      # per case, so that a failure names it
        a, b = eo[g], eo[g + 1]
        assert (got_pos[a:b], got_cnt[a:b]) == (pos[a:b], cnt[a:b]), c.name
    assert len(got_pos) == len(pos)


def _run_kmers(ctx, names=None, **kw):
    cs, (group_off, starts, lens, buf), ks, exp = _kmer_call(names)
    t0 = time.perf_counter()
    out, st = KM.count_kmers_packed(group_off, starts, lens, ks, seqs=buf, ctx=ctx, with_stats=True, **kw)
    print(f"count_kmers_packed: {len(cs)} groups, {st['dp_cells']} windows, {len(exp[1])} entries, {time.perf_counter() - t0:.3f} s")
    _assert_kmers(out, exp, cs)
    m = _model(cs)
    assert (st["n_fallback"], st["n_miss_reads"], st["dp_cells"]) == (m["n_fallback"], m["n_miss_reads"], m["dp_cells"])
    return out, st, m


def test_kmer_corpus_in_one_call(gpu_ctx):
    out, st, m = _run_kmers(gpu_ctx)
    assert m["n_fallback"] >= 8 and m["n_miss_reads"] >= 19 and st["n_sub_batches"] == 1
    again, _, _ = _run_kmers(gpu_ctx)
    for key in ("entry_off", "pos", "count"):
        assert out[key].tobytes() == again[key].tobytes()


def test_kmer_corpus_with_the_sort_path_cut(gpu_ctx):
    """One group of up to 4 096 padded elements per launch of k_kmers_sort, smaller ones together: the pieces the model predicts."""
    ws = 4096 * G.ELEM_BYTES
    _, st, m = _run_kmers(gpu_ctx, workspace_bytes=ws)
    pieces = G.sort_pieces(m["pow2"], ws)
    assert st["n_sub_batches"] == len(pieces) > 10 and any(p1 - p0 > 1 for p0, p1 in pieces)


@pytest.mark.parametrize("family", "abcdefgh")
def test_kmer_family_alone(gpu_ctx, family):
    names = tuple(c.name for c in G.kmer_cases() if c.family == family)
    _run_kmers(gpu_ctx, names)


def test_probe_order_does_not_show(gpu_ctx):
    """The same windows in two string orders: the same {window: count}, whatever the order in which the keys claim their slots."""
    names = tuple(c.name for c in G.kmer_cases() if c.family == "d")
    got = KM.count_kmers([G.by_name(n).group for n in names], G.PROBE_K, ctx=gpu_ctx)
    for n, d in zip(names, got):
        assert d == KR.count_dict(G.by_name(n).group, G.PROBE_K), n
    for n, d in zip(names, got):
        if n.endswith("/fwd"):
            assert d == got[names.index(n[:-3] + "rev")] and list(d) == sorted(d), n


@functools.lru_cache(None)
def _cons_groups():
    return tuple(c.group for c in G.cons_cases())


@functools.lru_cache(None)
def _best_rep_expect():
    return [BR.best_representative(g) for g in _cons_groups()]


def test_best_representatives_on_the_dedup_and_alphabet_groups(gpu_ctx):
    cs = G.cons_cases()
    off, starts, lens, buf = pack_groups(_cons_groups())
    t0 = time.perf_counter()
    out = CS.best_representatives_packed(off, starts, lens, seqs=buf, ctx=gpu_ctx)
    print(f"best_representatives_packed: {len(cs)} groups, {time.perf_counter() - t0:.3f} s")
    for g, (c, (idx, method, dist)) in enumerate(zip(cs, _best_rep_expect())):
        got = (int(out["index"][g]), int(out["method"][g]), int(out["dist_sum"][g]))
        assert got == (idx, METHOD[method], dist), c.name
    assert all(e[1] == "best_rep" for e in _best_rep_expect())


def test_consensus_on_the_dedup_groups(gpu_ctx):
    """k_poa's copy of the dedup: a collider taken for a duplicate changes a multiplicity and with it the heaviest path (or the
    method, where the group would seem to hold one distinct string)."""
    cs = [c for c in G.cons_cases() if c.family == "a"]
    groups = [c.group for c in cs]
    exp = [P.consensus(g) for g in groups]
    off, starts, lens, buf = pack_groups(groups)
    t0 = time.perf_counter()
    out = CS.consensus_packed(off, starts, lens, seqs=buf, ctx=gpu_ctx)
    print(f"consensus_packed: {len(cs)} groups, {time.perf_counter() - t0:.3f} s")
    text, soff = out["seqs"].tobytes(), out["seq_off"].tolist()
    for g, (c, (idx, method, seq, _limited)) in enumerate(zip(cs, exp)):
        got = (int(out["index"][g]), int(out["method"][g]), text[soff[g]:soff[g + 1]])
        assert got == (idx, METHOD[method], seq or b""), c.name
    assert {e[1] for e in exp} == {"poa"} and soff[-1] == len(text)
    # two distinct strings that collide and nothing else: not `single`
    two = [[b"AGA", b"CCC"], [b"CCC", b"AGA", b"AGA"]]
    out = CS.consensus_packed(*pack_groups(two)[:3], seqs=pack_groups(two)[3], ctx=gpu_ctx)
    text, soff = out["seqs"].tobytes(), out["seq_off"].tolist()
    for g, grp in enumerate(two):
        idx, method, seq, _ = P.consensus(grp)
        assert (int(out["index"][g]), int(out["method"][g]), text[soff[g]:soff[g + 1]]) == (idx, METHOD[method], seq)


def _raw(ctx, group_off, starts, lens, ks, buf, cap, pos, cnt, ws_bytes):
    """strk_count_kmers_ws itself (tests/test_gpu_kmers.py::_raw with the workspace bound)."""
    L = _lib.load()
    eo = np.full(len(group_off), -7, np.int64)
    p = lambda a: C.c_void_p(a.ctypes.data) if a is not None else None      # noqa: E731
    st = _lib.StrkStats()
    rc = L.strk_count_kmers_ws(ctx.handle, len(group_off) - 1, p(group_off), p(buf), None, buf.shape[0], p(starts), p(lens), p(ks),
                               cap, p(eo), p(pos), p(cnt), ws_bytes, C.byref(st))
    return rc, eo, st.as_dict()


def test_cap_between_the_pieces_of_the_sort_path(gpu_ctx):
    """The write pass of a piece runs only while the entries still fit: caps at and beside the end of the first piece, with
    hashed, spilled and general groups and a group without a window in one call of four sort launches."""
    cs = [G.by_name(n) for n in G.CAP_CALL]
    groups = [c.group for c in cs[:4]] + [()] + [c.group for c in cs[4:]]
    ks = np.array([c.k for c in cs[:4]] + [3] + [c.k for c in cs[4:]], np.int32)
    group_off, starts, lens, buf = pack_groups(groups)
    eo_ref, pos_ref, cnt_ref = KR.count_packed(group_off, starts, lens, ks, buf.tobytes())
    E = eo_ref[-1]
    routes = [G.route(g, int(k)) for g, k in zip(groups, ks)]
    sorted_groups = [g for g, r in enumerate(routes) if r.sorted]
    pieces = G.sort_pieces([G.pow2_above(routes[g].windows) for g in sorted_groups], G.CAP_WS_BYTES)
    assert len(pieces) >= 3
    first_end = eo_ref[sorted_groups[pieces[0][1] - 1] + 1]              # the entries up to the end of the first piece
    second_end = eo_ref[sorted_groups[pieces[1][1] - 1] + 1]
    assert 0 < first_end < first_end + 1 < second_end < E - 1
    args = (gpu_ctx, group_off, starts, lens, ks, buf)
    rc, eo, st = _raw(*args, 0, None, None, G.CAP_WS_BYTES)                # a size query
    assert rc == E and eo.tolist() == eo_ref and st["n_sub_batches"] == len(pieces)
    assert (st["n_fallback"], st["n_miss_reads"], st["dp_cells"]) == (
        sum(r.state == G.SPILLED for r in routes), sum(r.state == G.GENERAL for r in routes), sum(r.windows for r in routes))
    for cap in (first_end, first_end + 1, second_end, E - 1):            # short: the size, the offsets, and nothing written
        pos, cnt = np.full(cap, -1, np.int64), np.full(cap, -1, np.int32)
        rc, eo, st = _raw(*args, cap, pos, cnt, G.CAP_WS_BYTES)
        assert rc == E and eo.tolist() == eo_ref and st["n_sub_batches"] == len(pieces), cap
        assert (pos == -1).all() and (cnt == -1).all(), cap
    results = []
    for _ in range(2):                                                   # the same bytes from a second call on the context
        pos, cnt = np.full(E, -1, np.int64), np.full(E, -1, np.int32)
        rc, eo, _ = _raw(*args, E, pos, cnt, G.CAP_WS_BYTES)
        assert rc == E and eo.tolist() == eo_ref
        assert pos.tolist() == pos_ref and cnt.tolist() == cnt_ref
        results.append(eo.tobytes() + pos.tobytes() + cnt.tobytes())
    assert results[0] == results[1]
    pos, cnt = np.full(E + 5, -1, np.int64), np.full(E + 5, -1, np.int32)      # room to spare, the default workspace
    rc, eo, _ = _raw(*args, E + 5, pos, cnt, 0)
    assert rc == E and pos[:E].tolist() == pos_ref and cnt[:E].tolist() == cnt_ref and (pos[E:] == -1).all() and (cnt[E:] == -1).all()
