"""GPU half of the exact path's seam corpus (exact_cases.py): strk_score_table, strk_score_ref_table and the counting path
with the band off against the CPU oracle on every case — exact integer equality, no tolerance — and the class lists of each
call (strk_class_counts) against the histogram of strk_classify over the chunks."""
import time

import numpy as np
import pytest

import exact_cases as X
from helpers import oracle_count_pool

pytestmark = pytest.mark.gpu
LISTS = [f"c{c}" for c in range(X.NC)] + ["long", "generic"]


def _fmt(hist):
    return " ".join(f"{k}={int(v)}" for k, v in zip(LISTS, hist) if v)


def _score(cs, ctx, flags=15, force=False):
    """One strk_score_table call over the cases: scores bit for bit, class lists and stats against the claimed routes."""
    from strkit_amd.batch import class_counts, score_table
    lo, n = X.windows(cs)
    got, st = score_table(X.batch(cs), lo, n, flags, force, ctx=ctx, with_stats=True)
    counts = class_counts(ctx)
    exp = X.expected(cs, flags)
    bad = [(c.name, c.edge, c.side, c.route, g.tolist(), e.tolist()) for c, g, e in zip(cs, got, exp) if not np.array_equal(g, e)]
    assert not bad, f"flags {flags} force_generic {force}: {len(bad)} of {len(cs)} cases differ: {[x[0] for x in bad][:40]}; first: {bad[0]}"
    hist = X.route_histogram(cs, force)
    assert counts.tolist() == hist.tolist(), (_fmt(counts), _fmt(hist))
    assert st["n_long_reads"] == hist[X.LONG] and st["n_fallback"] == hist[X.GENERIC], st
    return got, hist, int(n.sum())


def _line(what, t0, calls, hist, n_cand):
    print(f"{what}: {calls} call(s), {int(hist.sum())} items [{_fmt(hist)}], {n_cand} candidates equal to the oracle's, {time.time() - t0:.2f} s")


@pytest.mark.parametrize("flags", [15, 0])
def test_whole_corpus_in_one_call(gpu_ctx, flags):
    t0 = time.time()
    cs = X.cases()
    _, hist, n_cand = _score(cs, gpu_ctx, flags)
    assert (hist > 0).all(), _fmt(hist)               # every fast class, the tiled kernel, the generic kernel
    _line(f"whole corpus, flags {flags}", t0, 1, hist, n_cand)


@pytest.mark.parametrize("family", list("abcdefghi"))
def test_each_family_in_a_call_of_its_own(gpu_ctx, family):
    """... and the occupancy calls of families e and f: a class's items share their waves with nothing else."""
    t0 = time.time()
    cs = X.cases(family)
    assert cs
    _, hist, n_cand = _score(cs, gpu_ctx)
    calls = 1
    for name, names in X.calls().items():
        if name.startswith(family + "/"):
            _, h, k = _score(X.by_name(names), gpu_ctx)
            assert h.sum() == len(names) and (h > 0).sum() == 1, (name, _fmt(h))
            hist, n_cand, calls = hist + h, n_cand + k, calls + 1
    _line(f"family {family}", t0, calls, hist, n_cand)


def test_all_sixteen_end_flags(gpu_ctx):
    t0 = time.time()
    cs = X.reduced()
    assert {X.LANES[c.route[0]] for c in cs if c.route[0] < X.NC} == set(X.LANE_COUNTS)
    assert sum(c.route == (X.LONG,) for c in cs) == 2 and sum(c.route == (X.GENERIC,) for c in cs) == 2
    cs = cs + X.edge_rows()
    X.prefetch(cs, range(16))
    total = 0
    for flags in range(16):
        _, hist, n_cand = _score(cs, gpu_ctx, flags)
        total += n_cand
    _line("reduced set, end flags 0..15", t0, 16, 16 * hist, total)


def test_force_generic_on_windows_of_up_to_400_bases(gpu_ctx):
    t0 = time.time()
    cs = [c for c in X.cases() if c.ndb <= 400]
    assert {c.family for c in cs} >= set("abcdefgi") and len(cs) > 120
    _, hist, n_cand = _score(cs, gpu_ctx, 15, force=True)
    _line("force_generic", t0, 1, hist, n_cand)


def _count_cases():
    """Families a, b, h with the true copy number as the estimate, +-7 on a third of the reads: some searches leave the window."""
    cs = X.cases("abh")
    rng = np.random.default_rng(2503)
    est = []
    for k, c in enumerate(cs):
        e = round(len(c.tr) / len(c.motif))
        est.append(max(0, e + (7 if rng.integers(2) else -7)) if k % 3 == 1 else e)
    return cs, X.batch(cs, est)


_COUNT_EXPECTED: dict = {}


@pytest.mark.parametrize("dedupe", [True, False], ids=["dedupe", "no-dedupe"])
@pytest.mark.parametrize("tie_rule", [0, 1], ids=["tie-first", "tie-last"])
def test_counting_path_with_the_band_off(fresh_ctx, tie_rule, dedupe):
    """count_loci(band=False): the speculative search inside k_dp_all and k_dp_long, k_sort_long's order, window-miss rounds."""
    from strkit_amd import _lib
    from strkit_amd.batch import class_counts, count_loci
    t0 = time.time()
    cs, b = _count_cases()
    if tie_rule not in _COUNT_EXPECTED:
        _COUNT_EXPECTED[tie_rule] = oracle_count_pool(b, tie_rule=tie_rule)
    exp = _COUNT_EXPECTED[tie_rule]
    _lib.load().strk_adaptive_reset()                 # the default window at its start, whatever ran before
    try:
        got, st = count_loci(b, tie_rule=tie_rule, ctx=fresh_ctx, with_stats=True, dedupe=dedupe, band=False)
    finally:
        _lib.load().strk_adaptive_reset()
    for k in ("cn", "score", "n_iters", "start"):
        bad = np.flatnonzero(got[k] != exp[k])
        assert bad.size == 0, (k, f"{bad.size} of {len(cs)} reads differ", [(cs[r].name, int(got[k][r]), int(exp[k][r])) for r in bad[:10]])
    assert st["n_band_reads"] == 0 and st["n_long_reads"] > 20 and st["n_miss_reads"] > 0, st
    print(f"counting path tie_rule={tie_rule} dedupe={dedupe}: {len(cs)} reads equal to the oracle's in cn, score, n_iters, start; "
          f"long {st['n_long_reads']} generic {st['n_fallback']} missed {st['n_miss_reads']} in {st['n_miss_rounds']} round(s); "
          f"last scoring call [{_fmt(class_counts(fresh_ctx))}], {time.time() - t0:.2f} s")


@pytest.mark.parametrize("force", [False, True], ids=["fast", "generic"])
def test_reference_side(gpu_ctx, force):
    from strkit_amd.batch import class_counts, score_ref_table
    t0 = time.time()
    cs = X.cases(ref=True)
    lo, n = X.windows(cs)
    got = score_ref_table(X.batch(cs), lo, n, force_generic=force, ctx=gpu_ctx)
    counts = class_counts(gpu_ctx)
    exp = X.expected(cs)
    bad = [(c.name, c.edge, c.side, [x.tolist() for x in g], [x.tolist() for x in e]) for c, g, e in zip(cs, got, exp)
           if not (np.array_equal(g[0], e[0]) and np.array_equal(g[1], e[1]))]
    assert not bad, f"force_generic {force}: {len(bad)} of {len(cs)} cases differ: {[x[0] for x in bad]}; first: {bad[0]}"
    hist = X.route_histogram(cs, force)
    assert counts.tolist() == hist.tolist() and hist[X.GENERIC] > 0, (_fmt(counts), _fmt(hist))
    assert force or hist[X.NC - 1] > 8
    _line(f"reference side, force_generic {force} (score and end_query)", t0, 1, hist, int(n.sum()))


def test_the_same_call_twice_gives_the_same_bytes(gpu_ctx):
    from strkit_amd.batch import class_counts
    t0 = time.time()
    cs = [c for c in X.cases() if c.cells() <= 4 * 10 ** 7]          # every family and every list, without the longest tables
    first, hist, n_cand = _score(cs, gpu_ctx)
    counts = class_counts(gpu_ctx)
    assert (hist > 0).all() and {c.family for c in cs} == set("abcdefghi")
    second, _, _ = _score(cs, gpu_ctx)
    assert np.concatenate(first).tobytes() == np.concatenate(second).tobytes() and class_counts(gpu_ctx).tolist() == counts.tolist()
    _line("repeat run", t0, 2, 2 * hist, 2 * n_cand)
