"""GPU half of the band pass's seam corpus (band_cases.py): what k_dp_band and k_dp_band_wide write (strk_band_tables) against the
restatement of the banded DP entry for entry, their bounds against band_ub as compiled for the host, the sandwich
S_band <= S <= max(S_band, ub) of the kernels' own numbers against the exact oracle, and the corpus through the counting path
with the number of fall-backs predicted exactly.  Everything is integers: no tolerance."""
import shutil
import time

import numpy as np
import pytest

if shutil.which("g++") is None:
    pytest.skip("no host C++ compiler", allow_module_level=True)

import band_cases as X   # noqa: E402
from helpers import end_probation   # noqa: E402

pytestmark = pytest.mark.gpu
K = X.K
# An entry without a cell in both bands.  The kernels have no mark for it: a fork row's sum takes kBandNeg16 = -20 000 where the
# backward column has no cell, so what they write there is the score of a real alignment (a forward cell of the fork row, the rest
# of the window and the right flank gapped) minus 20 000, not a value below -(1 << 27) as was supposed when the corpus was
# planned: measured on the MI355X, -20 464 for a/maxcol/in/clean, entry 12.  What is asserted follows from that: at most S - 20 000,
# and exactly the row's largest G-space value minus 20 000 where that value is a cell of the window (band_cases: e["top"]).
NONE_GAP = X.NONE_GAP


def _tables(cs, ctx, flags=15, tune=None, sort_wide=False, sandwich=False):
    """One strk_band_tables call over cases of one W (and one tune): classes, windows, scores, bounds against the expectations.
    Returns the raw arrays and the number of entries compared."""
    from strkit_amd.batch import BAND_ROW_UNTOUCHED, band_tables
    W = cs[0].W
    tune = cs[0].tune if tune is None else tuple(tune)
    assert all(c.W == W for c in cs)
    out, st = band_tables(X.batch(cs), W, flags, tune, sort_wide, ctx=ctx, with_stats=True)
    exp = [X.expected(c, flags, tune=tune) for c in cs]
    assert out["cls"].tolist() == [e["cls"] for e in exp], [(c.name, int(g), e["cls"]) for c, g, e in zip(cs, out["cls"], exp) if g != e["cls"]][:20]
    assert out["lo"].tolist() == [e["lo"] for e in exp] and out["n"].tolist() == [e["n"] for e in exp]
    assert st["n_band_reads"] == sum(e["cls"] != -1 for e in exp) and st["n_band_fallback"] == sum(e["cls"] == -2 for e in exp), st
    bad, n_ent = [], 0
    for r, (c, e) in enumerate(zip(cs, exp)):
        if e["cls"] < 0:
            assert (out["scores"][r] == BAND_ROW_UNTOUCHED).all() and (out["ub"][r] == BAND_ROW_UNTOUCHED).all(), c.name
            continue
        n = e["n"]
        got = out["scores"][r, :n].astype(np.int64)
        want = e["scores"].astype(np.int64)
        none = want == X.NONE
        below = X.exact(c, flags).astype(np.int64) - NONE_GAP if none.any() else want
        top = e["top"].astype(np.int64)            # ... and exactly this where the band's last diagonal is inside the window at that row
        off = none & ((got > below) | ((top != X.NONE) & (got != top - NONE_GAP)))
        if not np.array_equal(got[~none], want[~none]) or off.any():
            k = int(np.flatnonzero((got != want) & ~none | off)[0])
            want = np.where(none & (top != X.NONE), top - NONE_GAP, want)
            bad.append((c.name, c.edge, c.side, f"class {e['cls']}", f"entry {k} of {n}", f"kernel {int(got[k])}", f"restatement {int(want[k])}"))
        assert np.array_equal(out["ub"][r, :n], e["ub"]), (c.name, out["ub"][r, :n].tolist(), e["ub"].tolist())
        assert (out["scores"][r, n:] == BAND_ROW_UNTOUCHED).all(), c.name
        if sandwich:
            v = X.sandwich_violations(c, got, out["ub"][r, :n], flags)
            assert not v, (c.name, flags, v[:4])
        n_ent += n
    assert not bad, f"flags {flags} tune {tune}: {len(bad)} of {len(cs)} reads differ from the restatement: {[b[0] for b in bad][:40]}; first: {bad[0]}"
    return out, n_ent


def _line(what, t0, calls, reads, n_ent):
    print(f"{what}: {calls} call(s), {reads} reads, {n_ent} entries equal to the restatement's, {time.time() - t0:.2f} s")


@pytest.mark.parametrize("flags", [15, 0])
def test_whole_corpus_one_call_per_window(gpu_ctx, flags):
    """(A call plans all its reads with one W and one placement: a call per group of band_cases.groups().)"""
    t0 = time.time()
    X.prefetch(X.cases(), [flags])
    seen, n_ent, calls = set(), 0, 0
    for cs in X.groups().values():
        out, k = _tables(cs, gpu_ctx, flags, sandwich=True)
        seen |= set(out["cls"].tolist())
        n_ent, calls = n_ent + k, calls + 1
    assert seen == set(range(X.NCLS)) | {-1, -2}, seen
    _line(f"whole corpus, flags {flags}", t0, calls, len(X.cases()), n_ent)


def test_each_occupancy_call_on_its_own(gpu_ctx):
    t0 = time.time()
    n_ent = reads = 0
    for name, names in X.calls().items():
        cs = X.by_name(names)
        out, k = _tables(cs, gpu_ctx)
        assert len(set(out["cls"].tolist())) == 1 and out["cls"][0] >= 0, (name, out["cls"])
        n_ent, reads = n_ent + k, reads + len(cs)
    _line("occupancy calls", t0, len(X.calls()), reads, n_ent)


def test_all_sixteen_end_flags(gpu_ctx):
    t0 = time.time()
    cs = X.reduced()
    assert {c.cls for c in cs} >= set(range(X.NCLS))
    n_ent = calls = 0
    X.prefetch(cs, range(16), with_exact=False)   # (the sandwich of these entries at every setting: test_band_cases.py, on the restatement)
    for flags in range(16):
        for g in X.groups(cs).values():
            _, k = _tables(g, gpu_ctx, flags)
            n_ent, calls = n_ent + k, calls + 1
    _line("reduced set, end flags 0..15", t0, calls, 16 * len(cs), n_ent)


@pytest.mark.parametrize("tune", X.PLACEMENTS, ids=lambda t: "tune-%d-%d-%d" % t)
def test_both_placements_of_the_outer_candidates(gpu_ctx, tune):
    t0 = time.time()
    cs = X.cases("h")
    out, n_ent = _tables(cs, gpu_ctx, 15, tune=tune, sandwich=True)
    exp = [X.expected(c, 15, tune=tune) for c in cs]
    assert sum(e["cls"] >= 0 for e in exp) >= 10
    assert any((e["scores"] < e["ub"]).any() for e in exp if e["cls"] >= 0)      # outer candidates the band does not certify
    if tune == X.PLACEMENTS[0]:
        assert any((e["scores"] == X.NONE).any() for e in exp if e["cls"] >= 0)
    _line(f"family h under tune {tune}", t0, 1, len(cs), n_ent)


def test_sorted_wide_classes_and_a_repeated_call_give_the_same_bytes(gpu_ctx):
    t0 = time.time()
    n_ent = calls = 0
    for cs in X.groups().values():
        first, k = _tables(cs, gpu_ctx)
        for sort_wide in (True, False):
            again, _ = _tables(cs, gpu_ctx, sort_wide=sort_wide)
            assert all(first[key].tobytes() == again[key].tobytes() for key in ("lo", "n", "cls", "scores", "ub")), (cs[0].W, cs[0].tune, sort_wide)
        n_ent, calls = n_ent + 3 * k, calls + 3
    assert any(K["fly"][c.cls] for c in X.cases() if c.cls >= 0)
    _line("sorted wide lists and a repeated call", t0, calls, 3 * len(X.cases()), n_ent)


def _count_cases():
    """Every read a counting call can express: it clamps W to 15, and a negative estimate scores nothing, which the library
    reports as the reference's max() does (6 + 6 reads stay out)."""
    return [c for c in X.cases() if c.W <= 15 and c.est >= 0]


def test_counting_path_falls_back_exactly_where_the_certificate_says():
    """count_loci on contexts past their probation, no feedback, no dedupe, the library's own placement: answers equal the
    oracle's, and n_band_fallback is exactly the number of band reads whose search_replay_cert from the estimate, run on the host
    over the restatement's (S_band, ub), is uncertain (plus the reads the band kernel hands on).  The expected answers are the
    reference's search over the oracle's exact scores around the estimate (band_cases.count_expected)."""
    from strkit_amd import _lib
    from strkit_amd.batch import count_loci
    t0 = time.time()
    total = dict(reads=0, band=0, fallback=0, miss=0)
    seen = set()
    for (W, _), cs in sorted(X.groups(_count_cases()).items()):
        ts = min(31, 2 * (W + 7) + 1)                       # the stride a counting call gives its tables
        b = X.batch(cs)
        X.prefetch_count(cs, ts)
        exp = dict(zip(("cn", "score", "n_iters", "start"), np.array([X.count_expected(c) for c in cs], np.int64).T))
        band = fallback = miss = 0
        for c in cs:
            e = X.expected(c, 15, ts, tune=(0, 0, 0))
            if e["cls"] == -1:
                continue
            band += 1
            seen.add(e["cls"])
            if e["cls"] == -2:
                fallback += 1
                continue
            s = np.where(e["scores"] == X.NONE, -(1 << 28), e["scores"])
            cr = X.cert(c.est, s, e["ub"], e["lo"], e["n"])
            fallback += cr["uncertain"]
            miss += cr["miss"] and not cr["uncertain"]
        ctx = _lib.Context(0)
        try:
            end_probation(ctx)
            got, st = count_loci(b, window=W, feedback=False, dedupe=False, ctx=ctx, with_stats=True)
        finally:
            ctx.close()
        for k in ("cn", "score", "n_iters", "start"):
            bad = np.flatnonzero(got[k] != exp[k])
            assert bad.size == 0, (W, k, [(cs[r].name, int(got[k][r]), int(exp[k][r])) for r in bad[:10]])
        print(f"W {W}: {len(cs)} reads, band {st['n_band_reads']} (expected {band}), fall-backs {st['n_band_fallback']} (expected {fallback}), "
              f"certified searches that leave the window {miss}")
        assert st["n_band_reads"] == band and st["n_band_fallback"] == fallback, (W, st["n_band_reads"], band, st["n_band_fallback"], fallback)
        for k, v in (("reads", len(cs)), ("band", band), ("fallback", fallback), ("miss", miss)):
            total[k] += v
    assert seen == set(range(X.NCLS)) | {-2} and total["reads"] == len(X.cases()) - 12 and total["band"] >= 150 and 0 < total["fallback"] < total["band"], (seen, total)
    print(f"counting path: {total}, {time.time() - t0:.2f} s")
