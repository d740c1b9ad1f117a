"""CPU half of the band pass's seam corpus (band_cases.py): the claims against band_geometry, the C restatement of the banded DP
against its Python twin and, with a band that covers the whole matrix, against the exact oracle, and the sandwich
S_band <= S <= max(S_band, band_ub) of the restatement on every entry.  No device."""
import os
import shutil
import time

import numpy as np
import pytest

import oracle
from oracle import py_restatement as py

if shutil.which("g++") is None:
    pytest.skip("no host C++ compiler", allow_module_level=True)

import band_cases as X   # noqa: E402

K = X.K
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _timed(what, t0):
    print(f"{what}: {time.time() - t0:.2f} s")


def test_claims_equal_band_geometry_and_every_edge_has_both_sides():
    t0 = time.time()
    cs = X.cases()
    for c in cs:
        lo, n = c.window()
        g = c.geo() if n <= 32 else None
        want = g["cls"] if g else -1
        assert c.cls == (-2 if c.cls == -2 and g else want), (c.name, c.cls, want)
        if g:      # what the band kernels recompute from the class equals the search over the classes
            nfl, ntr, nfr, m = c.lens
            assert X.geometry(nfl, ntr, nfr, m, lo, n, c.tune, of_class=g["cls"]) == g, c.name
    assert {c.family for c in cs} == set("abcdefghij")
    assert {c.cls for c in cs} == set(range(X.NCLS)) | {-1, -2}
    for fam in "abcdefghij":
        assert len({c.cls for c in X.cases(fam) if c.cls >= 0}) >= (1 if fam in "i" else 2), fam
    # family a: every limit from both sides, and the far side is refused or moves to another class
    edges = {}
    for c in X.cases("a"):
        edges.setdefault(c.edge, {}).setdefault(c.side, set()).add(c.cls)
    two_sided = [e for e, s in edges.items() if "out" in s]
    assert len(two_sided) >= X.NCLS + 4 + 7, sorted(edges)
    for e in two_sided:
        assert edges[e]["in"] and all(k >= 0 for k in edges[e]["in"]) and not (edges[e]["in"] & edges[e]["out"]), (e, edges[e])
    widths = {c.edge: c for c in X.cases("a") if c.name.startswith("a/width") and c.side == "in"}
    for c in widths.values():
        lo, n = c.window()
        span, slack = X.span_slack(*c.lens[:3], c.lens[3], lo, n)
        slack = max(slack, K["kBandNarrowSlack"]) if K["D"][c.cls] == 12 else slack
        assert span + 2 * slack == K["wd"][c.cls], c.name
    for L in range(4):
        cin = X.by_name([f"a/maxdb/L{L}/in/clean"])[0]
        assert cin.ndb == K["max_db"][cin.cls] and K["layout"][cin.cls] == L
    for name, lim in (("a/nfr/127", K["kBandMaxFlank"]), ("a/fly-nfl/in", K["kBandFlyMaxFlank"]), ("a/fly-m/in", K["kBandFlyMaxMotif"])):
        c = X.by_name([name + "/clean"])[0]
        assert lim in c.lens and c.cls >= 0, name
    assert X.by_name(["a/n/32/clean"])[0].window()[1] == 32 and X.by_name(["a/n/33/clean"])[0].window()[1] == 33
    assert X.by_name(["a/n/1/clean"])[0].window() == (0, 1)
    c = X.by_name(["a/maxcol/in/clean"])[0]
    assert c.geo()["ncol"] == K["max_col"][c.cls]
    c = X.by_name(["a/rows/in/clean"])[0]
    assert c.rows() == K["max_db"][c.cls] + K["kBandRowSlack"]
    # what the builder restates of strk_dp_band.h is still what the header says
    text = open(os.path.join(ROOT, "strkit_amd", "csrc", "strk_dp_band.h")).read()
    squeeze = lambda t: "".join(t.split())            # noqa: E731  (the statements, however they are laid out)
    for f in X.LAYOUT_FORMULAS:
        assert squeeze(f) in squeeze(text), f
    _timed(f"claims of {len(cs)} cases", t0)


def test_families_reach_the_seams_they_name():
    t0 = time.time()
    # b: every named diagonal of every class is the end corner of some entry
    for c in range(X.NCLS):
        hit = set()
        for case in X.cases("b"):
            if case.cls == c:
                hit |= set(X.corner_hits(case))
        assert hit == set(X.seam_targets(c)), (c, set(X.seam_targets(c)) - hit)
    # c: every occupancy call holds reads of one lane count that differ in rows, -dlo and the first fork row
    for name, names in X.calls().items():
        cs = X.by_name(names)
        assert len({K["G"][c.cls] for c in cs}) == 1, name
        if len(cs) > 1:
            trip = {(c.rows(), c.geo()["dlo"], len(c.fl) + c.window()[0] * len(c.motif)) for c in cs}
            assert len({t[0] for t in trip}) == len(cs) and len({t[1] for t in trip}) > 1 and len({t[2] % 2 for t in trip}) == 2, (name, trip)
    per = {8: {1, 7, 8, 9}, 16: {1, 4, 5}, 32: {1, 2, 3}, 64: {1, 2}}
    got = {}
    for name, names in X.calls().items():
        got.setdefault(K["G"][X.by_name(names)[0].cls], set()).add(len(names))
    assert got == per, got
    # d: a first fork row inside the first G steps with nfl = 1, both parities, a fork row on every step
    d = X.cases("d")
    assert any(len(c.fl) == 1 and c.window()[0] == 0 and len(c.fl) < K["G"][c.cls] for c in d)
    assert {(len(c.fl) + c.window()[0] * len(c.motif)) % 2 for c in d} == {0, 1}
    assert any(len(c.motif) == 1 and c.window()[1] == 32 for c in d)
    # e: prefix rows on both sides of the first row staged between the passes; that row a flank row, three motif phases, a null row
    T = X.layout0_row_tail()
    e = X.cases("e")
    assert all(K["layout"][c.cls] == 0 for c in e)
    assert {c.rows() - T for c in e if c.edge.startswith("prefix rows")} == {-1, 0, 1}
    assert any(len(c.fl) > T for c in e)
    m = 7
    assert {(T - len(c.fl)) % m for c in e if c.edge == "row kRowTail" and len(c.fl) <= T and c.rows() > T} == {0, m - 1, m // 2}
    # f: on-the-fly classes only; the running address goes back at least three times; a motif that divides the period and one that does not
    f = X.cases("f")
    assert all(K["fly"][c.cls] for c in f)
    assert all((c.rows() - len(c.fl)) >= 3 * (X.FLY_PERIOD // len(c.motif)) * len(c.motif) for c in f)
    assert {len(c.fl) for c in f} >= {1, K["kBandFlyMaxFlank"] - 1, K["kBandFlyMaxFlank"]} and {len(c.fl) % 2 for c in f} == {0, 1}
    ms = {len(c.motif) for c in f}
    assert ms >= {1, 2, 3, K["kBandFlyMaxMotif"] - 1, K["kBandFlyMaxMotif"]} and any(X.FLY_PERIOD % k == 0 and X.FLY_PERIOD % (k + 1) for k in ms if k + 1 in ms)
    # g: with the candidate's end free the last-column term is what makes the best entry, in a class of every layout from 1 up
    for c in [c for c in X.cases("g") if c.edge.startswith("best alignment")]:
        e15 = X.expected(c, 15)
        nfl, ntr, nfr, mm = c.lens
        without = oracle.band_scores(c.fl, c.tr, c.fr, c.motif, e15["lo"], e15["n"], e15["geo"], False, 15)
        if K["lmax"][c.cls]:
            assert (e15["scores"] > without).any(), c.name
        else:
            assert np.array_equal(e15["scores"], without) and (X.exact(c, 15) > without).any(), c.name
    assert {K["layout"][c.cls] for c in X.cases("g")} == {0, 1, 2, 3}
    # h: an entry without a cell, candidates beyond both band edges, and both placements give bands
    none = X.by_name(["h/none/clean"])[0]
    assert (X.expected(none, 15)["scores"] == X.NONE).any()
    for tune in X.PLACEMENTS:
        assert sum(c.geo(tune=tune) is not None for c in X.cases("h")) >= 10, tune
    # j: nfr at its limit in every layout
    assert {K["layout"][c.cls] for c in X.cases("j")} == {0, 1, 2, 3} and all(len(c.fr) == K["kBandMaxFlank"] for c in X.cases("j"))
    _timed("seams", t0)


def test_c_restatement_equals_the_python_one_on_the_small_cases():
    t0 = time.time()
    cs = [c for c in X.cases() if X.small(c)]
    assert len(cs) >= 30 and {c.family for c in cs} >= set("abdghi")
    n = 0
    for k, c in enumerate(cs):
        for flags in (15, 0, (5 * k + 3) % 16):
            e = X.expected(c, flags)
            twin = py.band_scores(c.fl, c.tr, c.fr, c.motif, e["lo"], e["n"], e["geo"], bool(K["lmax"][e["cls"]]), flags)
            assert [X.NONE if v is None else v for v in twin] == e["scores"].tolist(), (c.name, flags)
            n += e["n"]
    _timed(f"C restatement == Python restatement on {len(cs)} cases, {n} entries", t0)


def _whole(c, lo, n):
    rows = len(c.fl) + (lo + n - 1) * len(c.motif)
    return {"dlo": -rows, "wd": rows + c.ndb + 1, "bdlo": -len(c.fr), "bwd": len(c.fr) + c.ndb + 1, "cmin": 0, "ncol": c.ndb + 1}


def test_restatement_against_the_exact_oracle():
    """A band that covers the whole matrix gives the oracle's score on every entry (with the last-column term; without it too while
    the candidate's end is not free); band_geometry's band gives the sandwich.  Oracle cells of the corpus stay under the exact corpus's cap."""
    t0 = time.time()
    cs = [c for c in X.cases() if c.cls >= 0]
    cells = sum(c.cells() for c in cs)
    assert cells < X.CELL_CAP, cells
    assert len(X.SAMPLED) <= 5
    X.prefetch(cs, [15, 0])
    for c in [c for c in cs if X.small(c)]:   # (flags 15 comes sixteen sizes at a time where the CPU allows: the same numbers)
        lo, n = c.window()
        assert X.exact(c, 15).tolist() == [oracle.candidate_score(c.tr, c.fl, c.fr, c.motif, lo + k, 15) for k in range(n)], c.name
    n_ent = 0
    for c in cs:
        for flags in (15, 0):
            e, s = X.expected(c, flags), X.exact(c, flags)
            ks = X.sampled_entries(c, e["n"])
            for lmax in (True,) if flags & 8 else (True, False):    # (candidate end free: the last-column term is part of S)
                full =oracle.band_scores(c.fl, c.tr, c.fr, c.motif, e["lo"], e["n"], _whole(c, e["lo"], e["n"]), lmax, flags)
                assert [int(full[k]) for k in ks] == [int(s[k]) for k in ks], (c.name, flags, lmax)
            bad = X.sandwich_violations(c, e["scores"], e["ub"], flags)
            assert not bad, (c.name, flags, bad[:4])
            n_ent += len(ks)
    # family b: a candidate whose end corner lies on the first diagonal outside the band loses score to the band (S_band < S) and
    # the bound covers it: 23 of the 25 such entries, in every class.  With free ends the best alignment need not end in the
    # corner: those of b/c5/m2/d-136/noisy and b/c3/m4/d-912/clean (both "below") end elsewhere and stay inside.
    lost = {}
    for c in X.cases("b"):
        e, s = X.expected(c, 15), X.exact(c, 15)
        for name, k in X.corner_hits(c).items():
            if name in ("below", "above"):
                lost.setdefault((c.cls, name), []).append(bool(e["scores"][k] < s[k] <= e["ub"][k]))
    assert set(lost) == {(k, side) for k in range(X.NCLS) for side in ("below", "above")}, lost
    assert all(any(any(lost[k, side]) for side in ("below", "above")) for k in range(X.NCLS)), lost
    assert sum(sum(v) for v in lost.values()) >= 23 and sum(len(v) for v in lost.values()) == 25, lost
    # ... and under every end-flag setting on the reduced set
    red = [c for c in X.reduced() if c.cls >= 0]
    X.prefetch(red, range(16))
    for c in red:
        for flags in range(16):
            e = X.expected(c, flags)
            bad = X.sandwich_violations(c, e["scores"], e["ub"], flags)
            assert not bad, (c.name, flags, bad[:4])
    inexact = sum(int((X.expected(c, 15)["scores"] < X.expected(c, 15)["ub"]).sum()) for c in cs)
    below = sum(int((X.expected(c, 15)["scores"][X.sampled_entries(c, X.expected(c, 15)["n"])] < X.exact(c, 15)[X.sampled_entries(c, X.expected(c, 15)["n"])]).sum()) for c in cs)
    assert inexact > 100 and below > 50       # the corpus does leave the band: entries the bound has to cover
    print(f"{len(cs)} band reads, {cells:.3g} oracle cells per end-flag setting, {n_ent} entries in the sandwich at flags 15 and 0; "
          f"{inexact} entries with S_band < ub, {below} with S_band < S at flags 15; sampled: {X.SAMPLED}")
    _timed("restatement against the oracle", t0)
