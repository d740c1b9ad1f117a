"""CPU: the corrections for multiple testing of `mi` (strkit_amd.mi.correct_for_multiple_testing, numpy) against hand-worked
vectors, against the loops of mi_restatement.py and against the identities of the methods.  statsmodels, whose multipletests
the reference calls, is not a dependency: this part of the rule is unpinned."""
import numpy as np
import pytest

import mi_restatement as R
from strkit_amd.mi import MT_METHODS, correct_for_multiple_testing as corr

P5 = [0.01, 0.04, 0.03, 0.005, 0.2]
HAND = {   # worked by hand from the definitions; ranks of P5 ascending: 0.005, 0.01, 0.03, 0.04, 0.2
    "bonferroni": [0.05, 0.2, 0.15, 0.025, 1.0],
    "holm": [0.04, 0.09, 0.09, 0.025, 0.2],                # 0.025 0.04 0.09 0.08 0.2 -> running maximum
    "simes-hochberg": [0.04, 0.08, 0.08, 0.025, 0.2],      # the same products -> running minimum from the right
    "fdr_bh": [0.025, 0.05, 0.05, 0.025, 0.2],             # p 5 / rank: 0.025 0.025 0.05 0.05 0.2
    "fdr_by": [x * (1 + 1 / 2 + 1 / 3 + 1 / 4 + 1 / 5) for x in [0.025, 0.05, 0.05, 0.025, 0.2]],
    "sidak": [1 - (1 - x) ** 5 for x in P5],
    "holm-sidak": [1 - (1 - 0.01) ** 4, 1 - (1 - 0.03) ** 3, 1 - (1 - 0.03) ** 3, 1 - (1 - 0.005) ** 5, 0.2],
}
VECTORS = [P5, [0.5, 0.5, 0.5, 0.001, 0.001, 0.02], [1.0, 0.9, 1e-12, 0.04, 0.04, 0.04, 0.0499, 0.3],
           [0.2, 0.01, 0.01, 0.01, 0.011, 0.012, 0.6]]


@pytest.mark.parametrize("method", sorted(HAND))
def test_hand_worked_vector(method):
    rej, adj = corr(P5, 0.05, method)
    assert adj.tolist() == pytest.approx(HAND[method], rel=1e-12)
    assert rej.tolist() == [a <= 0.05 for a in HAND[method]]


def test_a_vector_of_eight_by_hand():
    p = [0.001, 0.008, 0.039, 0.041, 0.042, 0.06, 0.074, 0.205]      # Benjamini & Hochberg's kind of example, in order
    _, adj = corr(p, 0.05, "fdr_bh")
    raw = [x * 8 / (i + 1) for i, x in enumerate(p)]                   # 0.008 0.032 0.104 0.082 0.0672 0.08 0.08457 0.205
    assert adj.tolist() == pytest.approx([0.008, 0.032, 0.0672, 0.0672, 0.0672, 0.08, raw[6], 0.205], rel=1e-12)
    rej, adj = corr(p, 0.05, "holm")
    assert adj.tolist() == pytest.approx([0.008, 0.056, 0.234, 0.234, 0.234, 0.234, 0.234, 0.234], rel=1e-12)
    assert rej.tolist() == [True] + [False] * 7


@pytest.mark.parametrize("method", MT_METHODS)
@pytest.mark.parametrize("k", range(len(VECTORS)))
def test_equals_the_loops_of_the_restatement(method, k):
    for alpha in (0.05, 0.25):      # (no adjusted p of these vectors lies at a level: there the two ways to reject may differ by a rounding)
        rej, adj = corr(VECTORS[k], alpha, method)
        want_rej, want_adj = R.multipletests(VECTORS[k], alpha, method)
        assert adj.tolist() == pytest.approx(want_adj, rel=1e-12, abs=0)
        assert rej.tolist() == want_rej, (method, alpha, adj.tolist())


@pytest.mark.parametrize("k", range(len(VECTORS)))
def test_identities(k):
    p = np.array(VECTORS[k])
    n = p.size
    adj = {m: corr(p, 0.05, m)[1] for m in MT_METHODS}
    assert np.array_equal(adj["none"], p)
    assert adj["bonferroni"].tolist() == pytest.approx(np.minimum(1.0, n * p).tolist(), rel=1e-15)
    assert (adj["holm"] >= adj["simes-hochberg"] - 1e-15).all()
    assert (adj["holm-sidak"] <= adj["holm"] + 1e-15).all() and (adj["sidak"] <= adj["bonferroni"] + 1e-15).all()
    order = np.argsort(p, kind="stable")
    bh = adj["fdr_bh"][order]
    assert (np.diff(bh) >= 0).all()                                   # monotone in p
    raw = p[order] * n / np.arange(1, n + 1)
    assert (bh <= np.minimum(raw, 1.0) + 1e-18).all() and bh[-1] == min(raw[-1], 1.0)      # = p n / rank before the running minimum
    cm = np.sum(1.0 / np.arange(1, n + 1))
    assert adj["fdr_by"].tolist() == pytest.approx(np.minimum(1.0, np.minimum.accumulate((raw * cm)[::-1])[::-1])[np.argsort(order)].tolist(), rel=1e-14)
    for m in MT_METHODS:
        assert (adj[m] <= 1.0).all() and (adj[m] >= p - 1e-18).all()
        for alpha in (0.01, 0.05, 0.5):
            rej, a = corr(p, alpha, m)
            assert rej.tolist() == ((p < alpha) if m == "none" else (a <= alpha)).tolist()
    # equal p-values get equal adjusted p-values
    for m in MT_METHODS:
        for v in np.unique(p):
            assert len(set(adj[m][p == v].tolist())) == 1, (m, v)


def test_two_stage_methods_are_refused_by_name():
    for m in ("fdr_tsbh", "fdr_tsbky"):
        with pytest.raises(ValueError, match=m):
            corr(P5, 0.05, m)
    with pytest.raises(ValueError, match="unknown"):
        corr(P5, 0.05, "hommel")


def test_edges():
    rej, adj = corr([], 0.05, "fdr_bh")
    assert rej.size == 0 and adj.size == 0
    rej, adj = corr([0.03], 0.05, "holm")
    assert adj.tolist() == [0.03] and rej.tolist() == [True]
    assert corr([1.0, 0.5], 0.05, "sidak")[1].tolist() == [1.0, 0.75]
