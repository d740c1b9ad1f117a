"""CPU: the restatement of the allele-calling rule for one to six alleles (tests/alleles_n_restatement.py)
against alleles_restatement for one and two alleles, against sklearn for more components, and on hand cases.  The
restatement is what tests/test_gpu_alleles_n.py holds the device to."""
import numpy as np
import pytest

import alleles_n_restatement as N
import alleles_restatement as R
from test_gpu_alleles import _locus


def test_one_and_two_alleles_equal_the_two_component_restatement():
    rng = np.random.default_rng(20261019)
    kinds = ["hifi"] * 6 + ["wide", "expansion", "tiny", "one"]
    params = [R.Params(), R.Params(force_gm_filter=1), R.Params(num_bootstrap=3, n_init=1), R.Params(max_iter=1)]
    for t in range(300):
        cn, w, nal = _locus(rng, kinds[int(rng.integers(len(kinds)))])
        p = params[t % len(params)] if t % 3 == 0 else params[0]
        seed = int(rng.integers(0, 1 << 63))
        exp = R.call_locus(cn, w, nal, seed, p)
        got = N.call_locus_n(cn, w, nal, seed, p, width=2)
        assert set(got) == set(exp)
        for k in exp:
            if k == "median_cands":
                assert len(got[k]) == len(exp[k])
                for (gw, gs), (ew, es) in zip(got[k], exp[k]):
                    assert gw.tobytes() == ew.tobytes() and gs.tobytes() == es.tobytes(), (t, k)
            elif k == "read_peak":
                assert got[k].tolist() == exp[k].tolist(), (t, k)
            elif k in ("means", "weights", "stdevs"):   # to the bit
                assert np.asarray(got[k]).tobytes() == np.asarray(exp[k]).tobytes(), (t, k, got[k], exp[k])
            else:
                assert got[k] == exp[k], (t, k, got[k], exp[k])


def _multi_locus(rng, n_alleles, n_per=12):
    """n_alleles alleles at least 5 apart, n_per reads each, +-1 noise on a quarter of the reads."""
    gaps = rng.integers(5, 15, n_alleles)
    truth = (int(rng.integers(5, 40)) + np.cumsum(gaps) - gaps[0]).tolist()
    cn = np.repeat(truth, n_per)
    noisy = rng.random(cn.shape[0]) < 0.25
    cn = cn + np.where(noisy, rng.choice([-1, 1], cn.shape[0]), 0)
    rng.shuffle(cn)
    return cn.astype(np.int32), truth


def _counts_row(cn, rng):
    v = np.unique(cn)
    sample = rng.choice(cn, size=cn.shape[0])
    c = np.array([(sample == x).sum() for x in v], dtype=np.int64)
    return c, v.astype(np.float64), int(cn.shape[0])


@pytest.mark.parametrize("c", [3, 4, 6])
def test_em_equals_sklearn_per_init(monkeypatch, c):
    """As tests/test_alleles_restatement.py does for two components: sklearn's fit from the restatement's seeds."""
    pytest.importorskip("sklearn")
    import sklearn.mixture._base as base
    from sklearn.mixture import GaussianMixture

    rng = np.random.default_rng(100 + c)
    p = R.Params()
    checked = 0
    for t in range(24):
        cn, _ = _multi_locus(rng, c if t % 3 else max(2, c - 1), n_per=int(rng.integers(6, 16)))
        cnt, v, m = _counts_row(cn, rng)
        if (cnt > 0).sum() < 2:
            continue
        C = cnt[None, :]
        key = R.mix64(t)
        X = np.repeat(v, cnt).reshape(-1, 1)
        first_idx = np.concatenate([[0], np.cumsum(cnt)[:-1]])
        for init in range(3):
            ks = N.kmeanspp_seeds_c(C, v, m, key, np.array([t]), init, c, r=t % 2)
            idx = first_idx[ks[0]]
            monkeypatch.setattr(base, "kmeans_plusplus", lambda *a, _i=idx, **k: (X[_i], _i))
            g = GaussianMixture(c, covariance_type="spherical", init_params="k-means++", n_init=1, tol=p.tol,
                                reg_covar=p.reg_covar, max_iter=p.max_iter, random_state=0).fit(X)
            means, var, weights, lb, n_iter = N.em_fit_c(C, v, m, v[ks], p)
            assert int(n_iter[0]) == g.n_iter_, (t, init)
            np.testing.assert_allclose(means[0], g.means_[:, 0], rtol=1e-9, atol=0)
            np.testing.assert_allclose(var[0], g.covariances_, rtol=1e-9, atol=1e-15 * float(np.max(v)) ** 2)
            np.testing.assert_allclose(weights[0], g.weights_, rtol=1e-9, atol=0)
            np.testing.assert_allclose(lb[0], g.lower_bound_, rtol=1e-9, atol=1e-6)
            checked += 1
    assert checked >= 60


@pytest.mark.parametrize("c", [3, 4, 6])
def test_kmeanspp_seeds_equal_sklearn_fed_the_same_uniforms(c):
    """sklearn's own _kmeans_plusplus on the expanded sample, its random_state answering with the stream's uniforms."""
    pytest.importorskip("sklearn")
    from sklearn.cluster._kmeans import _kmeans_plusplus
    from sklearn.utils.extmath import row_norms

    class Stream:
        """Stands in for the RandomState: choice(n, p=...) is the first centre, uniform(size=T) the trials of one centre."""

        def __init__(self, key, b, init, r, m):
            self.key, self.b, self.init, self.r, self.m, self.q = key, b, init, r, m, 0

        def choice(self, n, p=None):
            return min(int(np.floor(R.uniforms(self.key, 1, self.b, self.init, 64 * self.r) * self.m)), self.m - 1)

        def uniform(self, size=None):
            self.q += 1
            return R.uniforms(self.key, 1, self.b, self.init, 64 * self.r + 8 * (self.q - 1) + 1 + np.arange(size))

    rng = np.random.default_rng(7 * c)
    checked = 0
    for t in range(60):
        cn, _ = _multi_locus(rng, c if t % 4 else 2, n_per=int(rng.integers(4, 14)))
        cnt, v, m = _counts_row(cn, rng)
        if (cnt > 0).sum() < 2:
            continue
        key = R.mix64(1000 + t)
        r = t % 3
        ks = N.kmeanspp_seeds_c(cnt[None, :], v, m, key, np.array([5]), 2, c, r)
        X = np.repeat(v, cnt).reshape(-1, 1)
        centers, _ = _kmeans_plusplus(X, c, row_norms(X, squared=True), np.ones(m), Stream(key, 5, 2, r, m))
        assert centers[:, 0].tolist() == v[ks[0]].tolist(), (t, centers[:, 0], v[ks[0]])
        checked += 1
    assert checked >= 50


# ----------------------------------------------------------------------------------------------------------------------
# hand cases (tests/test_gpu_alleles_n.py runs the same loci on the device)

HAND_CASES = {
    # four alleles asked, two values far apart: 4 -> 2 (two useless) -> kept, or -> 1
    "reduce_4_2": (np.array([10] * 14 + [30] * 14 + [11, 29], np.int32), 4, R.Params()),
    # one dominant value and a few strays: every reduction ends at the single Gaussian
    "reduce_4_2_1": (np.array([20] * 36 + [21, 22, 23], np.int32), 4, R.Params(force_gm_filter=1)),
    # min_allele_reads so high that no component passes filter 1: all useless, the last fit is kept
    "all_useless": (np.array([10] * 6 + [20] * 6 + [30] * 6, np.int32), 3, R.Params(min_allele_reads=60)),
    # more alleles than distinct values: the k-means++ potential reaches 0
    "potential_0": (np.array([12] * 9 + [17] * 9, np.int32), 6, R.Params()),
    # fewer reads than alleles (min_reads lowered so that the check is the one that fires)
    "n_below_A": (np.array([5, 9, 14, 22], np.int32), 5, R.Params(min_reads=2)),
    "one_value_6": (np.full(9, 31, np.int32), 6, R.Params()),
}


def _rows(name, seed=77):
    cn, A, p = HAND_CASES[name]
    v_int = np.unique(cn)
    n = cn.shape[0]
    key = R.mix64(seed)
    bidx = np.arange(p.num_bootstrap)
    u = R.uniforms(key, 0, bidx[:, None], 0, np.arange(n)[None, :])
    pick = np.minimum((u * n).astype(np.int64), n - 1)
    C = np.zeros((p.num_bootstrap, v_int.shape[0]), dtype=np.int64)
    np.add.at(C, (np.repeat(bidx, n), np.searchsorted(v_int, cn)[pick].ravel()), 1)
    return N.fit_rows_n(C, v_int.astype(np.float64), n, A, key, bidx, p), C


def test_reduction_4_to_2_keeps_two_components_and_fills_two():
    (k, means, weights, stdevs), _ = _rows("reduce_4_2")
    assert set(k.tolist()) <= {1, 2, 3, 4} and (k == 2).sum() > 50   # most resamples end with the two-component fit
    two = np.nonzero(k == 2)[0]
    assert np.all(np.diff(means[two], axis=1) >= 0)
    # the two filled rows are copies of kept components: every row has exactly two distinct (mean, weight) pairs
    for b in two[:20]:
        assert len({(m, w) for m, w in zip(means[b], weights[b])}) == 2
    o = N.call_locus_n(HAND_CASES["reduce_4_2"][0], np.ones(30), 4, 77)
    assert o["modal_n"] == 2 and o["status"] == R.CALLED and sorted(set(o["call"][:4])) == [10, 30]
    assert sum(o["peak_n_reads"]) == 30 and set(o["read_peak"]) == {0, 1}
    assert o["call"][4:] == [-1, -1] and np.isnan(o["means"][4])


def test_reduction_4_to_2_to_1_ends_at_the_single_gaussian():
    (k, means, weights, stdevs), C = _rows("reduce_4_2_1")
    assert (k == 1).sum() > 50
    # the path itself: rows whose four-component fit has two useless components are fitted again with two components and
    # the draws of round 1; those with one useless component there end at the single Gaussian
    cn, A, p = HAND_CASES["reduce_4_2_1"]
    v, key, bidx = np.unique(cn).astype(np.float64), R.mix64(77), np.arange(p.num_bootstrap)
    gm, _, gw = N.fit_gmm_c(C, v, 39, key, bidx, p, 4, 0)
    via2 = np.nonzero(((C > 0).sum(axis=1) > 1) & (N.useless_components(gm, gw, 4, p) == 2))[0]
    gm, _, gw = N.fit_gmm_c(C[via2], v, 39, key, bidx[via2], p, 2, 1)
    nu2 = N.useless_components(gm, gw, 2, p)
    assert (nu2 == 1).sum() >= 10 and np.all(k[via2[nu2 == 1]] == 1) and np.all(k[via2[nu2 != 1]] == 2)
    one = np.nonzero(k == 1)[0]
    sm, sv = R.single_gaussian(C[one], np.unique(HAND_CASES["reduce_4_2_1"][0]).astype(np.float64), 39)
    for a in range(4):   # four copies of the single Gaussian, weight 1 each
        assert means[one, a].tobytes() == sm.tobytes() and np.all(weights[one, a] == 1.0)
        assert stdevs[one, a].tobytes() == np.sqrt(sv).tobytes()
    o = N.call_locus_n(HAND_CASES["reduce_4_2_1"][0], np.ones(39), 4, 77, HAND_CASES["reduce_4_2_1"][2])
    assert o["modal_n"] == 1 and o["call"][:4] == [20] * 4 and o["peak_n_reads"] == [39, 0]


def test_all_components_useless_keeps_the_last_fit():
    (k, means, weights, stdevs), _ = _rows("all_useless")
    # c = 3 with three useless components: c would fall to 0, the fit stays (two useless lead to the single Gaussian)
    assert np.all(k[(k > 1)] == 3) and (k == 3).sum() > 50
    o = N.call_locus_n(HAND_CASES["all_useless"][0], np.ones(18), 3, 77, HAND_CASES["all_useless"][2])
    assert o["modal_n"] == 3 and o["call"][:3] == [10, 20, 30]
    assert o["status"] == R.CALLED and o["peak_n_reads"] == [0, 0] and set(o["read_peak"]) == {-1}


def test_more_alleles_than_distinct_values():
    cn, A, p = HAND_CASES["potential_0"]
    v = np.unique(cn).astype(np.float64)
    C = np.array([[9, 9], [0, 18], [17, 1]])
    idx = N.kmeanspp_seeds_c(C, v, 18, R.mix64(3), np.arange(3), 0, 6)
    assert idx.shape == (3, 6) and set(idx[0, :2].tolist()) == {0, 1}
    assert idx[1].tolist() == [1] * 6   # potential 0 from the start: the first non-empty value every time
    assert idx[0, 2:].tolist() == [0] * 4   # potential 0 once both values are centres
    o = N.call_locus_n(cn, np.ones(18), A, 5, p)
    assert o["status"] == R.CALLED and sorted(set(o["call"][:6])) == [12, 17] and o["call"][6:] == []
    assert all(np.isfinite(o["means"])) and abs(sum(o["weights"]) - 1.0) < 1e-12


def test_fewer_reads_than_alleles_is_too_few():
    cn, A, p = HAND_CASES["n_below_A"]
    o = N.call_locus_n(cn, np.ones(4), A, 1, p)
    assert o["status"] == R.TOO_FEW and o["modal_n"] == 0 and o["call"] == [-1] * 6 and set(o["read_peak"]) == {-1}
    assert N.call_locus_n(cn, np.ones(4), 4, 1, p)["status"] != R.TOO_FEW
    # one distinct value answers before the check
    o = N.call_locus_n(np.full(4, 8, np.int32), np.ones(4), 6, 1, p)
    assert o["status"] == R.CALLED and o["call"] == [8] * 6 and o["weights"] == [1 / 6] * 6 and o["modal_n"] == 1


def test_local_trials_and_draw_indices():
    assert [N.local_trials(c) for c in range(2, 7)] == [2, 3, 3, 3, 3]
    # at r = 0, c = 2 the draws are those of the two-component rule
    rng = np.random.default_rng(1)
    for t in range(50):
        cn, _, _ = _locus(rng, "hifi")
        if np.unique(cn).shape[0] < 2:
            continue
        cnt, v, m = _counts_row(cn, rng)
        k0, k1 = R.kmeanspp_seeds(cnt[None, :], v, m, R.mix64(t), np.array([t]), 1)
        assert N.kmeanspp_seeds_c(cnt[None, :], v, m, R.mix64(t), np.array([t]), 1, 2)[0].tolist() == [k0[0], k1[0]]


# ----------------------------------------------------------------------------------------------------------------------
# recovery on simulated loci of three and four alleles


@pytest.mark.parametrize("A", [3, 4])
def test_simulated_loci_are_recovered(A):
    rng = np.random.default_rng(4242 + A)
    p = R.Params(num_bootstrap=50)
    n, exact = 12, 0
    for t in range(n):
        cn, truth = _multi_locus(rng, A)
        o = N.call_locus_n(cn, np.ones(cn.shape[0]), A, 900 + t, p)
        print(A, t, truth, o["call"][:A], o["modal_n"])
        assert o["status"] == R.CALLED and o["modal_n"] == A, (t, truth, o["call"], o["modal_n"])
        assert max(abs(a - b) for a, b in zip(o["call"][:A], truth)) <= 1, (t, truth, o["call"])
        exact += o["call"][:A] == truth
    assert exact / n >= 0.9, exact
