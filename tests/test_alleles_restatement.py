"""CPU: the allele-calling restatement (tests/alleles_restatement.py) against sklearn and against the edge rules of
DESIGN.md §9.  The restatement is what tests/test_gpu_alleles.py holds the device to."""
import numpy as np
import pytest

import alleles_restatement as R


def _hifi_locus(rng, n_reads=30, het=True):
    """Copy numbers shaped like HiFi data: two alleles, mostly exact, a few +-1 (rarely +-2) reads."""
    a1 = int(rng.integers(5, 60))
    a2 = a1 + int(rng.integers(1, 25)) if het else a1
    n1 = n_reads // 2 + int(rng.integers(-3, 4))
    truth = np.concatenate([np.full(n1, a1), np.full(n_reads - n1, a2)])
    noise = rng.choice([0, 0, 0, 0, 0, 0, 1, -1, 2, -2], size=n_reads, p=[.14] * 6 + [.07, .07, .01, .01])
    cn = (truth + noise).astype(np.int32)
    rng.shuffle(cn)
    return cn, sorted((a1, a2))


def _counts_row(cn, rng):
    """One bootstrap-like sample as (counts over distinct values, distinct values, m)."""
    v = np.unique(cn)
    sample = rng.choice(cn, size=cn.shape[0])
    c = np.array([(sample == x).sum() for x in v], dtype=np.int64)
    return c, v.astype(np.float64), int(cn.shape[0])


# ----------------------------------------------------------------------------------------------------------------------
# 1. the EM is sklearn's, init for init


def test_em_equals_sklearn_per_init(monkeypatch):
    pytest.importorskip("sklearn")
    import sklearn.mixture._base as base
    from sklearn.mixture import GaussianMixture

    rng = np.random.default_rng(11)
    p = R.Params()
    checked = 0
    for t in range(60):
        cn, _ = _hifi_locus(rng, n_reads=int(rng.integers(8, 60)), het=t % 4 != 0)
        c, v, m = _counts_row(cn, rng)
        if (c > 0).sum() < 2:
            continue
        C = c[None, :]
        key = R.mix64(t)
        X = np.repeat(v, c).reshape(-1, 1)
        first_idx = np.concatenate([[0], np.cumsum(c)[:-1]])
        for init in range(3):
            k0, k1 = R.kmeanspp_seeds(C, v, m, key, np.array([t]), init)
            idx = np.array([first_idx[k0[0]], first_idx[k1[0]]])
            monkeypatch.setattr(base, "kmeans_plusplus", lambda *a, _i=idx, **k: (X[_i], _i))
            g = GaussianMixture(2, covariance_type="spherical", init_params="k-means++", n_init=1, tol=p.tol,
                                reg_covar=p.reg_covar, max_iter=p.max_iter, random_state=0).fit(X)
            means, var, weights, lb, n_iter = R.em_fit(C, v, m, v[k0], v[k1], p)
            assert int(n_iter[0]) == g.n_iter_, (t, init)
            np.testing.assert_allclose(means[0], g.means_[:, 0], rtol=1e-9, atol=0)
            # var = E[x^2] - mean^2: its rounding error scales with mean^2, not with var (a collapsed component has
            # var = reg_covar + a few ulps of mean^2)
            np.testing.assert_allclose(var[0], g.covariances_, rtol=1e-9, atol=1e-15 * float(np.max(v)) ** 2)
            np.testing.assert_allclose(weights[0], g.weights_, rtol=1e-9, atol=0)
            # the expanded log density cancels terms of size mean^2 * precision (1e6 for a collapsed component): the lower
            # bound carries that absolute error, whatever the order of its sums
            np.testing.assert_allclose(lb[0], g.lower_bound_, rtol=1e-9, atol=1e-6)
            checked += 1
    assert checked >= 120


def test_kmeanspp_seeds_follow_sklearn_rule():
    """The candidate rule on counts equals sklearn's searchsorted on the expanded sample."""
    rng = np.random.default_rng(5)
    for t in range(200):
        cn, _ = _hifi_locus(rng, n_reads=int(rng.integers(6, 40)))
        c, v, m = _counts_row(cn, rng)
        if (c > 0).sum() < 2:
            continue
        key = R.mix64(t)
        k0, k1 = R.kmeanspp_seeds(c[None, :], v, m, key, np.array([3]), 1)
        X = np.repeat(v, c)
        s0 = min(int(np.floor(R.uniforms(key, 1, 3, 1, 0) * m)), m - 1)
        assert X[s0] == v[k0[0]]
        d2 = (X - X[s0]) ** 2
        pot = d2.sum()
        best, best_pot = None, None
        for tr in range(2):
            i = min(int(np.searchsorted(np.cumsum(d2), R.uniforms(key, 1, 3, 1, 1 + tr) * pot)), m - 1)
            cp = np.minimum(d2, (X - X[i]) ** 2).sum()
            if best is None or cp < best_pot:
                best, best_pot = i, cp
        assert X[best] == v[k1[0]]


# ----------------------------------------------------------------------------------------------------------------------
# 2. the whole loop against the same loop driven by stock sklearn

# Measured on 300 seeded loci (seed 2024, 30 reads, B 40): 297 of 300 calls agree, none differs by more than 1.
AGREEMENT_FLOOR = 0.97
LOOP_PARAMS = R.Params(num_bootstrap=40)   # 40 rather than 100 resamples keeps sklearn's share of the test under a minute


def _sklearn_loop_call(cn, w, n_alleles, seed, p=R.Params()):
    """call_alleles' loop with stock sklearn fits (random k-means++ seeds, n_init 3) on the restatement's resamples."""
    from sklearn.mixture import GaussianMixture

    rng = np.random.default_rng(seed)
    B = p.num_bootstrap
    v_int = np.unique(cn)
    if v_int.shape[0] == 1:
        return [int(v_int[0])] * n_alleles
    key = R.mix64(seed)
    cdf = np.cumsum(w)
    cdf /= cdf[-1]
    n = cn.shape[0]
    u = R.uniforms(key, 0, np.arange(B)[:, None], 0, np.arange(n)[None, :])
    samples = np.sort(cn[np.searchsorted(cdf, u, side="right")], axis=1, kind="stable")
    allele_filter = (p.min_allele_reads - 0.1) / B
    rows = []
    for s in samples:
        X = s.reshape(-1, 1).astype(np.float64)
        if np.unique(s).shape[0] == 1:
            means = np.array([X.mean()])
        else:
            g = GaussianMixture(2, covariance_type="spherical", init_params="k-means++", n_init=p.n_init,
                                random_state=int(rng.integers(0, 2 ** 31))).fit(X)
            wts, mns = g.weights_, g.means_[:, 0]
            srt = np.sort(mns)
            strict = p.force_gm_filter or srt[-1] < p.expansion_ratio * max(srt[0], R.SMALL_ALLELE_MIN)
            f = (wts > allele_filter) & (wts > (1 / (p.filter_factor * 2) if strict else R.EPS32))
            means = np.array([X.mean()]) if f.sum() == 1 else mns
        if means.shape[0] < n_alleles:
            means = np.repeat(means, 2)
        rows.append(np.sort(means)[:n_alleles])
    rows = np.sort(np.array(rows), axis=0)
    return [int(np.rint(x)) for x in rows[B // 2]]


def test_calls_agree_with_stock_sklearn_loop():
    pytest.importorskip("sklearn")
    rng = np.random.default_rng(2024)
    same = 0
    n = 300
    for t in range(n):
        cn, _ = _hifi_locus(rng, het=t % 3 != 0)
        w = np.ones(cn.shape[0])
        ours = R.call_locus(cn, w, 2, t, LOOP_PARAMS)["call"]
        ref = _sklearn_loop_call(cn, w, 2, t, LOOP_PARAMS)
        assert max(abs(a - b) for a, b in zip(ours, ref)) <= 1, (t, ours, ref)
        same += ours == ref
    print(f"{same} of {n} calls agree with the stock-sklearn loop")
    assert same / n >= AGREEMENT_FLOOR, same


# ----------------------------------------------------------------------------------------------------------------------
# 3. edge rules


def test_too_few_reads_is_not_called():
    o = R.call_locus(np.array([10, 12, 14], np.int32), np.ones(3), 2, 1)
    assert o["status"] == R.TOO_FEW and o["modal_n"] == 0 and list(o["read_peak"]) == [-1, -1, -1]
    assert R.call_locus(np.array([10, 12, 14, 16], np.int32), np.ones(4), 2, 1)["status"] != R.TOO_FEW


@pytest.mark.parametrize("n_alleles", [1, 2])
def test_one_value_skips_the_bootstrap(n_alleles):
    o = R.call_locus(np.full(7, 23, np.int32), np.linspace(0.1, 2, 7), n_alleles, 9)
    assert o["status"] == R.CALLED and o["modal_n"] == 1
    assert o["call"][:n_alleles] == [23] * n_alleles
    assert o["ci95"][:2 * n_alleles] == [23] * 2 * n_alleles and o["ci99"][:2 * n_alleles] == [23] * 2 * n_alleles
    assert o["weights"][:n_alleles] == [1.0 / n_alleles] * n_alleles and o["stdevs"][:n_alleles] == [0.0] * n_alleles
    assert o["peak_n_reads"] == [7, 0] and set(o["read_peak"]) == {0}


def test_allele_filter_divides_by_the_bootstrap_count():
    """min_allele_reads - 0.1 over B, not over n: with B = 4 a 3-of-40-read allele (weight ~0.075) fails the filter
    (1.9 / 4 = 0.475) and the locus collapses to one peak, with B = 100 (0.019) it survives."""
    cn = np.array([20] * 37 + [40] * 3, np.int32)
    w = np.ones(40)
    p100 = R.Params(force_gm_filter=0, expansion_ratio=1.5)
    assert R.call_locus(cn, w, 2, 3, p100)["call"] == [20, 40]
    p4 = R.Params(num_bootstrap=4, expansion_ratio=1.5)
    o = R.call_locus(cn, w, 2, 3, p4)
    assert o["modal_n"] == 1 and o["call"][0] == o["call"][1]


def test_expansion_ratio_lifts_the_weight_filter():
    """A large expansion with few reads keeps its peak (filter 2 drops to float32 eps) unless force_gm_filter."""
    cn = np.array([20] * 26 + [600] * 3, np.int32)
    w = np.ones(cn.shape[0])
    assert R.call_locus(cn, w, 2, 5)["call"] == [20, 600]
    forced = R.call_locus(cn, w, 2, 5, R.Params(force_gm_filter=1))
    assert forced["modal_n"] == 1 and forced["call"][1] < 600   # mostly one Gaussian over all reads


def test_one_component_is_duplicated_and_sorted():
    rng = np.random.default_rng(0)
    C = np.array([[5, 0, 0, 25]])
    v = np.array([10.0, 11.0, 12.0, 13.0])
    k, means, weights, stdevs = R.fit_rows(C, v, 30, 2, R.mix64(1), np.array([0]), R.Params(filter_factor=1))
    assert k[0] == 1 and means[0, 0] == means[0, 1] and weights[0].tolist() == [1.0, 1.0]
    assert stdevs[0, 0] == stdevs[0, 1] > 0
    k, means, *_ = R.fit_rows(C, v, 30, 2, R.mix64(1), np.array([0]), R.Params())
    assert k[0] == 2 and means[0, 0] <= means[0, 1]
    del rng


def test_stream_is_the_specified_splitmix():
    assert R.mix64(0) == 0
    key = R.mix64(42)
    x = R.mix64((key + R.GAMMA * (1 + ((1 << 60) | (7 << 40) | (2 << 36) | 5))) & R.M64)
    assert R.uniforms(key, 1, 7, 2, 5) == (x >> 11) * 2.0 ** -53
    assert R.locus_seed(1, 0) == R.mix64((1 + R.GAMMA) & R.M64)


def test_clean_two_allele_loci_give_their_alleles():
    rng = np.random.default_rng(77)
    for t in range(40):
        a1 = int(rng.integers(5, 80))
        a2 = a1 + int(rng.integers(3, 40))
        cn = np.array([a1] * 15 + [a2] * 15, np.int32)
        cn[rng.integers(0, 30, 3)] += rng.choice([-1, 1], 3)
        rng.shuffle(cn)
        o = R.call_locus(cn, np.ones(30), 2, t)
        assert o["status"] == R.CALLED and o["call"] == [a1, a2], (t, o["call"], a1, a2)
        assert o["modal_n"] == 2 and sorted(o["peak_n_reads"]) != [0, 30]
