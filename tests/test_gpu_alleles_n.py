"""GPU: strk_call_alleles_n (k_alleles_n) against strk_call_alleles for one and two alleles, byte for byte, and against the
CPU restatement (tests/alleles_n_restatement.py) for one to six, value for value."""
import ctypes as C
import math

import numpy as np
import pytest

import alleles_n_restatement as N
import alleles_restatement as R
from strkit_amd import _lib
from strkit_amd.alleles import MAX_ALLELES, AlleleParams, call_alleles, call_alleles_batch, call_alleles_n_batch
from test_alleles_n_restatement import HAND_CASES
from test_gpu_alleles import FLOAT_RTOL, _aparams, _close, _locus, _near_half

pytestmark = pytest.mark.gpu


def _flat(loci):
    read_off = np.concatenate([[0], np.cumsum([c.shape[0] for c, _, _ in loci])]).astype(np.int32)
    cn = np.concatenate([c for c, _, _ in loci]).astype(np.int32)
    w = np.concatenate([x for _, x, _ in loci])
    nal = np.array([a for _, _, a in loci], np.int32)
    return read_off, cn, w, nal


def _run_n(loci, seeds, p, ctx):
    read_off, cn, w, nal = _flat(loci)
    return read_off, call_alleles_n_batch(read_off, cn, w, nal, seeds, _aparams(p), ctx)


# ----------------------------------------------------------------------------------------------------------------------
# (a) one and two alleles: the bytes of strk_call_alleles


def test_one_and_two_alleles_equal_call_alleles_byte_for_byte(gpu_ctx):
    rng = np.random.default_rng(20261019)
    loci = [_locus(rng, ("hifi", "hifi", "expansion", "tiny")[t % 4]) for t in range(2000)]
    loci = [(cn, w, 1 + t % 2) for t, (cn, w, _) in enumerate(loci)]
    seeds = rng.integers(0, 1 << 63, len(loci), dtype=np.uint64)
    for p in (R.Params(), R.Params(force_gm_filter=1, n_init=1, num_bootstrap=37)):
        read_off, cn, w, nal = _flat(loci)
        old = call_alleles_batch(read_off, cn, w, nal, seeds, _aparams(p), gpu_ctx)
        new = call_alleles_n_batch(read_off, cn, w, nal, seeds, _aparams(p), gpu_ctx)
        assert set(old) == set(new)
        for k in old:
            if k in ("status", "modal_n", "peak_n_reads", "read_peak"):
                assert old[k].tobytes() == new[k].tobytes(), k
            else:
                assert new[k].shape[1] == MAX_ALLELES
                assert np.ascontiguousarray(new[k][:, :2]).tobytes() == old[k].tobytes(), k
                rest = new[k][:, 2:]
                assert np.all(np.isnan(rest)) if rest.dtype.kind == "f" else np.all(rest == -1), k
        assert set(old["status"].tolist()) == {0, 1, 2} and set(old["modal_n"].tolist()) == {0, 1, 2}


# ----------------------------------------------------------------------------------------------------------------------
# (b) the device against the restatement


def _locus_n(rng, A):
    """One locus for n_alleles = A: (cn, w, A)."""
    kind = int(rng.integers(0, 10))
    if kind < 6:     # up to A + 1 true alleles, mostly exact reads
        t = int(rng.integers(1, A + 2))
        centres = int(rng.integers(3, 60)) + np.cumsum(rng.integers(1, 20, t))
        n = int(rng.integers(A, 61))
        cn = centres[rng.integers(0, t, n)] + rng.choice([0, 0, 0, 1, -1, 2, -2], n)
    elif kind < 8:   # n and d up to 250
        n = int(rng.integers(100, 251))
        cn = rng.integers(1, 1 + int(rng.integers(2, 400)), n)
    elif kind == 8:  # about as many reads as alleles, few values
        n = A + int(rng.integers(0, 3))
        cn = rng.integers(10, 11 + A, n)
    else:            # fewer reads than alleles, or one value
        n = int(rng.integers(1, A + 3))
        cn = rng.integers(10, 12, n) if rng.random() < 0.5 else np.full(n, int(rng.integers(1, 100)))
    cn = np.asarray(cn, dtype=np.int32)
    wk = rng.integers(0, 3)
    if wk == 0:
        w = np.ones(cn.shape[0])
    elif wk == 1:
        w = rng.pareto(1.5, cn.shape[0]) + 1e-3
    else:
        w = rng.random(cn.shape[0]) * 1e-12 + 1e-14
    return cn, w, A


CORPUS_SEED = 20261019   # (see the note at MAX_DRIFT_FRACTION)


def corpus(seed=CORPUS_SEED):
    """Groups of (params, loci, seeds); about 400 loci in all, n_alleles 1..6 in turn, and the hand cases of
    test_alleles_n_restatement.py under their own parameters."""
    rng = np.random.default_rng(seed)
    groups = [
        (R.Params(), 198),
        (R.Params(force_gm_filter=1), 48),
        (R.Params(num_bootstrap=2), 36),
        (R.Params(num_bootstrap=3, n_init=1), 36),
        (R.Params(max_iter=1), 36),
        (R.Params(n_init=1, min_allele_reads=3, filter_factor=2, min_reads=2), 36),
    ]
    out = []
    for p, n in groups:
        loci = [_locus_n(rng, 1 + t % MAX_ALLELES) for t in range(n)]
        out.append((p, loci, rng.integers(0, 1 << 63, n, dtype=np.uint64)))
    for cn, A, p in HAND_CASES.values():
        out.append((p, [(cn, np.ones(cn.shape[0]), A)], np.array([77], np.uint64)))
    return out


_expected = {}


def expected(seed=CORPUS_SEED):
    """The restatement's result for every locus of the corpus, computed once."""
    if seed not in _expected:
        _expected[seed] = [[N.call_locus_n(cn, w, A, int(s), p) for (cn, w, A), s in zip(loci, seeds)]
                           for p, loci, seeds in corpus(seed)]
    return _expected[seed]


def differing_fields(got, l, exp, r0, r1):
    out = []
    for k in ("status", "modal_n", "call", "ci95", "ci99", "peak_n_reads"):
        if np.asarray(got[k][l]).ravel().tolist() != list(np.ravel(exp[k])):
            out.append(k)
    if np.asarray(got["read_peak"][r0:r1]).tolist() != exp["read_peak"].tolist():
        out.append("read_peak")
    for k in ("means", "weights", "stdevs"):
        if not _close(got[k][l], exp[k]):
            out.append(k)
    return out


def from_tied_bootstraps(got, l, exp, A) -> bool:
    """The weights and stdevs of locus l are those of bootstraps tied at the median: per allele a stdev of a tied
    bootstrap, and weights that are tied bootstraps' raw weights over one common total, their own sum."""
    cands = exp["median_cands"]
    gw, gs = np.asarray(got["weights"][l], np.float64), np.asarray(got["stdevs"][l], np.float64)
    for a in range(A):
        if not np.any(np.abs(cands[a][1] - gs[a]) <= FLOAT_RTOL * np.abs(cands[a][1])):
            return False
    totals = [cands[a][0] / gw[a] for a in range(A)]
    for T in totals[0]:
        pick = []
        for a in range(A):
            near = np.nonzero(np.abs(totals[a] - T) <= 4 * FLOAT_RTOL * T)[0]
            if near.size == 0:
                break
            pick.append(float(cands[a][0][near[0]]))
        if len(pick) == A and abs(sum(pick) - T) <= 4 * A * FLOAT_RTOL * T:
            return True
    return False


def compare(groups, exp_groups, got_of):
    """Every locus of the corpus: its result `got_of(group index, params, loci, seeds) -> (read_off, arrays)` against the
    restatement's.  Returns (checked, exempt, tied, tied_resolved, drift, broken): `drift` the loci that part otherwise than
    by the two exemptions, `broken` those among them that do not keep what a drifting locus must (calls within 1, equal
    status)."""
    exempt = tied = tied_resolved = checked = 0
    drift, broken = [], []
    for gi, ((p, loci, seeds), exps) in enumerate(zip(groups, exp_groups)):
        read_off, got = got_of(gi, p, loci, seeds)
        for l, ((cn, w, A), exp) in enumerate(zip(loci, exps)):
            ctx = (p, l, cn.tolist()[:20], A)
            r0, r1 = read_off[l], read_off[l + 1]
            checked += 1
            diff = differing_fields(got, l, exp, r0, r1)
            if exp["median_tie"]:
                tied += 1
                if {"weights", "stdevs"} & set(diff) and from_tied_bootstraps(got, l, exp, A):
                    tied_resolved += 1
                    diff = [k for k in diff if k not in ("weights", "stdevs")]
            if not diff:
                continue
            if set(diff) <= {"call", "ci95", "ci99"} and any(_near_half(x) for x in exp["means"] if not math.isnan(x)):
                exempt += 1   # a rounding at a half-point may go either way between two libms
                continue
            drift.append((f"group {gi} locus {l} (n_alleles {A}, {cn.shape[0]} reads)", diff,
                          {k: (np.asarray(got[k][l]).ravel()[:2 * A].tolist(), list(np.ravel(exp[k]))[:2 * A]) for k in diff
                           if k != "read_peak"}))
            if int(got["status"][l]) != exp["status"] or np.any(np.abs(np.asarray(got["call"][l]) - np.asarray(exp["call"])) > 1):
                broken.append((ctx, int(got["status"][l]), exp["status"], np.asarray(got["call"][l]).tolist(), exp["call"]))
    return checked, exempt, tied, tied_resolved, drift, broken


# Loci where device and restatement may part: at most 1 % of the corpus, each with calls within 1 and equal status.
# Device and host differ in the last bit of exp / log / sqrt, and the expanded log density magnifies it (tests/test_gpu_alleles.py
# names the ways in which that shows).  A fit of more components than the sample has clusters is less well conditioned than
# the two-component one: components that sit on one value share its weight in any split, and a weight can sit on a filter
# threshold exactly (one read of n split over s components against 1 / (filter_factor c)), so that the last bit decides a
# bootstrap's component count.
# The corpus was looked at on the CPU first: tools/alleles_n_ulp_probe.py runs the restatement against itself with exp / log /
# sqrt moved by one ulp at random on EVERY call.  That is far harsher than the device (whose functions agree with the host's
# on most arguments): 21 to 23 loci of this corpus part under it, 3 of them by more than 1 in a call, and three other
# seeds gave 14 to 23, so no seed stays within the cap under that probe.  What the probe did show is that the fill-up draw
# had to be made on the components in the order of their means: before, about 100 loci parted.
# Measured on the device: 3 of the 396 loci, the same 3 on every run (both sides are deterministic):
#   group 0 locus 55 (n_alleles 2, 10 reads): one bootstrap's mean crosses the median on the device, so the median is the
#     neighbouring bootstrap (means 57.50624 / 57.50962, 6e-5 apart) with its own weight and stdev;
#   group 1 locus 22 (n_alleles 5, 48 reads): the same at allele 3, between two bootstraps whose means are 5e-7 apart
#     (63.250036 / 63.250067: equal within the tolerance, but not a tie of 1e-9), so only weights and stdevs differ;
#   group 2 locus 17 (n_alleles 6, B = 2): a component collapsed onto one value (var = reg_covar + the cancellation noise);
#     its stdev 0.0010000018 / 0.0010000032 lies just beyond the float tolerance.
MAX_DRIFT_FRACTION = 0.01


def test_device_equals_restatement(gpu_ctx):
    groups = corpus()
    checked, exempt, tied, tied_resolved, drift, broken = compare(groups, expected(),
                                                                  lambda gi, p, loci, seeds: _run_n(loci, seeds, p, gpu_ctx))
    print(f"device == restatement on {checked - exempt - len(drift)} of {checked} loci (discrete outputs exact, floats "
          f"within {FLOAT_RTOL:g} relative); {exempt} exempt at a rounding half-point; {tied} with a tie at the median, "
          f"of which {tied_resolved} report the weights / stdevs of another of the tied bootstraps; "
          f"{len(drift)} drifted, differing in {[d[:2] for d in drift]}")
    for d in drift:
        print(d)
    assert 390 <= checked <= 410
    assert not broken, broken   # a drifting locus keeps its status, and its calls stay within 1
    assert len(drift) <= MAX_DRIFT_FRACTION * checked, [d[:2] for d in drift]
    # the corpus reaches what it is there for: called and too few (an empty peak needs at most two peaks: that code is
    # k_alleles', which the identity test reaches), and every modal number of peaks
    exps = [e for g in expected() for e in g]
    assert {e["status"] for e in exps} >= {0, 1} and {e["modal_n"] for e in exps} >= {0, 1, 2, 3, 4, 5, 6}


# ----------------------------------------------------------------------------------------------------------------------
# (c) a locus alone and inside a large call; two runs


def test_locus_alone_equals_locus_in_a_call_of_5000_and_runs_repeat(gpu_ctx):
    rng = np.random.default_rng(3)
    loci = [_locus_n(rng, 1 + t % MAX_ALLELES) for t in range(5000)]
    seeds = np.arange(5000, dtype=np.uint64) * np.uint64(7919) + np.uint64(1)
    p = R.Params()
    read_off, big = _run_n(loci, seeds, p, gpu_ctx)
    _, again = _run_n(loci, seeds, p, gpu_ctx)
    for k in big:
        assert big[k].tobytes() == again[k].tobytes(), k
    for l in (0, 1, 5, 777, 3210, 4999):
        _, one = _run_n([loci[l]], seeds[l:l + 1], p, gpu_ctx)
        for k in one:
            if k == "read_peak":
                assert np.array_equal(one[k], big[k][read_off[l]:read_off[l + 1]]), (l, k)
            else:
                assert one[k][0].tobytes() == big[k][l].tobytes(), (l, k)


# ----------------------------------------------------------------------------------------------------------------------
# (d) refusals


def _lib_call(ctx, read_off, cn, w, nal, seeds, p):
    n = len(read_off) - 1
    M = MAX_ALLELES
    outs = [np.full(n, 123, np.int32), np.full(n, 123, np.int32), np.full(M * n, 123, np.int32),
            np.full(2 * M * n, 123, np.int32), np.full(2 * M * n, 123, np.int32), np.full(M * n, 123.0), np.full(M * n, 123.0),
            np.full(M * n, 123.0), np.full(2 * n, 123, np.int32), np.full(len(cn), 123, np.int32)]
    arrs = [np.ascontiguousarray(a) for a in (read_off, cn, w, nal, seeds)]
    rc = _lib.load().strk_call_alleles_n(ctx.handle, n, *[C.c_void_p(a.ctypes.data) for a in arrs], C.byref(p._c()),
                                         *[C.c_void_p(a.ctypes.data) for a in outs], None)
    return rc, outs


def test_invalid_input_is_rejected_before_any_launch(gpu_ctx):
    ro = np.array([0, 5, 10], np.int32)
    cn = np.arange(10, dtype=np.int32)
    w = np.ones(10)
    nal = np.array([2, 6], np.int32)
    seeds = np.array([1, 2], np.uint64)
    ok = AlleleParams()
    cases = [
        (ro, cn, w, np.array([2, 7], np.int32), ok, "locus 1: n_alleles 7"),
        (ro, cn, w, np.array([0, 2], np.int32), ok, "locus 0: n_alleles 0"),
        (ro, cn, np.where(np.arange(10) == 7, 0.0, 1.0), nal, ok, "locus 1"),
        (ro, cn, np.where(np.arange(10) == 2, np.nan, 1.0), nal, ok, "locus 0"),
        (ro, cn, np.where(np.arange(10) == 6, -1.0, 1.0), nal, ok, "locus 1"),
        (ro, cn, w, nal, AlleleParams(num_bootstrap=1), "num_bootstrap"),
        (ro, cn, w, nal, AlleleParams(num_bootstrap=1025), "num_bootstrap"),
        (ro, cn, w, nal, AlleleParams(n_init=0), "n_init"),
        (ro, cn, w, nal, AlleleParams(n_init=16), "n_init"),
        (ro, cn, w, nal, AlleleParams(reg_covar=0.0), "reg_covar"),
    ]
    for r, c, ww, a, p, msg in cases:
        rc, outs = _lib_call(gpu_ctx, r, c, ww, a, seeds, p)
        assert rc == _lib.STRK_E_INVALID, msg
        err = _lib.load().strk_last_error().decode()
        assert msg in err and "strk_call_alleles_n" in err, err
        assert all(np.all(o == 123) for o in outs)   # nothing was written: no launch happened
    rc, outs = _lib_call(gpu_ctx, ro, cn, w, nal, seeds, ok)
    assert rc == 0 and not np.any(outs[0] == 123) and not np.any(outs[-1] == 123)


# ----------------------------------------------------------------------------------------------------------------------
# (e) the reference's signature


def test_reference_signature_with_four_alleles_equals_batch(gpu_ctx):
    rng = np.random.default_rng(8)
    called = 0
    for t in range(12):
        cn, w, _ = _locus_n(rng, 4)
        k = cn.shape[0] // 2
        seed = int(rng.integers(0, 1 << 62))
        cd = call_alleles(cn[:k], cn[k:], w[:k], w[k:], AlleleParams(), 4, 4, False, 10, seed, None, "", ctx=gpu_ctx)
        out = call_alleles_n_batch(np.array([0, cn.shape[0]], np.int32), cn, w, [4], [seed], AlleleParams(), gpu_ctx)
        if out["status"][0] == R.TOO_FEW:
            assert cd is None
            continue
        called += 1
        assert cd.call.tolist() == out["call"][0, :4].tolist() and cd.call.shape == (4,)
        assert cd.call_95_cis.tolist() == out["ci95"][0, :4].tolist()
        assert cd.call_99_cis.tolist() == out["ci99"][0, :4].tolist()
        assert cd.peak_modal_n == int(out["modal_n"][0])
        assert cd.peak_means.tobytes() == out["means"][0, :4].tobytes()
        assert cd.read_peaks.tolist() == out["read_peak"].tolist()
        d = cd.to_dict()
        assert d["peaks"]["modal_n"] == cd.peak_modal_n and len(d["peaks"]["means"]) == cd.peak_modal_n
        if cd.peak_modal_n > 2:
            assert d["peaks"]["n_reads"] == [] and set(cd.read_peaks.tolist()) == {-1}
        else:
            assert len(d["peaks"]["n_reads"]) == cd.peak_modal_n
    assert called >= 6
