"""GPU: strk_call_alleles (k_alleles) against the CPU restatement (tests/alleles_restatement.py), value for value."""
import math

import numpy as np
import pytest

import alleles_restatement as R
from strkit_amd import _lib
from strkit_amd.alleles import EMPTY_PEAK as EMPTY
from strkit_amd.alleles import AlleleParams, call_alleles, call_alleles_batch

pytestmark = pytest.mark.gpu


def _aparams(p: R.Params) -> AlleleParams:
    return AlleleParams(min_reads=p.min_reads, min_allele_reads=p.min_allele_reads, num_bootstrap=p.num_bootstrap,
                        n_init=p.n_init, max_iter=p.max_iter, filter_factor=p.filter_factor,
                        force_gm_filter=bool(p.force_gm_filter), tol=p.tol, reg_covar=p.reg_covar,
                        expansion_ratio=p.expansion_ratio)


def _locus(rng, kind):
    """One locus of a given shape: (cn, w, n_alleles)."""
    if kind == "hifi":
        n = int(rng.integers(1, 60))
        a1 = int(rng.integers(3, 120))
        a2 = a1 + int(rng.integers(0, 30))
        cn = np.where(rng.random(n) < 0.5, a1, a2) + rng.choice([0, 0, 0, 1, -1, 2, -2], n)
    elif kind == "wide":   # n and d up to 250
        n = int(rng.integers(100, 251))
        cn = rng.integers(1, 1 + int(rng.integers(2, 400)), n)
    elif kind == "expansion":
        n_small = int(rng.integers(8, 30))
        cn = np.concatenate([rng.integers(18, 22, n_small), rng.integers(590, 611, int(rng.integers(2, 4)))])
        rng.shuffle(cn)
    elif kind == "tiny":
        n = int(rng.integers(1, 8))
        cn = rng.integers(10, 14, n)
    else:   # one value
        cn = np.full(int(rng.integers(1, 40)), int(rng.integers(1, 100)))
    cn = np.asarray(cn, dtype=np.int32)
    wk = rng.integers(0, 3)
    if wk == 0:
        w = np.ones(cn.shape[0])
    elif wk == 1:
        w = rng.pareto(1.5, cn.shape[0]) + 1e-3     # skewed
    else:
        w = rng.random(cn.shape[0]) * 1e-12 + 1e-14  # tiny
    return cn, w, int(rng.integers(1, 3)) if rng.random() < 0.3 else 2


def _corpus():
    """Groups of (params, loci); about 3 000 loci in all."""
    rng = np.random.default_rng(20261016)
    kinds = ["hifi"] * 6 + ["wide", "expansion", "tiny", "one"]
    groups = [
        (R.Params(), 1800),
        (R.Params(force_gm_filter=1), 300),
        (R.Params(num_bootstrap=2), 200),
        (R.Params(num_bootstrap=3, n_init=1), 200),
        (R.Params(max_iter=1), 200),
        (R.Params(n_init=1, min_allele_reads=3, filter_factor=2), 260),
        (R.Params(num_bootstrap=1024), 40),
    ]
    out = []
    for p, n in groups:
        loci = [_locus(rng, kinds[int(rng.integers(len(kinds)))]) for _ in range(n)]
        seeds = rng.integers(0, 1 << 63, n, dtype=np.uint64)
        out.append((p, loci, seeds))
    return out


def _run(loci, seeds, p, ctx):
    read_off = np.concatenate([[0], np.cumsum([c.shape[0] for c, _, _ in loci])]).astype(np.int32)
    cn = np.concatenate([c for c, _, _ in loci]).astype(np.int32)
    w = np.concatenate([x for _, x, _ in loci])
    nal = np.array([a for _, _, a in loci], np.int32)
    return read_off, call_alleles_batch(read_off, cn, w, nal, seeds, _aparams(p), ctx)


def _near_half(x):
    return abs((x % 1.0) - 0.5) < 1e-7


# Float tolerance.  Device and host differ in the last bit of exp / log / sqrt; sklearn's expanded log density
# (mean^2 prec - 2 x mean prec + x^2 prec) cancels terms of size mean^2 * prec (up to 1e10 for a collapsed component
# at 100 copies), which turns such a bit into a relative difference of up to ~1e-8 in the EM's weights.
FLOAT_RTOL = 1e-6
_worst = [0.0]


def _close(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    both_nan = np.isnan(a) & np.isnan(b)
    with np.errstate(invalid="ignore", divide="ignore"):
        rel = np.where(both_nan | (a == b), 0.0, np.abs(a - b) / np.maximum(np.abs(b), 1e-300))
    ok = bool(np.all(rel <= FLOAT_RTOL))
    if ok:
        _worst[0] = max(_worst[0], float(np.max(rel)))
    return ok


def _worst_matching() -> float:
    return _worst[0]


# Loci where device and restatement part (measured: 4 of the 3 000, the same 4 on every run: both sides are
# deterministic).  Device and host differ in the last bit of exp / log / sqrt, and the expanded log density magnifies it.
# Where two inits of one bootstrap reach lower bounds equal to within that noise, the two sides keep different ones (both
# converged to tol), and that bootstrap's mean moves by up to ~tol (group 0 loci 384 and 932); where a read sits on the
# boundary of the peak rule (|peak - cn| / stdev against 1, or two equal log densities), it may change peak (group 0
# locus 1490); where a component has collapsed onto one value (var = reg_covar + the cancellation noise), its stdev may
# land just beyond the float tolerance (group 1 locus 121).  The calls stay within 1.
MAX_DRIFT = 5


def _differing_fields(got, l, exp, r0, r1):
    out = []
    for k in ("status", "modal_n", "call", "ci95", "ci99", "peak_n_reads"):
        if np.asarray(got[k][l]).ravel().tolist() != list(np.ravel(exp[k])):
            out.append(k)
    if got["read_peak"][r0:r1].tolist() != exp["read_peak"].tolist():
        out.append("read_peak")
    for k in ("means", "weights", "stdevs"):
        if not _close(got[k][l], exp[k]):
            out.append(k)
    return out


def _from_tied_bootstraps(got, l, exp, nal) -> bool:
    cands = exp["median_cands"]
    for a in range(nal):
        if not np.any(np.abs(cands[a][1] - got["stdevs"][l, a]) <= FLOAT_RTOL * np.abs(cands[a][1])):
            return False
    raw = [c[0] for c in cands]
    if nal == 1:
        return abs(got["weights"][l, 0] - 1.0) <= FLOAT_RTOL
    tot = raw[0][:, None] + raw[1][None, :]
    w0, w1 = raw[0][:, None] / tot, raw[1][None, :] / tot
    return bool(np.any((np.abs(w0 - got["weights"][l, 0]) <= FLOAT_RTOL * w0)
                       & (np.abs(w1 - got["weights"][l, 1]) <= FLOAT_RTOL * w1)))


def test_device_equals_restatement(gpu_ctx):
    exempt = tied = tied_resolved = checked = 0
    drift = []
    for gi, (p, loci, seeds) in enumerate(_corpus()):
        read_off, got = _run(loci, seeds, p, gpu_ctx)
        for l, (cn, w, nal) in enumerate(loci):
            exp = R.call_locus(cn, w, nal, int(seeds[l]), p)
            ctx = (p, l, cn.tolist()[:20], nal)
            r0, r1 = read_off[l], read_off[l + 1]
            checked += 1
            diff = _differing_fields(got, l, exp, r0, r1)
            if exp["median_tie"]:
                # Several bootstraps share the median mean (to 1e-9) with other weights / stdevs, and the last bits of
                # the means decide which one the stable sort puts at the median.  The device's weights and stdevs must
                # then be those of one of the tied bootstraps (weights renormalised over the alleles' picks).
                tied += 1
                if {"weights", "stdevs"} & set(diff) and _from_tied_bootstraps(got, l, exp, nal):
                    tied_resolved += 1
                    diff = [k for k in diff if k not in ("weights", "stdevs")]
            if not diff:
                continue
            if set(diff) <= {"call", "ci95", "ci99"} and any(_near_half(x) for x in exp["means"] if not math.isnan(x)):
                exempt += 1   # a rounding at a half-point may go either way between two libms
                continue
            assert int(got["status"][l]) == exp["status"] or EMPTY in (int(got["status"][l]), exp["status"]), ctx
            assert np.all(np.abs(got["call"][l] - np.asarray(exp["call"])) <= 1), (ctx, got["call"][l], exp["call"])
            drift.append((f"group {gi} locus {l}", diff))
    print(f"device == restatement on {checked - exempt - len(drift)} of {checked} loci (discrete outputs exact, floats "
          f"within {FLOAT_RTOL:g} relative); {exempt} exempt at a rounding half-point; {tied} with a tie at the median, "
          f"of which {tied_resolved} report the weights / stdevs of another of the tied bootstraps; "
          f"{len(drift)} drifted, differing in {drift}; largest relative float difference on the matching loci and "
          f"fields {_worst_matching():.2e}")
    assert len(drift) <= MAX_DRIFT, drift
    assert checked == 3000


def test_locus_alone_equals_locus_in_a_large_call_and_runs_repeat(gpu_ctx):
    rng = np.random.default_rng(3)
    loci = [_locus(rng, "hifi") for _ in range(20000)]
    seeds = np.arange(20000, dtype=np.uint64) * np.uint64(7919) + np.uint64(1)
    p = R.Params()
    read_off, big = _run(loci, seeds, p, gpu_ctx)
    _, again = _run(loci, seeds, p, gpu_ctx)
    for k in big:
        assert np.array_equal(big[k], again[k], equal_nan=True), k
        assert big[k].tobytes() == again[k].tobytes(), k
    for l in (0, 1, 777, 12345, 19999):
        _, one = _run([loci[l]], seeds[l:l + 1], p, gpu_ctx)
        for k in one:
            if k == "read_peak":
                assert np.array_equal(one[k], big[k][read_off[l]:read_off[l + 1]])
            else:
                assert one[k][0].tobytes() == big[k][l].tobytes(), (l, k)


def _lib_call(ctx, read_off, cn, w, nal, seeds, p):
    n = len(read_off) - 1
    outs = [np.zeros(n, np.int32), np.zeros(n, np.int32), np.zeros(2 * n, np.int32), np.zeros(4 * n, np.int32),
            np.zeros(4 * n, np.int32), np.zeros(2 * n), np.zeros(2 * n), np.zeros(2 * n), np.zeros(2 * n, np.int32),
            np.full(len(cn), 123, np.int32)]
    arrs = [np.ascontiguousarray(a) for a in (read_off, cn, w, nal, seeds)]
    import ctypes as C
    rc = _lib.load().strk_call_alleles(ctx.handle, n, *[C.c_void_p(a.ctypes.data) for a in arrs], C.byref(p._c()),
                                       *[C.c_void_p(a.ctypes.data) for a in outs], None)
    return rc, outs


def test_invalid_input_is_rejected_before_any_launch(gpu_ctx):
    ro = np.array([0, 5, 10], np.int32)
    cn = np.arange(10, dtype=np.int32)
    w = np.ones(10)
    nal = np.array([2, 2], np.int32)
    seeds = np.array([1, 2], np.uint64)
    ok = AlleleParams()
    cases = [
        (ro, cn, w, np.array([2, 3], np.int32), ok, "locus 1"),
        (ro, cn, w, np.array([0, 2], np.int32), ok, "locus 0"),
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
        assert msg in _lib.load().strk_last_error().decode()
        assert np.all(outs[-1] == 123)   # nothing was written: no launch happened
    big_ro = np.array([0, 65536], np.int32)
    rc, outs = _lib_call(gpu_ctx, big_ro, np.ones(65536, np.int32), np.ones(65536), np.array([2], np.int32),
                         seeds[:1], ok)
    assert rc == _lib.STRK_E_INVALID and "locus 0" in _lib.load().strk_last_error().decode()
    assert np.all(outs[-1] == 123)


def test_reference_signature_equals_batch(gpu_ctx):
    rng = np.random.default_rng(8)
    for t in range(20):
        cn, w, nal = _locus(rng, "hifi" if t % 4 else "expansion")
        k = cn.shape[0] // 2
        seed = int(rng.integers(0, 1 << 62))
        cd = call_alleles(cn[:k], cn[k:], w[:k], w[k:], AlleleParams(), 4, nal, False, 10, seed, None, "", ctx=gpu_ctx)
        out = call_alleles_batch(np.array([0, cn.shape[0]], np.int32), cn, w, [nal], [seed], AlleleParams(), gpu_ctx)
        if out["status"][0] == R.TOO_FEW:
            assert cd is None
            continue
        assert cd.call.tolist() == out["call"][0, :nal].tolist()
        assert cd.call_95_cis.tolist() == out["ci95"][0, :nal].tolist()
        assert cd.call_99_cis.tolist() == out["ci99"][0, :nal].tolist()
        assert cd.peak_modal_n == int(out["modal_n"][0])
        assert cd.peak_means.tobytes() == out["means"][0, :nal].tobytes()
        assert cd.read_peaks.tolist() == out["read_peak"].tolist()
        d = cd.to_dict()
        assert d["peaks"]["modal_n"] == cd.peak_modal_n and len(d["peaks"]["means"]) == cd.peak_modal_n
    with pytest.raises(NotImplementedError):
        call_alleles(np.array([5, 6, 7]), np.array([5, 6]), np.ones(3), np.ones(2), AlleleParams(), 4, 2, True, 1, 1,
                     None, "", ctx=gpu_ctx)


def test_calls_cut_into_pieces_equal_loci_called_alone(gpu_ctx):
    """A call is cut into pieces of at most 32 768 loci and 512 MB of workspace; loci of a later piece (relative read
    offsets, results written back at the piece's offset) equal the same loci called alone."""
    rng = np.random.default_rng(12)
    p = R.Params()
    loci = [_locus(rng, "hifi") for _ in range(40000)]
    seeds = rng.integers(0, 1 << 63, len(loci), dtype=np.uint64)
    read_off, big = _run(loci, seeds, p, gpu_ctx)
    for l in (32767, 32768, 32769, 39999):
        _, one = _run([loci[l]], seeds[l:l + 1], p, gpu_ctx)
        for k in one:
            if k == "read_peak":
                assert np.array_equal(one[k], big[k][read_off[l]:read_off[l + 1]]), (l, k)
            else:
                assert one[k][0].tobytes() == big[k][l].tobytes(), (l, k)
    exp = R.call_locus(*loci[39999][:2], loci[39999][2], int(seeds[39999]), p)
    assert big["call"][39999].tolist() == exp["call"] and big["status"][39999] == exp["status"]

    # workspace cut: 40 000 reads with B = 1024 take 2 x 1024 x 40 000 bytes of count rows (82 MB) per locus, so seven
    # such loci need two pieces of 512 MB
    pb = R.Params(num_bootstrap=1024)
    wide = []
    for _ in range(7):
        cn = rng.integers(20, 26, 40000).astype(np.int32)
        cn[rng.random(40000) < 0.5] += 12
        wide.append((cn, np.ones(40000), 2))
    wseeds = rng.integers(0, 1 << 63, 7, dtype=np.uint64)
    read_off, big = _run(wide, wseeds, pb, gpu_ctx)
    for l in (0, 6):
        _, one = _run([wide[l]], wseeds[l:l + 1], pb, gpu_ctx)
        for k in one:
            if k == "read_peak":
                assert np.array_equal(one[k], big[k][read_off[l]:read_off[l + 1]]), (l, k)
            else:
                assert one[k][0].tobytes() == big[k][l].tobytes(), (l, k)
    assert big["status"].tolist() == [0] * 7 and np.all(big["modal_n"] == 2)
