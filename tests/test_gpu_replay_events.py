"""k_replay with a lane per read (strk_replay.h): pass 1 searches the band tables a lane per read, and the walk takes only the
EVENTS — reads whose result differs from their start, a fraction reset, a missing or pending result — through its serial code;
the quiet reads between two events commit at once.  Every case is compared field for field with oracle.count_locus, with the
band on and off; the properties the cases are built for (where the events lie, that the reset branch is taken) are asserted on
the oracle's answers and the test's own restatement of the feedback, never on a device run.  HiFi-like loci: motifs of 3-6
bases, flanks of 60-80; est_cn is an input of the batch, so the cases set it."""
import functools

import numpy as np
import pytest

import deep_loci_cases as dc
from helpers import end_probation, hifi_locus, hifi_motif, hifi_seq, oracle_count_pool
from strkit_amd.synth import LocusBatch

pytestmark = pytest.mark.gpu
KEYS = ("cn", "score", "n_iters", "start")
COUNTS = ("dp_cells", "n_fallback", "n_miss_reads", "n_miss_rounds", "n_dedup_reads", "n_band_reads", "n_band_fallback", "band_bytes",
          "exact_bytes", "n_long_reads", "band_cells", "wide_cells", "exact_cells", "long_cells")


# ---- the cases (built once per process; no test changes them) ---------------------------------------------------------------------
def _light(seed, depth, **kw):
    return dc._light_locus(seed, depth, **{**dict(motif_len=(3, 6), flank=(60, 80)), **kw})


def _clean(seed, depth, m=4, cn=20):
    rng = np.random.default_rng(seed)
    return hifi_locus(rng, hifi_motif(rng, m), int(rng.integers(60, 81)), cn * m, int(rng.integers(60, 81)), depth)


@functools.lru_cache(maxsize=None)
def sizes_batch():
    """Loci of 1, 2, 63, 64, 65 and 130 reads, lightly mutated, estimates up to three sizes off: batches of the walk that are
    nearly empty, one short of full, full, one over, and two full ones and a bit."""
    parts = [_light(2100 + d, d) for d in (1, 2, 63, 64, 65, 130)]
    return LocusBatch.from_reads([p[0] for p in parts], [p[1] for p in parts])


@functools.lru_cache(maxsize=None)
def quiet_batch():
    """Loci of 30, 64 and 100 reads whose estimate is the tract's size: no event anywhere."""
    loci = [_clean(2110 + k, d, m=3 + k, cn=18 + k) for k, d in enumerate((30, 64, 100))]
    return LocusBatch.from_reads(loci, [[18 + k] * d for k, d in enumerate((30, 64, 100))])


@functools.lru_cache(maxsize=None)
def all_events_batch():
    """Three loci of 30 reads, estimates alternately one above and one below the tract's size: every read is an event."""
    loci = [_clean(2120 + k, 30, m=3 + k, cn=15 + 2 * k) for k in range(3)]
    return LocusBatch.from_reads(loci, [[15 + 2 * k + (1 if r % 2 else -1) for r in range(30)] for k in range(3)])


SINGLE = (0, 63, 64)


@functools.lru_cache(maxsize=None)
def single_event_batch():
    """Three loci of 130 clean reads with the tract's size as estimate, except one read per locus (in-locus index 0, 63, 64)
    whose estimate is one too small: the first event of the locus lies at the first lane of a batch, at its last lane, and at
    the first lane of the second batch."""
    loci = [_clean(2130 + k, 130, m=4, cn=20) for k in range(3)]
    est = [[20] * 130 for _ in range(3)]
    for k, p in enumerate(SINGLE):
        est[k][p] = 19
    return LocusBatch.from_reads(loci, est)


@functools.lru_cache(maxsize=None)
def reset_batch():
    """Two copies of a 4-base motif between flanks of 70: the first reads carry estimates four sizes above the tract (their result
    pulls the fraction to about -2), the reads behind them an estimate of 1, for which round(frac * est) < -est."""
    rng = np.random.default_rng(2140)
    loci, est = [], []
    for k in range(2):
        motif = hifi_motif(rng, 4 + k)
        loci.append((motif, [(hifi_seq(rng, 70), motif * 2, hifi_seq(rng, 70)) for _ in range(12)]))
        est.append([6, 1, 1, 6, 6, 1, 2, 1, 6, 1, 1, 2])
    return LocusBatch.from_reads(loci, est)


@functools.lru_cache(maxsize=None)
def dup_batch():
    """130 distinct reads, then copies: read 64 of read 63 (the last lane of the batch before), read 128 of read 5."""
    (motif, reads), e = _light(2150, 130, distinct=True)
    for r, q in ((64, 63), (128, 5)):
        reads[r], e[r] = reads[q], e[q]
    return LocusBatch.from_reads([(motif, reads)], [e])


UNCERTAIN_DEPTH, UNCERTAIN_KICK = 130, 40


@functools.lru_cache(maxsize=None)
def uncertain_batch():
    """deep_loci_cases.fanout_batch at 130 reads with the kick at in-locus index 40 (the same windows: its docstring has the
    arithmetic).  Every read certifies from its estimate; read 40 finds its size two above its start, so read 41 starts two sizes
    above its estimate, where its band table does not certify: pass 1 stops there with frac = 2 / 24."""
    rng = np.random.default_rng(2200)
    motif = hifi_motif(rng, dc.FANOUT_MOTIF)
    cn = 24
    reads = [(hifi_seq(rng, 66), motif * cn, hifi_seq(rng, 68)) for _ in range(UNCERTAIN_DEPTH)]
    est = [cn] * UNCERTAIN_DEPTH
    est[UNCERTAIN_KICK] = cn - dc.FANOUT_SHIFT
    return LocusBatch.from_reads([(motif, reads)], [est])


@functools.lru_cache(maxsize=None)
def settings_batch():
    parts = [_light(2160 + k, 30) for k in range(3)]
    return LocusBatch.from_reads([p[0] for p in parts], [p[1] for p in parts])


BATCHES = dict(sizes=sizes_batch, quiet=quiet_batch, all_events=all_events_batch, single=single_event_batch, reset=reset_batch,
               dup=dup_batch, uncertain=uncertain_batch, settings=settings_batch)


@functools.lru_cache(maxsize=None)
def _expected(name, **kw):
    exp = oracle_count_pool(BATCHES[name](), **kw)
    for v in exp.values():
        v.setflags(write=False)
    return exp


def _same(got, exp, b, what):
    for k in KEYS:
        bad = np.nonzero(got[k] != exp[k])[0]
        if bad.size:
            r = int(bad[0])
            l = int(np.searchsorted(b.read_off, r, side="right") - 1)
            assert False, (what, k, f"{bad.size} of {b.n_reads} reads differ", f"first: read {r} = locus {l} read {r - int(b.read_off[l])}",
                           [int(got[x][r]) for x in KEYS], [int(exp[x][r]) for x in KEYS])


def _run(b, ctx, **kw):
    from strkit_amd.batch import count_loci
    return count_loci(b, ctx=ctx, with_stats=True, **kw)


def _both(name, ctx, **kw):
    """The batch with the band on and off against the oracle; returns the statistics of the band run."""
    b = BATCHES[name]()
    exp = _expected(name, **kw)
    got, st = _run(b, ctx, **kw)
    print(name, kw, " ".join(f"{k}={st[k]}" for k in COUNTS))
    _same(got, exp, b, (name, "band"))
    got0, st0 = _run(b, ctx, band=False, **kw)
    _same(got0, exp, b, (name, "exact"))
    assert st0["n_band_reads"] == 0 and st0["n_band_fallback"] == 0, st0
    return b, exp, st


@pytest.fixture
def band_ctx(fresh_ctx):
    """A context of its own whose band is past probation, and the process-wide default window back at its start (+-8)."""
    from strkit_amd import _lib
    _lib.load().strk_adaptive_reset()
    end_probation(fresh_ctx)
    return fresh_ctx


def _feedback_walk(b, exp, l):
    """The caller's feedback restated on the oracle's copy numbers (call_locus.py:1129-1136, 1161): the starts it gives, and
    the reads at which the offset fell below -est and the fraction was reset."""
    frac, starts, resets = 0.0, [], []
    for r in range(int(b.read_off[l]), int(b.read_off[l + 1])):
        est = int(b.est_cn[r])
        off = round(frac * est)
        if off < -est:
            frac, off = 0.0, 0
            resets.append(r)
        starts.append(est + off)
        cn = int(exp["cn"][r])
        if cn != est + off:
            frac += (cn - (est + off)) / max(cn, 1)
    return starts, resets


# ---- the tests -----------------------------------------------------------------------------------------------------------------
def test_loci_of_1_2_63_64_65_and_130_reads(band_ctx):
    b, exp, st = _both("sizes", band_ctx)
    assert st["n_band_reads"] > b.n_reads // 2, st


def test_quiet_loci_commit_every_read_at_its_estimate(band_ctx):
    b, exp, st = _both("quiet", band_ctx)
    assert np.array_equal(exp["start"], b.est_cn) and np.array_equal(exp["cn"], b.est_cn)      # the case is what it says
    assert st["n_band_reads"] == b.n_reads and st["n_miss_reads"] == 0, st


def test_every_read_an_event(band_ctx):
    b, exp, st = _both("all_events", band_ctx)
    assert np.all(exp["cn"] != b.est_cn)
    assert np.any(exp["start"] != b.est_cn)


def test_a_first_event_at_lane_0_at_lane_63_and_at_the_first_lane_of_the_second_batch(band_ctx):
    b, exp, st = _both("single", band_ctx)
    for l, p in enumerate(SINGLE):
        r0 = int(b.read_off[l])
        assert np.array_equal(exp["start"][r0:r0 + p + 1], b.est_cn[r0:r0 + p + 1])             # nothing moves up to the planted read
        assert np.array_equal(exp["cn"][r0:r0 + p], b.est_cn[r0:r0 + p]) and exp["cn"][r0 + p] != b.est_cn[r0 + p]
        assert exp["start"][r0 + p + 1] != b.est_cn[r0 + p + 1]                                  # ... and the read behind it starts elsewhere


def test_a_fraction_below_minus_one_is_reset_at_a_read_with_estimate_1(band_ctx):
    b, exp, st = _both("reset", band_ctx)
    for l in range(b.n_loci):
        r0, r1 = int(b.read_off[l]), int(b.read_off[l + 1])
        starts, resets = _feedback_walk(b, exp, l)
        assert starts == [int(x) for x in exp["start"][r0:r1]]
        assert any(int(b.est_cn[r]) == 1 for r in resets), (l, resets)                             # the reset branch was taken


def test_a_copy_whose_first_occurrence_lies_in_the_batch_before(band_ctx):
    b, exp, st = _both("dup", band_ctx)
    assert dc.copies(b) == 2 and st["n_dedup_reads"] == 2, st


def test_an_uncertain_read_mid_locus_stops_pass_1_and_pass_2_resumes_with_the_fraction(band_ctx):
    """The rule for n_band_fallback: the reads whose search does not certify from their estimate (none here: the control run
    without feedback starts every search at its estimate and must report 0), and behind the first read that does not certify
    from its moved start that read and every later read of the locus that still has a band table: reads 41 .. 129, 89 reads."""
    b = uncertain_batch()
    got_c, st_c = _run(b, band_ctx, feedback=False)
    _same(got_c, _expected("uncertain", feedback=False), b, "control without feedback")
    assert st_c["n_band_reads"] == b.n_reads and st_c["n_band_fallback"] == 0, st_c
    b, exp, st = _both("uncertain", band_ctx)
    k = UNCERTAIN_KICK
    assert int(exp["cn"][k]) == int(b.est_cn[k]) + dc.FANOUT_SHIFT and int(exp["start"][k + 1]) == int(b.est_cn[k + 1]) + dc.FANOUT_SHIFT
    assert st["n_band_reads"] == b.n_reads and st["n_miss_reads"] == 0, st
    assert st["n_band_fallback"] == UNCERTAIN_DEPTH - (k + 1), st


@pytest.mark.parametrize("kw", [dict(feedback=False), dict(tie_rule=1), dict(narrowing=1), dict(narrowing=2), dict(narrowing=3)],
                         ids=["no-feedback", "tie-last", "narrow-decrement", "narrow-halve", "narrow-after-seed"])
def test_other_search_settings(band_ctx, kw):
    _both("settings", band_ctx, **kw)


def test_two_runs_on_one_context_give_equal_outputs_and_equal_counts(band_ctx):
    """The single-event loci and the locus with the uncertain read in one batch: events, a fan-out and a second pass, and few
    enough fall-backs (89 of 520 band reads) that the context keeps its band on for the second run."""
    b = LocusBatch.concat([single_event_batch(), uncertain_batch()])
    exp = {k: np.concatenate([_expected("single")[k], _expected("uncertain")[k]]) for k in KEYS}
    got1, st1 = _run(b, band_ctx)
    got2, st2 = _run(b, band_ctx)
    _same(got1, exp, b, "first run")
    for k in KEYS:
        assert np.array_equal(got1[k], got2[k]), k
    assert {k: st1[k] for k in COUNTS} == {k: st2[k] for k in COUNTS}
    assert st1["n_band_reads"] == b.n_reads and st1["n_band_fallback"] == UNCERTAIN_DEPTH - (UNCERTAIN_KICK + 1), st1
