"""The counting path on loci of 63 to 250 reads (the reference takes up to max_reads = 250 per locus).  k_replay is one wave per
locus with one lane per read: behind read 63 it runs a second chunk of 64 — the feedback fraction carried over the chunk edge,
the resume between its two passes at a position that is no multiple of 64, the fan-out of an uncertain certificate over more
than 64 trailing reads, copies whose first occurrence lies in an earlier chunk — and the host's miss rounds and sub-batches see
single loci larger than their thresholds.  Every expected value is the CPU oracle's (tests/deep_loci_cases.py holds the inputs,
tests/test_deep_loci_cases.py the conditions on them); a device run is never the expected value of another."""
import functools
import time

import numpy as np
import pytest

import deep_loci_cases as dc
from helpers import device_count, end_probation, oracle_count_pool
from strkit_amd.synth import LocusBatch

pytestmark = pytest.mark.gpu
KEYS = ("cn", "score", "n_iters", "start")
STATS = ("n_band_reads", "n_band_fallback", "n_dedup_reads", "n_miss_reads", "n_miss_rounds", "n_sub_batches", "n_long_reads", "n_fallback")


@functools.lru_cache(maxsize=None)
def _expected(name, **kw):
    """The oracle's answers for a batch of the corpus under one set of search parameters: computed once, shared by the band,
    dedupe and entry-point variants, and not changed by any of them."""
    b = getattr(dc, name)()
    b = b[0] if isinstance(b, tuple) else b
    t0 = time.perf_counter()
    exp = oracle_count_pool(b, **kw)
    print(f"oracle {name} {kw}: {b.n_reads} reads in {time.perf_counter() - t0:.2f} s")
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
    from strkit_amd.repeat_count_params import RepeatCountParams
    rc = RepeatCountParams("repalign", kw.pop("max_iters", 50), kw.pop("lsr", 3), kw.pop("step", 1))
    return count_loci(b, rc, ctx=ctx, with_stats=True, **kw)


def _show(what, st):
    print(what, " ".join(f"{k}={st[k]}" for k in STATS))


@pytest.fixture
def band_ctx(fresh_ctx):
    """A context of its own whose band is past probation, and the process-wide default window back at its start (+-8)."""
    from strkit_amd import _lib
    _lib.load().strk_adaptive_reset()
    end_probation(fresh_ctx)
    return fresh_ctx


# ---- 1. depth sweep ------------------------------------------------------------------------------------------------------
SEARCHES = {"tie-last-lsr1-step2": dict(tie_rule=1, lsr=1, step=2), "narrowing": dict(narrowing=1)}


@pytest.mark.parametrize("dedupe", [True, False], ids=["dedupe", "no-dedupe"])
@pytest.mark.parametrize("band", [True, False], ids=["band", "exact"])
@pytest.mark.parametrize("feedback", [True, False], ids=["feedback", "no-feedback"])
def test_depth_sweep(band_ctx, feedback, band, dedupe):
    """One locus per depth (63, 64, 65, 100, 128, 129 and 250 reads, lightly mutated, estimates up to three sizes off) in one
    batch: with the feedback on, the start of most reads behind in-locus index 64 depends on the fraction the first chunk hands
    to the second."""
    b = dc.sweep_batch()
    got, st = _run(b, band_ctx, feedback=feedback, band=band, dedupe=dedupe)
    _show(f"sweep feedback={feedback} band={band} dedupe={dedupe}", st)
    _same(got, _expected("sweep_batch", feedback=feedback), b, "sweep")
    assert (st["n_band_reads"] > b.n_reads // 2) if band else st["n_band_reads"] == 0, st
    assert st["n_dedup_reads"] == (dc.copies(b) if dedupe else 0), st


@pytest.mark.parametrize("search", list(SEARCHES))
def test_depth_sweep_under_other_search_parameters(band_ctx, search):
    b = dc.sweep_batch()
    kw = SEARCHES[search]
    got, st = _run(b, band_ctx, **dict(kw))
    _show(f"sweep {search}", st)
    _same(got, _expected("sweep_batch", **kw), b, search)
    assert st["n_band_reads"] > b.n_reads // 2, st


# ---- 2. resume position between the two replay passes ----------------------------------------------------------------------------
def test_pass_two_resumes_at_a_planted_exact_read_anywhere_in_the_locus(band_ctx):
    """Nine loci of 200 band reads with one read (two in the last locus) that only the exact kernels can score, at in-locus
    positions 0, 1, 63, 64, 65, 100, 128, 199 and 10 + 140: pass 1 of k_replay stops there, pass 2 takes the locus up from
    next_read[l] with the fraction of pass 1 — every start behind the first read of a locus is its estimate moved by that
    fraction.  A planted read with a right flank of 128-255 bases never enters the band lists (k_dp_long scores it); one with ten
    distinct symbols is listed by k_plan (the geometry fits), refused by the band kernel, and scored by the generic kernel."""
    b, planted = dc.resume_batch()
    n_flank = sum(lv == "flank" for _, _, lv in planted)
    n_symbols = sum(lv == "symbols" for _, _, lv in planted)
    assert n_flank == n_symbols == 5
    got, st = _run(b, band_ctx)
    _show("resume", st)
    _same(got, _expected("resume_batch"), b, "resume")
    assert st["n_long_reads"] >= n_flank, st
    assert st["n_fallback"] >= n_symbols and st["n_band_fallback"] >= n_symbols, st
    assert st["n_dedup_reads"] == 0 and st["n_band_reads"] + st["n_dedup_reads"] + n_flank == b.n_reads, st
    assert st["n_miss_reads"] == 0, st


# ---- 3. certificate fan-out over more than 64 trailing reads ------------------------------------------------------------------
def test_an_uncertain_certificate_sends_more_than_64_trailing_reads_to_the_exact_kernels(band_ctx):
    """deep_loci_cases.fanout_batch: 200 clean reads that all certify from their estimate; the feedback puts the start of read
    65 two sizes above its estimate, where its banded table is uncertain, and pass 1 of k_replay lists reads 65 .. 199 for the
    exact kernels — the only way to the fall-back counter in this batch.
    Control (a condition on the inputs, not an expected value): the first 64 reads as a batch of their own all certify."""
    b = dc.fanout_batch()
    head = LocusBatch.from_reads([(b.motif(0), [b.read(r) for r in range(dc.CHUNK)])], [[int(x) for x in b.est_cn[:dc.CHUNK]]])
    exp = _expected("fanout_batch")
    got0, st0 = _run(head, band_ctx)
    _show("fan-out control (first 64 reads)", st0)
    _same(got0, {k: v[:dc.CHUNK] for k, v in exp.items()}, head, "first 64 reads")
    assert st0["n_band_reads"] == dc.CHUNK and st0["n_band_fallback"] == 0, st0
    got, st = _run(b, band_ctx)
    _show("fan-out", st)
    _same(got, exp, b, "fan-out")
    assert st["n_band_reads"] == b.n_reads, st
    assert st["n_band_fallback"] >= 65, st           # a second trip of the fan-out loop: one trip lists at most 64 reads
    assert st["n_miss_reads"] == 0, st


# ---- 4. window misses in deep loci ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["miss_slice_batch", "miss_bulk_batch", "miss_copies_batch"])
def test_window_misses_in_deep_loci(fresh_ctx, case):
    """Estimates up to nine sizes off against tables of the estimate +-1 and +-3.  Three loci of 150 reads: the host fetches
    their slices, and from a locus's second round on it takes the reads behind the miss along — more than 48 items from one
    locus, the full-size-image upload.  Thirty loci of 70 reads: the bulk copies.  Three loci of 150 reads drawn from seven:
    copies in a later chunk are replayed on the table of a first occurrence in an earlier one."""
    b = getattr(dc, case)()
    exp = _expected(case)
    for window in (1, 3):
        got, st = _run(b, fresh_ctx, window=window)
        _show(f"{case} window={window}", st)
        _same(got, exp, b, (case, window))
        assert st["n_miss_reads"] > 0 and st["n_miss_rounds"] >= 2, st
        if case == "miss_copies_batch":
            assert st["n_dedup_reads"] == dc.copies(b), st


# ---- 5. duplicates across chunks ------------------------------------------------------------------------------------------------
def test_copies_of_a_read_in_another_chunk_share_its_table(band_ctx):
    """250 reads drawn from 5 (some copies with another estimate: not merged), 250 copies of one read, one pair of equal reads
    at in-locus indices 0 and 249, a first occurrence at 63 with copies at 64 and 128: dedupe merges exactly the reads that
    equal an earlier read of their locus in bytes, split and estimate, and the answers do not depend on it."""
    b = dc.dup_batch()
    exp = _expected("dup_batch")
    want = dc.copies(b)
    got, st = _run(b, band_ctx)
    _show("duplicates", st)
    _same(got, exp, b, "dedupe")
    assert st["n_dedup_reads"] == want, (st, want)
    got2, st2 = _run(b, band_ctx, dedupe=False)
    _show("duplicates, dedupe off", st2)
    _same(got2, exp, b, "no dedupe")
    assert st2["n_dedup_reads"] == 0 and st2["n_band_reads"] > st["n_band_reads"], st2      # every copy is an item of its own
    got3, st3 = _run(b, band_ctx, band=False)
    _same(got3, exp, b, "dedupe, exact kernels")
    assert st3["n_dedup_reads"] == want and st3["n_band_reads"] == 0


# ---- 6. entry points ---------------------------------------------------------------------------------------------------------
def test_sweep_through_the_resident_buffer_entry_point(band_ctx):
    b = dc.sweep_batch()
    got, st = device_count(b, band_ctx)
    _show("sweep, resident buffers", st)
    _same(got, _expected("sweep_batch", feedback=True), b, "resident buffers")
    assert st["n_band_reads"] > b.n_reads // 2 and st["n_dedup_reads"] == dc.copies(b)


def test_sweep_through_the_host_pipeline_with_loci_larger_than_a_sub_batch(monkeypatch):
    """STRKIT_AMD_PIPE_MB=1: the first three sub-batch budgets are an eighth, a quarter and a half of a megabyte, and the batch
    opens and ends with a 250-read locus that is larger than the first of them on its own."""
    from strkit_amd import _lib
    monkeypatch.setenv("STRKIT_AMD_PIPE_MB", "1")
    b, sweep = dc.pipe_batch(), dc.sweep_batch()
    mid = _expected("sweep_batch", feedback=True)
    pads = _expected("pipe_pads_batch")
    exp = {k: np.concatenate([pads[k][:250], mid[k], pads[k][250:]]) for k in KEYS}
    assert b.n_reads == sweep.n_reads + 500
    ctx = _lib.Context(0)
    try:
        got, st = _run(b, ctx)
        _show("sweep + padding, host pipeline", st)
        _same(got, exp, b, "host pipeline")
        assert st["n_sub_batches"] >= 2, st
    finally:
        ctx.close()


# ---- 7. the front end at depth -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("max_reads", [250, 70])
def test_call_gives_the_same_read_records_on_both_front_ends_at_80_reads_per_locus(gpu_ctx, tmp_path, max_reads):
    """Three loci of 80 error-free reads: with max_reads = 250 every read is called, with 70 the first 70 of a locus in file order
    (call_locus.py:1056-1058); the copy numbers are the writer's."""
    from strkit_amd.frontend import call_sample, load_loci, read_bam
    from strkit_amd.frontend.synth_dataset import make_dataset
    t = make_dataset(str(tmp_path), n_loci=3, reads_per_locus=80, read_len=1500)
    p = t["paths"]
    dev = call_sample(p["bam"], p["ref"], p["loci"], front_end="device", max_reads=max_reads)
    host = call_sample(p["bam"], p["ref"], p["loci"], front_end="host", max_reads=max_reads)
    assert dev["stage_times"]["front_end"] == "device" and host["stage_times"]["front_end"] == "host"
    assert dev["results"] == host["results"] and len(dev["results"]) == 3
    bam, (block,) = read_bam(p["bam"]), load_loci(p["loci"])
    for locus, res, truth in zip(block, dev["results"], t["loci"]):
        in_file_order = [s.name for s in bam.fetch(locus.contig, locus.left_flank_coord, locus.right_flank_coord)]
        assert len(in_file_order) == 80 and set(in_file_order) == set(truth["reads"])
        assert set(res["reads"]) == set(in_file_order[:max_reads]) and len(res["reads"]) == min(80, max_reads)
        for name, rd in res["reads"].items():
            assert rd["cn"] == truth["reads"][name] and rd["sc"] == 2.0
