"""CPU: the call driver without a device — error isolation and the paused collector, the three block feeds, options by
field name and the report's parameters block, the reader decision, and the gather codec without processes."""
import dataclasses
import gc

import pytest

from strkit_amd import _lib
from strkit_amd.alleles import AlleleParams
from strkit_amd.frontend import call
from strkit_amd.frontend.call import CallOptions, call_blocks, call_locus, call_sample
from strkit_amd.frontend.loci import Locus
from strkit_amd.repeat_count_params import RepeatCountParams


def _loci(n, contig="chr1"):
    return [Locus(i + 1, f"l{i + 1}", contig, 1000 * i + 100, 1000 * i + 130, "CAG") for i in range(n)]


class _Boom(RuntimeError):
    pass


def _isolation_run(monkeypatch, fail=(2, 4), other_error_at=None):
    loci = _loci(7)
    blocks = [loci[0:3], loci[3:4], loci[4:7]]
    calls = []

    def runner(block, records, opts, ctx, tm, known):
        calls.append([l.t_idx for l in block])
        assert known == [{"ref": l.t_idx} for l in block]
        if any(l.t_idx == other_error_at for l in block):
            raise _Boom("not the library's")
        if any(l.t_idx in fail for l in block):
            raise _lib.StrkError(-22, "made up")
        return [{"locus_index": l.t_idx} for l in reversed(block)], len(block)

    monkeypatch.setattr(call, "_call_block_python", runner)
    ref_cache = {id(l): {"ref": l.t_idx} for l in loci}
    return calls, lambda: call_blocks(blocks, object(), None, CallOptions(), ctx=object(), ref_cache=ref_cache)


@pytest.mark.parametrize("collector_on", [True, False])
def test_a_library_error_costs_only_the_locus_that_fails(monkeypatch, capsys, collector_on):
    calls, run = _isolation_run(monkeypatch)
    was_on = gc.isenabled()
    try:
        gc.enable() if collector_on else gc.disable()
        rows, n_depth, tm = run()
        assert gc.isenabled() == collector_on
        assert [r["locus_index"] for r in rows] == [1, 3, 5, 6, 7] and n_depth == 5
        assert [e["locus_index"] for e in tm["errors"]] == [2, 4] and all("made up" in e["error"] for e in tm["errors"])
        assert calls == [[1, 2, 3], [1], [2], [3], [4], [5, 6, 7]]
        err = capsys.readouterr().err
        assert err.count("skipping locus") == 2
        # any other exception is not the worker's to swallow, and the collector is left as it was found all the same
        calls, run = _isolation_run(monkeypatch, other_error_at=4)
        with pytest.raises(_Boom):
            run()
        assert gc.isenabled() == collector_on and calls == [[1, 2, 3], [1], [2], [3], [4]]
    finally:
        gc.enable() if was_on else gc.disable()


class _FakeIndexed:
    """Stands in for an IndexedBam: records every region() request."""

    def __init__(self, log):
        self.log = log

    def region(self, contig, beg, end, slot=0):
        self.log.append(("load", contig, beg, end, slot))
        return ("records", contig, beg, end)


def test_prefetch_feed_rotates_three_slots_and_stays_one_block_ahead():
    loci = _loci(10)
    blocks = [loci[2 * k:2 * k + 2] for k in range(5)]
    log, tm = [], {}
    feed = call._PrefetchFeed(blocks, _FakeIndexed(log), tm)
    try:
        for k, (block, records) in enumerate(feed):
            assert block == blocks[k]
            assert records == ("records", "chr1", block[0].left_flank_coord, block[-1].right_flank_coord + 1)
            if k + 1 < len(blocks):
                feed.fut.result()                  # (the request is in flight: wait for it so that the log's order is fixed)
            log.append(("run", k))
    finally:
        feed.close()
    loads = [e for e in log if e[0] == "load"]
    assert [e[4] for e in loads] == [0, 1, 2, 0, 1]
    for k in range(4):                             # block k + 1 is requested before block k is run
        assert log.index(loads[k + 1]) < log.index(("run", k))
    assert set(tm) == {"load_s", "load_wait_s"}
    empty = call._PrefetchFeed([], _FakeIndexed(log), {})
    assert list(empty) == []
    empty.close()


class _FakeStreamed:
    def __init__(self):
        self.log = []

    def plan(self, blocks):
        self.planned = blocks
        return [("chr1", 0, 10, blocks[:2]), ("chr2", 5, 9, blocks[2:])]

    def load_span(self, contig, beg, end):
        self.log.append((contig, beg, end))


def test_span_feed_loads_every_planned_group_once():
    a, b = _loci(3, "chr1"), _loci(3, "chr2")
    bam, tm = _FakeStreamed(), {}
    mixed = [a[0], a[1], b[0]]                      # a hand-made block that mixes contigs
    got = []
    for block, records in call._span_feed([mixed, [a[2]], [b[1], b[2]]], bam, tm):
        assert records is bam
        got.append((block, list(bam.log)))
    assert bam.planned == [[a[0], a[1]], [b[0]], [a[2]], [b[1], b[2]]]
    assert [blk for blk, _ in got] == bam.planned
    assert [len(seen) for _, seen in got] == [1, 1, 2, 2] and bam.log == [("chr1", 0, 10), ("chr2", 5, 9)]
    assert list(tm) == ["load_s"]


def test_one_contig_blocks_split_a_mixed_block_where_the_contig_changes():
    a, b = _loci(3, "chr1"), _loci(2, "chr2")
    assert call._one_contig_blocks([a[0], a[1], b[0], a[2], b[1]]) == [[a[0], a[1]], [b[0]], [a[2]], [b[1]]]
    assert call._one_contig_blocks(a) == [a] and call._one_contig_blocks([]) == []


NON_DEFAULT = dict(flank_size=50, realign=True, min_avg_phred=20, max_reads=100, respect_ref=True,
                   rc_params=RepeatCountParams("repalign", 50, 3, 1), min_read_align_score=0.5, tie_rule=1, end_flags=5, narrowing=2,
                   call_alleles=True, consensus=True, seed=7, n_alleles={"chrX": 1},
                   allele_params=AlleleParams(min_reads=5, min_allele_reads=3, num_bootstrap=50), large_consensus_length=800,
                   max_n_large_consensus_reads=10, count_kmers="both")


def test_every_option_reaches_call_options_by_its_name(monkeypatch):
    names = [f.name for f in dataclasses.fields(CallOptions)]
    assert sorted(NON_DEFAULT) == sorted(names)                  # a field added later has to be added here
    assert all(NON_DEFAULT[n] != getattr(CallOptions(), n) for n in names)
    seen = []

    def fake_call_blocks(blocks, bam, ref, opts=None, ctx=None, ref_cache=None):
        seen.append(opts)
        return [[{"locus_index": 1}], 0, {}]

    monkeypatch.setattr(call, "call_blocks", fake_call_blocks)
    locus = _loci(1)[0]
    for name in names:                                           # one at a time: no value can land in a neighbour's slot
        call_locus(locus, None, None, **{name: NON_DEFAULT[name]})
        assert seen[-1] == dataclasses.replace(CallOptions(), **{name: NON_DEFAULT[name]})
    call_locus(locus, None, None, **NON_DEFAULT)
    assert seen[-1] == CallOptions(**NON_DEFAULT)
    call_locus(locus, None, None, opts=CallOptions(**NON_DEFAULT), realign=False)
    assert seen[-1] == dataclasses.replace(CallOptions(**NON_DEFAULT), realign=False)
    for fn in (call_locus, call_sample):
        with pytest.raises(TypeError):
            fn("reads.bam", "ref.fa", "loci.bed", flanksize=70)
    with pytest.raises(ValueError, match="seed"):                # call_sample draws one; call_blocks wants it drawn
        call_blocks([], None, None, CallOptions(call_alleles=True))


class _FakeReader:
    references = ["chr1"]


class _FakeRef:
    references = ["chr1"]


def test_call_sample_builds_its_options_by_name_and_reports_them(monkeypatch, tmp_path):
    """call_sample with a ready reader and a stubbed block loop: the options that arrive, and the parameters block, for the
    defaults and for a set with every option away from its default."""
    seen = []

    def fake_call_blocks(blocks, bam, ref, opts=None, ctx=None, ref_cache=None):
        seen.append(opts)
        return [], 0, {"errors": []}

    monkeypatch.setattr(call, "call_blocks", fake_call_blocks)
    loci = tmp_path / "loci.bed"
    loci.write_text("chr1\t100\t130\tCAG\n")
    rep = call_sample(_FakeReader(), _FakeRef(), str(loci))
    assert seen[-1] == CallOptions()
    for name in (f.name for f in dataclasses.fields(CallOptions)):          # one at a time, as for call_locus above
        if name not in ("consensus", "count_kmers"):                        # (these two need call_alleles beside them)
            call_sample(_FakeReader(), _FakeRef(), str(loci), **{name: NON_DEFAULT[name]})
            want = dataclasses.replace(CallOptions(), **{name: NON_DEFAULT[name]})
            assert dataclasses.replace(seen[-1], seed=want.seed) == want and (name != "call_alleles" or isinstance(seen[-1].seed, int))
    call_sample(_FakeReader(), _FakeRef(), str(loci), call_alleles=True, seed=7, consensus=True, count_kmers="both")
    assert seen[-1] == CallOptions(call_alleles=True, seed=7, consensus=True, count_kmers="both")
    assert list(rep["parameters"].items()) == list({
        "flank_size": 70, "realign": False, "min_avg_phred": 13, "max_reads": 250, "respect_ref": False, "rc_method": "repalign",
        "min_read_align_score": 0.1, "processes": 1}.items())
    rep = call_sample(_FakeReader(), _FakeRef(), str(loci), processes=3, sample_id="s", **NON_DEFAULT)
    assert seen[-1] == CallOptions(**NON_DEFAULT) and rep["sample_id"] == "s"
    assert list(rep["parameters"].items()) == list({
        "flank_size": 50, "realign": True, "min_avg_phred": 20, "max_reads": 100, "respect_ref": True, "rc_method": "repalign",
        "min_read_align_score": 0.5, "processes": 3, "tie_rule": 1, "end_flags": 5, "narrowing": 2, "call_alleles": True,
        "seed": 7, "n_alleles": {"chrX": 1}, "min_reads": 5, "min_allele_reads": 3, "num_bootstrap": 50, "consensus": True,
        "large_consensus_length": 800, "max_n_large_consensus_reads": 10, "count_kmers": "both"}.items())
    rep = call_sample(_FakeReader(), _FakeRef(), str(loci), call_alleles=True)          # the seed is drawn once, and reported
    assert isinstance(seen[-1].seed, int) and rep["parameters"]["seed"] == seen[-1].seed
    assert rep["parameters"]["n_alleles"] == 2 and rep["parameters"]["num_bootstrap"] == AlleleParams().num_bootstrap
    assert "consensus" not in rep["parameters"] and "count_kmers" not in rep["parameters"]


def test_reader_decision_table():
    from strkit_amd.frontend.reader import DEVICE_SPANS, DEVICE_WHOLE, HOST_INDEXED, HOST_STREAM, RESIDENT_FACTOR, choose_reader
    free = 100 << 30
    small, large = 1 << 30, 20 << 30                  # 7.5 GiB and 150 GiB resident against 90 GiB usable
    assert small * RESIDENT_FACTOR < 0.9 * free < large * RESIDENT_FACTOR
    table = {
        # (front_end, file, index, distributed): reader
        ("auto", small, True, False): DEVICE_WHOLE, ("auto", small, False, False): DEVICE_WHOLE,
        ("auto", large, True, False): DEVICE_SPANS, ("auto", large, False, False): HOST_STREAM,
        ("auto", small, True, True): DEVICE_SPANS, ("auto", small, False, True): DEVICE_WHOLE,
        ("auto", large, True, True): DEVICE_SPANS, ("auto", large, False, True): HOST_STREAM,
        ("device", small, True, False): DEVICE_WHOLE, ("device", small, False, False): DEVICE_WHOLE,
        ("device", large, True, False): DEVICE_SPANS, ("device", large, False, False): DEVICE_WHOLE,
        ("device", small, True, True): DEVICE_SPANS, ("device", small, False, True): DEVICE_WHOLE,
        ("device", large, True, True): DEVICE_SPANS, ("device", large, False, True): DEVICE_WHOLE,
        ("host", small, True, False): HOST_INDEXED, ("host", small, False, False): HOST_STREAM,
        ("host", large, True, False): HOST_INDEXED, ("host", large, False, False): HOST_STREAM,
        ("host", small, True, True): HOST_INDEXED, ("host", small, False, True): HOST_STREAM,
        ("host", large, True, True): HOST_INDEXED, ("host", large, False, True): HOST_STREAM,
    }
    assert len(table) == 3 * 2 * 2 * 2
    for (front_end, size, index, distributed), want in table.items():
        assert choose_reader(front_end, size, free, index, distributed) == want, (front_end, size, index, distributed)
    # no device (no free memory known): nothing is small
    assert choose_reader("auto", small, 0, False, False) == HOST_STREAM and choose_reader("auto", small, 0, True, False) == DEVICE_SPANS
    for bad in ("gpu", "", "Device"):
        with pytest.raises(ValueError, match="front_end"):
            choose_reader(bad, small, free, True, False)


def test_gathered_records_decode_to_the_rows_they_were_made_from():
    """_encode_rows -> _decode_rows without processes, over the rows of the two-rank test: a skipped locus, a failed one, a
    score that is None, a realigned read, a name longer than the default field."""
    import numpy as np
    from helpers import FakeRef, fake_rows, gloo_blocks
    from strkit_amd.frontend.gather import _NAME_BYTES, _decode_rows, _encode_rows
    blocks, ref = gloo_blocks(), FakeRef()
    rows, _n, tm = fake_rows(blocks, ref)
    recs = [x for r in rows for x in (r.get("reads") or {}).values()]
    assert any("reads" not in r for r in rows) and tm["errors"]
    assert any(x["sc"] is None for x in recs) and any(x.get("realn") for x in recs)
    assert any(len(nm) > _NAME_BYTES for r in rows for nm in (r.get("reads") or {}))
    by_index = {l.t_idx: l for blk in blocks for l in blk}
    shuffled = rows[1::2] + rows[0::2]                          # as the ranks' shares arrive: not in catalog order
    loci_t, reads_t, names_t = _encode_rows(shuffled, tm["errors"])
    assert loci_t.dtype == reads_t.dtype == np.int64 and names_t.dtype == np.uint8 and names_t.shape[1] > _NAME_BYTES
    got, errors = _decode_rows(by_index, ref, False, loci_t, reads_t, names_t)
    assert got == sorted(rows, key=lambda r: r["locus_index"])
    assert [e["locus_index"] for e in errors] == sorted(e["locus_index"] for e in tm["errors"])
