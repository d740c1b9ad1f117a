"""The conditions the deep-locus corpus (tests/deep_loci_cases.py) has to meet for tests/test_gpu_deep_loci.py to test what it
says it tests, checked on the CPU with the oracle: which reads the feedback moves, where the planted reads sit and why no band or
fast exact class takes them, that the searches of the resume and fan-out cases stay inside the default window, how many reads
dedupe has to merge, and the byte sizes the host pipeline cuts by."""
import numpy as np

import deep_loci_cases as dc
from helpers import oracle_count_pool

DEFAULT_WINDOW = 8      # strk_policy.h: a process starts at 8 sizes either side of the estimate
REACH = 4               # a search scores local_search_range + step_size = 4 sizes beyond its start and beyond its result


def _locus(b, l):
    return int(b.read_off[l]), int(b.read_off[l + 1])


def _inside_default_window(b, exp):
    """A search scores no size further than REACH from its start or from the size it ends at: with both within 4 of the estimate
    it stays inside a table of the estimate +- 8."""
    return int(np.maximum(abs(exp["start"] - b.est_cn), abs(exp["cn"] - b.est_cn)).max()) + REACH <= DEFAULT_WINDOW


def test_sweep_has_the_depths_and_the_feedback_moves_starts_on_both_sides_of_read_64():
    b = dc.sweep_batch()
    depths = [d for d, _ in dc.SWEEP]
    assert {64, 65, 128, 129, 250, 100} <= set(depths) and np.diff(b.read_off).tolist() == depths
    assert int((b.nfl + b.ntr + b.nfr).max()) <= 512 and 58 <= int(b.nfl.min()) and int(b.nfr.max()) <= 72      # flanks of 60-70, an indel each at most
    exp = oracle_count_pool(b)
    flat = oracle_count_pool(b, feedback=False)
    assert np.array_equal(flat["start"], b.est_cn)
    behind = np.zeros(b.n_reads, bool)
    for l, depth in enumerate(depths):
        r0, r1 = _locus(b, l)
        behind[r0 + dc.CHUNK:r1] = True
        moved = exp["start"][r0:r1] != b.est_cn[r0:r1]
        assert moved[:dc.CHUNK].any(), depth
        if depth > dc.CHUNK:
            assert moved[dc.CHUNK:].any(), depth
    # ... and what the search returns depends on it: a wrong fraction behind the chunk edge shows in the compared outputs
    assert int(behind.sum()) == sum(max(0, d - dc.CHUNK) for d in depths)
    assert int(((exp["start"] != b.est_cn) & behind).sum()) > int(behind.sum()) // 2
    assert int(((exp["n_iters"] != flat["n_iters"]) & behind).sum()) > int(behind.sum()) // 4


def test_resume_case_plants_exact_reads_at_the_positions_and_every_start_depends_on_the_fraction():
    b, planted = dc.resume_batch()
    assert sorted({p for _, p, _ in planted if p not in (10, 140)}) == [0, 1, 63, 64, 65, 100, 128, 199]
    assert [(p, lv) for l, p, lv in planted if l == 8] == [(10, "flank"), (140, "symbols")]
    assert np.diff(b.read_off).tolist() == [dc.RESUME_DEPTH] * 9 and dc.copies(b) == 0
    at = {int(b.read_off[l]) + p: lv for l, p, lv in planted}
    for r in range(b.n_reads):
        n_sym = len(set(b.seqs[int(b.seq_off[r]):int(b.seq_off[r + 1])].tobytes()))
        if at.get(r) == "flank":
            assert 128 <= int(b.nfr[r]) <= 255 and n_sym <= 4       # strk_search.h kBandMaxFlank, strk_kernels.h kFastFlankMax: 127
        elif at.get(r) == "symbols":
            assert n_sym > 8 and int(b.nfr[r]) <= 70
        else:
            assert n_sym <= 4 and 60 <= int(b.nfr[r]) <= 70 and 60 <= int(b.nfl[r]) <= 70 and int(b.ntr[r]) <= 250
    exp = oracle_count_pool(b)
    assert _inside_default_window(b, exp)
    for l in range(b.n_loci):
        r0, r1 = _locus(b, l)
        assert exp["start"][r0] == b.est_cn[r0] and (exp["start"][r0 + 1:r1] != b.est_cn[r0 + 1:r1]).all()   # frac != 0 from read 1 on


def test_fanout_case_moves_only_the_start_of_the_read_behind_the_kick():
    b = dc.fanout_batch()
    assert b.n_loci == 1 and b.n_reads == dc.FANOUT_DEPTH >= 200 and dc.copies(b) == 0
    assert b.n_reads - (dc.FANOUT_KICK + 1) >= 2 * dc.CHUNK                      # more than two trips of the fan-out loop behind read 65
    exp = oracle_count_pool(b)
    moved = np.nonzero(exp["start"] != b.est_cn)[0].tolist()
    assert moved == [dc.FANOUT_KICK + 1] and exp["start"][dc.FANOUT_KICK + 1] == b.est_cn[dc.FANOUT_KICK + 1] + dc.FANOUT_SHIFT
    assert (exp["cn"] == 24).all() and (exp["score"] == 2 * (b.nfl + b.ntr + b.nfr)).all()    # clean reads
    assert _inside_default_window(b, exp)


def test_miss_cases_have_the_shapes_that_choose_the_slice_and_the_bulk_path():
    a, bulk, c = dc.miss_slice_batch(), dc.miss_bulk_batch(), dc.miss_copies_batch()
    assert np.diff(a.read_off).tolist() == [150] * 3 == np.diff(c.read_off).tolist() and np.diff(bulk.read_off).tolist() == [70] * 30
    assert a.n_loci <= 24 < bulk.n_loci and bulk.n_loci > bulk.n_loci // 64      # strk_host_miss.inc: bulk = n_pending > max(24, n_loci / 64)
    assert dc.copies(a) < 30 and dc.copies(c) > 300
    # copies behind in-locus index 64 of a read whose first occurrence lies in front of it, in every locus
    for l in range(c.n_loci):
        r0, r1 = _locus(c, l)
        key = lambda r: (c.read(r), int(c.est_cn[r]))  # noqa: E731
        first = {key(r) for r in range(r0, r0 + dc.CHUNK)}
        assert sum(key(r) in first for r in range(r0 + dc.CHUNK, r1)) > 20


def test_duplicate_case_counts():
    b = dc.dup_batch()
    assert np.diff(b.read_off).tolist() == [250, 250, 250, 130]
    per = [dc.copies(b.locus_slice(l, l + 1)) for l in range(4)]
    assert per[1] == 249 and per[2] == 1 and per[3] == 2 and 200 < per[0] < 245 and sum(per) == dc.copies(b)
    assert b.read(int(b.read_off[2])) == b.read(int(b.read_off[3]) - 1)
    r0 = int(b.read_off[3])
    assert b.read(r0 + 63) == b.read(r0 + 64) == b.read(r0 + 128)
    # same bytes, another estimate: in the first locus some copies must not merge
    l0 = b.locus_slice(0, 1)
    assert len({(l0.read(r), int(l0.est_cn[r])) for r in range(250)}) > len({l0.read(r) for r in range(250)}) == 5


def test_pipeline_padding_sizes():
    b, sweep = dc.pipe_batch(), dc.sweep_batch()
    size = lambda x, l0, l1: int(x.seq_off[x.read_off[l1]] - x.seq_off[x.read_off[l0]]) + 24 * int(x.read_off[l1] - x.read_off[l0])  # noqa: E731
    assert size(b, 0, b.n_loci) >= (1 << 20) // 2                    # strk_host_pipe.inc: smaller batches take the direct path
    for l in (0, b.n_loci - 1):
        assert size(b, l, l + 1) > (1 << 20) // 8                    # one locus is more than the first sub-batch budget
    assert b.n_reads - sweep.n_reads == dc.pipe_pads_batch().n_reads == 500 <= sweep.n_reads
