"""strk_realign over the realignment corpus (tests/realign_cases.py; what each cell holds is proved in
tests/test_realign_cases.py): score, end and CIGAR equal to the oracle's for every case, no tolerance, no case left out; and,
whatever the tie rules are, every device CIGAR is an alignment of the whole window that re-scores to the device's score and
ends where the device says."""
import ctypes as C
import time

import numpy as np
import pytest

import realign_cases as rc
from helpers import cigar_tuples, rescore_cigar
from strkit_amd import _lib
from strkit_amd.realign import _pack, realign_pairs

pytestmark = pytest.mark.gpu


def device_answers(cases, ctx):
    """realign_pairs over the cases, one call per set of gap costs; results by case."""
    groups = {}
    for k, c in enumerate(cases):
        groups.setdefault((c.open, c.ext, c.gap_pref), []).append(k)
    got = [None] * len(cases)
    for (o, e, p), idx in groups.items():
        for k, r in zip(idx, realign_pairs([cases[k].ref for k in idx], [cases[k].read for k in idx], o, e, p, context=ctx)):
            got[k] = r
    return got, len(groups)


def check_cell(cell, ctx, capsys):
    cases, exp = rc.cases(cell), rc.expected(cell)
    t = time.perf_counter()
    got, n_calls = device_answers(cases, ctx)
    wall = time.perf_counter() - t
    with capsys.disabled():
        print(f"\n[realign corpus on the device] {cell}: {len(cases)} cases in {n_calls} calls, {wall:.2f} s")
    bad = []
    for c, (sc, e2, cig), (o_sc, o_e2, o_cig, _) in zip(cases, got, exp):
        if (sc, e2, tuple(cigar_tuples(cig))) != (o_sc, o_e2, o_cig):
            bad.append((c.name, (sc, e2, len(cig)), (o_sc, o_e2, len(o_cig))))
        # independent of the oracle's tie rules: the device's CIGAR is worth the device's score
        assert rescore_cigar(c.ref, c.read, cig, c.open, c.ext) == (sc, len(c.ref), e2 + 1), c.name
    assert not bad, (len(bad), len(cases), bad[:8])
    return got


@pytest.mark.parametrize("cell", [c for c in rc.CELLS if c not in ("mixed", "bound")])
def test_cell_equals_the_oracle(gpu_ctx, capsys, cell):
    check_cell(cell, gpu_ctx, capsys)


def test_bound_inside_is_exact_and_outside_is_refused(gpu_ctx, capsys):
    """The gap-cost bound 2*open + (n1 - 2)*extend < 2^24 (strk_realign.h at kRealignNeg; strk_realign_plan::plan).  Inside:
    the last (open, extend, n1) taken, in 2 and 3 tiles, against reads of 1, 7 and 40 bases and a read that holds the window,
    equal to the oracle, whose own sentinel (-2^29 in score units) is far from these scores.  These cases are AT THE EDGE of
    what the unchanged kernel holds, not beyond it: by the derivation, and by the scalar restatement of the kernel's
    arithmetic (tests/test_realign_cases.py), the first length refused still gives the right scores and wrong ones begin
    about `open` further out.  Outside (one more window base): refused with STRK_E_INVALID and a message that names the pair
    and the bound, by the planner that runs before any device work of the call."""
    check_cell("bound", gpu_ctx, capsys)
    for c in rc.bound_outside():
        for refs, reads, p in (([c.ref], [c.read], 0), (["ACGT", "ACGTACGT", c.ref], ["ACGT", "ACGTACGT", c.read], 2)):
            with pytest.raises(_lib.StrkError) as e:
                realign_pairs(refs, reads, c.open, c.ext, c.gap_pref, context=gpu_ctx)
            assert e.value.code == _lib.STRK_E_INVALID, c.name
            assert f"pair {p}: gap costs beyond the number format" in str(e.value) and "must be below 16777216" in str(e.value), e.value
    # the same windows one base shorter are taken again afterwards (a refusal leaves nothing behind)
    c = rc.cases("bound")[0]
    (sc, e2, cig), = realign_pairs([c.ref], [c.read], c.open, c.ext, c.gap_pref, context=gpu_ctx)
    assert (sc, e2, tuple(cigar_tuples(cig))) == rc.expected("bound")[0][:3]


def test_mixed_one_call_many_chunks_and_alone(gpu_ctx, capsys, monkeypatch):
    """About 40 pairs of every class and tile count in one call: as one chunk (one launch and one queue slot per class), cut
    into chunks by a small trace budget (one pair beyond the budget on its own), and every pair alone: identical bytes, in the
    caller's order, and the cell count of the statistics is the sum of n1 * n2."""
    cases, exp = rc.cases("mixed"), rc.expected("mixed")
    refs, reads = [c.ref for c in cases], [c.read for c in cases]
    cells = sum(len(a) * len(b) for a, b in zip(refs, reads))
    as_bytes = lambda res: [(sc, e2, cig.tobytes()) for sc, e2, cig in res]   # noqa: E731
    t = time.perf_counter()
    one, st = realign_pairs(refs, reads, 7, 0, 0, with_stats=True, context=gpu_ctx)
    assert st["dp_cells"] == cells
    monkeypatch.setenv("STRKIT_AMD_TRACE_BYTES", str(rc.MIXED_BUDGET))
    many, st = realign_pairs(refs, reads, 7, 0, 0, with_stats=True, context=gpu_ctx)
    assert st["dp_cells"] == cells
    monkeypatch.delenv("STRKIT_AMD_TRACE_BYTES")
    alone = [realign_pairs([a], [b], 7, 0, 0, context=gpu_ctx)[0] for a, b in zip(refs, reads)]
    with capsys.disabled():
        print(f"\n[realign corpus on the device] mixed: {len(cases)} pairs, one call + {len(rc.chunks(cases, rc.MIXED_BUDGET))} chunks + "
              f"{len(cases)} single calls, {time.perf_counter() - t:.2f} s")
    assert as_bytes(one) == as_bytes(many) == as_bytes(alone)
    for c, (sc, e2, cig), (o_sc, o_e2, o_cig, _) in zip(cases, one, exp):
        assert (sc, e2, tuple(cigar_tuples(cig))) == (o_sc, o_e2, o_cig), c.name
        assert rescore_cigar(c.ref, c.read, cig) == (sc, len(c.ref), e2 + 1), c.name


# ---- CIGAR capacity through the raw C ABI ------------------------------------------------------------------------------------
MARK = 0xA5A5A5A5
GUARD = 7


def _raw(ctx, refs, reads, caps):
    """strk_realign with cigar_off[p + 1] - cigar_off[p] = caps[p], the ranges inside a buffer of MARK words with GUARD words
    in front and behind: (rc, score, end, n_cigar, buffer, cigar_off)."""
    n = len(refs)
    s1, o1 = _pack(refs)
    s2, o2 = _pack(reads)
    off = np.full(n + 1, GUARD, np.int64)
    off[1:] += np.cumsum(caps)
    buf = np.full(int(off[-1]) + GUARD, MARK, np.uint32)
    score, end, ncig = (np.full(n, -77, np.int32) for _ in range(3))
    p = lambda a: C.c_void_p(a.ctypes.data)   # noqa: E731
    rc_ = ctx._lib.strk_realign(ctx.handle, n, p(s1), p(o1), p(s2), p(o2), 7, 0, 0, p(score), p(end), p(ncig), p(buf), p(off), None)
    return rc_, score, end, ncig, buf, off


def test_cigar_capacity_exact_short_and_none(gpu_ctx):
    """Three pairs whose CIGARs have different run counts.  Exactly their run counts as capacities: the call succeeds, the
    CIGARs are the oracle's and no word outside the three ranges is written.  The middle pair one run short, or a pair with
    no capacity at all: STRK_E_INVALID, the message names the pair, and again nothing outside the ranges is written."""
    cases, exp = rc.cases("col_seams") + rc.cases("row_seams"), rc.expected("col_seams") + rc.expected("row_seams")
    pick, seen = [], set()
    for k, (c, e) in enumerate(zip(cases, exp)):
        if (c.open, c.ext, c.gap_pref) == (7, 0, 0) and len(e[2]) >= 2 and len(e[2]) not in seen and len(pick) < 3:
            seen.add(len(e[2]))
            pick.append(k)
    assert len(pick) == 3
    refs, reads = [cases[k].ref for k in pick], [cases[k].read for k in pick]
    runs = [len(exp[k][2]) for k in pick]
    L = _lib.load()

    def outside_untouched(buf, off):
        return (buf[:GUARD] == MARK).all() and (buf[int(off[-1]):] == MARK).all()

    rc_, score, end, ncig, buf, off = _raw(gpu_ctx, refs, reads, runs)
    assert rc_ == 0, L.strk_last_error()
    assert outside_untouched(buf, off) and ncig.tolist() == runs
    for q, k in enumerate(pick):
        assert (int(score[q]), int(end[q]), tuple(cigar_tuples(buf[off[q]:off[q + 1]]))) == exp[k][:3]
    for caps, p in (([runs[0], runs[1] - 1, runs[2]], 1), ([0, runs[1], runs[2]], 0), ([runs[0], runs[1], 0], 2),
                    ([runs[0], 0, runs[2]], 1)):
        rc_, score, end, ncig, buf, off = _raw(gpu_ctx, refs, reads, caps)
        assert rc_ == _lib.STRK_E_INVALID, caps
        assert f"pair {p}: CIGAR capacity {caps[p]} too small".encode() in L.strk_last_error(), L.strk_last_error()
        assert outside_untouched(buf, off), caps
        for q in range(3):   # what was written inside a range is that pair's CIGAR, from its start, and nothing of another's
            words = buf[off[q]:off[q + 1]]
            full = exp[pick[q]][3]
            assert all(w == MARK or w == full[i] for i, w in enumerate(words) if i < len(full)), (caps, q)
