"""Round 19 on the device: layout class 0 of the band kernels holds windows of up to 512 bases (the prefix rows that share their
LDS bytes with the backward row symbols are staged between the two passes), and one block of k_plan orders the band items of
strk_plan_scope() reads by a counting sort.  Results must equal the CPU oracle through the host-buffer and the resident-buffer
entry points, the planning must lose or duplicate no read at a block edge, and list order must not change from run to run."""
import numpy as np
import pytest

from helpers import device_count as _device_count, end_probation as _end_probation, hifi_locus as _hifi_locus, hifi_motif as _motif, oracle_count
from strkit_amd.synth import LocusBatch, make_config

pytestmark = pytest.mark.gpu
KEYS = ("cn", "score", "n_iters", "start")
ROW_SLACK = 96     # strk_search.h: kBandRowSlack


def _same(got, exp, b, what, loci=None):
    r1 = b.n_reads if loci is None else int(b.read_off[loci])
    for k in KEYS:
        bad = np.nonzero(got[k][:r1] != exp[k][:r1])[0]
        assert bad.size == 0, (what, k, int(bad.size), int(bad[0]), [int(got[x][bad[0]]) for x in KEYS], [int(exp[x][bad[0]]) for x in KEYS])


# ---- windows around the old (448) and the new (512) limit of layout class 0 -------------------------------------------------
WINDOWS = (447, 448, 449, 450, 511, 512, 513)


def _narrow(b, w):
    """Per read: does an 8-lane class (96 or 128 diagonals) take it, by the rule as the issue states it — window of at most 512
    bases, candidates' span plus slack inside the band, fork columns within 320, prefix rows within 512 + kBandRowSlack."""
    out = np.zeros(b.n_reads, bool)
    for l in range(b.n_loci):
        m = int(b.motif_off[l + 1] - b.motif_off[l])
        for r in range(int(b.read_off[l]), int(b.read_off[l + 1])):
            nfl, ntr, nfr, est = int(b.nfl[r]), int(b.ntr[r]), int(b.nfr[r]), int(b.est_cn[r])
            w_r = w + min(max(est, 0) >> 7, 7)           # k_plan widens the table by one size per 128 copies
            lo = max(est - w_r, 0)
            n = est + w_r - lo + 1
            ndb, rows = nfl + ntr + nfr, nfl + (lo + n - 1) * m
            span = max(ntr - lo * m, 0) - min(ntr - (lo + n - 1) * m, 0) + 1
            slack = max(ndb >> 5, 12)
            fits = lambda wd, sl: span + 2 * sl <= wd and ndb <= 512 and (n - 1) * m + wd <= 320 and rows <= 512 + ROW_SLACK   # noqa: E731
            out[r] = fits(96, max(slack, 22)) or fits(128, slack)
    return out


@pytest.mark.parametrize("m", [3, 4, 5, 6])
def test_windows_up_to_512_bases_take_the_narrow_band_and_513_still_gets_its_answer(fresh_ctx, m):
    """One locus per window length (447 .. 513 bases, flanks of 70), 8 reads each, tables of +-6 sizes: everything of up to 512
    bases is a band read of a 96- or 128-diagonal class — band_cells says which: at most 128 diagonals per row — and nothing
    runs in k_dp_band_wide; the 513-base reads take a 16-lane class and are answered all the same.  Two more loci of 512-base
    reads carry estimates so far above their tracts that the prefix rows come to exactly 512 + kBandRowSlack and to one row
    more.  (No 8-lane class can hold such an item: with a span that fits 128 diagonals the rows end at most 93 beyond the
    window.  They are there for the answer: a wider class or the exact kernels, and the host's rounds for a search that leaves
    its table.)"""
    from strkit_amd.batch import count_loci
    rng = np.random.default_rng(1910 + m)
    motif = _motif(rng, m)
    loci = [_hifi_locus(rng, motif, 70, W - 140, 70, 8) for W in WINDOWS]
    est = [[round((W - 140) / m)] * 8 for W in WINDOWS]
    # the table's last size `top` = est + 6 (+ 1 per 128 copies of the estimate): rows = nfl + top * m
    top, e = next((t, e) for t in range((512 + ROW_SLACK - 70) // m, 0, -1) for e in (t - 6, t - 7) if e + 6 + (e >> 7) == t)
    for extra in (0, 1):
        nfl = 512 + ROW_SLACK - top * m + extra
        loci.append(_hifi_locus(rng, motif, nfl, 512 - 70 - nfl, 70, 8))
        est.append([e] * 8)
    b = LocusBatch.from_reads(loci, est)
    ndb = b.nfl + b.ntr + b.nfr
    rows = b.nfl + (b.est_cn + 6 + np.minimum(b.est_cn >> 7, 7)) * m
    assert sorted(set(int(x) for x in ndb)) == list(WINDOWS)
    assert sorted(set(int(x) for x in rows[-16:])) == [512 + ROW_SLACK, 512 + ROW_SLACK + 1]
    narrow = _narrow(b, 6)
    assert int(narrow.sum()) == 48 and not narrow[48:].any()       # the six loci of 447 .. 512 bases
    exp = oracle_count(b)
    got, st = count_loci(b, ctx=fresh_ctx, with_stats=True, window=6)
    _same(got, exp, b, "host buffers")
    print("band reads", st["n_band_reads"], "of", b.n_reads, "fallback", st["n_band_fallback"], "band_cells", st["band_cells"], "wide_cells", st["wide_cells"],
          "missed reads", st["n_miss_reads"])
    assert st["n_dedup_reads"] == 0
    assert st["n_band_reads"] == b.n_reads == 72, st     # every read, the 513-base ones and the long-row ones too (a 16-lane class)
    assert st["wide_cells"] == 0, st
    # the narrow reads cost at most 128 diagonals per row, whatever else ran in k_dp_band at most 256 (a 16-lane class)
    cost = rows + b.nfr
    assert st["band_cells"] <= 128 * int(cost[narrow].sum()) + 256 * int(cost[~narrow].sum()), st
    assert st["band_cells"] >= 96 * int(cost[narrow].sum()), st
    got2, st2 = _device_count(b, fresh_ctx, window=6)
    _same(got2, exp, b, "resident buffers")
    assert st2["wide_cells"] == 0 and st2["n_band_reads"] == st["n_band_reads"]


# ---- the edges of k_plan's blocks ------------------------------------------------------------------------------------
def _edge_batch(n_reads, seed):
    """BASELINE config 2's loci (30 reads each: every band class that configuration uses, a third of the reads copies of
    others) up to the last full locus below n_reads, two loci of reads the band kernels cannot take (right flanks of 130
    bases), and the remainder as one more locus — so that a locus straddles every multiple of the scope the batch passes."""
    rng = np.random.default_rng(seed)
    n_exact = 2 * 3
    n_cfg = (n_reads - n_exact - 1) // 30
    parts = [make_config(2, n_loci=n_cfg, seed_shift=seed)] if n_cfg > 0 else []
    rest = n_reads - 30 * n_cfg - n_exact
    hand = [_hifi_locus(rng, _motif(rng, 3 + k), 40, 60, 130, 3) for k in range(2)] + [_hifi_locus(rng, _motif(rng, 5), 70, 90, 70, rest)]
    parts.append(LocusBatch.from_reads(hand))
    if n_cfg > 0:
        parts = [parts[0].locus_slice(0, 8), parts[1], parts[0].locus_slice(8, n_cfg)] if n_cfg > 8 else parts
    b = LocusBatch.concat(parts)
    assert b.n_reads == n_reads
    return b, n_exact


def _copies(b):
    """Reads that are byte-identical (same split, same estimate) to an earlier read of their locus."""
    n = 0
    for l in range(b.n_loci):
        seen = set()
        for r in range(int(b.read_off[l]), int(b.read_off[l + 1])):
            key = (b.seqs[int(b.seq_off[r]):int(b.seq_off[r + 1])].tobytes(), int(b.nfl[r]), int(b.ntr[r]), int(b.nfr[r]), int(b.est_cn[r]))
            n += key in seen
            seen.add(key)
    return n


BIN_SHIFT = (2, 3, 6, 7)    # strk_plan_order.h: plan_bin_shift per layout class (class & 3)


def _band_lists(ctx, n_reads):
    """The reads of each band class in the order k_plan listed them in ctx's last call (strk_band_list)."""
    from strkit_amd import _lib
    out = []
    for c in range(8):
        buf = np.zeros(max(n_reads, 1), np.int32)
        n = _lib.load().strk_band_list(ctx.handle, c, buf.ctypes.data, buf.size)
        assert 0 <= n <= n_reads, (c, n)
        out.append(buf[:n].copy())
    return out


def _check_list_order(b, lists, S, w):
    """Inside a block of S reads the items of a class are listed by (bin of the prefix rows, read index), and a block's items
    stand together (blocks take their places in the order they arrive, which may differ from run to run).  Returns the
    lists cut into {(class, block): reads}."""
    m_of = np.repeat(np.diff(b.motif_off), np.diff(b.read_off))
    rows = b.nfl + (b.est_cn + w + np.minimum(np.maximum(b.est_cn, 0) >> 7, 7)) * m_of
    seen, segs = set(), {}
    for c, lst in enumerate(lists):
        blocks = lst // S
        order = []
        for k, r in enumerate(lst):
            assert int(r) not in seen, ("listed twice", int(r))
            seen.add(int(r))
            if not order or order[-1] != int(blocks[k]):
                assert int(blocks[k]) not in order, ("a block's items are split", c, int(blocks[k]))
                order.append(int(blocks[k]))
            segs.setdefault((c, int(blocks[k])), []).append(int(r))
        for (cc, blk), seg in segs.items():
            if cc == c:
                keys = [(int(rows[r]) >> BIN_SHIFT[c & 3], r) for r in seg]
                assert keys == sorted(keys), ("order inside a block", c, blk, keys[:12])
    return segs


@pytest.mark.parametrize("edge", ["scope-1", "scope", "scope+1", "2scope+1", "large+1"])
def test_reads_at_the_edges_of_a_plan_block(fresh_ctx, edge):
    """Small calls plan in blocks of strk_plan_scope(1) reads, large ones in wider blocks: batches that end one read short of a
    block, on it, one read past it, one read past two blocks, and the smallest large call plus one block and a read."""
    from strkit_amd import _lib
    from strkit_amd.batch import count_loci
    S1 = _lib.plan_scope(1)
    first_large = next(n for n in range(S1, 1 << 22, S1) if _lib.plan_scope(n) > S1)
    assert S1 >= 256 and S1 % 64 == 0 and _lib.plan_scope(first_large - 1) == S1
    n_reads = {"scope-1": S1 - 1, "scope": S1, "scope+1": S1 + 1, "2scope+1": 2 * S1 + 1,
               "large+1": first_large + _lib.plan_scope(first_large) + 1}[edge]
    S = _lib.plan_scope(n_reads)
    assert S == (S1 if edge != "large+1" else _lib.plan_scope(first_large)) and S % S1 == 0
    b, n_exact = _edge_batch(n_reads, 1920 + len(edge))
    if n_reads > S:
        assert any(int(b.read_off[l]) < S < int(b.read_off[l + 1]) for l in range(b.n_loci))   # a locus straddles the first edge
    _lib.load().strk_adaptive_reset()
    # the first call of a fresh context: on probation, the band takes reads below 2 048 only — equal results all the same
    first, st0 = count_loci(b, ctx=fresh_ctx, with_stats=True, window=6)
    exact, _ = count_loci(b, ctx=fresh_ctx, with_stats=True, band=False, window=6)
    _same(first, exact, b, "probation call against the exact kernels")
    _same(first, oracle_count(b.locus_slice(0, 8)), b, "oracle, first 8 loci", loci=8)
    _end_probation(fresh_ctx)
    got, st = count_loci(b, ctx=fresh_ctx, with_stats=True, window=6)
    _same(got, exact, b, "band against the exact kernels")
    dups = _copies(b)
    print(edge, "reads", b.n_reads, "scope", S, "band", st["n_band_reads"], "dup", st["n_dedup_reads"], "fallback", st["n_band_fallback"], "band_cells", st["band_cells"],
          "| probation call: band", st0["n_band_reads"])
    assert st["n_dedup_reads"] == dups
    assert st["n_band_reads"] + st["n_dedup_reads"] + n_exact == b.n_reads, st     # nothing lost, nothing listed twice
    assert st0["n_band_reads"] <= min(2048, st["n_band_reads"])
    again, st2 = count_loci(b, ctx=fresh_ctx, with_stats=True, window=6)
    _same(again, got, b, "second run")
    assert (st2["band_cells"], st2["n_band_reads"], st2["n_band_fallback"], st2["dp_cells"]) == (st["band_cells"], st["n_band_reads"], st["n_band_fallback"], st["dp_cells"])
    # list order is a function of the batch: the class lists as k_plan wrote them, read back after two runs on resident buffers
    dev, st3 = _device_count(b, fresh_ctx, window=6)
    segs = _check_list_order(b, _band_lists(fresh_ctx, b.n_reads), S, 6)
    _same(dev, exact, b, "resident buffers")
    assert st3["n_band_reads"] == st["n_band_reads"] and st3["band_cells"] == st["band_cells"]
    assert sum(len(v) for v in segs.values()) == st3["n_band_reads"]
    _device_count(b, fresh_ctx, window=6)
    segs2 = _check_list_order(b, _band_lists(fresh_ctx, b.n_reads), S, 6)
    assert segs2 == segs, "the order inside a block changed from one run to the next"


def test_a_batch_of_one_read(fresh_ctx):
    from strkit_amd.batch import count_loci
    rng = np.random.default_rng(1930)
    b = LocusBatch.from_reads([_hifi_locus(rng, _motif(rng, 4), 70, 88, 70, 1)])
    exp = oracle_count(b)
    got, st = count_loci(b, ctx=fresh_ctx, with_stats=True)
    _same(got, exp, b, "host buffers")
    assert st["n_band_reads"] == 1 and st["n_dedup_reads"] == 0
    dev, _ = _device_count(b, fresh_ctx)
    _same(dev, exp, b, "resident buffers")
