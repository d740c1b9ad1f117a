"""k_dp_band's step forms (strk_dp_band.h: band_pass) on hand-built batches: the pairs of steps in front of a wave's first
fork row run without the fork-row test, so the answers must not depend on where the first fork row of a chunk falls, which
groups of a wave are idle, or how long the backward pass is.  Everything is compared with the CPU oracle, whether a read was
certified by the band kernel or re-scored by the exact ones, and the number of reads the band kernel could NOT certify is
bounded by what the parent commit gave on the same batch: a step form that skipped a lane's first fork row would leave its table
entries unset, the certificate would fail and the exact kernels would quietly repair the answer.  One more batch has tables
clipped at size 0 and estimates that send the search to the table's outer entries or out of it (the shipped band geometry: the
whole table)."""
import numpy as np
import pytest

from helpers import oracle_count
from strkit_amd.synth import LocusBatch

pytestmark = pytest.mark.gpu
KEYS = ("cn", "score", "n_iters", "start")
BASES = "ACGT"


def _seq(rng, n):
    return "".join(BASES[i] for i in rng.integers(4, size=n))


def _motif(rng, m):
    while True:
        s = _seq(rng, m)
        if all(s != s[:p] * (m // p) for p in range(1, m) if m % p == 0):   # not a repeat of a shorter motif
            return s


def _locus(rng, m, cn, nfl, nfr, n_reads, p_err=0.3):
    """Reads of one locus: flanks of exactly nfl / nfr bases, a tract of cn (or cn + 1) copies, now and then one substitution —
    distinct reads (the flanks differ), so that the dedupe leaves every one of them an item of its own."""
    motif = _motif(rng, m)
    reads = []
    for k in range(n_reads):
        tr = list(motif * (cn + (k & 1)))
        if tr and rng.random() < p_err:
            i = int(rng.integers(len(tr)))
            tr[i] = BASES[(BASES.index(tr[i]) + 1) % 4]
        reads.append((_seq(rng, nfl), "".join(tr), _seq(rng, nfr)))
    return motif, reads


def _check(b, ctx, flags, min_band=None, max_fallback=None, **kw):
    from strkit_amd.batch import count_loci
    got, st = count_loci(b, ctx=ctx, with_stats=True, end_flags=flags, **kw)
    exp = oracle_count(b, flags=flags)
    for k in KEYS:
        bad = np.nonzero(got[k] != exp[k])[0]
        assert bad.size == 0, (k, int(bad.size), int(bad[0]), [int(got[x][bad[0]]) for x in KEYS], [int(exp[x][bad[0]]) for x in KEYS],
                               b.read(int(bad[0])))
    print("band reads", st["n_band_reads"], "fallback", st["n_band_fallback"], "dup", st["n_dedup_reads"], "of", b.n_reads)
    if min_band is not None:
        assert st["n_band_reads"] >= min_band, st
    # max_fallback: what the commit before the test-free steps counted on this very batch.  The counts belong to the band
    # geometry and to these seeds: after a deliberate change of either, run this file with -s on the tree WITHOUT the change
    # under test (it prints "band reads .. fallback .." per batch) and put those counts here.
    if max_fallback is not None:
        assert st["n_band_fallback"] <= max_fallback, st
    return st


@pytest.mark.parametrize("flags,parent_fallback", [(0, 1), (15, 5)])
def test_an_early_fork_item_shares_its_chunk_with_seven_late_ones(fresh_ctx, flags, parent_fallback):
    """Eight items of one 8-lane class are one chunk.  One has its first fork row at step 0 (one flank base, table from size 0),
    the others theirs a hundred rows later: the wave's test-free stretch is empty, the late groups' fork rows fall deep into the
    tested one.  Right flanks of 1 and of 127 bases: the shortest and the longest backward pass in one wave."""
    rng = np.random.default_rng(1501)
    loci = [_locus(rng, 3, 2, 1, 1, 1)]
    loci += [_locus(rng, 3, 30 + k, 70, 127 if k % 2 else 1, 1) for k in range(7)]
    _check(LocusBatch.from_reads(loci), fresh_ctx, flags, min_band=8, max_fallback=parent_fallback)


@pytest.mark.parametrize("flags,parent_fallback", [(0, 0), (15, 1)])
def test_a_class_of_three_items_leaves_five_groups_idle(fresh_ctx, flags, parent_fallback):
    """Idle groups have no fork row and no last row: they must not shorten the test-free stretch of the three that work (their
    first event counts as never), and a wave of idle groups only must still end."""
    rng = np.random.default_rng(1502)
    loci = [_locus(rng, 4, 12, 40, 50, 1), _locus(rng, 4, 25, 2, 127, 1), _locus(rng, 4, 40, 70, 1, 1)]
    _check(LocusBatch.from_reads(loci), fresh_ctx, flags, min_band=3, max_fallback=parent_fallback)


@pytest.mark.parametrize("flags,parent_fallback", [(0, 12), (15, 142)])
def test_first_fork_rows_at_odd_and_even_steps_from_the_first_step_on(fresh_ctx, flags, parent_fallback):
    """fork0 = |left flank| + lo * |motif| of either parity, from 1 (first step, before the boundary pairs of the row-0 pattern
    and of the left boundary column) up to a few hundred, motifs of 1-6 bases, right flanks of 1, 2, 70, 126 and 127 bases: the
    test-free stretch ends at the pair that holds fork0 - 1 (forward) and |right flank| - 1 (backward), whichever step of the
    pair that is.  More than one chunk per class, chunks of mixed loci."""
    rng = np.random.default_rng(1503)
    loci = []
    for nfl in (1, 2, 3, 4, 7, 8, 69, 70):
        for m in (1, 2, 3, 5, 6):
            for cn in (1, 4, 9, 33):
                loci.append(_locus(rng, m, cn, nfl, (1, 2, 70, 126, 127)[len(loci) % 5], 2))
    b = LocusBatch.from_reads(loci)
    assert 300 <= b.n_reads <= 400
    _check(b, fresh_ctx, flags, min_band=b.n_reads // 2, max_fallback=parent_fallback)
    _check(b, fresh_ctx, flags, max_fallback=parent_fallback, dedupe=False)   # without the hashes


def test_tables_clipped_at_zero_and_estimates_that_reach_the_outer_entries(fresh_ctx):
    """A table clipped at size 0 (estimate below the window's half-width) has its first fork row right behind the left flank;
    an estimate five or six sizes off the truth makes the search end on the table's outer entries or leave it (band fall-backs,
    window misses).  Motifs of 2, 3, 6 and 7 bases side by side."""
    rng = np.random.default_rng(1504)
    loci, est = [], []
    for k in range(60):
        m = (6, 7, 3, 2)[k % 4]
        cn = (1, 2, 3, 5, 11, 24)[k % 6]
        motif, reads = _locus(rng, m, cn, 30 + k % 41, 20 + k % 50, 5, p_err=0.2)
        loci.append((motif, reads))
        off = (0, 5, -5, 6, -6)[k % 5]
        est.append([max(0, round(len(tr) / m) + (off if j >= 2 else 0)) for j, (_, tr, _) in enumerate(reads)])
    b = LocusBatch.from_reads(loci, est)
    _check(b, fresh_ctx, 15, min_band=b.n_reads // 2, max_fallback=102)


# ---- how the band items are listed and handed out in chunks (k_plan's class lists, band_kernel_body's chunk index) ----
@pytest.mark.parametrize("n_items", [8, 9])
def test_a_class_of_exactly_eight_and_of_nine_items(fresh_ctx, n_items):
    """The chunk boundary of an 8-lane class: eight items fill one chunk, the ninth is alone in a second one (seven idle groups)."""
    rng = np.random.default_rng(1505)
    loci = [_locus(rng, 3, 10 + 2 * k, 60, 60, 1, p_err=0.0) for k in range(n_items)]
    st = _check(LocusBatch.from_reads(loci), fresh_ctx, 15, min_band=n_items)
    assert st["n_band_reads"] == n_items and st["n_dedup_reads"] == 0


def test_a_locus_whose_thirty_reads_are_one_duplicate(fresh_ctx):
    """Thirty byte-identical reads are ONE band item: whatever counts reads ahead of the dedupe counts thirty where one is listed."""
    rng = np.random.default_rng(1506)
    loci = [_locus(rng, 4, 8 + k, 50, 50, 2, p_err=0.0) for k in range(20)]
    motif, reads = _locus(rng, 4, 15, 50, 50, 1, p_err=0.0)
    loci.insert(7, (motif, reads * 30))
    b = LocusBatch.from_reads(loci)
    st = _check(b, fresh_ctx, 15)
    assert st["n_dedup_reads"] == 29 and st["n_band_reads"] == b.n_reads - 29


def test_an_empty_class_between_two_that_have_items(fresh_ctx):
    """k_dp_band hands out the chunks of the 16 x 16, 16 x 12, 8 x 16 and 8 x 12 classes in that order.  Motifs of 3 bases sit in
    8 x 12, motifs of 10 bases with 20 and more copies in 16 x 12 (121 diagonals of candidates + slack > 128), nothing in 8 x 16
    (motifs of 5-6 bases would be): the chunk ranges of the empty classes have no width."""
    rng = np.random.default_rng(1507)
    loci = [_locus(rng, 3, 12 + k, 70, 70, 2, p_err=0.0) for k in range(11)] + [_locus(rng, 10, 20 + k, 70, 70, 2, p_err=0.0) for k in range(5)]
    b = LocusBatch.from_reads(loci)
    st = _check(b, fresh_ctx, 15)
    assert st["n_band_reads"] == b.n_reads and st["n_dedup_reads"] == 0


@pytest.mark.parametrize("dedupe", [True, False])
def test_first_call_of_a_context_bands_the_reads_below_2048_and_no_read_is_lost(fresh_ctx, dedupe):
    """A fresh context is on probation: only reads with an index below 2 048 may take the band kernel, the others go straight to
    the exact classes.  2 100 short reads, one locus of them thirty copies of one read (below 2 048), another one five copies
    (above): band items + duplicates + reads sent straight to the exact classes = reads, with every term known in advance — no
    item lost, none listed twice, whatever counted the band items ahead of k_plan agreed with it.  With the dedupe off the
    hashes are not computed at all (the block-local order)."""
    rng = np.random.default_rng(1508)
    # (motifs of 3 and 4 bases are band items at either window level a context may start with, +-6 or +-8)
    loci = [_locus(rng, 3 + k % 2, 6 + k % 30, 70, 70, 10, p_err=0.1) for k in range(203)]
    motif, reads = _locus(rng, 4, 15, 70, 70, 1, p_err=0.0)
    loci.insert(50, (motif, reads * 30))          # reads 500 .. 529
    motif, reads = _locus(rng, 5, 9, 70, 70, 1, p_err=0.0)
    loci.append((motif, reads * 5))               # reads 2060 .. 2064
    loci.append(_locus(rng, 3, 20, 70, 70, 35, p_err=0.1))
    b = LocusBatch.from_reads(loci)
    assert b.n_reads == 2100
    n_dup_lo, n_dup_hi = (29, 4) if dedupe else (0, 0)
    st = _check(b, fresh_ctx, 15, dedupe=dedupe)
    straight_to_exact = b.n_reads - 2048 - n_dup_hi
    assert st["n_dedup_reads"] == n_dup_lo + n_dup_hi, st
    assert st["n_band_reads"] == 2048 - n_dup_lo, st
    assert st["n_band_reads"] + st["n_dedup_reads"] + straight_to_exact == b.n_reads
