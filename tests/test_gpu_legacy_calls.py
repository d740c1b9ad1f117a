"""GPU: the oldest host calls (strk_repeat_count, strk_score_table, strk_score_ref_table, strk_ref_repeat_count, strk_count_loci
below the pipeline's threshold, strk_realign) in turn on ONE context, next to strk_call_alleles.  They share the context's side
stream, its timing events and a few carved staging buffers, so a copy left on another stream, or a pointer taken before the
buffer it points into grew, shows as a wrong result here: every counting and scoring result must equal the oracle's, every
alignment the restatement's.  And strk_realign cut into chunks whose second chunk holds a two-tile pair."""
import ctypes as C

import numpy as np
import pytest

import oracle
import phase_cases as PC
from helpers import ALPHA_WC, mutate, oracle_count, oracle_table, rand_seq, random_locus, realign_pair
from strkit_amd import _lib
from strkit_amd.alleles import call_alleles_batch
from strkit_amd.batch import count_loci, score_ref_table, score_table
from strkit_amd.repeat_count_params import RepeatCountParams
from strkit_amd.repeats import get_ref_repeat_count
from strkit_amd.synth import LocusBatch
from test_gpu_allele_calls import _on_a_context_of_its_own, _same_bytes
from test_gpu_realign import check_pairs

pytestmark = pytest.mark.gpu


def _scalar_count(ctx, start, tr, fl, fr, motif, max_iters=50, lsr=3, step=1):
    cn, sc, n = C.c_int32(), C.c_int32(), C.c_int32()
    b = [s.encode("ascii") for s in (tr, fl, fr, motif)]
    _lib.check(_lib.load().strk_repeat_count(ctx.handle, start, b[0], len(b[0]), b[1], len(b[1]), b[2], len(b[2]), b[3], len(b[3]),
                                             max_iters, lsr, step, C.byref(cn), C.byref(sc), C.byref(n)))
    return (cn.value, sc.value), n.value, cn.value - start


def _one_round(ctx, rng, big):
    """Every call once; `big`: shapes several times the first round's, so that each staging buffer has to grow."""
    cn, flank, reads_per_locus = ((20, 100), (60, 70), 64) if big else ((2, 12), (5, 20), 3)
    # 1. the scalar count: the fast path (one block), and in the big round a window too long for it (the general path)
    motif, reads = random_locus(rng, 1, motif_len=(2, 6), cn=cn, flank=flank)
    fl, tr, fr = reads[0]
    if big:
        tr = motif * (2000 // len(motif))
    assert (len(fl) + len(tr) + len(fr) + 1 > 1792) == big
    start = max(0, round(len(tr) / len(motif)) + int(rng.integers(-2, 3)))
    assert _scalar_count(ctx, start, tr, fl, fr, motif) == oracle.repeat_count(start, tr, fl, fr, motif)
    # 2. a score table of 3 reads
    b = LocusBatch.from_reads([random_locus(rng, 3, cn=cn, flank=flank, alpha=ALPHA_WC)])
    lo = np.maximum(0, b.est_cn - 3).astype(np.int32)
    n = np.full(b.n_reads, 12 if big else 5, np.int32)
    for got, exp in zip(score_table(b, lo, n, ctx=ctx), oracle_table(b, lo, n)):
        assert np.array_equal(got, exp)
    # 3. a reference-side table: the window and its reversal with the flanks swapped
    motif, reads = random_locus(rng, 1, motif_len=(1, 6), cn=cn, flank=flank)
    fl, tr, fr = reads[0]
    b = LocusBatch.from_reads([(motif, [(fl, tr, fr)]), (motif[::-1], [(fr[::-1], tr[::-1], fl[::-1])])])
    i0 = max(0, round(len(tr) / len(motif)) - 2)
    got = score_ref_table(b, np.full(2, i0, np.int32), np.full(2, 5, np.int32), ctx=ctx)
    for j in range(5):
        (fs, fa), (rs, ra) = oracle.score_ref_boundaries(fl + tr + fr, fl, fr, motif, i0 + j, len(tr))
        assert (int(got[0][0][j]), int(got[0][1][j]) + 1 - len(fl) - len(tr)) == (fs, fa)
        assert (int(got[1][0][j]), int(got[1][1][j]) + 1 - len(fr) - len(tr)) == (rs, ra)
    # 4. a reference-side count, a repeat copy hidden in either flank
    motif = rand_seq(rng, int(rng.integers(2, 6)))
    fl, tr, fr = rand_seq(rng, flank[1]) + motif, motif * cn[1], motif + rand_seq(rng, flank[1])
    rc = RepeatCountParams("repalign", 250, 3, 1)
    assert get_ref_repeat_count(cn[1] - 1, tr, fl, fr, motif, len(tr), 5, rc, context=ctx) == \
        oracle.ref_repeat_count(cn[1] - 1, tr, fl, fr, motif, len(tr), 5, rc.max_iters, 3, 1)
    # 5. a count of 2 loci with host bases (below the pipeline's threshold: the direct path)
    b = LocusBatch.from_reads([random_locus(rng, reads_per_locus, cn=cn, flank=flank, alpha=ALPHA_WC) for _ in range(2)])
    got, exp = count_loci(b, ctx=ctx), oracle_count(b)
    for k in ("cn", "score", "n_iters", "start"):
        assert np.array_equal(got[k], exp[k]), k
    # 6. an alignment of 4 pairs
    pairs = [realign_pair(rng, int(rng.integers(500, 700) if big else rng.integers(20, 120)), 1500 if big else 300, ins=10) for _ in range(4)]
    check_pairs([p[0] for p in pairs], [p[1] for p in pairs], context=ctx)
    # 7. allele calls of 2 loci: the same bytes as on a context that ran nothing else
    a = PC.pack([PC.make_locus(rng, 100 if big else 8, 2, 2, "none", "clean") for _ in range(2)], [3, 5], with_tags=False, with_snvs=False)
    plain = lambda c: call_alleles_batch(a["read_off"], a["cns"], a["weights"], a["n_alleles"], a["seeds"], ctx=c)   # noqa: E731
    _same_bytes(plain(ctx), _on_a_context_of_its_own(plain), "allele calls")


def test_calls_in_turn_on_one_context(fresh_ctx):
    rng = np.random.default_rng(14)
    _one_round(fresh_ctx, rng, big=False)
    _one_round(fresh_ctx, rng, big=True)


def _pair_with_a_short_read(rng, n_ref):
    """A window of n_ref bases and a read of about 300: around a copy of the window if that fits, else a mutated piece of it."""
    if n_ref <= 280:
        return realign_pair(rng, n_ref, 300, ins=(0 if n_ref < 50 else 8))
    ref = rand_seq(rng, n_ref)
    at = int(rng.integers(0, n_ref - 290))
    return ref, rand_seq(rng, 5) + mutate(rng, ref[at:at + 290], 0.02, 0.02) + rand_seq(rng, 5)


def test_realign_chunks_with_a_two_tile_pair_behind_the_first_chunk(fresh_ctx, monkeypatch):
    """A trace budget of 2 MiB and reads of about 300 bases (363 trace rows of 64 lanes x cl / 2 bytes): 45 KiB for a window of up
    to 256 bases, 91 KiB up to 512, 182 KiB up to 1 024, 363 KiB up to 2 048, 726 KiB for the 2 049 that need a second column tile
    and with it an edge range.  Five pairs of the widest class fill the first chunk; the second starts at pair 5 and holds a
    two-tile pair and all four classes; the last pair, two tiles again, runs alone."""
    rng = np.random.default_rng(15)
    n_ref = [2048, 1025, 2047, 1500, 2048, 2049, 3, 257, 513, 256, 1025, 2049]
    pairs = [_pair_with_a_short_read(rng, n) for n in n_ref]
    refs, reads = [p[0] for p in pairs], [p[1] for p in pairs]
    assert [len(r) for r in refs] == n_ref and all(280 <= len(q) <= 320 for q in reads)
    # the cut as the library makes it (strk_realign_plan.h), restated: trace bytes per pair, chunks by the budget
    cl = lambda n: 4 if n <= 256 else 8 if n <= 512 else 16 if n <= 1024 else 32                    # noqa: E731
    tiles = lambda n: -(-n // (64 * cl(n)))                                                         # noqa: E731
    trace = [(tiles(len(r)) * (len(q) + 63) * 64 * (cl(len(r)) // 2) + 255) // 256 * 256 for r, q in pairs]
    chunks, used = [[]], 0
    for p, t in enumerate(trace):
        if chunks[-1] and used + t > (2 << 20):
            chunks.append([])
            used = 0
        chunks[-1].append(p)
        used += t
    assert chunks == [[0, 1, 2, 3, 4], [5, 6, 7, 8, 9, 10], [11]]
    assert [tiles(n) for n in n_ref[5:]] == [2, 1, 1, 1, 1, 1, 2] and {cl(n) for n in n_ref[5:11]} == {4, 8, 16, 32}
    monkeypatch.setenv("STRKIT_AMD_TRACE_BYTES", str(2 << 20))
    check_pairs(refs, reads, context=fresh_ctx)
