"""Shared by tests/test_deep_loci_cases.py (CPU) and tests/test_gpu_deep_loci.py: seeded loci of 63 to 250 reads for the counting
path (k_hash -> k_plan -> band and exact kernels -> k_replay pass 1 and 2 -> resolve_misses).  k_replay is one wave per locus with
one lane per read, so everything behind read 63 of a locus runs its chunk loop, its resume between the passes and its fan-out on
a second (third, fourth) chunk of 64.  Generators only — no expected values; the windows are HiFi-sized (flanks of 60-70 bases,
tracts of up to about 250, motifs of 2-6), the depths and the positions inside a locus are what matters.  Each batch is built
once per process and must not be changed by a test."""
import functools

import numpy as np

from helpers import hifi_locus, hifi_motif, hifi_seq, random_locus
from strkit_amd.synth import LocusBatch

CHUNK = 64                                   # strk_replay.h: reads of a locus a wave of k_replay holds at a time


def copies(b: LocusBatch) -> int:
    """Reads that are byte-identical (same split, same estimate) to an earlier read of their locus: what dedupe merges."""
    n = 0
    for l in range(b.n_loci):
        seen = set()
        for r in range(int(b.read_off[l]), int(b.read_off[l + 1])):
            key = (b.seqs[int(b.seq_off[r]):int(b.seq_off[r + 1])].tobytes(), int(b.nfl[r]), int(b.ntr[r]), int(b.nfr[r]), int(b.est_cn[r]))
            n += key in seen
            seen.add(key)
    return n


def _light_locus(seed, depth, off=3, distinct=False, **kw):
    """random_locus with lightly mutated reads and estimates up to `off` sizes away from round(|tract| / |motif|).  (Error-free
    reads of one allele come out equal now and then; distinct=True changes a base of the left flank until no two are.)"""
    rng = np.random.default_rng(seed)
    motif, reads = random_locus(rng, depth, **{**dict(motif_len=(2, 6), cn=(8, 50), flank=(60, 70), edits=(0, 3)), **kw})
    seen = set()
    for k, (fl, tr, fr) in enumerate(reads):
        while distinct and (fl, tr, fr) in seen:
            i = int(rng.integers(len(fl)))
            fl = fl[:i] + "ACGT"[("ACGT".index(fl[i]) + 1 + int(rng.integers(3))) % 4] + fl[i + 1:]
        seen.add((fl, tr, fr))
        reads[k] = (fl, tr, fr)
    est = [max(0, round(len(tr) / len(motif)) + int(d)) for (_, tr, _), d in zip(reads, rng.integers(-off, off + 1, size=depth))]
    return (motif, reads), est


# ---- 1. depth sweep: one locus per depth -------------------------------------------------------------------------------
# (depth, seed): the seeds are picked so that in every locus deeper than 64 the feedback moves the start of a read on either
# side of in-locus index 64 (tests/test_deep_loci_cases.py checks it with the oracle)
SWEEP = ((64, 2001), (65, 2002), (128, 2003), (129, 2004), (250, 2005), (100, 2006), (63, 2007))


@functools.lru_cache(maxsize=None)
def sweep_batch() -> LocusBatch:
    parts = [_light_locus(seed, depth) for depth, seed in SWEEP]
    return LocusBatch.from_reads([p[0] for p in parts], [p[1] for p in parts])


# ---- 2. one exact read planted in 200 band reads ----------------------------------------------------------------------------
RESUME_DEPTH = 200
# planted positions per locus, and the lever that makes the planted read an exact one: "flank" = a right flank of 128-255 bases
# (neither the band kernels nor the fast exact classes take it: k_dp_long), "symbols" = ten distinct symbols in the window (the
# band kernels take the six letters of a wildcarded read only, the exact kernels eight symbol classes: the generic kernel, which
# scores and does not search)
RESUME = (((0,), "flank"), ((1,), "symbols"), ((63,), "flank"), ((64,), "symbols"), ((65,), "flank"), ((100,), "symbols"),
          ((128,), "flank"), ((199,), "symbols"), ((10, 140), "both"))


def _plant(rng, read, lever):
    fl, tr, fr = read
    if lever == "flank":
        return fl, tr, fr + hifi_seq(rng, int(rng.integers(128 - len(fr), 256 - len(fr))))
    fl = list(fl)
    for k, ch in enumerate("RYSWKM"):             # six IUPAC codes next to A, C, G, T
        fl[5 + 7 * k] = ch
    return "".join(fl), tr, fr


@functools.lru_cache(maxsize=None)
def resume_batch():
    """(batch, [(locus, in-locus position, lever), ...]).  Every estimate of a locus is one size off the tract's, to the same
    side: the first read finds the tract's size, and from then on the feedback fraction (1 / cn or -1 / cn, carried over the
    chunk edges and over the stop between the two passes) puts every start one size away from its estimate."""
    rng = np.random.default_rng(2100)
    loci, est, planted = [], [], []
    for l, (pos, lever) in enumerate(RESUME):
        m = 2 + l % 5
        motif = hifi_motif(rng, m)
        cn = int(rng.integers(14, 36))
        motif, reads = hifi_locus(rng, motif, int(rng.integers(60, 71)), cn * m, int(rng.integers(60, 71)), RESUME_DEPTH)
        for k, p in enumerate(pos):
            lv = lever if lever != "both" else ("flank", "symbols")[k]
            reads[p] = _plant(rng, reads[p], lv)
            planted.append((l, p, lv))
        loci.append((motif, reads))
        est.append([cn + (1 if l % 2 else -1)] * RESUME_DEPTH)
    return LocusBatch.from_reads(loci, est), planted


# ---- 3. one uncertain certificate with more than 64 reads behind it ------------------------------------------------------------
FANOUT_DEPTH = 200
FANOUT_KICK = 64          # in-locus index of the read whose estimate is off; the read behind it starts where its table is uncertain
FANOUT_SHIFT = 2
FANOUT_MOTIF = 5


@functools.lru_cache(maxsize=None)
def fanout_batch() -> LocusBatch:
    """One locus of 200 clean reads of a 5-base motif, 24 copies.  Reads 0-63 and 65-199 carry the exact estimate, read 64 one
    that is two sizes too small.  Every read certifies from its ESTIMATE in the band kernel (strk_search.h: an entry is exact
    when its score reaches band_ub = twice the longest diagonal outside the two bands, here 2 |window| - 128 in the 128-diagonal
    class; a candidate k copies too small scores 7 * 5 * k below the perfect 2 |window|, one k copies too large 5 * 5 * k):
    read 64 searches [est - 4, est - 1] = [cn - 6, cn - 3], whose best entry is 105 < 128 below the perfect score.  The feedback
    fraction is 0 up to read 64, which finds its size two above its start, so read 65 starts two sizes above its estimate and
    searches [cn + 3, cn + 6] at the top of a table laid around cn - 8 .. cn + 8: those candidates' corners lie 24 + 5 (8 - k)
    diagonals inside the forward band, their bounds are 48 + 10 (8 - k) below the perfect score, and the best of them, cn + 3 at
    -75, lies below the bound of cn + 6 at -68.  k_replay pass 1 must hand reads 65-199 to the exact kernels: 135 reads, three
    trips of the fan-out loop.  Read 65's search ends at cn; the fraction is back at 0 from read 66 on."""
    rng = np.random.default_rng(2200)
    motif = hifi_motif(rng, FANOUT_MOTIF)
    cn = 24
    reads = [(hifi_seq(rng, 66), motif * cn, hifi_seq(rng, 68)) for _ in range(FANOUT_DEPTH)]
    est = [cn] * FANOUT_DEPTH
    est[FANOUT_KICK] = cn - FANOUT_SHIFT
    return LocusBatch.from_reads([(motif, reads)], [est])


# ---- 4. window misses in deep loci -----------------------------------------------------------------------------------------
def _bad_estimates(b, seed):
    rng = np.random.default_rng(seed)
    b.est_cn = np.maximum(0, b.est_cn + rng.integers(-9, 10, size=b.n_reads)).astype(np.int32)
    return b


@functools.lru_cache(maxsize=None)
def miss_slice_batch() -> LocusBatch:
    """Three loci of 150 reads, estimates up to nine sizes off: few pending loci (their slices are fetched one by one)."""
    return _bad_estimates(LocusBatch.from_reads([_light_locus(2300 + k, 150, off=0, cn=(8, 40))[0] for k in range(3)]), 2310)


@functools.lru_cache(maxsize=None)
def miss_bulk_batch() -> LocusBatch:
    """Thirty loci of 70 reads: more than 24 pending loci (one bulk copy per array)."""
    return _bad_estimates(LocusBatch.from_reads([_light_locus(2320 + k, 70, off=0, cn=(8, 40))[0] for k in range(30)]), 2360)


@functools.lru_cache(maxsize=None)
def miss_copies_batch() -> LocusBatch:
    """Three loci of 150 reads drawn from seven distinct ones, with estimates drawn from three values per distinct read: the
    copies of a later chunk go through the miss rounds on the table of a first occurrence in an earlier chunk."""
    rng = np.random.default_rng(2370)
    loci, est = [], []
    for k in range(3):
        (motif, reads), _ = _light_locus(2371 + k, 7, off=0, cn=(8, 40))
        pick = rng.integers(0, 7, size=150)
        base = [round(len(reads[i][1]) / len(motif)) for i in range(7)]
        shift = rng.integers(-9, 10, size=(7, 3))
        loci.append((motif, [reads[i] for i in pick]))
        est.append([max(0, base[i] + int(shift[i, j])) for i, j in zip(pick, rng.integers(0, 3, size=150))])
    return LocusBatch.from_reads(loci, est)


# ---- 5. duplicates across chunks ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def dup_batch() -> LocusBatch:
    """Four loci: 250 reads drawn, shuffled, from 5 distinct ones, some copies with another estimate (they must not merge);
    250 copies of one read; 250 distinct reads of which only the first and the last are equal; 130 distinct reads with a first
    occurrence at index 63 and its copies at 64 and 128."""
    rng = np.random.default_rng(2400)
    loci, est = [], []
    (motif, reads), _ = _light_locus(2401, 5, off=0)
    pick = rng.integers(0, 5, size=250)
    e = [round(len(reads[i][1]) / len(motif)) for i in pick]
    for r in range(0, 250, 7):
        e[r] += 2
    for r in range(3, 250, 11):
        e[r] = max(0, e[r] - 3)
    loci.append((motif, [reads[i] for i in pick]))
    est.append(e)
    (motif, reads), e1 = _light_locus(2402, 1)
    loci.append((motif, reads * 250))
    est.append(e1 * 250)
    (motif, reads), e = _light_locus(2403, 250, distinct=True)
    reads[249], e[249] = reads[0], e[0]
    loci.append((motif, reads))
    est.append(e)
    (motif, reads), e = _light_locus(2404, 130, distinct=True)
    for r in (64, 128):
        reads[r], e[r] = reads[63], e[63]
    loci.append((motif, reads))
    est.append(e)
    return LocusBatch.from_reads(loci, est)


# ---- 6. padding for the host pipeline -----------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def pipe_pads_batch() -> LocusBatch:
    """Two loci of 250 reads whose windows (about 620 bases: 250 reads x (window + 24 bytes) is more than an eighth of a
    megabyte) make each of them larger than the host pipeline's first sub-batch budget at STRKIT_AMD_PIPE_MB=1."""
    pads = []
    for k in range(2):
        rng = np.random.default_rng(2500 + k)
        pads.append(hifi_locus(rng, hifi_motif(rng, 5 + k), 70, 480 + 10 * k, 70, 250))
    return LocusBatch.from_reads(pads)


@functools.lru_cache(maxsize=None)
def pipe_batch() -> LocusBatch:
    """The sweep batch between the two padding loci: more than the half megabyte below which the pipeline is not used."""
    pads = pipe_pads_batch()
    return LocusBatch.concat([pads.locus_slice(0, 1), sweep_batch(), pads.locus_slice(1, 2)])
