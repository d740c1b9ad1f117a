"""GPU: how the calls of a context hand their arrays to the device (Staging, strkit_amd/csrc/strk_host.h): small arrays travel
through one page-locked image, arrays of 262 144 bytes or more from and to where they lie.  An allele call either side of that
size equals the same loci called in two halves (another split into gathered and direct parts) and the restatement; calls of
every family in turn on one context, which share the image and reuse their buffers at other sizes, equal the same calls on
contexts of their own; and calls whose optional arrays are absent or whose pieces are empty give what the restatements and
the host twins give."""
import ctypes as C
import functools

import numpy as np
import pytest

import alleles_restatement as R
import consensus_restatement as BR
import kmers_restatement as KR
import mi_cases
import phase_cases as PC
import poa_restatement as P
import test_gpu_alleles as TA
import test_gpu_phase as TP
from helpers import hip_runtime
from strkit_amd import _lib, mi
from strkit_amd import consensus as CS
from strkit_amd import kmers as KM
from strkit_amd._groups import pack_groups
from strkit_amd.alleles import call_alleles_batch
from strkit_amd.phasing import PhaseParams, call_alleles_phased_batch

pytestmark = pytest.mark.gpu

DIRECT = 262144            # Staging::kDirectBytes
READS = 32                 # per locus
SEAM_PARAMS = R.Params(num_bootstrap=2, n_init=1)    # the smallest the input check accepts


@functools.lru_cache(maxsize=None)
def _seam_loci():
    """2 049 loci of 32 reads (two alleles eight copies apart with a little noise, weights that differ) and their seeds."""
    rng = np.random.default_rng(31)
    n = 65568 // READS
    a1 = rng.integers(5, 60, n)
    cn = np.where(rng.random((n, READS)) < 0.5, a1[:, None], a1[:, None] + 8) + rng.choice([0, 0, 0, 0, 1, -1], (n, READS))
    return cn.astype(np.int32).ravel(), 0.5 + rng.random(n * READS), rng.integers(0, 1 << 63, n, dtype=np.uint64)


@functools.lru_cache(maxsize=None)
def _seam_restated(l: int):
    cn, w, seeds = _seam_loci()
    return R.call_locus(cn[READS * l:READS * (l + 1)], w[READS * l:READS * (l + 1)], 2, int(seeds[l]), SEAM_PARAMS)


def _seam_call(ctx, l0, l1):
    cn, w, seeds = _seam_loci()
    off = np.arange(l1 - l0 + 1, dtype=np.int32) * READS
    return call_alleles_batch(off, cn[READS * l0:READS * l1], w[READS * l0:READS * l1], np.full(l1 - l0, 2, np.int32), seeds[l0:l1],
                              TA._aparams(SEAM_PARAMS), ctx)


@pytest.mark.parametrize("n_reads", (32736, 32768, 32800, 65504, 65536, 65568))
def test_allele_call_either_side_of_the_direct_size(gpu_ctx, n_reads):
    # w (8 bytes a read) crosses the size at 32 768 reads, cn and read_peak (4 bytes a read) at 65 536
    assert (32736 * 8 < DIRECT == 32768 * 8 < 32800 * 8) and (65504 * 4 < DIRECT == 65536 * 4 < 65568 * 4)
    n = n_reads // READS
    whole, first, second = _seam_call(gpu_ctx, 0, n), _seam_call(gpu_ctx, 0, n // 2), _seam_call(gpu_ctx, n // 2, n)
    for k in whole:
        assert whole[k].tobytes() == np.concatenate([first[k], second[k]]).tobytes(), k
    picks = sorted(set(np.linspace(0, n - 1, 16).astype(int).tolist()))
    assert len(picks) == 16 and picks[0] == 0 and picks[-1] == n - 1
    for l in picks:
        exp = _seam_restated(l)
        diff = TA._differing_fields(whole, l, exp, READS * l, READS * (l + 1))
        if exp["median_tie"] and {"weights", "stdevs"} & set(diff) and TA._from_tied_bootstraps(whole, l, exp, 2):
            diff = [k for k in diff if k not in ("weights", "stdevs")]   # (tests/test_gpu_alleles.py: a tie at the median)
        assert not diff, (l, diff)


def _alone(call):
    ctx = _lib.Context(0)
    try:
        return call(ctx)
    finally:
        ctx.close()


def _same(a: dict, b: dict, what):
    assert a.keys() - {"stats"} == b.keys() - {"stats"}, what
    for k in a.keys() - {"stats"}:
        assert np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes(), (what, k)


def _kmer_groups(rng):
    """300 groups: most with a few dozen windows (the small table), every tenth with more than 384 (the large one, some of
    them for the sort kernel), a few without a window."""
    groups, ks = [], []
    for g in range(300):
        if g % 10 == 3:
            groups.append([bytes(rng.choice(list(b"ACGT"), int(rng.integers(150, 900))).tolist()) for _ in range(int(rng.integers(3, 7)))])
        elif g % 37 == 5:
            groups.append([b"AC"] if g % 2 else [])
        else:
            unit = bytes(rng.choice(list(b"ACGT"), int(rng.integers(2, 7))).tolist())
            groups.append([unit * int(rng.integers(3, 12)) + b"T" * int(rng.integers(0, 3)) for _ in range(int(rng.integers(1, 6)))])
        ks.append(int(rng.integers(3, 9)))
    return groups, np.array(ks, np.int32)


def _consensus_groups(rng):
    """60 groups: reads of about 24 bytes that differ (POA), every third of about 70 (beyond the median bound of 40: the
    best-representative pass in mid-call), some identical, some empty."""
    groups = []
    for g in range(60):
        base = bytes(rng.choice(list(b"ACGT"), 70 if g % 3 == 1 else 24).tolist())
        if g % 11 == 7:
            groups.append([])
        elif g % 13 == 4:
            groups.append([base] * 3)
        else:
            groups.append([P.mutate(rng, base, 0.08) for _ in range(int(rng.integers(3, 8)))])
    return groups


def test_calls_of_every_family_in_turn_share_one_image(fresh_ctx):
    ctx = fresh_ctx
    rng = np.random.default_rng(77)
    al_loci = [TA._locus(rng, "hifi") for _ in range(2000)]
    al_seeds = rng.integers(0, 1 << 63, 2000, dtype=np.uint64)
    al_p = R.Params(num_bootstrap=20)
    alleles = lambda n: (lambda c: TA._run(al_loci[:n], al_seeds[:n], al_p, c)[1])                          # noqa: E731
    first = alleles(2000)(ctx)
    _same(first, _alone(alleles(2000)), "1 alleles")

    groups, ks = _kmer_groups(rng)
    off, starts, lens, buf = pack_groups(groups)
    kmers = lambda c: KM.count_kmers_packed(off, starts, lens, ks, seqs=buf, ctx=c, with_stats=True)       # noqa: E731
    got, st = kmers(ctx)
    _same(got, _alone(kmers)[0], "2 k-mers")
    n_windows = [KR.n_windows(g, int(k)) for g, k in zip(groups, ks)]
    assert min(n_windows) == 0 and sum(0 < w <= 384 for w in n_windows) > 200 and sum(w > 384 for w in n_windows) >= 30
    assert st["n_sub_batches"] >= 1                                            # the sort kernel's pieces ran as well
    eo, pos, cnt = KR.count_packed(off, starts, lens, ks, buf.tobytes())
    assert (got["entry_off"].tolist(), got["pos"].tolist(), got["count"].tolist()) == (eo, pos, cnt)

    cgroups = _consensus_groups(rng)
    coff, cstarts, clens, cbuf = pack_groups(cgroups)
    cons = lambda c: CS.consensus_packed(coff, cstarts, clens, seqs=cbuf, max_mdn_poa_length=40, ctx=c)    # noqa: E731
    got = cons(ctx)
    _same(got, _alone(cons), "3 consensus")
    methods = set(got["method"].tolist())
    assert methods == {CS.NONE, CS.SINGLE, CS.BEST_REP, CS.POA} and got["seqs"] is not None and got["seqs"].size > 0
    text, so = got["seqs"].tobytes(), got["seq_off"].tolist()
    for g in range(12):
        idx, method, seq, _ = P.consensus(cgroups[g], max_mdn_poa_length=40)
        assert (int(got["index"][g]), CS.METHOD_NAMES[int(got["method"][g])], text[so[g]:so[g + 1]]) == (idx, method, seq or b""), g

    trio = mi.pack_loci([mi_cases.random_trio(rng, 30) for _ in range(200)])
    trios = lambda c: mi.mi_trio_batch(trio["gt"], trio["ci95"], trio["grp_off"], trio["cn"], test="wmw", ctx=c)   # noqa: E731
    got = trios(ctx)
    _same(got, _alone(trios), "4 trio")
    _same(got, mi.mi_trio_batch(trio["gt"], trio["ci95"], trio["grp_off"], trio["cn"], test="wmw", device="host"), "4 trio, host twin")

    ph_loci, ph_seeds = PC.corpus(seed=5, n_loci=150)
    a = PC.pack(ph_loci, ph_seeds, True, False)
    phased = lambda c: call_alleles_phased_batch(a["read_off"], a["cns"], a["weights"], a["n_alleles"], a["seeds"], a["hp"], a["ps"],   # noqa: E731
                                                 fallback=False, ctx=c)
    _same(phased(ctx), _alone(phased), "5 phased, tags")

    _same(alleles(50)(ctx), _alone(alleles(50)), "6 alleles, 50 loci")
    _same(alleles(2000)(ctx), first, "7 alleles again")


def test_trio_without_a_test_and_without_optional_arrays(gpu_ctx):
    pk = mi.pack_loci(mi_cases.all_loci()[0])
    # no test: no reads go up, only `respects` comes down
    got = mi.mi_trio_batch(pk["gt"], pk["ci95"], pk["grp_off"], pk["cn"], pk["ci99"], pk["seq_id"], pk["seq_len"], test="none", ctx=gpu_ctx)
    mi_cases.compare(got, "none")
    host = mi.mi_trio_batch(pk["gt"], pk["ci95"], pk["grp_off"], pk["cn"], pk["ci99"], pk["seq_id"], pk["seq_len"], test="none", device="host")
    _same(got, host, "test none")
    assert np.isnan(got["p"]).all() and (got["config"] == -1).all()           # the wrapper's initial values: nothing was written
    bare = mi.mi_trio_batch(pk["gt"], pk["ci95"], test="none", ctx=gpu_ctx)       # nor are the reads' arrays needed
    assert bare["respects"].tobytes() == mi.mi_trio_batch(pk["gt"], pk["ci95"], test="none", device="host")["respects"].tobytes()
    # a test, without the 99 % intervals and the sequences
    for kw in ({}, {"piece_loci": 7}):
        got = mi.mi_trio_batch(pk["gt"], pk["ci95"], pk["grp_off"], pk["cn"], test="wmw", sig_level=mi_cases.SIG, ctx=gpu_ctx, **kw)
        host = mi.mi_trio_batch(pk["gt"], pk["ci95"], pk["grp_off"], pk["cn"], test="wmw", sig_level=mi_cases.SIG, device="host")
        _same(got, host, ("no ci99, no seq_id", kw))


def test_phased_call_without_snvs_and_with_pieces_that_hold_no_read(gpu_ctx):
    loci, seeds = PC.corpus(seed=9, n_loci=120)
    empty = [l for l, x in enumerate(loci) if len(x["cn"]) == 0]
    assert len(empty) >= 3
    exp = PC.restate(loci, seeds, tags=True, snvs=False)
    a, got = TP._run(loci, seeds, gpu_ctx, True, False)
    TP._compare(loci, a, got, exp, False)
    assert got["snv_status"].size == 0
    # one locus a piece: the pieces of the loci without reads send and fetch empty arrays; with SNVs as well
    for snvs in (False, True):
        a, whole = TP._run(loci, seeds, gpu_ctx, True, snvs)
        _, (cut, st) = TP._run(loci, seeds, gpu_ctx, True, snvs, phase_params=PhaseParams(piece_loci=1), with_stats=True)
        assert st["n_sub_batches"] == len(loci)
        _same(whole, cut, ("piece_loci 1", snvs))
    TP._compare(loci, a, cut, PC.restate(loci, seeds), True)


def test_groups_without_a_window_and_bases_on_the_device(gpu_ctx):
    groups = [[b"ACG", b"AC"], [], [b""], [b"ACGTAC"]]
    off, starts, lens, buf = pack_groups(groups)
    ks = np.array([4, 2, 1, 7], np.int32)
    got = KM.count_kmers_packed(off, starts, lens, ks, seqs=buf, ctx=gpu_ctx)
    eo, pos, cnt = KR.count_packed(off, starts, lens, ks, buf.tobytes())
    assert eo == [0] * 5 and (got["entry_off"].tolist(), got["pos"].tolist(), got["count"].tolist()) == (eo, pos, cnt)

    rng = np.random.default_rng(4)
    groups = [[P.mutate(rng, b"ACGGTCAT" * int(rng.integers(1, 9)), 0.1) for _ in range(int(rng.integers(0, 6)))] for _ in range(40)]
    off, starts, lens, buf = pack_groups(groups)
    hip = hip_runtime()
    d = C.c_void_p()
    assert hip.hipSetDevice(gpu_ctx.device) == 0 and hip.hipMalloc(C.byref(d), C.c_size_t(buf.shape[0])) == 0
    try:
        assert hip.hipMemcpy(d, C.c_void_p(buf.ctypes.data), C.c_size_t(buf.shape[0]), 1) == 0   # hipMemcpyHostToDevice
        got = CS.best_representatives_packed(off, starts, lens, d_seqs=d.value, n_seq_bytes=buf.shape[0], ctx=gpu_ctx)
    finally:
        hip.hipFree(d)
    _same(got, CS.best_representatives_packed(off, starts, lens, seqs=buf, ctx=gpu_ctx), "device bases")
    exp = [BR.best_representative(g) for g in groups]
    method = {"none": CS.NONE, "single": CS.SINGLE, "best_rep": CS.BEST_REP}
    assert (got["index"].tolist(), got["method"].tolist(), got["dist_sum"].tolist()) == \
        ([e[0] for e in exp], [method[e[1]] for e in exp], [e[2] for e in exp])
