"""GPU: the calls that take groups of sequences, and strk_call_alleles, one after another on ONE context.  They share the
context's side stream and its timing events, and each family keeps its device copy of the input between calls, so a call
must leave nothing behind that the next one trips over: every result equals the same call on a context of its own, and the
restatements the neighbouring tests use (exactly: all of it is integers and bytes)."""
import ctypes as C

import numpy as np
import pytest

import consensus_restatement as BR
import kmers_restatement as KR
import poa_restatement as P
from helpers import hip_runtime
from strkit_amd import _lib
from strkit_amd import consensus as CS
from strkit_amd import kmers as KM
from strkit_amd._groups import pack_groups
from strkit_amd.alleles import TOO_FEW, AlleleParams, call_alleles_batch

pytestmark = pytest.mark.gpu

METHOD = {"none": CS.NONE, "single": CS.SINGLE, "best_rep": CS.BEST_REP, "poa": CS.POA}
MAX_MDN = 20      # the median length up to which a group goes to POA in this test

KMERS_FIRST = ([[b"CAGCAGCAGCAT", b"CAGCAG"], [b"ACGTACGTAC"]], [3, 2])
CONSENSUS = [[b"CAGCAGCAT", b"CAGCAGCAG", b"CAGCAGCAG", b"CAGCATCAG"],                      # reads that differ: POA
             [b"ACGT" * 10, b"ACGT" * 9 + b"ACGA", b"ACGT" * 10 + b"A", b"TCGT" + b"ACGT" * 9],   # median 40 > MAX_MDN: best rep.
             [],
             [b"GATTACA" * 9] * 5]                                                          # identical reads (63 bytes)
BEST_REP = [[b"AAAT", b"AAAA", b"AAAT"], [b"CAG"]]
KMERS_SECOND = ([[b"CAG" * 20 + b"CAT", b"CAG" * 21, b"CAA" + b"CAG" * 19], [], [b"A" * 64, b"A" * 63 + b"C"],
                 [b"ACGTTGCA" * 8] * 6, [b"", b"GT", b"GTGTGTGA"], [bytes(range(64))]], [3, 5, 6, 8, 2, 1])
ALLELES = dict(read_off=np.array([0, 12, 20], np.int32),
               cns=np.array([10, 10, 11, 10, 10, 25, 25, 24, 25, 26, 25, 10, 7, 7, 7, 8, 7, 7, 7, 7], np.int32),
               weights=np.ones(20), n_alleles=np.array([2, 1], np.int32), seeds=np.array([11, 12], np.uint64),
               params=AlleleParams(num_bootstrap=20))


def _on_a_context_of_its_own(call):
    ctx = _lib.Context(0)
    try:
        return call(ctx)
    finally:
        ctx.close()


def _same(a: dict, b: dict, what):
    assert a.keys() == b.keys(), what
    for key in a:
        assert np.array_equal(a[key], b[key], equal_nan=a[key].dtype.kind == "f"), (what, key)


def _kmers(ctx, groups, ks, what, dev=None):
    off, starts, lens, buf = pack_groups(groups)
    where = dict(seqs=buf) if dev is None else dict(d_seqs=dev(buf), n_seq_bytes=buf.shape[0])
    call = lambda c: KM.count_kmers_packed(off, starts, lens, np.array(ks, np.int32), ctx=c, **where)      # noqa: E731
    out = call(ctx)
    _same(out, _on_a_context_of_its_own(call), what)
    eo, pos, cnt = KR.count_packed(off, starts, lens, np.array(ks, np.int32), buf.tobytes())
    assert (out["entry_off"].tolist(), out["pos"].tolist(), out["count"].tolist()) == (eo, pos, cnt), what


def _consensus(ctx, groups, what, dev=None):
    off, starts, lens, buf = pack_groups(groups)
    where = dict(seqs=buf) if dev is None else dict(d_seqs=dev(buf), n_seq_bytes=buf.shape[0])
    call = lambda c: CS.consensus_packed(off, starts, lens, max_mdn_poa_length=MAX_MDN, ctx=c, **where)    # noqa: E731
    out = call(ctx)
    _same(out, _on_a_context_of_its_own(call), what)
    exp = [P.consensus(g, max_mdn_poa_length=MAX_MDN) for g in groups]
    assert [e[1] for e in exp] == ["poa", "best_rep", "none", "single"]       # every route of the call
    text, so = out["seqs"].tobytes(), out["seq_off"].tolist()
    for g, (idx, method, seq, _limited) in enumerate(exp):
        got = (int(out["index"][g]), int(out["method"][g]), text[so[g]:so[g + 1]])
        assert got == (idx, METHOD[method], seq or b""), (what, g)
    assert exp[1][0] == BR.best_representative(groups[1])[0]                  # the nested pass: the Levenshtein reference's pick


def _best_rep(ctx, groups, what):
    off, starts, lens, buf = pack_groups(groups)
    call = lambda c: CS.best_representatives_packed(off, starts, lens, seqs=buf, ctx=c)                    # noqa: E731
    out = call(ctx)
    _same(out, _on_a_context_of_its_own(call), what)
    exp = [BR.best_representative(g) for g in groups]
    assert (out["index"].tolist(), out["method"].tolist(), out["dist_sum"].tolist()) == \
        ([e[0] for e in exp], [METHOD[e[1]] for e in exp], [e[2] for e in exp]), what


def test_calls_of_every_family_in_turn_on_one_context(fresh_ctx):
    ctx = fresh_ctx
    assert max(len(s) for gs in (KMERS_FIRST[0], CONSENSUS, BEST_REP, KMERS_SECOND[0]) for g in gs for s in g) <= 64
    assert max(len(g) for gs in (KMERS_FIRST[0], CONSENSUS, BEST_REP, KMERS_SECOND[0]) for g in gs) <= 6
    _kmers(ctx, *KMERS_FIRST, "1 k-mers")
    _consensus(ctx, CONSENSUS, "2 consensus")
    _best_rep(ctx, BEST_REP, "3 best representatives")
    _kmers(ctx, *KMERS_SECOND, "4 k-mers, a larger list")
    alleles = lambda c: call_alleles_batch(ctx=c, **ALLELES)                                               # noqa: E731
    got = alleles(ctx)
    _same(got, _on_a_context_of_its_own(alleles), "5 alleles")
    assert (got["status"] != TOO_FEW).all()          # 12 and 8 reads against min_reads = 4: both loci went through the kernel
    # 1 and 2 once more, the bases in device memory of the test's own
    hip = hip_runtime()
    held = []

    def dev(buf):
        d = C.c_void_p()
        assert hip.hipSetDevice(ctx.device) == 0 and hip.hipMalloc(C.byref(d), C.c_size_t(buf.shape[0])) == 0
        held.append(d)
        assert hip.hipMemcpy(d, C.c_void_p(buf.ctypes.data), C.c_size_t(buf.shape[0]), 1) == 0   # hipMemcpyHostToDevice
        return d.value

    try:
        _kmers(ctx, *KMERS_FIRST, "1 k-mers, device bases", dev)
        _consensus(ctx, CONSENSUS, "2 consensus, device bases", dev)
    finally:
        for d in held:
            hip.hipFree(d)
