"""GPU: strk_call_alleles_phased (k_phase_group, k_phase_pack, k_alleles, k_phase_finish) against the CPU restatement
tests/phase_restatement.py (rule A-F of DESIGN.md §13)."""
import numpy as np
import pytest

import alleles_restatement as AR
import phase_cases as PC
import phase_restatement as PR
from strkit_amd import _lib
from strkit_amd.alleles import AlleleParams, call_alleles_batch
from strkit_amd.phasing import (ASSIGN_NONE, NOT_PHASED, PhaseParams, call_alleles_phased_batch, call_locus_phased)

pytestmark = pytest.mark.gpu

FLOAT_RTOL = 1e-6   # the tolerance of tests/test_gpu_alleles.py
INT_KEYS = ("status", "modal_n", "call", "ci95", "ci99", "peak_n_reads", "method", "reason", "ps")
FLOAT_KEYS = ("means", "weights", "stdevs")


def _close(a, b):
    a, b = np.asarray(a, np.float64).ravel(), np.asarray(b, np.float64).ravel()
    same = (np.isnan(a) & np.isnan(b)) | (a == b)
    with np.errstate(invalid="ignore", divide="ignore"):
        rel = np.where(same, 0.0, np.abs(a - b) / np.maximum(np.abs(b), 1e-300))
    return bool(np.all(rel <= FLOAT_RTOL))


def _run(loci, seeds, ctx, tags=True, snvs=True, fallback=False, phase_params=None, with_stats=False):
    a = PC.pack(loci, seeds, tags, snvs)
    return a, call_alleles_phased_batch(a["read_off"], a["cns"], a["weights"], a["n_alleles"], a["seeds"], a.get("hp"), a.get("ps"),
                                        a.get("snv_off"), a.get("snv_base"), a.get("snv_qual"), None, phase_params, fallback, ctx,
                                        with_stats)


def _compare(loci, a, got, exp_all, snvs=True):
    """Every locus of a call against its restatement.  Returns the number of loci whose two group means differ by less than
    the float tolerance (either peak order is accepted there)."""
    close = 0
    for l, (x, exp) in enumerate(zip(loci, exp_all)):
        r0, r1 = int(a["read_off"][l]), int(a["read_off"][l + 1])
        ctx = (l, len(x["cn"]), x["base"].shape[1], x["n_alleles"])
        got_rp = got["read_peak"][r0:r1]
        g = {k: np.asarray(got[k][l]).ravel() for k in INT_KEYS + FLOAT_KEYS}
        if exp["close_means"] and not np.array_equal(got_rp, exp["read_peak"]):
            close += 1   # the same call with the peaks the other way round
            assert np.array_equal(np.where(got_rp >= 0, 1 - got_rp, -1), exp["read_peak"]), ctx
            for k in ("call", "peak_n_reads", "means", "stdevs"):
                g[k] = g[k][::-1]
            for k in ("ci95", "ci99"):
                g[k] = g[k].reshape(2, 2)[::-1].ravel()
        else:
            assert np.array_equal(got_rp, exp["read_peak"]), (ctx, got_rp, exp["read_peak"])
        for k in INT_KEYS:
            assert g[k].tolist() == list(np.ravel(exp[k])), (ctx, k, g[k], exp[k])
        for k in FLOAT_KEYS:
            assert _close(g[k], exp[k]), (ctx, k, g[k], exp[k])
        if snvs:
            s0, s1 = int(a["snv_off"][l]), int(a["snv_off"][l + 1])
            assert np.array_equal(got["snv_status"][s0:s1], exp["snv_status"]), (ctx, got["snv_status"][s0:s1], exp["snv_status"])
            if not (exp["close_means"] and not np.array_equal(got_rp, exp["read_peak"])):
                assert np.array_equal(got["snv_call"][s0:s1], exp["snv_call"]), ctx
                assert np.array_equal(got["snv_rcs"][s0:s1], exp["snv_rcs"]), ctx
            else:
                assert np.array_equal(got["snv_call"][s0:s1, ::-1], exp["snv_call"]), ctx
                assert np.array_equal(got["snv_rcs"][s0:s1, ::-1], exp["snv_rcs"]), ctx
    return close


@pytest.fixture(scope="module")
def corpus():
    loci, seeds = PC.corpus()
    return loci, seeds, PC.restate(loci, seeds)


def test_corpus_with_tags_and_snvs_equals_restatement(gpu_ctx, corpus):
    loci, seeds, exp = corpus
    sizes = {len(x["cn"]) for x in loci}
    assert sizes >= set(PC.SIZES) | {1024} and {x["base"].shape[1] for x in loci} >= set(PC.SNV_COUNTS)
    a, got = _run(loci, seeds, gpu_ctx)
    close = _compare(loci, a, got, exp)
    methods = np.bincount(got["method"], minlength=4)
    reasons = np.bincount(got["reason"], minlength=6)
    print(f"{len(loci)} loci: methods none/hp/snv/snv+dist {methods.tolist()}, reasons {reasons.tolist()}; "
          f"{close} loci with group means closer than {FLOAT_RTOL:g} relative (either peak order accepted)")
    assert methods.min() > 0 and len(loci) >= 2000
    # both sides of the LDS / workspace cut took the SNV path
    for n in (PC.LDS_CUT, PC.LDS_CUT + 1, 250, 1024):
        assert any(len(x["cn"]) == n and e["labels"] is not None and len(e["labels"]) > (PC.LDS_CUT if n > PC.LDS_CUT else 2)
                   for x, e in zip(loci, exp)), n


@pytest.mark.parametrize("tags,snvs", [(True, False), (False, True), (False, False)], ids=["tags_only", "snvs_only", "neither"])
def test_corpus_slice_with_one_kind_of_input_equals_restatement(gpu_ctx, corpus, tags, snvs):
    loci, seeds = corpus[0][:500], corpus[1][:500]
    exp = PC.restate(loci, seeds, tags=tags, snvs=snvs)
    a, got = _run(loci, seeds, gpu_ctx, tags, snvs)
    _compare(loci, a, got, exp, snvs)
    if not tags and not snvs:
        assert set(got["method"].tolist()) == {ASSIGN_NONE}
        assert set(got["reason"][got["status"] == NOT_PHASED].tolist()) == {PR.REASON_NO_TAGS}


def test_hand_vectors_on_the_device(gpu_ctx):
    close = 0
    for name, x, tags, snvs, want in PC.hand_vectors():
        seeds = [AR.locus_seed(1, 0)]
        exp = PC.restate([x], seeds, tags=tags, snvs=snvs)
        a, got = _run([x], seeds, gpu_ctx, tags, snvs)
        close += _compare([x], a, got, exp, snvs)
        one = {k: (got[k] if k.startswith("snv_") or k == "read_peak" else got[k][0]) for k in got}
        PC.check_expected(name, one, want)
    print(f"hand vectors: {close} with group means closer than {FLOAT_RTOL:g} relative")
    assert close == 0


def test_locus_alone_equals_locus_in_a_large_call_and_runs_repeat(gpu_ctx, corpus):
    loci, seeds, _ = corpus
    a, big = _run(loci, seeds, gpu_ctx)
    _, again = _run(loci, seeds, gpu_ctx)
    for k in big:
        assert big[k].tobytes() == again[k].tobytes(), k
    picks = [l for l in (0, 17, 500, len(loci) // 2, len(loci) - 1)]
    picks += [next(l for l in range(len(loci)) if big["method"][l] == m) for m in (1, 2, 3)]
    for l in picks:
        b, one = _run([loci[l]], seeds[l:l + 1], gpu_ctx)
        r0, r1, s0, s1 = a["read_off"][l], a["read_off"][l + 1], a["snv_off"][l], a["snv_off"][l + 1]
        for k in one:
            if k == "read_peak":
                assert np.array_equal(one[k], big[k][r0:r1]), (l, k)
            elif k.startswith("snv_"):
                assert np.array_equal(one[k], big[k][s0:s1]), (l, k)
            else:
                assert one[k][0].tobytes() == big[k][l].tobytes(), (l, k)


def test_call_cut_into_pieces_equals_the_uncut_call(gpu_ctx, corpus):
    loci, seeds = corpus[0][:600], corpus[1][:600]
    _, (whole, st1) = _run(loci, seeds, gpu_ctx, with_stats=True)
    _, (by_loci, st2) = _run(loci, seeds, gpu_ctx, phase_params=PhaseParams(piece_loci=37), with_stats=True)
    _, (by_bytes, st3) = _run(loci, seeds, gpu_ctx, phase_params=PhaseParams(ws_budget=1 << 20), with_stats=True)
    assert st1["n_sub_batches"] == 1 and st2["n_sub_batches"] == -(-600 // 37) and st3["n_sub_batches"] > 3
    for k in whole:
        assert whole[k].tobytes() == by_loci[k].tobytes(), k
        assert whole[k].tobytes() == by_bytes[k].tobytes(), k


def test_fallback_calls_the_unphased_loci_as_call_alleles_batch_does(gpu_ctx, corpus):
    loci, seeds = corpus[0][:600], corpus[1][:600]
    a, plain = _run(loci, seeds, gpu_ctx)
    _, merged = _run(loci, seeds, gpu_ctx, fallback=True)
    dist = call_alleles_batch(a["read_off"], a["cns"], a["weights"], a["n_alleles"], a["seeds"], AlleleParams(), gpu_ctx)
    none = np.nonzero(plain["method"] == ASSIGN_NONE)[0]
    rest = np.nonzero(plain["method"] != ASSIGN_NONE)[0]
    assert none.size > 50 and rest.size > 50
    assert not np.any(merged["status"] == NOT_PHASED)
    for k in ("status", "modal_n", "call", "ci95", "ci99", "means", "weights", "stdevs", "peak_n_reads"):
        assert merged[k][none].tobytes() == dist[k][none].tobytes(), k
        assert merged[k][rest].tobytes() == plain[k][rest].tobytes(), k
    for l in range(len(loci)):
        r0, r1 = a["read_off"][l], a["read_off"][l + 1]
        src = dist if plain["method"][l] == ASSIGN_NONE else plain
        assert np.array_equal(merged["read_peak"][r0:r1], src["read_peak"][r0:r1]), l
    for k in ("method", "reason", "ps", "snv_status", "snv_call", "snv_rcs"):
        assert merged[k].tobytes() == plain[k].tobytes(), k


def test_per_locus_convenience_sets_the_assign_method(gpu_ctx):
    vec = {v[0]: v for v in PC.hand_vectors()}
    _, x, _, _, _ = vec["hp_order_kept"]
    cd, snvs = call_locus_phased(x["cn"], x["w"], 2, 9, x["hp"], x["ps"], ctx=gpu_ctx)
    assert cd.get_assign_method_str() == "hp" and cd.ps == 4 and snvs == [] and cd.call.tolist() == [20, 10]
    _, x, _, _, _ = vec["snv_calls"]
    cd, snvs = call_locus_phased(x["cn"], x["w"], 2, 9, snv_base=x["base"], snv_qual=x["qual"], ctx=gpu_ctx)
    assert cd.get_assign_method_str() == "snv" and cd.call.tolist() == [10, 20] and cd.read_peaks.tolist() == [0] * 4 + [1] * 4
    assert snvs == [(0, ("A", "T"), [4, 4]), (1, ("A", "T"), [4, 4]), (2, ("C", "G"), [2, 4]), (3, ("A", "G"), [2, 4])]
    _, x, _, _, _ = vec["snv_and_dist"]
    cd, snvs = call_locus_phased(x["cn"], x["w"], 2, 9, snv_base=x["base"], snv_qual=x["qual"], ctx=gpu_ctx)
    assert cd.get_assign_method_str() == "snv+dist" and len(snvs) == 1
    _, x, _, _, _ = vec["no_tags"]
    cd, snvs = call_locus_phased(x["cn"], x["w"], 2, 9, ctx=gpu_ctx)
    assert cd.get_assign_method_str() == "dist" and cd.to_dict()["peaks"]["modal_n"] in (1, 2)
    cd, _ = call_locus_phased([10, 11], [1.0, 1.0], 2, 9, ctx=gpu_ctx)
    assert cd is None


def test_invalid_inputs_are_rejected_before_any_launch(gpu_ctx):
    rng = np.random.default_rng(2)
    loci = [PC.make_locus(rng, 12, 3, 2, "clean", "clean") for _ in range(4)]
    seeds = [1, 2, 3, 4]
    a = PC.pack(loci, seeds)

    def call(**kw):
        b = {**a, **kw}
        return call_alleles_phased_batch(b["read_off"], b["cns"], b["weights"], b["n_alleles"], b["seeds"], b["hp"], b["ps"],
                                         b["snv_off"], b["snv_base"], b["snv_qual"], None, None, False, gpu_ctx, with_stats=True)

    _, st = call()
    launches = st["n_dp_launches"]
    assert launches == 4

    def refused(text, **kw):
        with pytest.raises(_lib.StrkError) as e:
            call(**kw)
        assert e.value.code == _lib.STRK_E_INVALID and "strk_call_alleles_phased" in str(e.value) and text in str(e.value), str(e.value)

    big = [PC.make_locus(rng, 12, 65, 2, "none", "clean")] + loci[1:]
    refused("SNVs (at most 64)", **PC.pack(big, seeds))
    big = [PC.make_locus(rng, 1025, 1, 2, "none", "clean")] + loci[1:]
    refused("reads (at most 1024)", **PC.pack(big, seeds))
    refused("hp and ps", ps=None)
    refused("cells", snv_base=a["snv_base"][:-1], snv_qual=a["snv_qual"][:-1])
    w = a["weights"].copy()
    w[17] = 0.0
    refused("weight", weights=w)
    w[17] = -2.0
    refused("weight", weights=w)
    # the context still serves a valid call
    out, _ = call()
    assert set(out["method"].tolist()) <= {0, 1, 2, 3} and out["status"].shape == (4,)
