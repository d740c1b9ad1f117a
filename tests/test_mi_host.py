"""CPU: the library's host function strk_mi_trio_host (strk_mi.h compiled for the host) against the oracle of
mi_restatement.py on the corpus of mi_cases.py, under the tolerances of DESIGN.md §16; every input check with its message;
pieces of 1, 7 and all loci give equal bytes.  Nothing here needs a GPU; nothing is skipped."""
import numpy as np
import pytest

import mi_cases as cases
import mi_restatement as R
from strkit_amd import _lib, mi


@pytest.fixture(scope="module")
def packed():
    return mi.pack_loci(cases.all_loci()[0])


def run(pk, test, **kw):
    return mi.mi_trio_batch(pk["gt"], pk["ci95"], pk["grp_off"], pk["cn"], pk["ci99"], pk["seq_id"], pk["seq_len"], test=test,
                            sig_level=kw.pop("sig_level", cases.SIG), device="host", **kw)


def test_corpus_covers_what_it_should():
    loci, names = cases.all_loci()
    assert {"hand", "d2", "d5", "d15", "d30", "d250", "exact", "wide", "deep", "tiny"} == set(names)
    sizes = np.array([sum(len(g) for g in l["reads"]) for l in loci])
    assert sizes.max() > 1500 and (sizes > 256).sum() > 10 and (sizes <= 256).sum() > 200
    wide = cases.cells()["wide"][0]["reads"]
    assert min(min(g) for g in wide) == 0 and max(max(g) for g in wide) == 5000
    # the exact branch: no tied value, a short side of at most 8; and its neighbour 9, which is asymptotic
    n_exact = 0
    for l in cases.cells()["exact"]:
        vals = [v for g in l["reads"] for v in g]
        assert len(vals) == len(set(vals))
        n_exact += min(len(l["reads"][0]) + len(l["reads"][1]), len(l["reads"][2]) + len(l["reads"][4])) <= 8
    assert n_exact >= 20 and any(max(len(g) for g in l["reads"]) >= 150 for l in cases.cells()["exact"])
    for test in cases.TESTS:
        st = np.bincount([e["status"] for e in cases.oracle(test)], minlength=4)
        assert st[R.TESTED] > 300 and st[R.EMPTY_PARENT] > 0 and st[R.EMPTY_CHILD] > 0 and (test == "x2" or st[R.OVERLAP] > 0)
        froms = {e["mutation_from"] for e in cases.oracle(test)}
        assert froms >= {"none", "?", "mat", "pat"}, (test, froms)
    # chi-square statistics above 1 417 (where e^(-statistic / 2) is denormal or 0) over tens to hundreds of bins, p still above 1e-300
    deep = [e for e, name in zip(cases.oracle("x2"), names) if name == "deep"]
    assert len(deep) == 5 and all(1e-300 < p < 1e-200 for e in deep for p in e["config_ps"]), [e["config_ps"] for e in deep]
    assert all(len(set(e["config_ps"])) == 4 for e in deep)
    tiny = [e["p"] for e in cases.oracle("x2")[-4:]]
    assert tiny[0] > 1e-300 and min(tiny) < 1e-300


@pytest.mark.parametrize("test", cases.TESTS)
def test_few_loci_need_a_lenient_case(test):
    share = cases.lenient_share(test)
    print({k: round(v, 3) for k, v in share.items()})
    assert max(share.values()) <= cases.MAX_LENIENT_SHARE, share


@pytest.mark.parametrize("test", ("none",) + cases.TESTS)
def test_host_function_equals_the_oracle(packed, test):
    print(cases.compare(run(packed, test), test))


def test_widen_and_another_level(packed):
    got = run(packed, "none", widen=0.1)
    print(cases.compare(got, "none", widen=0.1))
    assert (got["respects"] != run(packed, "none")["respects"]).any()
    print(cases.compare(run(packed, "wmw", sig_level=0.3), "wmw", sig_level=0.3))


def test_intervals_at_99_percent_fill_their_slot(packed):
    got = mi.mi_trio_batch(packed["gt"], packed["ci95"], ci99=packed["ci95"], device="host")
    assert np.array_equal(got["respects"][:, 3], got["respects"][:, 2]) and (run(packed, "none")["respects"][:, 3] == -1).all()


def test_pieces_do_not_change_a_byte(packed):
    for test in cases.TESTS:
        ref = run(packed, test, piece_loci=0)
        for piece in (1, 7, len(cases.all_loci()[0])):
            got = run(packed, test, piece_loci=piece)
            for k in ("respects", "p", "config", "mutation_from", "status"):
                assert got[k].tobytes() == ref[k].tobytes(), (test, piece, k)


def test_no_loci_is_a_valid_call():
    got = mi.mi_trio_batch(np.zeros((0, 6)), np.zeros((0, 12)), np.zeros(1), np.zeros(0), test="x2", device="host")
    assert got["p"].size == 0


def refusal(pk, test="x2", **change):
    args = dict(pk)
    kw = {k: change.pop(k) for k in ("sig_level", "widen", "piece_loci") if k in change}
    args.update(change)
    with pytest.raises(_lib.StrkError) as e:
        mi.mi_trio_batch(args["gt"], args["ci95"], args["grp_off"], args["cn"], args["ci99"], args["seq_id"], args["seq_len"], test=test,
                         device="host", **kw)
    assert e.value.code == _lib.STRK_E_INVALID and "strk_mi_trio_host: " in str(e.value)
    return str(e.value)


def test_every_input_check_names_what_is_wrong():
    loci = [cases.hand_cases()[k] for k in ("strict", "de_novo_pat", "seq_not_strict")]
    pk = mi.pack_loci(loci)
    off = pk["grp_off"].copy(); off[8] = off[7] - 1
    assert "locus 1: grp_off is decreasing at group 1" in refusal(pk, grp_off=off)
    off = pk["grp_off"].copy(); off[-1] += 1
    assert "locus 2: group 5 ends at read" in refusal(pk, grp_off=off)
    off = pk["grp_off"].copy(); off[0] = 1
    assert "grp_off[0] must be 0" in refusal(pk, grp_off=off)
    big_off = np.zeros(19, np.int64); big_off[10:] = 65536
    assert "locus 1: group 3 has 65536 reads (at most 65535)" in refusal(pk, grp_off=big_off, cn=np.zeros(65536, np.int32))
    cn = pk["cn"].copy(); cn[int(pk["grp_off"][6]) + 2] = -4
    assert "locus 1: read" in refusal(pk, cn=cn) and "copy number -4" in refusal(pk, cn=cn)
    for bad in (0.0, 1.0, -0.1, float("nan")):
        assert "sig_level" in refusal(pk, sig_level=bad) and "outside (0, 1)" in refusal(pk, sig_level=bad)
    assert "widen" in refusal(pk, widen=-0.5) and "widen" in refusal(pk, widen=float("nan"))
    assert "piece_loci" in refusal(pk, piece_loci=-1)
    ci = pk["ci95"].copy(); ci[2, 4], ci[2, 5] = 9, 8
    assert "locus 2: ci95 of allele 2 has its lower bound 9 above its upper bound 8" in refusal(pk, ci95=ci)
    assert "locus 2: ci99 of allele 2" in refusal(pk, ci99=ci)
    assert "seq_id is given without seq_len" in refusal(pk, seq_len=None)
    assert "seq_len is given without seq_id" in refusal(pk, seq_id=None)
    assert "NULL argument" in refusal(pk, grp_off=None)
    # without a test the reads are not looked at
    got = mi.mi_trio_batch(pk["gt"], pk["ci95"], None, None, None, pk["seq_id"], pk["seq_len"], device="host")
    assert got["respects"].shape == (3, 7)
    with pytest.raises(ValueError):
        mi.mi_trio_batch(pk["gt"], pk["ci95"], test="t")


def test_header_binding_and_exports():
    import os
    import re
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "strkit_amd.h")).read()
    L = _lib.load()
    for name in ("strk_mi_trio", "strk_mi_trio_host", "strk_mi_constants"):
        assert re.search(r"\b%s\(" % name, text) and name in _lib.EXPORTS and hasattr(L, name)
    assert mi.small_threshold() == 256
