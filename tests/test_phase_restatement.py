"""CPU: the restatement of the phased allele calls (tests/phase_restatement.py, rule A-F of DESIGN.md §13) against stock
sklearn, against a literal transcription of the reference's distance function, and on hand vectors; and the C-ABI surface of
strk_call_alleles_phased."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import alleles_restatement as AR
import phase_cases as PC
import phase_restatement as PR
from strkit_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _tie_heavy_inputs(n_inputs: int, seed: int):
    """Distance inputs as SNV cells make them: few SNVs, gaps, out-of-range cells, low qualities, pure and mixed distances;
    n from 2 to 60 and a few at 250."""
    rng = np.random.default_rng(seed)
    for it in range(n_inputs):
        m = 250 if it % 200 == 199 else int(rng.integers(2, 61))
        S = int(rng.integers(1, 7))
        base = rng.choice(np.frombuffer(b"ACGT-_", np.uint8), size=(m, S), p=[.3, .3, .1, .1, .1, .1])
        qual = rng.choice([10, 20, 40], size=(m, S)).astype(np.uint8)
        cn = rng.integers(8, 14, size=m)
        yield cn, base, qual, bool(it & 1)


def test_chain_partition_equals_sklearn_on_every_tie_heavy_input():
    cluster = pytest.importorskip("sklearn.cluster")
    n = 0
    for cn, base, qual, pure in _tie_heavy_inputs(1200, 5):
        dm = PR.distance_matrix(cn, base, qual, pure)
        got = PR.nn_chain_two_clusters(dm)
        sk = cluster.AgglomerativeClustering(n_clusters=2, metric="precomputed", linkage="average").fit(dm).labels_
        want = (sk != sk[0]).astype(np.int32)   # cluster 0 holds the first read
        assert np.array_equal(got, want), (n, dm.shape)
        n += 1
    assert n >= 1000


def _reference_distance(cn, base, qual, pure, few=0.2, many=0.1, many_q=3, thr=20):
    """calculate_read_distance (call_locus.py:91-174) word for word, driven by read dicts."""
    items = [(f"r{i}", {"cn": int(cn[i]), "snvu": tuple((chr(b), int(q)) for b, q in zip(base[i], qual[i]))}) for i in range(len(cn))]
    n_reads, n_useful = len(items), base.shape[1]
    rng_u = tuple(range(n_useful))
    dm = np.zeros((n_reads, n_reads), dtype=np.float64)

    def skip_set(idx):
        u = items[idx][1]["snvu"]
        return set(filter(lambda y: u[y][0] == "-" or (u[y][0] != "_" and u[y][1] < thr), rng_u))

    for i in range(n_reads - 1):
        r1 = items[i][1]
        r1_skip = skip_set(i)
        for j in range(i + 1, n_reads):
            r2 = items[j][1]
            d, n_comparable = 0.0, 0
            r2_skip = skip_set(j)
            for z in rng_u:
                if z in r1_skip or z in r2_skip:
                    continue
                if r1["snvu"][z][0] != r2["snvu"][z][0]:
                    d += 1.0
                n_comparable += 1
            if not pure:
                d += abs(r1["cn"] - r2["cn"]) * (many if n_comparable >= many_q else few)
            dm[i, j] = dm[j, i] = d
    return dm


def test_distance_matrix_equals_the_reference_function():
    for k, (cn, base, qual, pure) in enumerate(_tie_heavy_inputs(60, 9)):
        if base.shape[0] > 60:
            continue
        assert np.array_equal(PR.distance_matrix(cn, base, qual, pure), _reference_distance(cn, base, qual, pure)), k


@pytest.mark.parametrize("vec", PC.hand_vectors(), ids=lambda v: v[0])
def test_hand_vectors(vec):
    name, x, tags, snvs, exp = vec
    got = PR.call_locus(x["cn"], x["w"], x["n_alleles"], AR.locus_seed(1, 0), x["hp"] if tags else None, x["ps"] if tags else None,
                        x["base"] if snvs else None, x["qual"] if snvs else None)
    PC.check_expected(name, got, exp)
    assert not got["close_means"]


def test_hand_vectors_cover_every_reason_and_snv_status_that_can_occur():
    exps = [v[4] for v in PC.hand_vectors()]
    assert {e["reason"] for e in exps if "reason" in e} >= {PR.REASON_NONE, PR.REASON_NO_TAGS, PR.REASON_TAG_THRESHOLDS,
                                                             PR.REASON_FEW_SNV_READS, PR.REASON_GROUP_NOT_CALLED,
                                                             PR.REASON_NO_SNV_CALLED}
    seen = {int(s) for e in exps for s in e.get("snv_status", [])}
    assert seen >= {PR.SNV_CALLED, PR.SNV_ZERO_TOTAL, PR.SNV_ONLY_OUT_OF_RANGE, PR.SNV_CROSS_TALK}


def test_a_failed_haplotag_call_falls_through_to_the_snvs():
    # the haplotag step applies but one HP group has a single read: the SNVs then make the call
    x = PC._locus([10, 10, 11, 10, 20, 21, 20, 20, 10, 10], hp=[1] * 8 + [2, 1], ps=[4] * 10,
                  cells=["AA"] * 4 + ["TT"] * 4 + ["AA"] * 2)
    got = PR.call_locus(x["cn"], x["w"], 2, 5, x["hp"], x["ps"], x["base"], x["qual"])
    assert (got["method"], got["reason"], got["ps"]) == (PR.ASSIGN_SNV, PR.REASON_NONE, -1)
    assert got["peak_n_reads"] == [6, 4]


def test_symbol_is_declared_listed_and_exported():
    src = open(os.path.join(ROOT, "include", "strkit_amd.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    assert re.search(r"\bstrk_call_alleles_phased\s*\(", src)
    assert "strk_call_alleles_phased" in _lib.EXPORTS
    lib = _lib.load()
    assert lib.strk_call_alleles_phased is not None
    assert C.sizeof(_lib.StrkPhaseParams) == 40
    for name in ("STRK_ASSIGN_SNV_DIST", "STRK_PHASE_NO_SNV_CALLED", "STRK_ALLELE_NOT_PHASED", "STRK_SNV_CROSS_TALK"):
        assert re.search(r"#define\s+%s\b" % name, src), name


def test_null_context_is_refused_by_name_without_touching_a_device():
    lib = _lib.load()
    rc = lib.strk_call_alleles_phased(None, 0, *([None] * 5), None, None, *([None] * 5), 0, *([None] * 16), None)
    assert rc == _lib.STRK_E_INVALID
    assert b"strk_call_alleles_phased" in lib.strk_last_error()
