"""strkit_amd/alleles.py on the CPU: what call_alleles_batch and call_alleles_phased_batch share before the library is entered
(the coercion and span check of the five inputs, the output arrays, the key order of the C signature) and _lib.ptr."""
import numpy as np
import pytest

from strkit_amd import _lib
from strkit_amd.alleles import ALLELE_KEYS, batch_inputs, batch_outputs, call_alleles_batch
from strkit_amd.phasing import call_alleles_phased_batch

SPAN = "read_off must span cns, and cns and weights must have one entry per read"


def test_batch_inputs_coerces_and_broadcasts():
    read_off, cns, weights, n_alleles, seeds, n_loci = batch_inputs([0, 2, 5], np.arange(10, dtype=np.int64)[::2], [1, 2, 3, 4, 5],
                                                                   2, [7, 2 ** 64 - 1])
    assert n_loci == 2
    assert [a.dtype for a in (read_off, cns, weights, n_alleles, seeds)] == [np.int32, np.int32, np.float64, np.int32, np.uint64]
    assert all(a.flags["C_CONTIGUOUS"] for a in (read_off, cns, weights, n_alleles, seeds))
    assert cns.tolist() == [0, 2, 4, 6, 8] and weights.tolist() == [1.0, 2.0, 3.0, 4.0, 5.0]
    assert n_alleles.tolist() == [2, 2] and seeds.tolist() == [7, 2 ** 64 - 1]
    n_alleles[0] = 1                                                  # a broadcast scalar became an array of its own
    assert n_alleles.tolist() == [1, 2]
    *_, n_alleles, seeds, n_loci = batch_inputs([0], [], [], 2, 1)     # no loci: a valid call
    assert n_loci == 0 and n_alleles.shape == seeds.shape == (0,)
    assert batch_inputs([0, 0], [], [], [1], [1])[5] == 1             # a locus without reads


@pytest.mark.parametrize("read_off,cns,weights", [
    ([], [], []),                       # an empty read_off: no locus count
    ([0, 2], [1, 2, 3], [1, 1, 1]),     # read_off ends before cns does
    ([0, 4], [1, 2, 3], [1, 1, 1]),     # ... and behind it
    ([0, 3], [1, 2, 3], [1, 1]),        # a weight missing
])
def test_both_calls_refuse_a_bad_span_before_they_enter_the_library(read_off, cns, weights):
    with pytest.raises(ValueError, match=SPAN):
        batch_inputs(read_off, cns, weights, 2, 1)
    no_ctx = object()                   # never looked at: the refusal comes first
    with pytest.raises(ValueError, match=SPAN):
        call_alleles_batch(read_off, cns, weights, 2, 1, ctx=no_ctx)
    with pytest.raises(ValueError, match=SPAN):
        call_alleles_phased_batch(read_off, cns, weights, 2, 1, ctx=no_ctx)


def test_batch_outputs_has_the_arrays_of_the_c_signature():
    out = batch_outputs(3, 7)
    assert tuple(out) == (*ALLELE_KEYS, "read_peak")                  # the order strk_call_alleles takes them in
    assert ALLELE_KEYS == ("status", "modal_n", "call", "ci95", "ci99", "means", "weights", "stdevs", "peak_n_reads")
    shapes = dict(status=(3,), modal_n=(3,), call=(3, 2), ci95=(3, 2, 2), ci99=(3, 2, 2), means=(3, 2), weights=(3, 2),
                  stdevs=(3, 2), peak_n_reads=(3, 2), read_peak=(7,))
    for k, a in out.items():
        assert a.shape == shapes[k] and a.dtype == (np.float64 if k in ("means", "weights", "stdevs") else np.int32), k
        assert a.flags["C_CONTIGUOUS"] and a.flags["OWNDATA"], k
    assert [a.size for a in batch_outputs(0, 0).values()] == [0] * 10


def test_ptr_is_null_for_none_and_the_address_otherwise():
    a = np.arange(4, dtype=np.int32)
    assert _lib.ptr(None) is None
    assert _lib.ptr(a).value == a.ctypes.data
    assert _lib.ptr(a[1:]).value == a.ctypes.data + 4
