"""GPU: strk_call_alleles and strk_call_alleles_phased in turn on ONE context.  The two calls share the context's side stream
and timing events and carve their device buffers the same way, so neither may leave behind what the other trips over: every
result equals, byte for byte, the same call on a context of its own.  (Both sides run the same code, so this is no check of the
scatter of a piece's rows at a locus > 0: a cut call against the uncut one in tests/test_gpu_phase.py is.)"""
import numpy as np
import pytest

import phase_cases as PC
from strkit_amd import _lib
from strkit_amd.alleles import call_alleles_batch
from strkit_amd.phasing import PhaseParams, call_alleles_phased_batch

pytestmark = pytest.mark.gpu


def _on_a_context_of_its_own(call):
    ctx = _lib.Context(0)
    try:
        return call(ctx)
    finally:
        ctx.close()


def _same_bytes(a: dict, b: dict, what):
    assert a.keys() == b.keys(), what
    for key in a:
        assert a[key].dtype == b[key].dtype and a[key].tobytes() == b[key].tobytes(), (what, key)


def test_plain_phased_plain_on_one_context_equal_calls_on_fresh_contexts(fresh_ctx):
    rng = np.random.default_rng(13)
    # three loci of 8 reads and 2 SNVs, and one without reads in front of the last (a piece that copies no read up or down)
    loci = [PC.make_locus(rng, n, 2, 2, tag_kind, "clean") for n, tag_kind in ((8, "clean"), (8, "none"), (0, "none"), (8, "clean"))]
    a = PC.pack(loci, [3, 5, 7, 11])
    assert np.diff(a["read_off"]).tolist() == [8, 8, 0, 8] and np.diff(a["snv_off"]).tolist() == [2, 2, 2, 2]
    five = (a["read_off"], a["cns"], a["weights"], a["n_alleles"], a["seeds"])
    plain = lambda c: call_alleles_batch(*five, ctx=c)                                                     # noqa: E731
    phased = lambda c: call_alleles_phased_batch(*five, a["hp"], a["ps"], a["snv_off"], a["snv_base"], a["snv_qual"],   # noqa: E731
                                                 phase_params=PhaseParams(piece_loci=1), fallback=False, ctx=c, with_stats=True)
    first = plain(fresh_ctx)
    _same_bytes(first, _on_a_context_of_its_own(plain), "1 plain")
    got, st = phased(fresh_ctx)
    assert st["n_sub_batches"] == 4 and st["n_dp_launches"] == 16        # one piece per locus: rows land at l0 = 1, 2, 3
    _same_bytes(got, _on_a_context_of_its_own(phased)[0], "2 phased")
    again = plain(fresh_ctx)
    _same_bytes(again, _on_a_context_of_its_own(plain), "3 plain again")
    _same_bytes(again, first, "3 plain again, against 1")
