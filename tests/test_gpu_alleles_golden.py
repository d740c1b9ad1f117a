"""GPU: strk_call_alleles, strk_call_alleles_n and strk_call_alleles_phased against tests/golden/alleles_parent.npz, the
outputs recorded with the commit before k_alleles and k_alleles_n became one kernel template (tests/golden/
make_alleles_golden.py): every output array byte for byte, NaN slots included."""
import importlib.util
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _maker():
    spec = importlib.util.spec_from_file_location("make_alleles_golden", os.path.join(GOLDEN, "make_alleles_golden.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_three_entry_points_return_the_recorded_bytes(gpu_ctx):
    M = _maker()
    with np.load(os.path.join(GOLDEN, "alleles_parent.npz")) as f:
        stored = {k: f[k] for k in f.files}
    inputs = {k: v for k, v in stored.items() if k.split("_B")[0] not in ("plain", "n", "phased")}
    want = {k: v for k, v in stored.items() if k not in inputs}
    got = M.run_all(inputs, gpu_ctx)
    assert set(got) == set(want) and len(want) == 2 * (10 + 10 + 16)
    for k in sorted(want):
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, k
        as_int = np.dtype(f"u{want[k].dtype.itemsize}")   # NaN slots compare by their bits
        diff = np.nonzero(np.ascontiguousarray(got[k]).view(as_int).ravel() != np.ascontiguousarray(want[k]).view(as_int).ravel())[0]
        assert diff.size == 0, (k, diff[:8].tolist(), got[k].ravel()[diff[:8]], want[k].ravel()[diff[:8]])
    # the fixture reaches what it is there for: refused loci (too few reads; fewer reads than alleles), every modal number
    # of peaks, phased and unphased loci
    assert set(want["plain_B100_modal_n"].tolist()) == {0, 1, 2} and set(want["n_B100_modal_n"].tolist()) == set(range(7))
    assert (want["n_B100_status"] == 1).sum() > (want["plain_B100_status"] == 1).sum() > 0
    assert {0, 3} <= set(want["phased_B100_status"].tolist())
