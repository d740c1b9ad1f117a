"""GPU: strk_dbam_select_reads (k_select_small, k_select_large) over a DeviceBam of the corpus of tests/select_cases.py equals
strk_select_reads over a NativeBam of it, byte for byte (reason, status, n_kept), for all eight `rules` and the caps around the
number of survivors; the same call twice and cut into pieces of 7 loci gives the same bytes; a rec_off in mid-record is
STRK_E_INVALID with the item named, and the handle is good for the next call."""
import numpy as np
import pytest

from select_cases import caps, corpus, expected
from strkit_amd import _lib
from strkit_amd.frontend.native import DeviceBam, NativeBam
from strkit_amd.frontend.select import select_items

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def readers(tmp_path_factory, gpu_ctx):
    path = corpus().write(str(tmp_path_factory.mktemp("select_gpu") / "corpus.bam"))
    dev = DeviceBam(path)
    yield NativeBam(path), dev
    dev.close()


def test_device_equals_host_for_all_rules_and_caps(readers):
    host, dev = readers
    c = corpus()
    assert np.array_equal(host.rec_off, dev.rec_off)
    loci = list(c.loci)
    item_off, rec_off = c.item_arrays(host.rec_off, loci)
    sizes = np.diff(item_off)
    assert (sizes > c.constants["small_items"]).sum() >= 2 and (sizes <= c.constants["small_items"]).sum() >= 10      # both kernels run
    n_calls = 0
    for rules in range(8):
        for cap in caps(c, rules):
            h = select_items(host, rec_off, item_off, rules, cap)
            d = select_items(dev, rec_off, item_off, rules, cap)
            for a, b, what in zip(h, d, ("reason", "status", "n_kept")):
                assert a.tobytes() == b.tobytes(), (rules, cap, what, np.nonzero(a != b)[0][:5])
            n_calls += 1
    e = expected(c, loci, 7, 250)            # (the host entry against the restatement: tests/test_select_rule.py; once here too)
    d = select_items(dev, rec_off, item_off, 7, 250)
    assert all(np.array_equal(a, b) for a, b in zip(e, d))
    print("strk_dbam_select_reads == strk_select_reads: %d calls, %d loci, %d items each" % (n_calls, len(loci), rec_off.size))


def test_twice_and_in_pieces_of_7_loci_the_same_bytes(readers):
    host, dev = readers
    c = corpus()
    loci = list(c.loci)
    item_off, rec_off = c.item_arrays(host.rec_off, loci)
    for rules, cap in ((7, 250), (4, 3), (0, 100)):
        first = select_items(dev, rec_off, item_off, rules, cap)
        again = select_items(dev, rec_off, item_off, rules, cap)
        assert all(a.tobytes() == b.tobytes() for a, b in zip(first, again))
        parts = []
        for l0 in range(0, len(loci), 7):
            io, ro = c.item_arrays(host.rec_off, loci[l0:l0 + 7])
            parts.append(select_items(dev, ro, io, rules, cap))
        for k in range(3):
            assert np.concatenate([p[k] for p in parts]).tobytes() == first[k].tobytes(), (rules, cap, k)


def test_a_rec_off_in_mid_record_is_refused_and_the_handle_lives_on(readers):
    host, dev = readers
    c = corpus()
    loci = ["size_65", "size_%d" % (c.constants["small_items"] + 1), "flags_all"]
    item_off, rec_off = c.item_arrays(host.rec_off, loci)
    good = select_items(host, rec_off, item_off, 7, 250)
    for item in (3, 65 + 700):                         # one in a small locus, one in a large one
        bad = rec_off.copy()
        bad[item] += 5
        with pytest.raises(_lib.StrkError) as ei:
            select_items(dev, bad, item_off, 7, 250)
        assert ei.value.code == _lib.STRK_E_INVALID and "item %d:" % item in str(ei.value) and "malformed" in str(ei.value)
        after = select_items(dev, rec_off, item_off, 7, 250)
        assert all(a.tobytes() == b.tobytes() for a, b in zip(good, after))
    for off in (-1, dev.n_bytes - 8):                  # outside the stream: refused before any launch
        bad = rec_off.copy()
        bad[2] = off
        with pytest.raises(_lib.StrkError) as ei:
            select_items(dev, bad, item_off, 7, 250)
        assert ei.value.code == _lib.STRK_E_INVALID and "item 2:" in str(ei.value) and "outside" in str(ei.value)


def test_two_malformed_records_name_the_first(readers):
    """Two items in mid-record in one small locus, then one in a small and one in a large locus (the two kernels): the call
    names the lower item, and the handle gives the same bytes afterwards."""
    host, dev = readers
    c = corpus()
    loci = ["size_65", "size_%d" % (c.constants["small_items"] + 1), "flags_all"]
    item_off, rec_off = c.item_arrays(host.rec_off, loci)
    assert item_off[1] == 65 <= c.constants["small_items"]
    good = select_items(host, rec_off, item_off, 7, 250)
    for items in ((40, 3), (65 + 700, 3)):
        bad = rec_off.copy()
        bad[list(items)] += 5
        with pytest.raises(_lib.StrkError) as ei:
            select_items(dev, bad, item_off, 7, 250)
        assert ei.value.code == _lib.STRK_E_INVALID and "item 3: malformed" in str(ei.value)
        with pytest.raises(_lib.StrkError, match="item 3: malformed"):
            select_items(host, bad, item_off, 7, 250)
        after = select_items(dev, rec_off, item_off, 7, 250)
        assert all(a.tobytes() == b.tobytes() for a, b in zip(good, after))
