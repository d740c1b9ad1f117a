"""GPU: strk_dbam_discover_snvs (k_snv_span, k_snv_pileup, k_snv_pick) over a DeviceBam of the corpus of snv_discover_cases.py
gives the bytes of the host function (which tests/test_snv_discover_host.py holds against the rule) under both windows; a call
cut into pieces of 37 items and a repeated call give them again; the refusals before a launch; an offset that is not a record
start is refused naming the item."""
import numpy as np
import pytest

import snv_discover_cases as cases
from strkit_amd import _lib
from strkit_amd.frontend import DeviceBam, NativeBam, write_bam
from strkit_amd.frontend import snv_discovery as sd

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def readers(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("snv_discover_gpu") / "corpus.bam")
    write_bam(path, [cases.CONTIG], cases.corpus()["records"])
    nb, db = NativeBam(path), DeviceBam(path)
    assert np.array_equal(nb.rec_off, db.rec_off)
    yield nb, db
    db.close()


def _same(got, want):
    assert np.array_equal(got[0], want[0]), [lc["name"] for lc, a, b in zip(cases.corpus()["loci"], np.diff(got[0]), np.diff(want[0])) if a != b]
    assert np.array_equal(got[1], want[1])
    assert got[0].dtype == want[0].dtype and got[1].dtype == want[1].dtype


@pytest.mark.parametrize("window", cases.WINDOWS)
def test_the_kernels_give_the_host_function_and_the_rule(readers, window):
    host = cases.library(readers[0], window)
    _same(cases.library(readers[1], window), host)
    _same(host, cases.expected(window))
    assert int(np.diff(host[0]).max()) == 1024


@pytest.mark.parametrize("window", cases.WINDOWS)
def test_a_call_cut_into_pieces_and_a_repeated_call_give_the_same_bytes(readers, window):
    host = cases.library(readers[0], window)
    for piece in (37, 1, 0, 0):
        _same(cases.library(readers[1], window, piece_items=piece), host)


def test_other_thresholds_and_a_window_of_one_tile_and_of_sixteen(readers):
    c = cases.corpus()
    for window, mbq, mar in ((1, 20, 2), (4096, 0, 1), (4097, 31, 3), (65536, 20, 5)):
        got, want = (sd.library_discover_snvs(b, c["item_file_index"], c["item_locus"], c["left"], c["right"], c["kept_off"], c["kept_item"],
                                              alt=c["alt"], window=window, min_base_qual=mbq, min_allele_reads=mar) for b in (readers[1], readers[0]))
        _same(got, want)
        assert want[1].size > 0, window


def _raw(db, rec_off, item_locus, left, right, kept_off, kept_item, window=8192, mbq=20, mar=2, piece=0, cap=4096):
    off, pos = np.zeros(left.size + 1, np.int32), np.zeros(cap, np.int64)
    rc = _lib.load().strk_dbam_discover_snvs(db._h, int(rec_off.size), _lib.ptr(rec_off), _lib.ptr(item_locus), int(left.size), _lib.ptr(left),
                                             _lib.ptr(right), _lib.ptr(kept_off), _lib.ptr(kept_item), None, None, None, 100, 250, window, mbq, mar,
                                             piece, _lib.ptr(off), _lib.ptr(pos), cap)
    return int(rc), off, pos


def test_device_refusals_and_the_size_query(readers):
    L = _lib.load()
    nb, db = readers
    c = cases.corpus()
    n9 = 9
    rec = np.ascontiguousarray(nb.rec_off[c["item_file_index"][:n9]], np.int64)
    loc = np.zeros(n9, np.int32)
    left, right = c["left"][:1].copy(), c["right"][:1].copy()
    koff, kit = np.array([0, n9], np.int32), np.arange(n9, dtype=np.int32)
    rc, off, pos = _raw(db, rec, loc, left, right, koff, kit)
    assert rc == 3 and off.tolist() == [0, 3] and pos[:3].tolist() == [0, 5, 299]          # (nine of the ten reads of cut_at_0: a_thr is 2 still)
    rc, off, pos = _raw(db, rec, loc, left, right, koff, kit, cap=2)
    assert rc == 3 and off.tolist() == [0, 3] and not pos.any()                             # the size query writes no position

    def refused(needle, *args, **kw):
        rc, _, _ = _raw(db, *args, **kw)
        assert rc == _lib.STRK_E_INVALID and needle.encode() in L.strk_last_error(), (needle, rc, L.strk_last_error())

    refused("window must be in 1 .. 65536", rec, loc, left, right, koff, kit, window=0)
    refused("window must be in 1 .. 65536", rec, loc, left, right, koff, kit, window=65537)
    refused("min_base_qual", rec, loc, left, right, koff, kit, mbq=256)
    refused("min_allele_reads", rec, loc, left, right, koff, kit, mar=0)
    refused("bad argument", rec, loc, left, right, koff, kit, piece=-1)
    refused("left_coord > right_coord", rec, loc, right + 1, right, koff, kit)
    refused("item_locus out of range", rec, loc + 1, left, right, koff, kit)
    refused("belongs to locus", rec, np.array([0] * 8 + [1], np.int32), np.repeat(left, 2), np.repeat(right, 2), np.array([0, n9, n9], np.int32), kit)
    bad = rec.copy()
    bad[3] = int(nb.data.size) - 3
    refused("item 3: rec_off outside the buffer", bad, loc, left, right, koff, kit)
    many = np.zeros(sd.MAX_KEPT_READS + 1, np.int32)
    refused("65536 kept reads (at most 65535", rec, loc, left, right, np.array([0, many.size], np.int32), many)
    # an offset that is not a record start: the kernel's parser refuses the item (the first of the two), nothing outside the stream
    # is read, and the handle gives the corpus's bytes afterwards
    for piece in (0, 4):
        bad = rec.copy()
        bad[[8, 1]] += 2
        rc, _, _ = _raw(db, bad, loc, left, right, koff, kit, piece=piece)
        assert rc == _lib.STRK_E_INVALID and L.strk_last_error() == b"strk_dbam_discover_snvs: item 1: malformed BAM record"
    _same(cases.library(db, 5000), cases.library(nb, 5000))
