"""GPU: k_dbam_methyl over a DeviceBam of the corpus of methyl_cases.py gives the bytes of the host function strk_methyl (which
tests/test_methyl_host.py holds against the rule): status, sites, known, mc.  The corpus holds the shapes made from the
kernel's size constants as built (bases per pass, MM bytes per pass, ordinals per window); a call cut into pieces of 37 items
and a repeated call give the same bytes; a hostile record fails with STRK_E_INVALID."""
import numpy as np
import pytest

import methyl_cases as cases
from strkit_amd import _lib
from strkit_amd.frontend import DeviceBam, NativeBam, write_bam
from strkit_amd.frontend import methyl as me

pytestmark = pytest.mark.gpu
KEYS = ("status", "sites", "known", "mc")


@pytest.fixture(scope="module")
def readers(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("methyl_gpu") / "corpus.bam")
    write_bam(path, [cases.CONTIG], cases.corpus()["records"])
    nb, db = NativeBam(path), DeviceBam(path)
    assert np.array_equal(nb.rec_off, db.rec_off)
    yield nb, db
    db.close()


@pytest.fixture(scope="module")
def host(readers):
    c = cases.corpus()
    return me.methyl(readers[0], np.arange(len(c["records"])), c["coords"], c["alt"])


def _same(a, b):
    c = cases.corpus()
    for k in KEYS:
        bad = np.nonzero(a[k] != b[k])[0]
        assert bad.size == 0, (k, c["records"][int(bad[0])]["name"], c["kinds"][int(bad[0])], len(c["records"][int(bad[0])]["seq"]),
                               [int(a[x][bad[0]]) for x in KEYS], [int(b[x][bad[0]]) for x in KEYS], bad[:10].tolist())


def test_the_corpus_holds_the_kernel_s_shapes(host):
    c = cases.corpus()
    k = c["constants"]
    lens = {len(r["seq"]) for r in c["records"]}
    assert {k["seq_pass_bases"] - 1, k["seq_pass_bases"], k["seq_pass_bases"] + 1} <= lens
    assert (host["sites"] >= k["window"] + 1).any() and (host["sites"] == k["window"]).any() and (host["sites"] == k["window"] - 1).any()
    n_numbers = {r["tags"].split(b"\0")[0].count(b",") for r in c["records"] if r["tags"].startswith(b"MMZC+m,")}
    assert {1, k["mm_pass_bytes"] - 1, k["mm_pass_bytes"], k["mm_pass_bytes"] + 1, 1000} <= n_numbers
    assert any(r["tags"].startswith(b"MMZC+m;") for r in c["records"])                    # no numbers
    assert any(r["tags"][3:].find(b";") == k["mm_pass_bytes"] - 1 for r in c["records"])  # a ';' on a pass's last byte
    print("methyl corpus: %d items, statuses %s" % (len(c["records"]), np.bincount(host["status"], minlength=6).tolist()))


def test_device_equals_the_host_function(readers, host):
    c = cases.corpus()
    got = me.methyl(readers[1], np.arange(len(c["records"])), c["coords"], c["alt"])
    _same(got, host)
    print("k_dbam_methyl == strk_methyl on %d items (status, sites, known, mc)" % len(c["records"]))


def test_pieces_of_37_items_and_a_repeated_call(readers, host):
    c = cases.corpus()
    idx = np.arange(len(c["records"]))
    _same(me.methyl(readers[1], idx, c["coords"], c["alt"], piece_items=37), host)
    _same(me.methyl(readers[1], idx, c["coords"], c["alt"]), host)


def test_another_threshold_and_a_subset(readers):
    c = cases.corpus()
    idx = np.arange(3, len(c["records"]), 5)
    alt = {k: c["alt"][int(i)] for k, i in enumerate(idx) if int(i) in c["alt"]}
    for thr in (0, 200, 255):
        a = me.methyl(readers[1], idx, c["coords"][idx], alt, threshold=thr)
        b = me.methyl(readers[0], idx, c["coords"][idx], alt, threshold=thr)
        for k in KEYS:
            assert np.array_equal(a[k], b[k]), (thr, k)


def test_a_hostile_record_and_bad_arguments_fail_before_anything_is_trusted(readers):
    nb, db = readers
    c = cases.corpus()
    L = _lib.load()
    # an offset that is not a record start: the kernel's parser refuses the item, nothing outside the stream is read
    off = nb.rec_off[:3].copy()
    off[1] += 2
    co = np.ascontiguousarray(c["coords"][:3])
    out = [np.zeros(3, np.int32) for _ in range(4)]
    rc = L.strk_dbam_methyl(db._h, 3, _lib.ptr(off), _lib.ptr(co), None, None, None, 127, 0, *[_lib.ptr(o) for o in out])
    assert rc == _lib.STRK_E_INVALID and "item 1" in L.strk_last_error().decode()
    with pytest.raises(_lib.StrkError, match="threshold"):
        me.methyl(db, np.arange(2), c["coords"][:2], None, threshold=256)
    off[1] = nb.data.size
    rc = L.strk_dbam_methyl(db._h, 3, _lib.ptr(off), _lib.ptr(co), None, None, None, 127, 0, *[_lib.ptr(o) for o in out])
    assert rc == _lib.STRK_E_INVALID and "rec_off" in L.strk_last_error().decode()


def _first(bam, n, **kw):
    """The first n items of the corpus (a partly filled last workgroup of k_dbam_methyl for n = 9)."""
    c = cases.corpus()
    return me.methyl(bam, np.arange(n), c["coords"][:n], {k: v for k, v in c["alt"].items() if k < n}, **kw)


@pytest.mark.parametrize("piece", [1, 8, 9, 10, 2 ** 31 - 1])
def test_piece_seams_of_nine_items(readers, piece):
    a, b = _first(readers[1], 9, piece_items=piece), _first(readers[0], 9)
    for k in KEYS:
        assert np.array_equal(a[k], b[k]), (piece, k)


@pytest.mark.parametrize("piece", [0, 4])
def test_two_malformed_records_name_the_first(readers, host, piece):
    """Items 8 and 1 of 9 point two bytes into a record: different workgroups of four items, and with piece_items = 4 different
    launches.  The call names item 1, and the handle gives the corpus's bytes afterwards."""
    nb, db = readers
    c = cases.corpus()
    L = _lib.load()
    off = nb.rec_off[:9].copy()
    off[[8, 1]] += 2
    co = np.ascontiguousarray(c["coords"][:9])
    out = [np.zeros(9, np.int32) for _ in range(4)]
    rc = L.strk_dbam_methyl(db._h, 9, _lib.ptr(off), _lib.ptr(co), None, None, None, 127, piece, *[_lib.ptr(o) for o in out])
    assert rc == _lib.STRK_E_INVALID and L.strk_last_error() == b"strk_dbam_methyl: item 1: malformed BAM record or auxiliary fields"
    _same(me.methyl(db, np.arange(len(c["records"])), c["coords"], c["alt"]), host)
