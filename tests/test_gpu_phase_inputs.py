"""GPU: k_dbam_phase_cells, k_snv_useful and k_snv_gather over a DeviceBam of the corpus of phase_inputs_cases.py give the bytes
of the host functions (which tests/test_phase_inputs_host.py holds against the rule): tags, cells, snv_off, candidate indices
and the packed matrices; a call cut into pieces of 37 items and a repeated call give them again."""
import numpy as np
import pytest

import phase_inputs_cases as cases
from strkit_amd import _lib
from strkit_amd.frontend import DeviceBam, NativeBam, write_bam
from strkit_amd.frontend import phase_inputs as pi

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def readers(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("phase_inputs_gpu") / "corpus.bam")
    write_bam(path, [cases.CONTIG], cases.corpus()["records"])
    nb, db = NativeBam(path), DeviceBam(path)
    assert np.array_equal(nb.rec_off, db.rec_off)
    yield nb, db
    db.close()


def _cells(bam, alt=True, **kw):
    c = cases.corpus()
    return pi.phase_cells(bam, c["item_file_index"], c["item_locus"], c["cand_off"], c["cand_pos"], alt=c["alt"] if alt else None, **kw)


@pytest.fixture(scope="module")
def host(readers):
    cells = _cells(readers[0])
    kept_off, kept_item = cases.kept_reads()
    return cells, pi.library_useful_snvs(cells, kept_off, kept_item, 2)


def _same_cells(a, b):
    for k in ("hp", "ps", "base", "qual"):
        bad = np.nonzero(a[k] != b[k])[0]
        assert bad.size == 0, (k, int(bad[0]), a[k][bad[:8]], b[k][bad[:8]])


def _same_snvs(a, b):
    for k in ("snv_off", "snv_cand", "snv_base", "snv_qual"):
        assert np.array_equal(a[k], b[k]), k


def test_device_cells_and_useful_snvs_equal_the_host_functions(readers, host):
    kept_off, kept_item = cases.kept_reads()
    got = _cells(readers[1], download=True)
    _same_cells(got, host[0])
    assert int(np.diff(host[1]["snv_off"]).max()) == pi.MAX_USEFUL_SNVS and (np.diff(host[1]["snv_off"]) == 10).any()   # (the two-haplotype loci)
    _same_snvs(pi.library_useful_snvs(got, kept_off, kept_item, 2), host[1])
    # without the substitute alignments, and with every read kept
    got = _cells(readers[1], alt=False, download=True)
    plain = _cells(readers[0], alt=False)
    _same_cells(got, plain)
    n_loci = cases.corpus()["n_loci"]
    all_off = np.concatenate(([0], np.cumsum(np.bincount(cases.corpus()["item_locus"], minlength=n_loci)))).astype(np.int32)
    all_item = np.arange(cases.corpus()["item_locus"].size, dtype=np.int32)
    _same_snvs(pi.library_useful_snvs(got, all_off, all_item, 3), pi.library_useful_snvs(plain, all_off, all_item, 3))


def test_a_call_cut_into_pieces_and_a_repeated_call_give_the_same_bytes(readers, host):
    kept_off, kept_item = cases.kept_reads()
    for piece in (37, 0, 0):
        got = _cells(readers[1], piece_items=piece, download=True)
        _same_cells(got, host[0])
        _same_snvs(pi.library_useful_snvs(got, kept_off, kept_item, 2), host[1])


def test_device_refusals(readers):
    L = _lib.load()
    nb, db = readers
    c = cases.corpus()
    # a hostile record cannot be written with write_bam; the checks before the launch are those of the host function
    with pytest.raises(_lib.StrkError, match="ascending"):
        pi.phase_cells(db, c["item_file_index"][:2], np.zeros(2, np.int32), np.array([0, 2], np.int32), np.array([9, 3], np.int64))
    with pytest.raises(_lib.StrkError, match="no cells"):      # a refused call leaves no cells behind
        pi.library_useful_snvs({"device": db, "cand_off": np.array([0, 2], np.int32)}, np.array([0, 0], np.int32), np.zeros(0, np.int32), 2)
    cells = _cells(db)
    with pytest.raises(_lib.StrkError, match="loci"):
        pi.library_useful_snvs({"device": db, "cand_off": np.array([0, 2], np.int32)}, np.array([0, 0], np.int32), np.zeros(0, np.int32), 2)
    kept_off, kept_item = cases.kept_reads()
    wrong = kept_item.copy()
    wrong[0] = c["item_locus"].size
    with pytest.raises(_lib.StrkError, match="out of range"):
        pi.library_useful_snvs(cells, kept_off, wrong, 2)
    # an offset that is not a record start: the kernel's parser refuses the item, nothing outside the stream is read
    off = nb.rec_off[c["item_file_index"][:3]].copy()
    off[1] += 2
    hp, ps, loc = np.zeros(3, np.int32), np.zeros(3, np.int32), np.zeros(3, np.int32)
    cand_off, cand = np.array([0, 1], np.int32), np.array([1005], np.int64)
    rc = L.strk_dbam_phase_cells(db._h, 3, _lib.ptr(off), _lib.ptr(loc), 1, _lib.ptr(cand_off), _lib.ptr(cand), None, None, None, 100, 250, 0,
                                 _lib.ptr(hp), _lib.ptr(ps))
    assert rc == _lib.STRK_E_INVALID and b"item 1" in L.strk_last_error()


def _first(bam, n, **kw):
    """The first n items of the corpus (a partly filled last workgroup of k_dbam_phase_cells for n = 9)."""
    c = cases.corpus()
    alt = {k: v for k, v in c["alt"].items() if k < n}
    return pi.phase_cells(bam, c["item_file_index"][:n], c["item_locus"][:n], c["cand_off"], c["cand_pos"], alt=alt, **kw)


@pytest.mark.parametrize("piece", [1, 8, 9, 10, 2 ** 31 - 1])
def test_piece_seams_of_nine_items(readers, piece):
    _same_cells(_first(readers[1], 9, piece_items=piece, download=True), _first(readers[0], 9))


@pytest.mark.parametrize("piece", [0, 4])
def test_two_malformed_records_name_the_first(readers, host, piece):
    """Items 8 and 1 of 9 point two bytes into a record: different workgroups of four items, and with piece_items = 4 different
    launches.  The call names item 1, and the handle gives the corpus's bytes afterwards."""
    L = _lib.load()
    nb, db = readers
    c = cases.corpus()
    off = nb.rec_off[c["item_file_index"][:9]].copy()
    off[[8, 1]] += 2
    hp, ps, loc = np.zeros(9, np.int32), np.zeros(9, np.int32), np.zeros(9, np.int32)
    cand_off, cand = np.array([0, 1], np.int32), np.array([1005], np.int64)
    rc = L.strk_dbam_phase_cells(db._h, 9, _lib.ptr(off), _lib.ptr(loc), 1, _lib.ptr(cand_off), _lib.ptr(cand), None, None, None, 100, 250, piece,
                                 _lib.ptr(hp), _lib.ptr(ps))
    assert rc == _lib.STRK_E_INVALID and L.strk_last_error() == b"strk_dbam_phase_cells: item 1: malformed BAM record or auxiliary fields"
    _same_cells(_cells(db, download=True), host[0])
