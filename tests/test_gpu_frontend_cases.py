"""GPU: the device file front end (k_dbam_scan, k_dbam_extract1 / 2, k_dbam_names, DeviceBam.segment, strk_dbam_voffsets) on the
corpus of tests/frontend_cases.py - several contigs, H / N / P and zero-length operations, CG-tag CIGARs, records without
qualities, all sixteen base codes, unmapped records, interleaved spans - against the rule (frontend/extract.py, read_bam) first
and the host library (which tests/test_frontend_cases.py holds against the same rule) second.  Integers and bytes: no tolerance."""
import ctypes as C
import os

import numpy as np
import pytest

import frontend_cases as fc
from strkit_amd import _lib
from strkit_amd.frontend import DeviceBam, IndexedBam, NativeBam, extract_reads
from strkit_amd.frontend.bam import _bgzf_blocks

pytestmark = pytest.mark.gpu

FIELDS = ("rec_off", "tid", "pos", "end", "flag", "l_seq", "clip_l", "clip_r")


@pytest.fixture(scope="module")
def readers():
    path = fc.corpus_file()["path"]
    nb, db = NativeBam(path), DeviceBam(path)
    yield nb, db
    db.close()


@pytest.fixture(scope="module")
def handle():
    """A device reader of its own for the tests that load other stretches."""
    h = C.c_void_p()
    _lib.check(_lib.load().strk_dbam_open(0, C.byref(h)))
    yield h
    _lib.load().strk_dbam_close(h)


def _scan(h, starts, cap):
    """strk_dbam_scan called directly: (its return value, the arrays of capacity `cap`)."""
    starts = np.ascontiguousarray(starts, np.int64)
    out = {"rec_off": np.full(cap, -7, np.int64), **{k: np.full(cap, -7, np.int32) for k in FIELDS[1:] + ("l_name",)}}
    n = _lib.load().strk_dbam_scan(h, _lib.ptr(starts), starts.size, cap, *(_lib.ptr(out[k]) for k in FIELDS + ("l_name",)))
    return int(n), out


def _scan_both_ways(h, starts, want, lo=0, hi=None, shift=0):
    """The count alone (cap == 0), then the filled arrays: records [lo, hi) of `want`, offsets relative to `shift`."""
    hi = len(want["tid"]) if hi is None else hi
    n, _ = _scan(h, starts, 0)
    assert n == hi - lo, (n, lo, hi, _lib.load().strk_last_error())
    n, out = _scan(h, starts, hi - lo)
    assert n == hi - lo
    for k in FIELDS + ("l_name",):
        assert np.array_equal(out[k], want[k][lo:hi] - (shift if k == "rec_off" else 0)), k


def _seqs(db, n):
    got = np.zeros(int(n), np.uint8)
    if n:
        _lib.check(_lib.load().strk_dbam_download_seqs(db._h, int(n), _lib.ptr(got)))
    return got


# ---- scan --------------------------------------------------------------------------------------------------------------------
def test_indexed_open_gives_the_records_of_read_bam(readers):
    nb, db = readers
    f = fc.corpus_file()
    lin = IndexedBam._read_bai(f["path"] + ".bai", len(fc.CONTIGS))
    assert lin[1].size == 0 and len(np.unique(np.concatenate(lin))) >= 16          # many entry points; none on the empty contig
    assert db.n_records == nb.n_records == len(f["bam"].segments) and db.references == nb.references
    for k in FIELDS:
        assert np.array_equal(getattr(db, k), f["fields"][k]), k
        assert np.array_equal(getattr(db, k), getattr(nb, k)), k
    assert np.array_equal(db.l_name, f["fields"]["l_name"])


@pytest.mark.parametrize("which", ["first", "every", "seventh", 255, 256, 257])
def test_scan_from_other_entry_points_gives_the_same_arrays(readers, which):
    _, db = readers
    want = fc.corpus_file()["fields"]
    n = want["rec_off"].size
    pick = {"first": np.array([0]), "every": np.arange(n), "seventh": np.arange(0, n, 7)}.get(which)
    if pick is None:
        pick = np.unique(np.linspace(0, n - 1, which).astype(np.int64))
        assert pick.size == which and pick[0] == 0
    _scan_both_ways(db._h, want["rec_off"][pick], want)


def test_an_entry_point_inside_a_record_is_refused_and_the_reader_goes_on(readers):
    _, db = readers
    want = fc.corpus_file()["fields"]
    k = int(np.nonzero(want["tid"] == 0)[0][40])            # (two bytes in: the upper half of block_size and the lower of refID 0 read as 0)
    starts = np.array([want["rec_off"][0], want["rec_off"][k] + 2, want["rec_off"][k + 9]], np.int64)
    for cap in (0, want["rec_off"].size):
        n, _ = _scan(db._h, starts, cap)
        assert n == _lib.STRK_E_INVALID and b"malformed" in _lib.load().strk_last_error()
    _scan_both_ways(db._h, want["rec_off"][[0, k, k + 9]], want)


# ---- stretches ---------------------------------------------------------------------------------------------------------------
def test_a_file_cut_inside_its_last_record_is_truncated(handle):
    L = _lib.load()
    f = fc.corpus_file()
    want = f["fields"]
    cut = f["stream"][:int(want["rec_off"][-1]) + 21]
    comp = np.frombuffer(_bgzf_blocks(cut), np.uint8)
    nxt = C.c_int64(0)
    assert L.strk_dbam_inflate(handle, _lib.ptr(comp), comp.size, 0, 1 << 40, C.byref(nxt)) == len(cut) and nxt.value == comp.size
    for starts in (want["rec_off"][:1], want["rec_off"]):
        n, _ = _scan(handle, starts, 0)
        assert n == _lib.STRK_E_INVALID and b"truncated" in L.strk_last_error()
    # the same bytes as a stretch that stops in front of the end of its buffer: the cut record is the next stretch's business
    assert L.strk_dbam_inflate(handle, _lib.ptr(comp), comp.size, 0, len(cut) - 1, C.byref(nxt)) > 0 and nxt.value < comp.size
    n_in = int(np.searchsorted(f["rec_end"], (len(cut) - 1) // 0xFF00 * 0xFF00, side="right"))
    _scan_both_ways(handle, want["rec_off"][:1], want, 0, n_in)


@pytest.mark.parametrize("which", ["first block", "two in the middle", "tail"])
def test_block_ranges_of_the_file_give_the_records_that_lie_wholly_inside(handle, which):
    L = _lib.load()
    f = fc.corpus_file()
    want, (coff, uoff, ulen) = f["fields"], f["layout"]
    size = os.path.getsize(f["path"])
    nb_ = coff.size                                        # (the last block is the empty end-of-file marker)
    k0, k1 = {"first block": (0, 1), "two in the middle": (nb_ // 2, nb_ // 2 + 2), "tail": (nb_ - 4, nb_)}[which]
    lo, hi = int(coff[k0]), int(coff[k1]) if k1 < nb_ else size
    u_lo, u_hi = int(uoff[k0]), int(uoff[k1 - 1] + ulen[k1 - 1])
    assert L.strk_dbam_inflate_file_range(handle, os.fsencode(f["path"]), lo, hi, 0, None) == u_hi - u_lo
    got = np.zeros(u_hi - u_lo, np.uint8)
    _lib.check(L.strk_dbam_download(handle, 0, got.size, _lib.ptr(got)))
    assert got.tobytes() == f["stream"][u_lo:u_hi]
    # every record start the index could name, mapped into the stretch
    voff = np.ascontiguousarray(f["voff"], np.uint64)
    off = np.zeros(voff.size, np.int64)
    _lib.check(L.strk_dbam_voffsets(handle, _lib.ptr(voff), voff.size, _lib.ptr(off)))
    inside = (want["rec_off"] >= u_lo) & (want["rec_off"] < u_hi)
    assert np.array_equal(off[inside], want["rec_off"][inside] - u_lo) and (off[~inside] == -1).all()
    first, last = int(np.argmax(inside)), int(np.searchsorted(f["rec_end"], u_hi, side="right"))
    cut = bool(((want["rec_off"] < u_hi) & (f["rec_end"] > u_hi)).any())
    assert cut == (which != "tail") and last - first > 20                          # a record runs across the end, except at EOF
    for starts in (off[inside], off[inside][:1], off[inside][::5]):
        _scan_both_ways(handle, starts, want, first, last, shift=u_lo)
    if which == "tail":
        assert last == want["rec_off"].size and (want["tid"][first:last] == -1).any()
    # an offset equal to its block's length is the start of the next block; the end of the stretch; blocks that are not resident
    other = 2 if k0 > 2 else nb_ - 3
    assert nb_ > 8 and not k0 <= other < k1
    probe = np.array([(int(coff[k0]) << 16) | int(ulen[k0]), (int(coff[k1 - 1]) << 16) | int(ulen[k1 - 1]),
                      (int(coff[k0]) << 16) | (int(ulen[k0]) + 1), (int(coff[k0]) + 1) << 16, (int(coff[other]) << 16) | 5], np.uint64)
    out = np.zeros(probe.size, np.int64)
    _lib.check(L.strk_dbam_voffsets(handle, _lib.ptr(probe), probe.size, _lib.ptr(out)))
    assert out.tolist() == [int(ulen[k0]), u_hi - u_lo, -1, -1, -1] and 0 < int(ulen[k0]) < 65536


# ---- extraction --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("param", fc.PARAMS)
@pytest.mark.parametrize("with_alt", [False, True])
def test_extraction_equals_the_rule_and_the_host_bytes(readers, param, with_alt):
    nb, db = readers
    c = fc.corpus()
    alt = c["alt"] if with_alt else None
    ed = extract_reads(db, c["item_rec"], c["coords"], *param, alt=alt)
    seqs = _seqs(db, ed["seq_off"][-1])
    fc.same_extraction(ed, seqs, fc.expected(param, with_alt))
    eh = extract_reads(nb, c["item_rec"], c["coords"], *param, alt=alt)
    for k in ("status", "nfl", "ntr", "nfr", "seq_off"):
        assert np.array_equal(ed[k], eh[k]), k
    assert np.array_equal(seqs, eh["seqs"]) and ed["d_seqs"]
    # the call again: the same bytes
    again = extract_reads(db, c["item_rec"], c["coords"], *param, alt=alt)
    assert all(np.array_equal(again[k], ed[k]) for k in ("status", "nfl", "ntr", "nfr", "seq_off"))
    assert np.array_equal(_seqs(db, again["seq_off"][-1]), seqs)


def test_extraction_without_alt_start_and_of_nothing(readers):
    nb, db = readers
    c = fc.corpus()
    for param in fc.PARAMS:
        got, seqs = fc.raw_extract(db, c["alt0_rec"], c["alt0_coords"], c["alt0"], param, alt_start=False)
        fc.same_extraction(got, seqs, fc.expected_alt0(param))
        assert np.array_equal(got["name_len"], fc.corpus_file()["fields"]["l_name"][c["alt0_rec"]] - 1)
    got, seqs = fc.raw_extract(db, np.zeros(0, np.int64), np.zeros((0, 4), np.int64), None, fc.PARAMS[0])
    assert got["rc"] == 0 and got["seq_off"].tolist() == [0] and seqs.size == 0


@pytest.mark.parametrize("piece", [1, 31, 32, 33, 257])
def test_extraction_in_pieces_gives_the_concatenation(readers, piece):
    """k_dbam_extract2 takes 32 items per workgroup: pieces on both sides of that, one item at a time, and more than one
    workgroup of k_dbam_extract1 (256 items)."""
    _, db = readers
    c = fc.corpus()
    param = fc.PARAMS[0]
    want = fc.expected(param, True)
    n = len(c["item_rec"])
    for lo in range(0, n, piece):
        hi = min(n, lo + piece)
        alt = {it - lo: c["alt"][it] for it in range(lo, hi) if it in c["alt"]}
        got, seqs = fc.raw_extract(db, c["item_rec"][lo:hi], c["coords"][lo:hi], alt, param)
        fc.same_extraction(got, seqs, want, lo, hi)


# ---- names and segments ------------------------------------------------------------------------------------------------------
def test_names(readers):
    nb, db = readers
    c, segs = fc.corpus(), fc.corpus_file()["bam"].segments
    assert db.names(c["names"]) == ["", "x", "n" * 254] == nb.names(c["names"])
    assert db.names(c["names"][:1]) == [""] and db.name(int(c["names"][2])) == "n" * 254
    idx = np.random.default_rng(3).integers(0, db.n_records, 700)
    idx[100:110] = idx[0]
    assert len(idx) > 256 and len(set(idx.tolist())) < len(idx) and (np.diff(idx) < 0).any()
    assert db.names(idx) == [segs[i].name for i in idx.tolist()] == nb.names(idx)
    assert db.names(np.arange(db.n_records)) == [s.name for s in segs]


def test_segments_and_interval_queries(readers):
    nb, db = readers
    c, f = fc.corpus(), fc.corpus_file()
    segs = f["bam"].segments
    for i in np.unique(np.concatenate((c["hand"], c["cg"], c["no_qual"], c["unmapped"]))).tolist():
        fc.same_segment(db.segment(i), segs[i])
    for contig in ("chrA", "chrC"):
        starts = np.array([0, 1000, 1010, 1040, 20000, 20100, 20150, 7000, 7400, 399000], np.int64)
        ends = starts + np.array([10 ** 6, 100, 100, 5, 400, 400, 1, 700, 300, 1000], np.int64)
        a, na = nb.fetch_many(contig, starts, ends, 250)
        b, nd = db.fetch_many(contig, starts, ends, 250)
        assert np.array_equal(a, b) and np.array_equal(na, nd) and na.sum() > 250
        for k in range(1, len(starts)):
            assert [segs[i].name for i in db.fetch_indices(contig, int(starts[k]), int(ends[k]))] == \
                [s.name for s in f["bam"].fetch(contig, int(starts[k]), int(ends[k]))]


# ---- refusals ----------------------------------------------------------------------------------------------------------------
def test_extract_refuses_offsets_outside_the_stream(readers):
    """Every offset here is refused by the host walk in front of the launches, or (two bytes inside a record) by the parser's own
    bounds inside the stream: nothing is passed that a kernel would follow outside the buffer."""
    L = _lib.load()
    nb, db = readers
    c, want = fc.corpus(), fc.corpus_file()["fields"]
    n_data = db.n_bytes
    assert n_data == len(fc.corpus_file()["stream"])
    rec = c["item_rec"][:3]
    good = want["rec_off"][rec]
    for bad in (-1, -(1 << 40), n_data, n_data - 1, n_data - 2, n_data - 3, n_data - 35, (1 << 63) - 2):
        got, _ = fc.raw_extract(db, rec, c["coords"][:3], None, fc.PARAMS[0], rec_off=np.array([good[0], bad, good[2]], np.int64), check=False)
        assert got["rc"] == _lib.STRK_E_INVALID and b"item 1:" in L.strk_last_error() and b"outside the stream" in L.strk_last_error(), bad
    k = int(np.nonzero(want["tid"] == 0)[0][40])
    got, _ = fc.raw_extract(db, rec, c["coords"][:3], None, fc.PARAMS[0], rec_off=np.array([good[0], good[1], want["rec_off"][k] + 2], np.int64),
                            check=False)
    assert got["rc"] == _lib.STRK_E_INVALID and L.strk_last_error() == b"item 2: malformed BAM record"
    got, seqs = fc.raw_extract(db, c["item_rec"][:300], c["coords"][:300], None, fc.PARAMS[0])     # the handle works afterwards
    fc.same_extraction(got, seqs, fc.expected(fc.PARAMS[0], False), 0, 300)


def test_names_refuses_offsets_and_slices_outside_the_stream(readers):
    L = _lib.load()
    _, db = readers
    want = fc.corpus_file()["fields"]
    n_data = db.n_bytes
    out = np.zeros(1 << 12, np.uint8)
    r = want["rec_off"]
    cases = [(np.array([r[0], -1, r[2]]), np.array([0, 3, 6, 9]), b"item 1:"),
             (np.array([r[0], r[1], n_data]), np.array([0, 3, 6, 9]), b"item 2:"),
             (np.array([r[0], r[1], r[2]]), np.array([0, 5, 3, 9]), b"item 1:"),                  # not ascending
             (np.array([r[0], r[1], r[2]]), np.array([1, 5, 6, 9]), b"item 0:"),                  # not from 0
             (np.array([r[0], r[1], r[-1]]), np.array([0, 3, 6, 6 + (1 << 11)]), b"item 2:"),     # a slice past the end of the stream
             (np.array([r[0], n_data - 36, r[2]]), np.array([0, 3, 4, 9]), b"item 1:")]
    for rec_off, out_off, msg in cases:
        rec_off, out_off = rec_off.astype(np.int64), out_off.astype(np.int64)
        rc = L.strk_dbam_names(db._h, 3, _lib.ptr(rec_off), _lib.ptr(out_off), _lib.ptr(out))
        assert rc == _lib.STRK_E_INVALID and msg in L.strk_last_error(), (msg, L.strk_last_error())
    assert db.names(np.arange(5)) == [s.name for s in fc.corpus_file()["bam"].segments[:5]]


def test_two_malformed_records_name_the_first(readers):
    """Items 299 and 3 of 300, in different workgroups of k_dbam_extract1, point two bytes into a record (inside the stream: the
    kernel's parser refuses them): the call names item 3, and the handle gives the corpus's bytes afterwards."""
    L = _lib.load()
    nb, db = readers
    c, want = fc.corpus(), fc.corpus_file()["fields"]
    rec, coords = c["item_rec"][:300], c["coords"][:300]
    off = want["rec_off"][rec].copy()
    off[[299, 3]] = want["rec_off"][int(np.nonzero(want["tid"] == 0)[0][40])] + 2
    got, _ = fc.raw_extract(db, rec, coords, None, fc.PARAMS[0], rec_off=off, check=False)
    assert got["rc"] == _lib.STRK_E_INVALID and L.strk_last_error() == b"item 3: malformed BAM record"
    got, seqs = fc.raw_extract(db, rec, coords, None, fc.PARAMS[0])
    fc.same_extraction(got, seqs, fc.expected(fc.PARAMS[0], False), 0, 300)


def test_extract_checks_the_substitute_alignments_before_any_launch(readers):
    """The malformed triples get the host entry's refusal, word for word, from the check in front of the launches; a triple
    without operations, with or without its starts, gives the bytes of the call without substitute alignments."""
    L = _lib.load()
    nb, db = readers
    c = fc.corpus()
    n = 40
    rec, coords = c["item_rec"][:n], c["coords"][:n]
    for triple, msg in fc.malformed_alt(n):
        for bam in (nb, db):
            got, _ = fc.raw_extract(bam, rec, coords, None, fc.PARAMS[0], alt_raw=triple, check=False)
            assert got["rc"] == _lib.STRK_E_INVALID and L.strk_last_error() == msg, (msg, L.strk_last_error())
    plain, plain_seqs = fc.raw_extract(nb, rec, coords, None, fc.PARAMS[0])
    for start in (np.full(n, 7, np.int64), None):
        got, seqs = fc.raw_extract(db, rec, coords, None, fc.PARAMS[0], alt_raw=(np.zeros(1, np.uint32), np.zeros(n + 1, np.int64), start))
        assert all(np.array_equal(got[k], plain[k]) for k in ("status", "nfl", "ntr", "nfr", "seq_off")) and np.array_equal(seqs, plain_seqs)
