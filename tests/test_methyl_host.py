"""CPU: the library's host function strk_methyl (the walks of strk_methyl.h compiled for the host) against the readable statement
of the rule, frontend/methyl.py, on the seeded corpus of methyl_cases.py; hostile auxiliary chains; the argument checks.
Nothing here needs a GPU; nothing is skipped."""
import struct

import numpy as np
import pytest

import methyl_cases as cases
from strkit_amd import _lib
from strkit_amd.frontend import NativeBam, write_bam
from strkit_amd.frontend import methyl as me
from strkit_amd.frontend.synth_methyl import mm_tags

KEYS = ("status", "sites", "known", "mc")


@pytest.fixture(scope="module")
def bam(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("methyl") / "corpus.bam")
    write_bam(path, [cases.CONTIG], cases.corpus()["records"])
    return NativeBam(path)


def test_corpus_covers_what_it_should(bam):
    c, e = cases.corpus(), cases.expected()
    n = len(c["records"])
    assert n >= 2000 and bam.rec_off.size == n
    assert [bam.name(i) for i in (0, 1, n - 1)] == [c["records"][i]["name"] for i in (0, 1, n - 1)]   # file order = item order
    counts = np.bincount(e["status"], minlength=6)
    assert counts.min() > 0 and counts[0] >= n / 4, counts
    assert c["alt"] and any(r.get("long_cigar") for r in c["records"]) and any(not r["tags"] for r in c["records"])
    q_l = c["coords"][:, 1] - np.array([r["pos"] for r in c["records"]])
    assert (q_l % 2 == 0).sum() > 200 and (q_l % 2 == 1).sum() > 200
    assert {r["flag"] for r in c["records"]} == {0, 16}
    assert (e["known"] < e["sites"]).any() and (e["mc"] > 0).any()


def test_host_function_equals_the_rule(bam):
    c, e = cases.corpus(), cases.expected()
    got = me.methyl(bam, np.arange(len(c["records"])), c["coords"], c["alt"])
    for k in KEYS:
        bad = np.nonzero(got[k] != e[k])[0]
        assert bad.size == 0, (k, c["records"][int(bad[0])]["name"], c["kinds"][int(bad[0])], int(got[k][bad[0]]), int(e[k][bad[0]]),
                               [int(got[x][bad[0]]) for x in KEYS], [int(e[x][bad[0]]) for x in KEYS])


def test_without_the_substitute_alignments_those_items_do_not_span(bam):
    c, e = cases.corpus(), cases.expected()
    got = me.methyl(bam, np.arange(len(c["records"])), c["coords"], None)
    idx = np.array(sorted(c["alt"]))
    assert (got["status"][idx] == _lib.STRK_METHYL_NOT_SPANNING).all() and (e["status"][idx] != _lib.STRK_METHYL_NOT_SPANNING).any()
    rest = np.setdiff1d(np.arange(len(c["records"])), idx)
    for k in KEYS:
        assert np.array_equal(got[k][rest], e[k][rest])


def test_another_threshold(bam):
    c = cases.corpus()
    idx = np.arange(0, len(c["records"]), 7)
    got = me.methyl(bam, idx, c["coords"][idx], {k: c["alt"][int(i)] for k, i in enumerate(idx) if int(i) in c["alt"]}, threshold=200)
    from strkit_amd.frontend.bam import AlignedSegment
    for k, i in enumerate(idx.tolist()):
        r = c["records"][i]
        seg = AlignedSegment(r["name"], r["flag"], r["contig"], r["pos"], 60, cases.cigar_array(r["cigar"]), r["seq"], r["qual"], r["tags"])
        assert tuple(int(got[x][k]) for x in KEYS) == me.segment_methylation(seg, c["coords"][i], c["alt"].get(i), 200)


# ---- hostile records ----------------------------------------------------------------------------------------------------
def _call_raw(buf: bytes, rec_off, coords=(100, 101, 102, 103), threshold=127, alt=(None, None, None)):
    L = _lib.load()
    data = np.frombuffer(buf, np.uint8).copy()               # exactly the bytes: nothing behind them belongs to the buffer
    n = len(rec_off)
    rec_off = np.asarray(rec_off, np.int64)
    co = np.tile(np.asarray(coords, np.int64), n)
    out = [np.full(n, -7, np.int32) for _ in range(4)]
    rc = L.strk_methyl(_lib.ptr(data), data.size, n, _lib.ptr(rec_off), _lib.ptr(co), *[_lib.ptr(a) if a is not None else None for a in alt],
                       threshold, *[_lib.ptr(o) for o in out])
    return rc, L.strk_last_error().decode(), [o.tolist() for o in out]


ACGA = bytes([0x12, 0x41])       # A C G A packed: with the boundaries below the tract is the C, its G one past it


def test_hostile_auxiliary_chains_name_the_item():
    good = cases.raw_record(100, [4 << 4], ACGA, 4, mm_tags([("C+m", [0], [200])]))
    rc, _, out = _call_raw(good + good, [0, len(good)])
    assert rc == 0 and out == [[0, 0], [1, 1], [1, 1], [1, 1]]                                # one site, called
    tags = mm_tags([("C+m", [0], [200])])
    for bad_tags in (tags[:-1], b"MMZC+m,0", b"XY", b"MLBC" + struct.pack("<I", 9) + b"\1", b"MLBx" + struct.pack("<I", 0), b"XXq1",
                     tags + b"ZZZ", b"MLBC\xff\xff\xff\xff"):
        bad = cases.raw_record(100, [4 << 4], ACGA, 4, bad_tags)
        rc, msg, _ = _call_raw(good + bad + good, [0, len(good), len(good) + len(bad)])
        assert rc == _lib.STRK_E_INVALID and "item 1" in msg and "strk_methyl" in msg, (bad_tags, rc, msg)
        rc, msg, _ = _call_raw(bad, [0])                                                       # the record ends the buffer
        assert rc == _lib.STRK_E_INVALID and "item 0" in msg
    # an offset that is no record start, a record cut off by the end of the buffer
    rc, msg, _ = _call_raw(good + good, [0, 2])
    assert rc == _lib.STRK_E_INVALID and "item 1" in msg
    rc, msg, _ = _call_raw((good + good)[:-1], [0, len(good)])
    assert rc == _lib.STRK_E_INVALID and "item 1" in msg


def test_an_alignment_longer_than_its_bases():
    """Extraction cuts its flanks to flank_size before it asks whether they lie inside the bases, so it keeps such a read with a
    small flank size: the read has a value as long as its TRACT lies inside the bases, and none where the tract itself ends past them."""
    seq6 = bytes([0x12, 0x41, 0x24])                      # A C G A C G
    rec = cases.raw_record(100, [8 << 4], seq6, 6, mm_tags([("C+m", [0], [200])]))      # 8M over 6 bases
    rc, _, out = _call_raw(rec, [0], coords=(100, 101, 104, 107))                        # q = 0, 1, 4, 7: the right flank ends past the bases
    assert rc == 0 and [o[0] for o in out] == [_lib.STRK_METHYL_OK, 1, 1, 1]
    data = np.frombuffer(rec, np.uint8).copy()
    one = lambda: np.zeros(1, np.int32)  # noqa: E731
    status, nfl, ntr, nfr, seq_off = one(), one(), one(), one(), np.zeros(2, np.int64)
    off, co = np.zeros(1, np.int64), np.array([100, 101, 104, 107], np.int64)
    for flank, want in ((1, 0), (2, 0), (3, 1), (70, 1)):                                # extraction: kept up to the flank size that reaches past the bases
        assert _lib.load().strk_extract_reads(_lib.ptr(data), data.size, 1, _lib.ptr(off), _lib.ptr(co), None, None, None, flank, 0, -1, _lib.ptr(status),
                                              _lib.ptr(nfl), _lib.ptr(ntr), _lib.ptr(nfr), None, 0, _lib.ptr(seq_off)) == 0
        assert status[0] == want and (want or ntr[0] == 3)
    rc, _, out = _call_raw(rec, [0], coords=(100, 101, 107, 107))                        # the tract itself ends at 7 > 6
    assert rc == 0 and [o[0] for o in out] == [_lib.STRK_METHYL_NOT_SPANNING, 0, 0, 0]
    from strkit_amd.frontend.bam import AlignedSegment
    seg = AlignedSegment("r", 0, "chr1", 100, 60, cases.cigar_array([(8, "M")]), "ACGACG", None, mm_tags([("C+m", [0], [200])]))
    assert me.segment_methylation(seg, (100, 101, 104, 107)) == (_lib.STRK_METHYL_OK, 1, 1, 1)
    assert me.segment_methylation(seg, (100, 101, 107, 107))[0] == _lib.STRK_METHYL_NOT_SPANNING


def test_argument_checks():
    good = cases.raw_record(100, [4 << 4], ACGA, 4, mm_tags([("C+m", [0], [200])]))
    for thr in (-1, 256):
        rc, msg, _ = _call_raw(good, [0], threshold=thr)
        assert rc == _lib.STRK_E_INVALID and "threshold" in msg
    for thr in (0, 255):
        assert _call_raw(good, [0], threshold=thr)[0] == 0
    for off in (-1, len(good) - 3, len(good) + 5):
        rc, msg, _ = _call_raw(good, [off])
        assert rc == _lib.STRK_E_INVALID and "rec_off" in msg
    ops = np.array([4 << 4], np.uint32)
    rc, msg, _ = _call_raw(good, [0], alt=(ops, None, None))
    assert rc == _lib.STRK_E_INVALID and "alt_cigar" in msg
    rc, msg, _ = _call_raw(good, [0], alt=(ops, np.array([1, 1], np.int64), None))
    assert rc == _lib.STRK_E_INVALID and "alt_cigar_off[0]" in msg
    rc, msg, _ = _call_raw(good + good, [0, len(good)], alt=(ops, np.array([0, 1, 0], np.int64), None))
    assert rc == _lib.STRK_E_INVALID and "decreasing" in msg
    rc, msg, out = _call_raw(good, [0], alt=(ops, np.array([0, 1], np.int64), np.array([100], np.int64)))
    assert rc == 0 and out[0] == [0]
    L = _lib.load()
    assert L.strk_methyl(None, 0, 0, None, None, None, None, None, 127, None, None, None, None) == 0      # no items: nothing to do
    assert L.strk_methyl(None, 0, -1, None, None, None, None, None, 127, None, None, None, None) == _lib.STRK_E_INVALID
    data = np.frombuffer(good, np.uint8).copy()
    off, co = np.zeros(1, np.int64), np.array([100, 101, 102, 103], np.int64)
    assert L.strk_methyl(_lib.ptr(data), data.size, 1, _lib.ptr(off), _lib.ptr(co), None, None, None, 127, None, None, None, None) == _lib.STRK_E_INVALID
    assert "NULL" in L.strk_last_error().decode()


def test_two_malformed_records_name_the_first(bam):
    """2 100 items drawn with repetition from the corpus's first records, two threads at 1 024 items per thread where there
    are two cores: items 1 500 and 5 point two bytes into a record, and the call names item 5 (it named the last one)."""
    L = _lib.load()
    n = 2100
    pick = np.random.default_rng(30).integers(0, 64, n)
    off = bam.rec_off[pick].copy()
    off[[1500, 5]] += 2
    co = np.ascontiguousarray(cases.corpus()["coords"][pick], np.int64)
    out = [np.zeros(n, np.int32) for _ in range(4)]

    def call():
        rc = L.strk_methyl(_lib.ptr(bam.data), bam.data.size, n, _lib.ptr(off), _lib.ptr(co), None, None, None, 127, *[_lib.ptr(o) for o in out])
        return rc, L.strk_last_error().decode()

    for _ in range(3):
        assert call() == (_lib.STRK_E_INVALID, "strk_methyl: item 5: malformed BAM record or auxiliary fields")
    off[5] -= 2
    assert call() == (_lib.STRK_E_INVALID, "strk_methyl: item 1500: malformed BAM record or auxiliary fields")
    off[1500] -= 2
    assert call()[0] == 0


def test_constants_are_exported():
    k = me.methyl_constants()
    assert k["seq_pass_bases"] == 64 * k["chunk_bases"] and k["mm_pass_bytes"] == 64 and k["window"] % 4 == 0 and k["window"] >= 64
