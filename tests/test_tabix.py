"""CPU: the tabix index reader (frontend/tabix.py) against the writer of frontend/synth_snvs.py and the corpus of vcf_cases.py:
round trip, block ranges that cover every wanted record, refusals, the stale-index warning."""
import gzip
import os
import struct
import warnings

import numpy as np
import pytest

import vcf_cases
from strkit_amd.frontend.synth_large import _reg2bin
from strkit_amd.frontend.synth_snvs import _block, index_snv_vcf, make_dbsnp_like
from strkit_amd.frontend.tabix import TabixIndex, reg2bins


def _records(text: bytes, block_bytes: int, block_off):
    """(contig, pos0, end0, virtual offset of the line, virtual offset of its end, compressed offset of the block that holds its
    last byte) of every placeable data line."""
    u = 0
    for raw in text.split(b"\n"):
        a, u = u, u + len(raw) + 1
        f = raw.split(b"\t")
        if not raw or raw[:1] == b"#" or len(f) < 4 or not f[1].isdigit() or not 0 < int(f[1]) <= 1 << 29:
            continue
        e = min(u, len(text))
        yield (f[0].decode(), int(f[1]) - 1, int(f[1]) - 1 + max(1, len(f[3].rstrip(b"\r"))),
               (int(block_off[a // block_bytes]) << 16) | a % block_bytes, (int(block_off[e // block_bytes]) << 16) | e % block_bytes,
               int(block_off[(e - 1) // block_bytes]))


def _block_offsets(path: str) -> list[int]:
    raw = open(path, "rb").read()
    offs, off = [], 0
    while off < len(raw):
        offs.append(off)
        off += struct.unpack_from("<H", raw, off + 16)[0] + 1
    return offs


def test_corpus_coverage():
    got = vcf_cases.check_coverage()
    assert got["cases"] >= 30


def test_writer_reader_round_trip(tmp_path):
    plain = str(tmp_path / "d.vcf")
    text = make_dbsnp_like(plain, 3000, step=40)
    gz = index_snv_vcf(plain, block_bytes=4096)
    ix = TabixIndex(gz + ".tbi", gz)
    assert ix.names == ["chr1"] and ix.resolve("1") == "chr1" and ix.resolve("chr2") is None
    offs = _block_offsets(gz)
    recs = list(_records(text, 4096, offs))
    assert len(recs) == 3000
    for _c, p0, e0, v0, v1, _b in recs:
        chunks = ix.bins[0][_reg2bin(p0, e0)]
        assert ((chunks[:, 0] <= v0) & (v1 <= chunks[:, 1])).any()
        assert _reg2bin(p0, e0) in reg2bins(p0, e0)
        for w in range(p0 >> 14, ((e0 - 1) >> 14) + 1):
            assert 0 < ix.linear[0][w] <= v0
    # every window has an entry from the first record's on (empty ones take the preceding window's)
    first = recs[0][1] >> 14
    assert (ix.linear[0][first:] > 0).all() and (np.diff(ix.linear[0][first:].astype(np.int64)) >= 0).all()


def test_block_range_covers_every_wanted_record_of_the_corpus(tmp_path):
    n_single = 0
    for case in vcf_cases.cases():
        if not case.indexable:
            continue
        gz = vcf_cases.written(case, str(tmp_path))
        ix = TabixIndex(gz + ".tbi", gz)
        offs = _block_offsets(gz)
        recs = list(_records(case.text, case.block_bytes, offs))
        for contig, beg, end in case.windows:
            wanted = [r for r in recs if r[0] == contig and beg <= r[1] < end]
            rng = ix.block_range(contig, beg, end)
            if contig not in ix.names:
                assert rng is None
                continue
            if not wanted:
                continue
            assert rng is not None, (case.name, contig, beg, end)
            start, last = rng
            for r in wanted:
                assert start <= r[3] and r[5] <= last, (case.name, beg, end, r, rng)
            n_single += (start >> 16) == last and "single_block_range" in case.tags
    assert n_single > 0
    # a contig the index does not have, an empty window
    ix = TabixIndex(vcf_cases.written(vcf_cases.cases()[0], str(tmp_path)) + ".tbi")
    assert ix.block_range("chr9", 0, 1000) is None and ix.block_range("chr1", 150, 150) is None
    assert ix.block_range("1", 0, 1000) == ix.block_range("chr1", 0, 1000) is not None


def test_index_fill_points_in_front_of_the_window_and_a_long_ref_does_not_cut_the_range(tmp_path):
    by = {c.name: c for c in vcf_cases.cases()}
    gz = vcf_cases.written(by["index_fill"], str(tmp_path))
    ix = TabixIndex(gz + ".tbi")
    recs = list(_records(by["index_fill"].text, 64, _block_offsets(gz)))
    start, _ = ix.block_range("chr1", 20000, 50000)
    assert start == recs[0][3] and recs[0][1] < 20000        # the entry of the empty window 1 is window 0's: the record at 99
    gz = vcf_cases.written(by["long_ref"], str(tmp_path))
    ix = TabixIndex(gz + ".tbi")
    recs = list(_records(by["long_ref"].text, 512, _block_offsets(gz)))
    start, last = ix.block_range("chr1", 33000, 46000)
    d = [r for r in recs if r[1] == 45000][0]
    assert start == recs[0][3] and last >= d[3] >> 16
    # what a stop taken from the linear index would have been: the entry of the window behind the region's, in front of `d`
    assert int(ix.linear[0][(46000 >> 14) + 1]) < d[3]


def _tbi(payload: bytes, path) -> str:
    path.write_bytes(_block(payload, 6) + bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000"))
    return str(path)


def test_refusals_each_give_a_message(tmp_path):
    case = vcf_cases.cases()[0]
    gz = vcf_cases.written(case, str(tmp_path))
    good = gzip.open(gz + ".tbi").read()
    with pytest.raises(ValueError, match="bad magic"):
        TabixIndex(_tbi(b"BAI\x01" + good[4:], tmp_path / "magic.tbi"))
    with pytest.raises(ValueError, match="not the index of a VCF"):
        TabixIndex(_tbi(good[:8] + struct.pack("<i", 0) + good[12:], tmp_path / "format.tbi"))     # format 0: generic
    with pytest.raises(ValueError, match="not the index of a VCF"):
        TabixIndex(_tbi(good[:16] + struct.pack("<i", 4) + good[20:], tmp_path / "col.tbi"))       # col_beg 4
    for cut in (20, 40, len(good) - 9, len(good) - 1):
        with pytest.raises(ValueError, match="truncated"):
            TabixIndex(_tbi(good[:cut], tmp_path / f"cut{cut}.tbi"))
    raw = open(gz + ".tbi", "rb").read()
    (tmp_path / "half.tbi").write_bytes(raw[:len(raw) // 2])
    with pytest.raises(ValueError, match="not a tabix index"):
        TabixIndex(str(tmp_path / "half.tbi"))
    TabixIndex(_tbi(good + struct.pack("<Q", 3), tmp_path / "tail.tbi"))      # the optional trailing count is fine


def test_an_index_older_than_its_file_warns(tmp_path):
    gz = vcf_cases.written(vcf_cases.cases()[0], str(tmp_path))
    os.utime(gz + ".tbi", (1_000_000, 1_000_000))
    with pytest.warns(RuntimeWarning, match="older than"):
        TabixIndex(gz + ".tbi", gz)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        TabixIndex(gz + ".tbi")         # no file named: nothing to compare with
