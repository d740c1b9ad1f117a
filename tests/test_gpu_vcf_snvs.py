"""GPU: strk_dbam_vcf_snvs (k_lines_count / k_lines_scan / k_lines_starts of strk_lines.h, k_vcf_parse / k_vcf_compact) on the corpus of vcf_cases.py:
identical to the host twin (strk_vcf_snvs) and to read_snv_vcf on every case and window, for both tile sizes, over whole files,
whole index ranges and one-block pieces; the refusals match."""
import ctypes as C
import os

import numpy as np
import pytest

import vcf_cases
from strkit_amd import _lib
from strkit_amd.frontend.snv_vcf import IndexedSnvVcf

pytestmark = pytest.mark.gpu

CASES = vcf_cases.cases()


@pytest.fixture(scope="module")
def dbam():
    L = _lib.load()
    h = C.c_void_p()
    _lib.check(L.strk_dbam_open(0, C.byref(h)))
    yield h
    L.strk_dbam_close(h)


@pytest.fixture(scope="module")
def corpus_dir(tmp_path_factory):
    return str(tmp_path_factory.mktemp("vcf_corpus"))


def _load(L, dbam, case, corpus_dir) -> int:
    path = vcf_cases.written(case, corpus_dir)
    n = L.strk_dbam_inflate_file(dbam, os.fsencode(path), 0, None)
    assert n == len(case.text), (_lib.load().strk_last_error(), n)
    return int(n)


def _err():
    return _lib.load().strk_last_error().decode()


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_device_equals_host_twin_and_oracle(dbam, corpus_dir, case):
    L = _lib.load()
    n = _load(L, dbam, case, corpus_dir)
    buf = np.frombuffer(case.text, np.uint8).copy()
    for tile in vcf_cases.TILES:
        for contig, beg, end in case.windows:
            host = vcf_cases.query(L, buf, n, case.start, contig, beg, end)
            host_msg = _err() if host[0] < 0 else ""
            dev = vcf_cases.query(L, dbam, n, case.start, contig, beg, end, tile=tile)
            print(case.name, tile, contig, beg, end, "host", host[0], "device", dev[0])
            if vcf_cases.refuses(case):
                assert host[0] == dev[0] == _lib.STRK_E_INVALID
                assert _err().replace("strk_dbam_vcf_snvs", "strk_vcf_snvs") == host_msg and "line at byte" in host_msg
                continue
            assert dev[0] >= 0, _err()
            assert dev == host, (case.name, tile, contig, beg, end)
            assert dev[1:4] == vcf_cases.expected(case, contig, beg, end), (case.name, tile, contig, beg, end)


def test_pieces_with_resume_equal_the_oracle_on_the_device(dbam, corpus_dir):
    """The stream cut at block boundaries by hand: every piece is a prefix of the file's blocks (strk_dbam_inflate up to a block
    boundary), not final, resumed at end_off — the same walk test_vcf_snvs_host.py makes over a host buffer."""
    L = _lib.load()
    for case in (c for c in CASES if c.block_bytes == 256 and not vcf_cases.refuses(c)):
        path = vcf_cases.written(case, corpus_dir)
        comp = np.fromfile(path, np.uint8)
        bounds = []
        off = 0
        while off < comp.size:
            off += (int(comp[off + 16]) | int(comp[off + 17]) << 8) + 1
            bounds.append(off)
        for contig, beg, end in case.windows:
            got = ([], [], [])
            at, prev, seen = case.start, -1, 0
            for b in bounds[:-1]:                      # (the last block is the empty EOF marker)
                nxt = C.c_int64(0)
                n = L.strk_dbam_inflate(dbam, comp.ctypes.data, b, 0, 1 << 30, C.byref(nxt))
                assert n >= 0 and nxt.value == b, _err()
                if n <= at:
                    continue
                final = int(b == bounds[-2])
                k, pos, ids, ref, end_off, _past, _ = vcf_cases.query(L, dbam, int(n), at, contig, beg, end, final=final, prev=prev, seen=seen, tile=256)
                assert k >= 0, _err()
                for g, x in zip(got, (pos, ids, ref)):
                    g.extend(x)
                if pos:
                    prev, seen = pos[-1], 1
                at = end_off
            assert tuple(got) == vcf_cases.expected(case, contig, beg, end), (case.name, contig, beg, end)


@pytest.mark.parametrize("piece_bytes", [1, 32 << 20])
def test_indexed_reader_on_the_device_equals_the_oracle(corpus_dir, piece_bytes):
    for case in CASES:
        if not case.indexable or case.start:
            continue
        r = IndexedSnvVcf(vcf_cases.written(case, corpus_dir), front_end="device", piece_bytes=piece_bytes, tile_bytes=256 if piece_bytes == 1 else 0)
        try:
            for contig, beg, end in case.windows:
                if vcf_cases.refuses(case):
                    with pytest.raises(_lib.StrkError, match="not coordinate-sorted|POS is not 1 to 18"):
                        r.window(contig, beg, end)
                    continue
                w = r.window(contig, beg, end)
                assert (w.pos.tolist(), list(w.ids), list(w.ref)) == vcf_cases.expected(case, contig, beg, end), (case.name, contig, beg, end)
            assert r.window("chr9", 0, 100) is None
            assert r.kernel_s() > 0 or not any(len(vcf_cases.expected(case, *w)[0]) for w in case.windows if not vcf_cases.refuses(case))
        finally:
            r.close()


def test_offsets_are_checked_before_any_launch(dbam, corpus_dir):
    L = _lib.load()
    case = CASES[0]
    n = _load(L, dbam, case, corpus_dir)
    for start in (n + 1, -1, 1 << 40):
        k, *_ = vcf_cases.query(L, dbam, n, start, "chr1", 0, 100)
        assert k == _lib.STRK_E_INVALID and "outside the text" in _err()
    k, *_ = vcf_cases.query(L, dbam, n, 0, "chr1", 0, 100, tile=100)
    assert k == _lib.STRK_E_INVALID and "tile_bytes" in _err()
    # a start at the very end: nothing to read, nothing launched
    k, pos, _ids, _ref, end_off, past, id_bytes = vcf_cases.query(L, dbam, n, n, "chr1", 0, 100)
    assert (k, pos, end_off, past, id_bytes) == (0, [], n, 0, 0)
    out3 = (C.c_int32 * 3)()
    L.strk_vcf_constants(out3)
    assert list(out3) == [1024, 256, vcf_cases.LINES_PER_WAVE] and 1024 in vcf_cases.TILES and 256 in vcf_cases.TILES
