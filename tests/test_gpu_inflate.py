"""k_bgzf_inflate (strk_inflate.h compiled for the device, one lane per BGZF block) against zlib on the corpus of
tests/inflate_cases.py: every block type, several deflate blocks per BGZF block, code shapes zlib never writes, every copy
branch at its edges, headers of other writers — and one malformed body per error return, which must be refused under the
right block index.  The same bodies pass tests/test_frontend.py on the host compile and tools/inflate_asan.sh under the
sanitizers; expected bytes are zlib's throughout."""
import bisect
import ctypes as C
import os
import re

import numpy as np
import pytest

import inflate_cases as ic
from strkit_amd import _lib

pytestmark = pytest.mark.gpu

EOF_BLOCK = ("empty", b"\x03\x00", b"")


@pytest.fixture(scope="module")
def dbam(gpu_ctx):
    L = _lib.load()
    h = C.c_void_p()
    _lib.check(L.strk_dbam_open(0, C.byref(h)))
    yield L, h
    L.strk_dbam_close(h)


@pytest.fixture(scope="module")
def whole():
    """The accepted cases in a seeded shuffled order, as one file: (cases, file, block offsets, byte offsets, zlib's bytes)."""
    ic.check_coverage()
    some = ic.shuffled(ic.accepted())
    return (some,) + ic.bgzf_file(some)


def _inflate(L, h, comp: bytes, coff: int = 0, max_out: int = 1 << 40):
    """(return value, next_coff, the bytes on the device) of strk_dbam_inflate."""
    arr = np.frombuffer(comp, np.uint8)
    nxt = C.c_int64(-1)
    n = L.strk_dbam_inflate(h, arr.ctypes.data, arr.size, coff, max_out, C.byref(nxt))
    got = np.empty(max(int(n), 0), np.uint8)
    if n > 0:
        _lib.check(L.strk_dbam_download(h, 0, int(n), got.ctypes.data))
    return n, nxt.value, got.tobytes()


def _same(got: bytes, want: bytes, some, uoff) -> None:
    """got == want, or the name of the first block that differs and where."""
    if got == want:
        return
    a, b = np.frombuffer(got, np.uint8), np.frombuffer(want, np.uint8)
    assert a.size == b.size, (a.size, b.size)
    at = int(np.flatnonzero(a != b)[0])
    k = bisect.bisect_right(uoff, at) - 1
    raise AssertionError(f"block {k} ({some[k][0]}) differs from zlib at byte {at - uoff[k]} of its {len(some[k][2])}: "
                         f"{a[at]:#x} for {b[at]:#x}")


def _check_file(L, h, some) -> None:
    comp, _, uoff, raw = ic.bgzf_file(some)
    n, nxt, got = _inflate(L, h, comp)
    assert n == len(raw) and nxt == len(comp), (n, len(raw), L.strk_last_error())
    _same(got, raw, some, uoff)


def test_every_accepted_body_gives_zlibs_bytes(dbam, whole):
    L, h = dbam
    some, comp, coff, uoff, raw = whole
    assert {(c[1][0] >> 1) & 3 for c in some[:64] if c[1]} == {0, 1, 2}          # the first wave holds every block type
    n, nxt, got = _inflate(L, h, comp)
    assert n == len(raw) and nxt == len(comp), (n, len(raw), L.strk_last_error())
    _same(got, raw, some, uoff)
    arr = np.frombuffer(comp, np.uint8)
    assert L.strk_bgzf_inflate(arr.ctypes.data, arr.size, None, 0, 0) == n


@pytest.mark.parametrize("n_blocks", [1, 63, 64, 65, 129])
def test_grid_edges(dbam, whole, n_blocks):
    L, h = dbam
    _check_file(L, h, whole[0][:n_blocks])
    _check_file(L, h, whole[0][-n_blocks:])


def test_lane_edges_and_buffer_reuse(dbam, whole):
    L, h = dbam
    some = whole[0]
    # empty blocks (ISIZE 0) in lanes 0 and 63 of the first workgroup and lane 0 of the second
    _check_file(L, h, [EOF_BLOCK] + some[:62] + [EOF_BLOCK, EOF_BLOCK] + some[62:100] + [EOF_BLOCK])
    # 64 copies of the slowest body (the most tokens: 65000 literals under Z_HUFFMAN_ONLY), the fastest among them: 63 lanes
    # of the first workgroup run long after one has finished
    by_name = {c[0]: c for c in some}
    slow, fast = by_name["zlib/qual65000/L9huff"], by_name["zlib/len7/L1fixed"]
    _check_file(L, h, [slow] * 32 + [fast] + [slow] * 32)
    # the handle's buffers shrink and grow again: big, small, big
    _check_file(L, h, some)
    _check_file(L, h, some[:3])
    _check_file(L, h, some)


def test_stretch_takes_whole_blocks_only(dbam, whole):
    L, h = dbam
    some, comp, coff, uoff, raw = whole
    first = len(some) // 2
    for n_take, inside in ((40, 1), (1, 5), (70, 1000)):
        while len(some[first + n_take][2]) < 2:                                     # (the limit falls inside a block)
            n_take += 1
        last = first + n_take                                                       # the block that no longer fits
        max_out = uoff[last] - uoff[first] + min(inside, len(some[last][2]) - 1)
        n, nxt, got = _inflate(L, h, comp, coff[first], max_out)
        assert n == uoff[last] - uoff[first] and nxt == coff[last], (n, nxt, L.strk_last_error())
        _same(got, raw[uoff[first]:uoff[last]], some[first:last], [u - uoff[first] for u in uoff[first:last]])
    n, nxt, got = _inflate(L, h, comp, coff[first], 0)                                 # nothing fits: nothing is taken
    assert (n, nxt) == (0, coff[first])


def test_file_path_equals_the_buffer_path(dbam, whole, tmp_path):
    L, h = dbam
    some, comp, coff, uoff, raw = whole
    path = str(tmp_path / "corpus.bgzf")
    with open(path, "wb") as fh:
        fh.write(comp)
    ks = [0, 1, len(some) // 3, len(some) - 1]
    voff = np.array([coff[k] << 16 | min(3, max(len(some[k][2]) - 1, 0)) for k in ks] + [(coff[1] + 1) << 16, len(comp) << 16], np.uint64)
    res = []
    for threads in (0, 2):
        nc = C.c_int64(0)
        n = L.strk_dbam_inflate_file(h, os.fsencode(path), threads, C.byref(nc))
        assert n == len(raw) and nc.value == len(comp), (n, L.strk_last_error())
        got = np.empty(len(raw), np.uint8)
        _lib.check(L.strk_dbam_download(h, 0, len(raw), got.ctypes.data))
        _same(got.tobytes(), raw, some, uoff)
        a = np.empty(voff.size, np.int64)
        _lib.check(L.strk_dbam_voffsets(h, voff.ctypes.data, voff.size, a.ctypes.data))
        res.append(a)
    assert _inflate(L, h, comp)[0] == len(raw)
    b = np.empty(voff.size, np.int64)
    _lib.check(L.strk_dbam_voffsets(h, voff.ctypes.data, voff.size, b.ctypes.data))
    assert all(np.array_equal(a, b) for a in res), (res, b)
    assert [int(x) for x in b[:len(ks)]] == [uoff[k] + min(3, max(len(some[k][2]) - 1, 0)) for k in ks] and b[len(ks)] == -1


def test_headers_of_other_writers(dbam, tmp_path):
    """dbam_block_at, through the buffer and through the file: subfields around BC, XLEN above 6, any MTIME / XFL / OS, empty
    blocks in mid-file are accepted; a header without BC, a BSIZE past the file or inside the header and an ISIZE above 65536
    are refused with the block's byte offset."""
    L, h = dbam
    files = ic.header_files()
    path = str(tmp_path / "h.bgzf")

    def from_file(comp):
        with open(path, "wb") as fh:
            fh.write(comp)
        n = L.strk_dbam_inflate_file(h, os.fsencode(path), 1, None)
        got = np.empty(max(int(n), 0), np.uint8)
        if n > 0:
            _lib.check(L.strk_dbam_download(h, 0, int(n), got.ctypes.data))
        return n, got.tobytes()
    for name, (comp, raw) in files["ok"].items():
        n, nxt, got = _inflate(L, h, comp)
        assert n == len(raw) and nxt == len(comp) and got == raw, (name, n, L.strk_last_error())
        assert from_file(comp) == (len(raw), raw), (name, L.strk_last_error())
    for name, (comp, at) in files["bad"].items():
        for walk in (lambda: _inflate(L, h, comp)[0], lambda: from_file(comp)[0]):
            n = walk()
            msg = L.strk_last_error()
            assert n == _lib.STRK_E_INVALID and re.search(rb"BGZF block.* at byte %d\b" % at, msg), (name, n, msg)
    _check_file(L, h, ic.small_good(5))


def _with_bad(good, bad: dict):
    """The good cases with the refusals of `bad` {index: case} put in at their indices."""
    some = list(good)
    for k in sorted(bad):
        some.insert(k, bad[k])
    return some


def _refused(L, h, some, k: int, crc: bool) -> None:
    n, _, _ = _inflate(L, h, ic.bgzf_file(some)[0])
    msg = L.strk_last_error()
    assert n == _lib.STRK_E_INVALID and b"corrupt BGZF block %d of the stretch" % k in msg, (some[k][0], k, n, msg)
    assert (b"CRC mismatch" in msg) == crc and (b"inflate failed" in msg) != crc, (some[k][0], msg)


@pytest.mark.parametrize("name", [c[0] for c in ic.refusals()])
def test_malformed_body_is_refused_under_its_block_index(dbam, name):
    """(each of these bodies has been through tools/inflate_asan.sh: whatever the decoder returns, it stays inside the
    payload + 16 bytes and inside the block's output)"""
    L, h = dbam
    case = next(c for c in ic.refusals() if c[0] == name)
    good = ic.small_good(100)
    crc = ic.corpus()["aim"][name] == ic.E_CRC
    for k in (5, 70):                                                                # the first workgroup, the second
        _refused(L, h, _with_bad(good, {k: case}), k, crc)
        _check_file(L, h, good)


def test_the_lower_of_two_bad_blocks_is_named_with_its_own_error(dbam):
    L, h = dbam
    by_name = {c[0]: c for c in ic.refusals()}
    good = ic.small_good(100)
    crc, other = by_name["refuse/wrong_crc"], by_name["refuse/distance_pos_plus_1"]
    _refused(L, h, _with_bad(good, {7: other, 90: crc}), 7, False)
    _refused(L, h, _with_bad(good, {7: crc, 90: other}), 7, True)
    _refused(L, h, _with_bad(good, {66: other, 67: by_name["refuse/btype_3"]}), 66, False)
    _refused(L, h, _with_bad(good, {63: crc, 64: crc}), 63, True)
    _check_file(L, h, good)
