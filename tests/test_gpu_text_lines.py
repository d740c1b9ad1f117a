"""GPU: strk_dbam_text_lines (k_lines_count / k_lines_scan / k_lines_starts, the line split both text readers begin with) against
line starts found in Python with bytes.find over the same bytes: exactly equal, for both tile sizes, as a piece and as the text
that ends its file, at every seam of the passes (word, step, tile, the start offset, the end of the text)."""
import ctypes as C
import os

import numpy as np
import pytest

from strkit_amd import _lib
from strkit_amd.frontend.synth_snvs import write_bgzf_vcf

pytestmark = pytest.mark.gpu

TILES = (256, 1024)


def _text(n: int, newlines) -> bytes:
    t = bytearray(b"x" * n)
    for p in newlines:
        t[p] = 10
    return bytes(t)


SEAMS = _text(1101, (0, 3, 255, 256, 257, 1023, 1024, 1100))
STARTS_TEXT = _text(600, (0, 1, 2, 3, 254, 255, 256, 257, 598, 599))      # a '\n' at start - 1 and at start, for every start below
STARTS = (0, 1, 3, 255, 256, 257, 599, 600)
TEXTS = {
    "seams": SEAMS,
    "seams_no_last_newline": SEAMS[:-1],
    "none_5": _text(5, ()), "none_256": _text(256, ()), "none_257": _text(257, ()),
    "run_of_300": b"x" * 900 + b"\n" * 300 + b"xy",                        # 176 hits in the step from 1024 on; crosses a step and a tile
    **{f"short_{n}": _text(n, range(0, n, 2)) for n in (1, 2, 3, 5, 1021)},   # the last aligned word reaches past n
    "every_37_of_70000": _text(70000, range(36, 70000, 37)),               # 274 tiles of 256: k_lines_scan sums more than one count per thread
    "starts": STARTS_TEXT,
}


def expected(text: bytes, start: int, final: int):
    """(n_lines, starts, end_off) by the rule of strk_lines.h, with bytes.find."""
    starts, p = [start], start
    while (q := text.find(b"\n", p)) >= 0:
        p = q + 1
        starts.append(p)
    n_nl = len(starts) - 1
    n_lines = n_nl + (1 if final and starts[-1] < len(text) else 0)
    return n_lines, starts, (len(text) if n_lines > n_nl else starts[-1])


@pytest.fixture(scope="module")
def dbam():
    L = _lib.load()
    h = C.c_void_p()
    _lib.check(L.strk_dbam_open(0, C.byref(h)))
    yield h
    L.strk_dbam_close(h)


@pytest.fixture(scope="module")
def text_dir(tmp_path_factory):
    return str(tmp_path_factory.mktemp("text_lines"))


def _load(L, dbam, name: str, text_dir: str) -> bytes:
    path = os.path.join(text_dir, name + ".gz")
    if not os.path.exists(path):
        write_bgzf_vcf(path, TEXTS[name])
    n = L.strk_dbam_inflate_file(dbam, os.fsencode(path), 0, None)
    assert n == len(TEXTS[name]), (L.strk_last_error(), n)
    return TEXTS[name]


def _lines(L, dbam, start: int, final: int, tile: int, cap: int):
    """-> (return value, the cap starts with a guard word behind them, end_off, n_starts)"""
    starts = np.full(cap + 1, -7, np.int64)
    end_off, n_starts = C.c_int64(-7), C.c_int64(-7)
    k = L.strk_dbam_text_lines(dbam, start, final, tile, cap, starts.ctypes.data, C.byref(end_off), C.byref(n_starts))
    return int(k), starts.tolist(), int(end_off.value), int(n_starts.value)


@pytest.mark.parametrize("name", [n for n in TEXTS if n != "starts"])
def test_line_starts_equal_bytes_find(dbam, text_dir, name):
    L = _lib.load()
    text = _load(L, dbam, name, text_dir)
    for tile in TILES:
        for final in (0, 1):
            want_lines, want_starts, want_end = expected(text, 0, final)
            k, starts, end_off, n_starts = _lines(L, dbam, 0, final, tile, len(text) + 1)
            print(name, tile, final, "lines", k, "starts", n_starts, "end_off", end_off)
            assert k >= 0, L.strk_last_error()
            assert (k, n_starts, end_off) == (want_lines, len(want_starts), want_end), (name, tile, final)
            assert starts[:n_starts] == want_starts and set(starts[n_starts:]) == {-7}, (name, tile, final)


def test_every_start_offset(dbam, text_dir):
    """A '\\n' at start - 1 must not count, one at start must; start == n: nothing to read."""
    L = _lib.load()
    text = _load(L, dbam, "starts", text_dir)
    assert STARTS[-1] == len(text) and all(text[s - 1] == 10 for s in STARTS if s) and all(text[s] == 10 for s in STARTS[:-1])
    for tile in TILES:
        for final in (0, 1):
            for start in STARTS:
                want_lines, want_starts, want_end = expected(text, start, final)
                k, starts, end_off, n_starts = _lines(L, dbam, start, final, tile, len(text) + 1)
                assert k >= 0, L.strk_last_error()
                assert (k, n_starts, end_off) == (want_lines, len(want_starts), want_end), (tile, final, start)
                assert starts[:n_starts] == want_starts and set(starts[n_starts:]) == {-7}, (tile, final, start)
    assert _lines(L, dbam, len(text), 1, 0, 4)[::2] == (0, len(text))


def test_capacity_bounds_what_is_written(dbam, text_dir):
    L = _lib.load()
    text = _load(L, dbam, "seams", text_dir)
    want_lines, want_starts, want_end = expected(text, 0, 1)
    for cap in (0, 2, len(want_starts)):
        k, starts, end_off, n_starts = _lines(L, dbam, 0, 1, 0, cap)
        assert (k, n_starts, end_off) == (want_lines, len(want_starts), want_end)
        assert starts[:cap] == want_starts[:cap] and starts[cap] == -7


def test_refusals_come_before_any_launch(dbam, text_dir):
    L = _lib.load()
    n = len(_load(L, dbam, "seams", text_dir))
    ms = L.strk_dbam_kernel_ms(dbam)
    assert _lines(L, dbam, 0, 1, 100, 4)[0] == _lib.STRK_E_INVALID and b"tile_bytes" in L.strk_last_error()
    for start in (-1, n + 1):
        assert _lines(L, dbam, start, 1, 0, 4)[0] == _lib.STRK_E_INVALID and b"outside the text" in L.strk_last_error()
    k, starts, end_off, n_starts = _lines(L, dbam, n, 1, 0, 4)
    assert (k, end_off, n_starts, starts[0]) == (0, n, 1, n)
    assert L.strk_dbam_kernel_ms(dbam) == ms      # nothing was launched
