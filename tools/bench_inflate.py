"""Kernel time of k_bgzf_inflate (HIP events: strk_dbam_kernel_ms around strk_dbam_inflate) on a file of the project's own
writer (44 MB in level-1 blocks) and on the corpus of tests/inflate_cases.py (every block type and code shape, eight times over).
STRKIT_AMD_LIB=<another build> compares two states of the decoder on the same bytes.  One JSON line."""
import ctypes as C
import json
import os
import sys

import numpy as np

sys.path[:0] = [os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."), os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests")]
import inflate_cases as ic  # noqa: E402
from strkit_amd import _lib  # noqa: E402
from strkit_amd.frontend.bam import _bgzf_blocks  # noqa: E402


def main() -> None:
    rng = np.random.default_rng(5)
    raw = rng.integers(0, 24, size=44_000_000, dtype=np.uint8)
    raw[1_000_000:3_000_000] = 7
    files = {"writer_44MB": _bgzf_blocks(raw.tobytes()), "corpus_x8": ic.bgzf_file(ic.shuffled(ic.accepted()) * 8)[0]}
    L = _lib.load()
    h = C.c_void_p()
    _lib.check(L.strk_dbam_open(0, C.byref(h)))
    res = {"lib": os.environ.get("STRKIT_AMD_LIB", "tree")}
    for name, comp in files.items():
        arr = np.frombuffer(comp, np.uint8)
        nxt = C.c_int64(0)
        ms = []
        for _ in range(8):
            t0 = L.strk_dbam_kernel_ms(h)
            n = L.strk_dbam_inflate(h, arr.ctypes.data, arr.size, 0, 1 << 40, C.byref(nxt))
            assert n > 0, L.strk_last_error()
            ms.append(round(L.strk_dbam_kernel_ms(h) - t0, 4))
        res[name] = {"bytes_in": int(arr.size), "bytes_out": int(n), "kernel_ms": ms, "median_ms_after_two": float(np.median(ms[2:]))}
    L.strk_dbam_close(h)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
