"""CPU: the front end of `--count-kmers` (parser, options, exported symbols, argument checks that need no device)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from strkit_amd import _lib
from strkit_amd.__main__ import build_parser
from strkit_amd.frontend.call import CallOptions, call_blocks, call_sample

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BASE = ["call", "reads.bam", "--ref", "ref.fa", "--loci", "loci.bed"]


def test_parser_accepts_count_kmers():
    p = build_parser()
    assert p.parse_args(BASE).count_kmers == "none"
    assert p.parse_args(BASE + ["-k"]).count_kmers == "peak"
    assert p.parse_args(BASE + ["--count-kmers"]).count_kmers == "peak"
    assert p.parse_args(BASE + ["-k", "both"]).count_kmers == "both"
    assert p.parse_args(BASE + ["--count-kmers", "read"]).count_kmers == "read"
    with pytest.raises(SystemExit):
        p.parse_args(BASE + ["-k", "all"])


def test_peak_counts_need_allele_calls():
    assert CallOptions().count_kmers == "none"
    for mode in ("peak", "both"):
        with pytest.raises(ValueError, match="call_alleles"):
            call_blocks([], None, None, CallOptions(count_kmers=mode))
        with pytest.raises(ValueError, match="call_alleles"):
            call_sample("reads.bam", "ref.fa", "loci.bed", count_kmers=mode)


def test_unknown_mode_is_rejected():
    with pytest.raises(ValueError, match="count_kmers"):
        call_blocks([], None, None, CallOptions(count_kmers="all"))
    with pytest.raises(ValueError, match="count_kmers"):
        call_sample("reads.bam", "ref.fa", "loci.bed", count_kmers="all", call_alleles=True)


def test_symbols_are_declared_and_exported():
    src = open(os.path.join(ROOT, "include", "strkit_amd.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    declared = set(re.findall(r"\b(strk_[a-z0-9_]+)\s*\(", src))
    lib = _lib.load()
    for name in ("strk_count_kmers", "strk_count_kmers_dseqs"):
        assert name in declared and name in _lib.EXPORTS
        assert getattr(lib, name) is not None


def test_null_context_is_rejected_without_touching_a_device():
    lib = _lib.load()
    eo = np.zeros(2, np.int64)
    off, start, ln, k = np.array([0, 1], np.int32), np.zeros(1, np.int64), np.array([3], np.int32), np.array([3], np.int32)
    p = lambda a: C.c_void_p(a.ctypes.data)      # noqa: E731
    buf = np.frombuffer(b"CAG", np.uint8)
    for fn in (lib.strk_count_kmers, lib.strk_count_kmers_dseqs):
        assert fn(None, 1, p(off), p(buf), 3, p(start), p(ln), p(k), 0, p(eo), None, None, None) == _lib.STRK_E_INVALID
        assert b"strk_count_kmers" in lib.strk_last_error()
    assert lib.strk_count_kmers_ws(None, 1, p(off), p(buf), None, 3, p(start), p(ln), p(k), 0, p(eo), None, None, 0, None) == _lib.STRK_E_INVALID
