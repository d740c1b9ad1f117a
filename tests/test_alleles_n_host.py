"""CPU: the C surface of strk_call_alleles_n without a device: the declaration, the export, refusals that need no context,
and the host-only input check (strk_alleles_check.h with a limit of six alleles) under its own driver."""
import os
import re
import shutil
import subprocess

import pytest

from strkit_amd import _lib, alleles

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_entry_point_is_declared_exported_and_refuses_a_null_context():
    src = open(os.path.join(ROOT, "include", "strkit_amd.h")).read()
    assert re.search(r"\bstrk_call_alleles_n\s*\(", src) and re.search(r"#define\s+STRK_MAX_ALLELES\s+6\b", src)
    assert "strk_call_alleles_n" in _lib.EXPORTS and alleles.MAX_ALLELES == 6
    lib = _lib.load()
    assert lib.strk_call_alleles_n.argtypes == lib.strk_call_alleles.argtypes
    rc = lib.strk_call_alleles_n(None, 0, *([None] * 5), None, *([None] * 10), None)
    assert rc == _lib.STRK_E_INVALID and b"strk_call_alleles_n" in lib.strk_last_error()
    # the two-allele entry point keeps its own words for a count that is not 1 or 2
    old = open(os.path.join(ROOT, "strkit_amd", "csrc", "strk_alleles_check.h")).read()
    assert "n_alleles %d is not 1 or 2" in old


def test_the_input_check_accepts_and_refuses_what_it_should(tmp_path):
    """Host build of tools/alleles_n_asan.cpp under AddressSanitizer and UBSan (a program of its own: nothing is preloaded):
    random valid calls, every refusal by its message, arrays of exactly their length."""
    if shutil.which("g++") is None:
        pytest.skip("no host C++ compiler")
    exe = tmp_path / "alleles_n_check"
    src = os.path.join(ROOT, "tools", "alleles_n_asan.cpp")
    san = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", str(exe), src],
                         capture_output=True, text=True)
    if san.returncode != 0:      # a compiler without the sanitizers' runtimes: the plain build still checks every message
        subprocess.run(["g++", "-O2", "-std=c++17", "-o", str(exe), src], check=True)
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert " 0 failed" in run.stdout, run.stdout
