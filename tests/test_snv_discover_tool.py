"""CPU: builds tools/snv_discover_asan.cpp without a sanitizer and runs it (no HIP in strk_snv_discover.h outside its kernels):
the host twin of the pileup over random well-formed records against a base-by-base pileup, the window and tile geometry, the
nearest-1 024 rule, every hostile record refused, and the input checker over every refusal; the program counts its own failures
and exits 0 without one.  The same program runs under the sanitizers with g++ -fsanitize=address,undefined."""
import os
import shutil
import subprocess

import pytest

from strkit_amd.frontend import snv_discovery  # noqa: F401  (the rule the program's header states for the library)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_discovery_walks_and_checker_accept_and_refuse_what_they_should(tmp_path):
    if shutil.which("g++") is None:
        pytest.skip("no host C++ compiler")
    exe = tmp_path / "snv_discover_check"
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-o", str(exe), os.path.join(ROOT, "tools", "snv_discover_asan.cpp")], check=True)
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert " 0 failed" in run.stdout, run.stdout
