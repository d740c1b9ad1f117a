"""CPU: builds tools/methyl_asan.cpp without a sanitizer and runs it (no HIP in strk_methyl.h outside its kernel): the
auxiliary-chain finder, the MM scans, the target masks and the site test over random well-formed records against a base-by-base
walk of the read as sequenced, every hostile record refused, random MM strings, and the input checker over every refusal; the
program counts its own failures and exits 0 without one.  tools/methyl_asan.sh runs the same program under the sanitizers."""
import os
import shutil
import subprocess

import pytest

from strkit_amd.frontend import methyl  # noqa: F401  (the rule the program's header states for the library)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_methyl_walks_and_checker_accept_and_refuse_what_they_should(tmp_path):
    if shutil.which("g++") is None:
        pytest.skip("no host C++ compiler")
    exe = tmp_path / "methyl_check"
    subprocess.run(["g++", "-O2", "-std=c++17", "-o", str(exe), os.path.join(ROOT, "tools", "methyl_asan.cpp")], check=True)
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert " 0 failed" in run.stdout, run.stdout
