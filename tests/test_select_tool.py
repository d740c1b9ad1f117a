"""CPU: builds tools/select_asan.cpp without a sanitizer and runs it (no HIP in strk_select.h outside its kernels): the host
rule over a seeded corpus against a map-and-loop statement of it, and the input checker and the record pre-pass over hostile and
truncated streams; the program counts its own failures and exits 0 without one.  tools/select_asan.sh runs the same program
under the sanitizers."""
import os
import shutil
import subprocess

import pytest

from strkit_amd.frontend import select  # noqa: F401  (the rule the program's header states for the library)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_select_rule_and_checker_accept_and_refuse_what_they_should(tmp_path):
    if shutil.which("g++") is None:
        pytest.skip("no host C++ compiler")
    exe = tmp_path / "select_check"
    subprocess.run(["g++", "-O2", "-std=c++17", "-o", str(exe), os.path.join(ROOT, "tools", "select_asan.cpp")], check=True)
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert " 0 failed" in run.stdout, run.stdout
