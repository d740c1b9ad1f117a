"""CPU: builds tools/phase_inputs_asan.cpp without a sanitizer and runs it (no HIP in strk_phase_inputs.h outside its kernels):
the auxiliary-field walk, the cell walk and the choice of the useful SNVs over random well-formed records against a base-by-base
expansion, every hostile record refused, and the input checkers of strk_phase_cells / strk_useful_snvs over every refusal; the
program counts its own failures and exits 0 without one.  tools/phase_inputs_asan.sh runs the same program under the sanitizers."""
import os
import shutil
import subprocess

import pytest

from strkit_amd.frontend import phase_inputs  # noqa: F401  (the rule the program's header states for the library)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_phase_input_walks_and_checkers_accept_and_refuse_what_they_should(tmp_path):
    if shutil.which("g++") is None:
        pytest.skip("no host C++ compiler")
    exe = tmp_path / "phase_inputs_check"
    subprocess.run(["g++", "-O2", "-std=c++17", "-o", str(exe), os.path.join(ROOT, "tools", "phase_inputs_asan.cpp")], check=True)
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert " 0 failed" in run.stdout, run.stdout
