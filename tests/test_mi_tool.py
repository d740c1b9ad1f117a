"""CPU: builds tools/mi_asan.cpp without a sanitizer and runs it (no HIP in strk_mi.h outside its kernels): the special
functions against the C library and closed forms, the exact Mann-Whitney tail against the enumeration of every arrangement,
the per-locus routine behind strk_mi_trio_host on hand and random loci, and the input checker over every refusal; the program
counts its own failures and exits 0 without one.  tools/mi_asan.sh runs the same program under the sanitizers."""
import os
import shutil
import subprocess

from strkit_amd import _build
from strkit_amd import mi  # noqa: F401  (the module whose library routine the program drives)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_mi_routine_and_checker_accept_and_refuse_what_they_should(tmp_path):
    # g++, or the clang++ that stands next to the hipcc the library itself is built with: a machine that can build the package
    # can build this program, so the test never passes over it
    cxx = shutil.which("g++") or shutil.which("c++") or os.path.join(os.path.dirname(os.path.dirname(os.path.realpath(_build._hipcc()))), "llvm", "bin", "clang++")
    assert os.path.exists(cxx), "no host C++ compiler: neither g++ / c++ nor the clang++ of the HIP toolchain"
    exe = tmp_path / "mi_check"
    subprocess.run([cxx, "-O2", "-std=c++17", "-o", str(exe), os.path.join(ROOT, "tools", "mi_asan.cpp")], check=True)
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert " 0 failed" in run.stdout, run.stdout
