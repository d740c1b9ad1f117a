"""CPU: builds tools/threads_asan.cpp without a sanitizer and runs it (no HIP in strk_threads.h, none in strk_bamrec.h for the
host compiler): the two thread fans cover their items exactly once around their thresholds on 1 to 32 threads, FirstBad keeps
the minimum, the piece loop covers its items in order up to INT32_MAX, check_alt gives every refusal by its message, and the
copy plan of a staged buffer (strk_stage_plan.h, no HIP in it either) covers every byte that goes up exactly once; the
program counts its own failures and exits 0 without one.  tools/threads_asan.sh runs the same program under the sanitizers."""
import os
import shutil
import subprocess

from strkit_amd import _build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_fans_first_bad_pieces_and_alt_check(tmp_path):
    # g++, or the clang++ that stands next to the hipcc the library itself is built with: a machine that can build the package
    # can build this program, so the test never passes over it
    cxx = shutil.which("g++") or shutil.which("c++") or os.path.join(os.path.dirname(os.path.dirname(os.path.realpath(_build._hipcc()))), "llvm", "bin", "clang++")
    assert os.path.exists(cxx), "no host C++ compiler: neither g++ / c++ nor the clang++ of the HIP toolchain"
    exe = tmp_path / "threads_check"
    subprocess.run([cxx, "-O2", "-std=c++17", "-pthread", "-o", str(exe), os.path.join(ROOT, "tools", "threads_asan.cpp")], check=True)
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert " 0 failed" in run.stdout, run.stdout
