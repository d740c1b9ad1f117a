#!/bin/bash
# The inflater under AddressSanitizer + UBSan on the host (no GPU needed): a synthetic BAM, the accepted blocks of the corpus of
# tests/inflate_cases.py (every block type, code shape and copy path) in one file, its refusals (one malformed body per error
# return) in a second.
set -e
D=${TMPDIR:-/tmp}/strk_inflate_asan
mkdir -p $D
g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-omit-frame-pointer -o $D/inflate_asan tools/inflate_asan.cpp -lz
python3 - "$D" <<'PY'
import sys
sys.path[:0] = [".", "tests"]
import inflate_cases as ic
from strkit_amd.frontend.synth_dataset import make_dataset
d = sys.argv[1]
make_dataset(d, n_loci=40, reads_per_locus=12, read_len=4000, seed=21, sub=0.01, indel=0.01)
ic.check_coverage()
open(d + "/accepted.bgzf", "wb").write(ic.bgzf_file(ic.accepted())[0])
open(d + "/refused.bgzf", "wb").write(ic.bgzf_file(ic.refusals())[0])
PY
$D/inflate_asan $D/reads.bam $D/accepted.bgzf
$D/inflate_asan --refuse $D/refused.bgzf
