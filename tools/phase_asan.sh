#!/bin/bash
# The input checks of strk_call_alleles and strk_call_alleles_phased and the latter's piece cutting under AddressSanitizer + UBSan on the host (no GPU needed).
set -e
D=${TMPDIR:-/tmp}/strk_phase_asan
mkdir -p $D
g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=undefined -fno-omit-frame-pointer -o $D/phase_asan tools/phase_asan.cpp
$D/phase_asan
