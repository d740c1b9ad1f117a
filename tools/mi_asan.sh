#!/bin/bash
# The per-locus routine of strk_mi.h (special functions, exact Mann-Whitney tail, host_locus) and the input check of strk_mi_check.h under AddressSanitizer + UBSan on the host (no GPU needed).
set -e
D=${TMPDIR:-/tmp}/strk_mi_asan
mkdir -p $D
g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=undefined -fno-omit-frame-pointer -o $D/mi_asan tools/mi_asan.cpp
$D/mi_asan
