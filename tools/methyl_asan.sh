#!/bin/bash
# The walks and the input check of strk_methyl.h (auxiliary chain, MM entries and numbers, targets, sites) under AddressSanitizer + UBSan on the host (no GPU needed).
set -e
D=${TMPDIR:-/tmp}/strk_methyl_asan
mkdir -p $D
g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=undefined -fno-omit-frame-pointer -o $D/methyl_asan tools/methyl_asan.cpp
$D/methyl_asan
