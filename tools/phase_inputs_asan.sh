#!/bin/bash
# The walks and input checks of strk_phase_inputs.h (tags, SNV cells, useful SNVs) under AddressSanitizer + UBSan on the host (no GPU needed).
set -e
D=${TMPDIR:-/tmp}/strk_phase_inputs_asan
mkdir -p $D
g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=undefined -fno-omit-frame-pointer -o $D/phase_inputs_asan tools/phase_inputs_asan.cpp
$D/phase_inputs_asan
