#!/bin/bash
# The input check, chunks and workspace layout of strk_realign (strk_realign_plan.h) under AddressSanitizer + UBSan on the host (no GPU needed).
set -e
D=${TMPDIR:-/tmp}/strk_realign_asan
mkdir -p $D
g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=undefined -fno-omit-frame-pointer -o $D/realign_asan tools/realign_asan.cpp
$D/realign_asan
