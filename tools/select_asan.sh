#!/bin/bash
# The input check, the record pre-pass and the host rule of strk_select.h (read selection) under AddressSanitizer + UBSan on the host (no GPU needed).
set -e
D=${TMPDIR:-/tmp}/strk_select_asan
mkdir -p $D
g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=undefined -fno-omit-frame-pointer -o $D/select_asan tools/select_asan.cpp
$D/select_asan
