#!/bin/bash
# k_replay's walk by events against the walk read by read (strk_search.h: replay_walk_events / replay_walk_serial) on 10^6 random
# loci under AddressSanitizer + UBSan on the host (no GPU needed).
set -e
D=${TMPDIR:-/tmp}/strk_replay_walk_asan
mkdir -p $D
g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=undefined -fno-omit-frame-pointer -o $D/replay_walk_asan tools/replay_walk_asan.cpp
$D/replay_walk_asan "${1:-1000000}"
