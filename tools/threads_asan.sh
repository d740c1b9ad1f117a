#!/bin/bash
# The thread fans, FirstBad and the piece loop of strk_threads.h check_alt of strk_bamrec.h and the copy plan of strk_stage_plan.h on the host (no GPU needed): once under AddressSanitizer + UBSan, once under ThreadSanitizer.
set -e
D=${TMPDIR:-/tmp}/strk_threads_asan
mkdir -p $D
g++ -O1 -g -std=c++17 -pthread -fsanitize=address,undefined -fno-sanitize-recover=undefined -fno-omit-frame-pointer -o $D/threads_asan tools/threads_asan.cpp
$D/threads_asan
g++ -O1 -g -std=c++17 -pthread -fsanitize=thread -fno-omit-frame-pointer -o $D/threads_tsan tools/threads_asan.cpp
$D/threads_tsan
