#!/bin/bash
# k_plan's counting sort (strk_plan_order.h) on 10^6 random key sets under AddressSanitizer + UBSan on the host (no GPU needed).
set -e
D=${TMPDIR:-/tmp}/strk_plan_order_asan
mkdir -p $D
g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=undefined -fno-omit-frame-pointer -o $D/plan_order_asan tools/plan_order_asan.cpp
$D/plan_order_asan "${1:-1000000}"
