#!/bin/bash
# The rule of a VCF line, the host walk (as one slice and in slices of three lines) and the closing pass of strk_vcf.h under AddressSanitizer + UBSan on the host (no GPU needed), over the
# corpus of tests/vcf_cases.py and every truncation of its texts.
set -e
D=${TMPDIR:-/tmp}/strk_vcf_snvs_asan
mkdir -p $D
python -c "import sys; sys.path.insert(0, 'tests'); sys.path.insert(0, '.'); import vcf_cases; vcf_cases.dump('$D/corpus')"
g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=undefined -fno-omit-frame-pointer -o $D/vcf_snvs_asan tools/vcf_snvs_asan.cpp
$D/vcf_snvs_asan $D/corpus
