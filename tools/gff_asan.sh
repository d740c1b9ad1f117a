#!/bin/bash
# The rule of a GFF3 / GTF line, the id of a feature, the host walk with its join and the closing pass of strk_gff.h under
# AddressSanitizer + UBSan on the host (no GPU needed), over the corpus of tests/annot_cases.py and truncations of its texts.
set -e
D=${TMPDIR:-/tmp}/strk_gff_asan
mkdir -p $D
python -c "import sys; sys.path.insert(0, 'tests'); sys.path.insert(0, '.'); import annot_cases; annot_cases.dump('$D/corpus')"
g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=undefined -fno-omit-frame-pointer -o $D/gff_asan tools/gff_asan.cpp
$D/gff_asan $D/corpus
