"""CPU: the readable rule of methylation from MM / ML tags (frontend/methyl.py) against a second, brute-force
statement (tests/methyl_restatement.py) on a seeded corpus, and on hand vectors with written expectations."""
import struct

import numpy as np
import pytest

import methyl_cases as cases
import methyl_restatement as rs
from strkit_amd import _lib
from strkit_amd.frontend import methyl as me
from strkit_amd.frontend.synth_methyl import mm_tags

OK, NOT_SPANNING, NO_TAGS, CLIPPED, MALFORMED, NO_SITES = range(6)


def test_status_constants_are_the_library_s():
    assert (_lib.STRK_METHYL_OK, _lib.STRK_METHYL_NOT_SPANNING, _lib.STRK_METHYL_NO_TAGS, _lib.STRK_METHYL_CLIPPED,
            _lib.STRK_METHYL_MALFORMED, _lib.STRK_METHYL_NO_SITES) == (OK, NOT_SPANNING, NO_TAGS, CLIPPED, MALFORMED, NO_SITES)
    assert (rs.OK, rs.NOT_SPANNING, rs.NO_TAGS, rs.CLIPPED, rs.MALFORMED, rs.NO_SITES) == tuple(range(6))


def test_the_two_statements_agree_on_the_corpus():
    corpus = cases.rule_corpus()
    n_status = np.zeros(6, np.int64)
    lengths, strands = set(), set()
    for seq, flag, cig, tags, q_l, q_r in corpus:
        a = me.read_methylation(seq, flag, cig, tags, q_l, q_r, 127)
        b = rs.brute(seq, flag, cig, tags, q_l, q_r, 127)
        assert a == b, (seq, flag, tags, q_l, q_r, a, b)
        n_status[a[0]] += 1
        lengths.add(len(seq))
        strands.add(flag & 16)
    assert lengths == set(cases.RULE_LENGTHS) and strands == {0, 16}
    assert n_status.min() > 0, n_status                       # every status occurs
    assert n_status[OK] >= len(corpus) / 4, n_status          # (it cannot pass on refusals alone)


def test_other_thresholds_agree_too():
    for seq, flag, cig, tags, q_l, q_r in cases.rule_corpus()[:600]:
        for thr in (0, 128, 254, 255):
            assert me.read_methylation(seq, flag, cig, tags, q_l, q_r, thr) == rs.brute(seq, flag, cig, tags, q_l, q_r, thr)


def _m(seq, tags, q_l=0, q_r=None, flag=0, cigar=None, threshold=127):
    cig = cases.cigar_array(cigar or [(len(seq), "M")])
    got = me.read_methylation(seq, flag, cig, tags, q_l, len(seq) if q_r is None else q_r, threshold)
    assert got == rs.brute(seq, flag, cig, tags, q_l, len(seq) if q_r is None else q_r, threshold)
    return got


def test_hand_vectors_forward_and_reverse():
    # CGCG: sites at 0 and 2.  Forward, the first C (ordinal 0) is called: the other is known with probability 0
    assert _m("CGCG", mm_tags([("C+m", [0], [200])])) == (OK, 2, 2, 1)
    # reverse: the targets are the Gs from the end (3, then 1); ordinal 0 is the G at 3 = the site at 2
    assert _m("CGCG", mm_tags([("C+m", [0], [200])]), flag=16) == (OK, 2, 2, 1)
    assert _m("CGCG", mm_tags([("C+m", [0], [200])]), flag=16, q_r=2) == (OK, 1, 1, 0)     # only the site at 0: its G (1) is ordinal 1
    assert _m("CGCG", mm_tags([("C+m", [1], [200])]), flag=16, q_r=2) == (OK, 1, 1, 1)
    assert _m("CGCG", mm_tags([("C+m", [0], [200])]), q_l=1) == (OK, 1, 1, 0)               # forward, only the site at 2 (ordinal 1)


def test_hand_vectors_modes():
    seq = "ACGTCGTCG"                                           # Cs at 1, 4, 7: three sites
    assert _m(seq, mm_tags([("C+m?", [1], [255])])) == (OK, 3, 1, 1)     # '?': the uncalled sites are unknown
    assert _m(seq, mm_tags([("C+m.", [1], [255])])) == (OK, 3, 3, 1)     # '.': known, probability 0
    assert _m(seq, mm_tags([("C+m", [1], [255])])) == (OK, 3, 3, 1)      # no mode is '.'
    assert _m(seq, mm_tags([("C+m?", [], [])])) == (NO_SITES, 3, 0, 0)
    assert _m(seq, mm_tags([("C+m", [], [])])) == (OK, 3, 3, 0)
    assert _m("ACATTA", mm_tags([("C+m", [0], [255])])) == (NO_SITES, 0, 0, 0)


def test_hand_vectors_strides_and_offsets():
    seq = "CGACGACG"
    # C+mh / C+hm: two ML bytes per number, m first / second
    assert _m(seq, mm_tags([("C+mh", [0, 0, 0], [200, 1, 2, 201, 202, 3])])) == (OK, 3, 3, 2)
    assert _m(seq, mm_tags([("C+hm", [0, 0, 0], [200, 1, 2, 201, 202, 3])])) == (OK, 3, 3, 1)
    # an entry in front moves `off`: A+a owns two bytes
    assert _m(seq, mm_tags([("A+a", [0, 0], [250, 250]), ("C+m", [0, 0, 0], [1, 2, 250])])) == (OK, 3, 3, 1)
    assert _m(seq, mm_tags([("G-m", [0], [250]), ("C+h", [0], [250]), ("C+12345", [1], [250]), ("C+m", [2], [250])])) == (OK, 3, 3, 1)
    # entries that are not taken: C+h alone, G-m, a ChEBI code
    assert _m(seq, mm_tags([("C+h", [0], [250]), ("G-m", [0], [250]), ("C+27551", [0], [250])])) == (NO_TAGS, 0, 0, 0)
    # only the first C+m entry is taken
    assert _m(seq, mm_tags([("C+m", [0], [0]), ("C+m", [0], [255])])) == (OK, 3, 3, 0)


def test_hand_vectors_edges():
    # a G at q_r belongs to the last site; a C at l_seq - 1 is no site
    assert _m("ACGA", mm_tags([("C+m", [0], [255])]), q_l=0, q_r=2) == (OK, 1, 1, 1)
    assert _m("ACGA", mm_tags([("C+m", [0], [255])]), q_l=0, q_r=1) == (NO_SITES, 0, 0, 0)
    assert _m("AGAC", mm_tags([("C+m", [0], [255])])) == (NO_SITES, 0, 0, 0)
    # probabilities 127 and 128 around the default threshold
    assert _m("CGCG", mm_tags([("C+m", [0, 0], [127, 128])])) == (OK, 2, 2, 1)
    assert _m("CGCG", mm_tags([("C+m", [0, 0], [127, 128])]), threshold=126) == (OK, 2, 2, 2)
    assert _m("CGCG", mm_tags([("C+m", [0, 0], [127, 128])]), threshold=128) == (OK, 2, 2, 0)
    # a missing final ';', an empty string
    assert _m("CGCG", mm_tags([("C+m", [0, 0], [200, 200])], final_semicolon=False)) == (OK, 2, 2, 2)
    assert _m("CGCG", b"MMZ\0MLBC" + struct.pack("<I", 0)) == (NO_TAGS, 0, 0, 0)
    # only the codes 2 and 4 are targets: S (C or G) is neither
    assert _m("SGCG", mm_tags([("C+m", [0], [200])])) == (OK, 1, 1, 1)


def _raw(text: bytes, ml: bytes, sub: bytes = b"C") -> bytes:
    return b"MMZ" + text + b"\0MLB" + sub + struct.pack("<I", len(ml)) + ml


@pytest.mark.parametrize("text,ml", [
    (b"C+m,x;", b"\1"), (b"C+m,12345678901;", b"\1"), (b"C+m,2147483648;", b"\1"), (b"C+m,;", b""), (b"C+m,1,;", b"\1"), (b"C+m,-1;", b"\1"),
    (b"C+m;;", b""), (b";", b""), (b"C+M,0;", b"\1"), (b"X+m,0;", b"\1"), (b"C*m,0;", b"\1"), (b"C+;", b""), (b"C+m.?,0;", b"\1"),
    (b"C+m1,0;", b"\1"), (b"C+m, 0;", b"\1"), (b"C", b""), (b"C+m,0;A", b"\1"),
])
def test_every_malformed_string(text, ml):
    assert _m("CGCG", _raw(text, ml)) == (MALFORMED, 0, 0, 0)


def test_malformed_ml_and_skips():
    assert _m("CGCG", _raw(b"C+m,0,0;", b"\1")) == (MALFORMED, 0, 0, 0)                       # a short ML
    assert _m("CGCG", _raw(b"C+m,0;", b"\1\2")) == (MALFORMED, 0, 0, 0)                       # a long one
    assert _m("CGCG", _raw(b"C+m,0;", b"\1", b"c")) == (MALFORMED, 0, 0, 0)                   # ML:B,c
    assert _m("CGCG", _raw(b"C+m,2;", b"\1")) == (MALFORMED, 0, 0, 0)                         # a skip past the last target
    assert _m("CGCG", _raw(b"C+m,1;", b"\1")) == (OK, 2, 2, 0)
    assert _m("CGCG", _raw(b"C+m,2147483647;", b"\1")) == (MALFORMED, 0, 0, 0)                # of the grammar, but past the bases
    assert _m("CGCG", _raw(b"A+a,5,5;C+m,0;", b"\1\1\xff")) == (OK, 2, 2, 1)                  # only the taken entry is checked against the bases
    assert _m("CGCG", b"MMZC+m,0;\0") == (MALFORMED, 0, 0, 0)                                 # MM without ML: ML has no bytes
    assert _m("CGCG", b"MMZC+m;\0") == (OK, 2, 2, 0)
    assert _m("CGCG", b"MLBC" + struct.pack("<I", 1) + b"\1") == (NO_TAGS, 0, 0, 0)           # ML without MM


def test_hard_clips_and_mn():
    tags = mm_tags([("C+m", [0], [200])])
    assert _m("CGCG", tags, cigar=[(3, "H"), (4, "M")]) == (CLIPPED, 0, 0, 0)
    assert _m("CGCG", tags, cigar=[(4, "M"), (3, "H")]) == (CLIPPED, 0, 0, 0)
    assert _m("CGCG", tags, cigar=[(2, "S"), (2, "M")]) == (OK, 2, 2, 1)
    assert _m("CGCG", tags + cases.int_tag(b"MN", "i", 4)) == (OK, 2, 2, 1)
    assert _m("CGCG", tags + cases.int_tag(b"MN", "C", 5)) == (CLIPPED, 0, 0, 0)
    assert _m("CGCG", cases.int_tag(b"MN", "s", 9) + tags) == (CLIPPED, 0, 0, 0)
    assert _m("CGCG", tags + b"MNZ9\0") == (OK, 2, 2, 1)                                      # an MN that is no integer
    assert _m("CGCG", cases.int_tag(b"MN", "i", 9)) == (NO_TAGS, 0, 0, 0)                     # no MM: nothing to refuse


def test_lower_case_tags_and_first_occurrence():
    low = mm_tags([("C+m", [0], [200])], lower=True)
    assert _m("CGCG", low) == (OK, 2, 2, 1)
    # a record that has MM or ML does not use Mm / Ml
    assert _m("CGCG", low + b"MLBC" + struct.pack("<I", 0)) == (NO_TAGS, 0, 0, 0)
    assert _m("CGCG", mm_tags([("C+m", [1], [0])]) + low) == (OK, 2, 2, 0)
    # the first MM and the first ML
    assert _m("CGCG", mm_tags([("C+m", [0], [200])]) + mm_tags([("C+m", [1], [0])])) == (OK, 2, 2, 1)
    # behind and in front of Z and B fields
    assert _m("CGCG", b"RGZgrp\0" + b"ZBBs" + struct.pack("<Ihh", 2, 1, 2) + mm_tags([("C+m", [0], [200])]) + b"XXZy\0") == (OK, 2, 2, 1)


def test_not_spanning_and_broken_chains():
    tags = mm_tags([("C+m", [0], [200])])
    cig = cases.cigar_array([(4, "M")])
    assert me.read_methylation("CGCG", 0, cig, tags, None, None) == (NOT_SPANNING, 0, 0, 0)
    for bad in (tags[:-1], b"MMZC+m", b"XY", b"MLBC" + struct.pack("<I", 9) + b"\1", b"MLBx" + struct.pack("<I", 0), b"XXq1"):
        with pytest.raises(ValueError):
            me.read_methylation("CGCG", 0, cig, bad, 0, 4)
        with pytest.raises(ValueError):
            rs.brute("CGCG", 0, cig, bad, 0, 4)
        with pytest.raises(ValueError):                      # a broken chain comes before everything else
            me.read_methylation("CGCG", 0, cig, bad, None, None)


def test_parse_mm():
    assert me.parse_mm(b"") == []
    got = me.parse_mm(b"C+mh?,1,22;N-12345.;A+a")
    assert got == [{"base": "C", "strand": "+", "codes": ["m", "h"], "mode": "?", "skips": [1, 22]},
                   {"base": "N", "strand": "-", "codes": ["12345"], "mode": ".", "skips": []},
                   {"base": "A", "strand": "+", "codes": ["a"], "mode": "", "skips": []}]
    assert me.parse_mm(b"C+m,0000000009")[0]["skips"] == [9]
    with pytest.raises(me.MalformedMM):
        me.parse_mm(b"C+m,00000000009")


def test_allele_means():
    assert me.allele_means([0, 1, 0, 1], [0.5, 1.0, None, 0.0], [2, 4, None, 0], 2) == ([0.5, 0.5], [2.0, 2.0])
    assert me.allele_means([0, 0, 1], [0.5, 0.25, None], [1, 1, None], 2) is None            # a peak without a value
    assert me.allele_means([0, None, 1], [0.1, 0.9, 0.3], [1, 9, 3], 2) == ([0.1, 0.3], [1.0, 3.0])                    # a read without a peak counts nowhere
    am, amc = me.allele_means([0, 0, 0], [0.1, 0.2, 0.3], [1, 2, 4], 1)
    assert am == [(0.1 + 0.2 + 0.3) / 3] and amc == [7 / 3]                                   # one rounding per addition, in read order
    assert me.allele_means([], [], [], 0) is None
