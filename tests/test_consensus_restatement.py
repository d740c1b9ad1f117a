"""The CPU restatement of the best-representative rule (tests/consensus_restatement.py): known answers and invariants."""
import numpy as np

import consensus_restatement as R


def _brute(group):
    """The definition word for word: no duplicate collapsing, every ordered pair."""
    g = [R._b(s) for s in group]
    D = [sum(R.lev_plain(a, b) for b in g) for a in g]
    i = min(range(len(g)), key=lambda k: (D[k], k))
    return i, D[i]


def test_known_distances():
    assert R.lev("kitten", "sitting") == 3
    assert R.lev_plain("kitten", "sitting") == 3
    assert R.lev("", "") == 0
    assert R.lev("", "ACGT") == 4 and R.lev("ACGT", "") == 4
    assert R.lev("CAGCAG", "CAGCAG") == 0
    assert R.lev("A", "a") == 1   # case-sensitive
    assert R.lev("flaw", "lawn") == 2
    assert R.lev(b"\x00\xff", b"\xff") == 1


def test_group_rule():
    assert R.best_representative([]) == (-1, "none", 0)
    assert R.best_representative(["CAG"]) == (0, "single", 0)
    assert R.best_representative(["CAG"] * 7) == (0, "single", 0)
    assert R.best_representative(["", ""]) == (0, "single", 0)
    assert R.best_representative(["", "AC"]) == (0, "best_rep", 2)
    # a tie: two strings have the same sum, the first index wins
    assert R.best_representative(["AAAA", "AAAT"]) == (0, "best_rep", 1)
    assert R.best_representative(["AAAT", "AAAA"]) == (0, "best_rep", 1)
    # AAAA, AATT, TTTT: the middle one is the medoid (2 + 2 against 2 + 4)
    assert R.best_representative(["AAAA", "TTTT", "AATT"]) == (2, "best_rep", 4)


def test_duplicates_count_as_often_as_they_occur():
    # without the duplicates AATT is the medoid; three copies of TTTT pull it to TTTT (first copy)
    g = ["AAAA", "AATT", "TTTT", "TTTT", "TTTT"]
    # D(AAAA) = 2 + 12 = 14, D(AATT) = 2 + 6 = 8, D(TTTT) = 4 + 2 = 6
    assert R.best_representative(g) == (2, "best_rep", 6)
    assert _brute(g) == (2, 6)
    # a duplicate of the first string makes the earlier copy the answer
    assert R.best_representative(["ACGT", "ACGA", "ACGT"])[0] == 0


def test_vectorised_row_equals_the_double_loop():
    rng = np.random.default_rng(7)
    for _ in range(400):
        alpha = [b"A", b"AC", b"ACGT", b"ACGTN"][int(rng.integers(0, 4))]
        a = bytes(alpha[int(k)] for k in rng.integers(0, len(alpha), int(rng.integers(0, 40))))
        b = bytes(alpha[int(k)] for k in rng.integers(0, len(alpha), int(rng.integers(0, 40))))
        assert R.lev(a, b) == R.lev_plain(a, b), (a, b)


def test_symmetry_and_triangle_inequality():
    rng = np.random.default_rng(11)
    for _ in range(150):
        s = [bytes(b"ACGT"[int(k)] for k in rng.integers(0, 4, int(rng.integers(0, 60)))) for _ in range(3)]
        ab, ba = R.lev(s[0], s[1]), R.lev(s[1], s[0])
        assert ab == ba
        assert R.lev(s[0], s[2]) <= ab + R.lev(s[1], s[2])
        assert abs(len(s[0]) - len(s[1])) <= ab <= max(len(s[0]), len(s[1]))


def test_group_rule_equals_the_word_for_word_definition():
    rng = np.random.default_rng(13)
    for _ in range(120):
        base = bytes(b"ACGT"[int(k)] for k in rng.integers(0, 4, int(rng.integers(0, 25))))
        g = []
        for _ in range(int(rng.integers(2, 9))):
            s = bytearray(base)
            for _ in range(int(rng.integers(0, 3))):
                if s and rng.random() < 0.5:
                    del s[int(rng.integers(0, len(s)))]
                else:
                    s.insert(int(rng.integers(0, len(s) + 1)), b"ACGT"[int(rng.integers(0, 4))])
            g.append(bytes(s))
        idx, method, dist = R.best_representative(g)
        if method == "single":
            assert all(x == g[0] for x in g) and idx == 0 and dist == 0
        else:
            assert (idx, dist) == _brute(g), g
