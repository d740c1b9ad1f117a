"""The CPU restatement of the k-mer count (tests/kmers_restatement.py): hand-worked answers and invariants."""
import numpy as np

import kmers_restatement as R


def test_cag_tract():
    got = R.count_group(["CAG" * 5], 3)
    assert [(w, c) for w, c, _ in got] == [(b"AGC", 4), (b"CAG", 5), (b"GCA", 4)]
    assert [f for _, _, f in got] == [(0, 1), (0, 0), (0, 2)]
    assert list(R.count_dict(["CAG" * 5], 3)) == [b"AGC", b"CAG", b"GCA"]


def test_window_lengths_around_the_string():
    assert R.count_group(["ACCA"], 1) == [(b"A", 2, (0, 0)), (b"C", 2, (0, 1))]
    assert R.count_group(["ACCA"], 4) == [(b"ACCA", 1, (0, 0))]          # k = len
    assert R.count_group(["ACCA"], 5) == []                               # k > len
    assert R.count_group(["ACCA", "AC"], 3) == [(b"ACC", 1, (0, 0)), (b"CCA", 1, (0, 1))]   # the short string has no window


def test_empty_string_and_empty_group():
    assert R.count_group([], 3) == []
    assert R.count_group([""], 1) == []
    assert R.count_group(["", "A", ""], 1) == [(b"A", 1, (1, 0))]


def test_first_occurrence_is_string_then_offset():
    got = R.count_group(["TTAC", "ACAC", "AC"], 2)
    assert got == [(b"AC", 4, (0, 2)), (b"CA", 1, (1, 1)), (b"TA", 1, (0, 1)), (b"TT", 1, (0, 0))]


def test_duplicate_strings_count_as_often_as_they_occur():
    one = R.count_dict(["CAGCAA"], 3)
    assert R.count_dict(["CAGCAA"] * 3, 3) == {w: 3 * c for w, c in one.items()}


def test_case_sensitive_and_unsigned_order():
    assert [w for w, _, _ in R.count_group(["aAaA"], 1)] == [b"A", b"a"]
    got = R.count_group([b"\xffA\x00\x7f\x80"], 1)
    assert [w for w, _, _ in got] == [b"\x00", b"A", b"\x7f", b"\x80", b"\xff"]      # a byte above 127 sorts last
    assert R.count_group([b"\xff\xff\xff"], 2) == [(b"\xff\xff", 2, (0, 0))]


def test_overlapping_slices_of_one_buffer():
    buf = b"CAGCAGCAA"
    # two groups over the same bytes: slices [0:6] + [3:9] (overlapping), and the whole buffer
    eo, pos, cnt = R.count_packed([0, 2, 3], [0, 3, 0], [6, 6, 9], [3, 3], buf)
    assert eo == [0, 4, 8]
    assert [(buf[p:p + 3], c) for p, c in zip(pos[:4], cnt[:4])] == [(b"AGC", 2), (b"CAA", 1), (b"CAG", 3), (b"GCA", 2)]
    assert pos[:4] == [1, 6, 0, 2]
    assert [(buf[p:p + 3], c) for p, c in zip(pos[4:], cnt[4:])] == [(b"AGC", 2), (b"CAA", 1), (b"CAG", 2), (b"GCA", 2)]


def test_conservation_on_random_groups():
    rng = np.random.default_rng(11)
    for _ in range(200):
        k = int(rng.integers(1, 9))
        group = [bytes(b"ACGT"[int(x)] for x in rng.integers(0, 4, int(rng.integers(0, 40)))) for _ in range(int(rng.integers(0, 6)))]
        got = R.count_group(group, k)
        assert sum(c for _, c, _ in got) == R.n_windows(group, k) == sum(max(len(s) - k + 1, 0) for s in group)
        assert [w for w, _, _ in got] == sorted({w for w, _, _ in got})
        for w, _c, (si, i) in got:
            assert group[si][i:i + k] == w
            assert all(w not in R.windows(s, k) for s in group[:si]) and w not in R.windows(group[si], k)[:i]
