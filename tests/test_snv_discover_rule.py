"""CPU: the rule of frontend/snv_discovery.py on the hand-made loci of snv_discover_cases.py, with the expected positions written
out there (`want`); its operation-by-operation walk against phase_inputs.alignment_cells cell by cell; and its tie to the
existing rule: where every base is A C G T of good quality, the discovered positions that also pass useful_snvs' second
threshold are the positions useful_snvs selects from cells taken at every window position."""
import numpy as np
import pytest

import snv_discover_cases as cases
from strkit_amd.frontend import phase_inputs as pi
from strkit_amd.frontend import snv_discovery as sd


@pytest.mark.parametrize("window", cases.WINDOWS)
def test_the_rule_gives_the_positions_written_out(window):
    c = cases.corpus()
    off, pos = cases.expected(window)
    assert c["n_loci"] == 37 and max(len(lc["reads"]) for lc in c["loci"]) == 65
    n_checked = 0
    for l, lc in enumerate(c["loci"]):
        got = pos[off[l]:off[l + 1]].tolist()
        assert got == sorted(got), lc["name"]
        if lc["want"] is not None:
            assert got == lc["want"][window], (lc["name"], window)
            n_checked += 1
    assert n_checked == c["n_loci"] - 1        # (all but the substitute alignments, below)


def test_substitute_alignments_are_walked():
    c = cases.corpus()
    l = [lc["name"] for lc in c["loci"]].index("substitute")
    lc = c["loci"][l]
    p = lc["left"] - 300
    plain = sd.discover_candidates(c["entries"][l], [(s, False) for s, _ in c["kept_entries"][l]], lc["left"], lc["right"], 8192, 20, 2)
    assert plain.tolist() == [p]               # four ALT reads at p under the records' own alignments
    off, pos = cases.expected(8192)
    got = pos[off[l]:off[l + 1]].tolist()
    # walked one base to the right, those four reads carry at x the reference base of x - 1: a site wherever the two differ
    ref = cases._REF
    moved = lambda x: cases.alt_base(p) if x == p + 1 else ref[x - 1]  # noqa: E731
    assert got == [x for x in range(lc["left"] - 599, lc["left"] - 100) if moved(x) != ref[x]] and len(got) > 300
    # a realigned read whose alignment the caller does not have counts as a kept read and contributes nothing: n = 14, a_thr = 3
    more = c["kept_entries"][l][4:] + [(c["kept_entries"][l][0][0], True)] * 8
    assert sd.discover_candidates(c["entries"][l], more, lc["left"], lc["right"], 8192, 20, 2).tolist() == []


def test_no_reads_no_gate_no_window():
    c = cases.corpus()
    l = [lc["name"] for lc in c["loci"]].index("near")
    lc, e, k = c["loci"][l], c["entries"][l], c["kept_entries"][l]
    assert sd.discover_candidates(e, [], lc["left"], lc["right"]).size == 0
    assert sd.discover_candidates(e, k, lc["left"], lc["right"], allowed=False).size == 0
    assert sd.discover_candidates(e, k, lc["left"], lc["right"], window=1).tolist() == [lc["left"] - 1, lc["right"]]
    assert sd.discover_candidates(e, k, lc["left"], lc["right"], min_allele_reads=6).size == 0       # 5 / 5 reads
    assert sd.window_positions(3, 10, 5).tolist() == [0, 1, 2, 10, 11, 12, 13, 14]


def test_the_walk_by_operations_gives_alignment_cells():
    c = cases.corpus()
    names = {"ops_63_64_65", "ops_130", "zero_H", "clip_left_100", "clip_right_100", "clip_right_99", "long_cigar", "under_D", "under_N", "after_I",
             "sixteen_codes", "no_qual", "substitute", "cut_at_0"}
    n = 0
    for l, lc in enumerate(c["loci"]):
        if lc["name"] not in names:
            continue
        for entry in c["kept_entries"][l][:6]:
            cigar, start, seg = sd._alignment_of(entry)
            p0, p1 = max(start - 40, 0), seg.end + 40
            want = pi.alignment_cells(cigar, start, seg.query_sequence, seg.query_qualities, np.arange(p0, p1))
            got = sd.window_bytes(cigar, start, seg.query_sequence, seg.query_qualities, p0, p1)
            assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), (lc["name"], seg.name)
            # and a window that cuts the alignment on both sides
            a, b = start + 7, seg.end - 9
            got = sd.window_bytes(cigar, start, seg.query_sequence, seg.query_qualities, a, b)
            assert np.array_equal(got[0], want[0][a - p0:b - p0]) and np.array_equal(got[1], want[1][a - p0:b - p0]), (lc["name"], seg.name)
            n += 1
    assert n >= 60


@pytest.mark.parametrize("name", ["near", "ops_65", "reads_65", "at_threshold", "n_13", "hom_alt", "shared_b", "nearest_1024"])
def test_discovery_and_useful_snvs_ask_the_same_question(name):
    """All bases of these loci are A C G T with quality 30.  Cells are taken with alignment_cells at every window position that a
    read of the locus can reach; useful_snvs picks its first 64; the discovered positions with enough counted cells (t_thr) are the same."""
    c = cases.corpus()
    l = [lc["name"] for lc in c["loci"]].index(name)
    lc, kept = c["loci"][l], c["kept_entries"][l]
    window = 8192
    lo, hi = min(s.start for s, _ in kept), max(s.end for s, _ in kept)
    cols = sd.window_positions(lc["left"], lc["right"], window)
    cols = cols[(cols >= lo) & (cols < hi)]
    cells = np.array([pi.segment_cells(s, cols)[0] for s, _ in kept], np.uint8)
    via_cells = cols[pi.useful_snvs(cells, cases.MIN_ALLELE_READS)]
    found = sd.discover_candidates(c["entries"][l], kept, lc["left"], lc["right"], window, cases.MIN_BASE_QUAL, cases.MIN_ALLELE_READS)
    if name == "nearest_1024":      # (the 1 101 sites themselves, before the nearest-1 024 rule: useful_snvs sees every column)
        assert found.size == pi.MAX_CANDIDATES
        found = np.array(sorted(p for p, b in zip(cols, cells.T) if len(set(b.tolist()) - {ord("-"), ord("_")}) > 1), np.int64)
        assert found.size == 1101
    t_thr = pi.useful_thresholds(len(kept), cases.MIN_ALLELE_READS)[1]
    counted = {int(p): int(((b != ord("-")) & (b != ord("_"))).sum()) for p, b in zip(cols, cells.T)}
    want = [int(p) for p in found if counted[int(p)] >= t_thr][:pi.MAX_USEFUL_SNVS]
    assert via_cells.tolist() == want and len(want) > 0
