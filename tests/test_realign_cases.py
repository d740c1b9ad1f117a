"""The realignment corpus (tests/realign_cases.py) proves, from the oracle alone, that each cell holds what it is named for:
a change to a generator that empties a cell fails here, without a device.  These are conditions on the corpus; where a
generated case misses one, the generator is what changes."""
import itertools
import time

import numpy as np
import pytest

import oracle
import realign_cases as rc
from helpers import cigar_tuples, rand_seq, rescore_cigar


def runs(cig):
    """(op, length, first window index, first read position) of every run of a CIGAR given as (length, op) tuples."""
    out, i, j = [], 0, 0
    for n, op in cig:
        out.append((op, n, i, j))
        i += n if op in "=XI" else 0
        j += n if op in "=XD" else 0
    return out


def encode_cigar(cig):
    return [(n << 4) | "MIDNSHP=X".index(op) for n, op in cig]


def expand(cig):
    """One letter per alignment column ('X' as '='), so that a moved gap merges with what it lands next to."""
    return "".join(("=" if op == "X" else op) * n for n, op in cig)


def compress(s):
    return [(len(list(g)), op) for op, g in itertools.groupby(s)]


def gap_runs(s):
    """[a, b) of every gap run of an expanded CIGAR but the free leading D run."""
    out, a = [], len(s) - len(s.lstrip("D"))
    while a < len(s):
        b = a + 1
        if s[a] in "ID":
            while b < len(s) and s[b] == s[a]:
                b += 1
            out.append((a, b))
        a = b
    return out


def scores_as(c, s, score):
    """An expanded CIGAR aligns the whole window inside the read and re-scores to `score`."""
    try:
        got = rescore_cigar(c.ref, c.read, encode_cigar(compress(s)), c.open, c.ext)
    except IndexError:
        return False
    return got[0] == score and got[1] == len(c.ref) and got[2] <= len(c.read)


def check_consistent(c, exp):
    sc, e2, cig, words = exp
    assert rescore_cigar(c.ref, c.read, words, c.open, c.ext) == (sc, len(c.ref), e2 + 1), c.name
    assert 0 <= e2 < len(c.read), c.name


@pytest.mark.parametrize("cell", rc.CELLS)
def test_oracle_cigars_rescore_to_the_oracle_scores(cell, capsys):
    t = time.perf_counter()
    exp = rc.expected(cell)
    wall = time.perf_counter() - t
    cases = rc.cases(cell)
    assert len(cases) == len(exp) > 0
    assert len({c.name for c in cases}) == len(cases)
    for c, e in zip(cases, exp):
        check_consistent(c, e)
    with capsys.disabled():
        print(f"\n[realign corpus] {cell}: {len(cases)} cases, {sum(len(c.ref) * len(c.read) for c in cases):.3g} cells, oracle {wall:.1f} s")


def test_grid_is_the_full_product_and_holds_every_class_and_tile_count():
    cases = rc.cases("grid")
    shapes = {(len(c.ref), len(c.read)) for c in cases if (c.open, c.ext, c.gap_pref) == (7, 0, 0)}
    assert shapes == {(a, b) for a in rc.GRID_N1 for b in rc.GRID_N2}
    for pars in ((7, 1, 1), (5, 5, 0)):
        assert {(len(c.ref), len(c.read)) for c in cases if (c.open, c.ext, c.gap_pref) == pars} == \
            {(a, b) for a in rc.GRID_OPENS_A_CLASS for b in rc.GRID_N2}
    geo = {rc.geometry(n1) for n1 in rc.GRID_N1}
    # what the planner can make up to three tiles: the narrow classes never tile (their windows end where the next begins)
    assert {(cl, nt) for cl, nt, _ in geo} == {(4, 1), (8, 1), (16, 1), (32, 1), (32, 2), (32, 3)}
    assert {nt for _, nt, pad in geo if pad == 0} >= {1, 2}
    assert rc.geometry(256) == (4, 1, 0) and rc.geometry(257) == (8, 1, 255) and rc.geometry(4097) == (32, 3, 2047)
    # a read that is long enough holds the window: most of it comes back as matches
    for c, (sc, _, _, _) in zip(cases, rc.expected("grid")):
        if len(c.read) >= len(c.ref) and c.ext == 0 and len(c.ref) > 200:
            assert sc > len(c.ref), c.name


def test_tracts_have_an_equal_scoring_neighbour():
    """At least two optimal alignments for every case: the oracle's CIGAR with one gap moved by one motif, or the whole of it
    moved by one motif along the read, re-scores to the oracle's score.  Which one the oracle (and the device) reports is the
    tie rule's doing alone."""
    cases, exp = rc.cases("tracts"), rc.expected("tracts")
    labels, fallbacks, unique = set(), [], []
    for c, (sc, e2, cig, _) in zip(cases, exp):
        assert c.kind == "tie" and c.motif >= 1
        s = expand(cig)
        variants = []
        for m in ((c.motif,) if c.motif > 1 else (1, 2)):
            variants.append("D" * m + s)                       # the whole alignment, one motif along the read
            if s.startswith("D" * m):
                variants.append(s[m:])
            for a, b in gap_runs(s):                            # one gap, one motif along the alignment
                if a >= m and set(s[a - m:a]) == {"="}:
                    variants.append(s[:a - m] + s[a:b] + s[a - m:a] + s[b:])
                if set(s[b:b + m]) == {"="} and len(s) >= b + m:
                    variants.append(s[:a] + s[b:b + m] + s[a:b] + s[b + m:])
        found = any(scores_as(c, v, sc) for v in variants if v != s)
        if not found:
            # No single shift does it (the runs are many: free gaps, or gaps dearer than what the flank is worth).  Then the
            # oracle's answer under the other gap preference, and for the pair read backwards (the rightmost choices where
            # it made the leftmost), turned round: each re-scored like any other candidate.
            fallbacks.append(c.name)
            _, _, other = oracle.realign(c.ref, c.read, c.open, c.ext, 1 - c.gap_pref)
            variants = [expand(cigar_tuples(other))]
            for pref in (0, 1):
                _, re2, rcig = oracle.realign(c.ref[::-1], c.read[::-1], c.open, c.ext, pref)
                back = expand(cigar_tuples(rcig))
                variants.append("D" * (len(c.read) - 1 - re2) + back.lstrip("D")[::-1])
            found = any(scores_as(c, v, sc) for v in variants if v != s)
        if not found:
            unique.append((c.name, cig))
        labels.add(c.name.split("/")[1])
        if c.name.split("/")[1] in rc.TRACT_GEOMETRY:
            assert rc.geometry(len(c.ref))[:2] == rc.TRACT_GEOMETRY[c.name.split("/")[1]], c.name
    assert not unique, (len(unique), unique[:5])
    assert labels == set(rc.TRACT_GEOMETRY) | {"two-letter"}
    assert len(fallbacks) < len(cases) // 4, len(fallbacks)   # the shifted gap is the rule
    assert {(c.open, c.ext, c.gap_pref) for c in cases if "/tiles3/" in c.name} == set(rc.PARAMS8)
    # expansions and contractions come back as gaps inside the tract where a gap is cheaper than what it saves
    kinds = {op for c, (_, _, cig, _) in zip(cases, exp) if (c.open, c.ext) == (7, 0) for _, op in cig[1:]}
    assert {"I", "D"} <= kinds


def test_col_seams_have_an_I_run_on_their_seam():
    """span: one I run covers window indices i_s - 1 and i_s (the last column of a lane or tile and the first of the next);
    ends / begins: an I run ends at i_s / begins at i_s (a run of one base can only do one of the two); leading / trailing:
    the CIGAR begins / ends with an I run of the bases the read lacks."""
    cases, exp = rc.cases("col_seams"), rc.expected("col_seams")
    seen = set()
    for c, (sc, e2, cig, _) in zip(cases, exp):
        ins = [(i, i + n) for op, n, i, _ in runs(cig) if op == "I"]
        cl, ntiles, pad = rc.geometry(len(c.ref))
        if c.kind in ("span", "ends", "begins"):
            col = c.seam + pad
            assert 0 < c.seam < len(c.ref) and col % cl == 0, c.name
            if ntiles > 1:
                assert col % (64 * cl) == 0, c.name
            if c.kind == "span":
                assert any(a <= c.seam - 1 and c.seam + 1 <= b for a, b in ins), (c.name, cig)
            elif c.kind == "ends":
                assert any(b == c.seam for a, b in ins), (c.name, cig)
            else:
                assert any(a == c.seam for a, b in ins), (c.name, cig)
        elif c.kind == "leading":
            assert cig[0] == (c.seam, "I"), (c.name, cig[:3])
        else:
            assert c.kind == "trailing" and cig[-1] == (c.seam, "I") and e2 == len(c.read) - 1, (c.name, cig[-3:])
        seen.add((c.name.split("/")[1], c.kind))
    for label, n1, cols, _ in rc.COL_WINDOWS:
        assert {(label, k) for k in ("span", "ends", "begins")} <= seen
        cl = rc.geometry(n1)[0]
        lengths = {int(c.name.split("/")[3].lstrip("spanedbgi")) for c in cases if c.name.startswith(f"col_seams/{label}/col")}
        assert lengths == {1, 2, cl, cl + 1, 3 * cl}, label
    assert {(c.open, c.ext, c.gap_pref) for c in cases if "/tiles3/" in c.name} == set(rc.PARAMS8)


def test_row_seams_have_a_D_run_on_their_seam():
    """span: a D run that is not the free leading one covers read positions j_s - 1 and j_s (the last row of a 64-step block
    or of a 1 024-symbol strip and the first of the next); begins / ends: such a run begins / ends at j_s.  What cannot be
    built is not in the corpus: a run that ends at the seam needs window bases in front of it (rc.row_placements)."""
    cases, exp = rc.cases("row_seams"), rc.expected("row_seams")
    placed = set()
    for c, (sc, e2, cig, _) in zip(cases, exp):
        dels = [(j, j + n) for op, n, i, j in runs(cig) if op == "D" and i > 0]
        if c.kind == "span":
            assert any(a <= c.seam - 1 and c.seam + 1 <= b for a, b in dels), (c.name, cig)
        elif c.kind == "begins":
            assert any(a == c.seam for a, b in dels), (c.name, cig)
        elif c.kind == "ends":
            assert any(b == c.seam for a, b in dels), (c.name, cig)
        elif c.kind == "first":
            assert cig[0][1] == "=" and sc == 2 * len(c.ref), (c.name, cig[:3])
        else:
            assert c.kind == "last" and e2 == len(c.read) - 1 and sc == 2 * len(c.ref), (c.name, e2)
        if c.seam > 0:
            placed.add((c.name.split("/")[1], c.seam, c.kind, int(c.name.split("/")[3].lstrip("spanedbgi"))))
    for label, _, _ in rc.ROW_WINDOWS:
        assert {p[1:] for p in placed if p[0] == label} == {(j, k, n) for k, j, _, n in rc.row_placements()}, label
    # every run length spans or touches every seam; all three kinds at every seam
    assert {(j, n) for _, j, _, n in placed} == {(j, n) for j in rc.ROW_SEAMS for n in rc.ROW_RUNS}
    assert {(j, k) for _, j, k, _ in placed} == {(j, k) for j in rc.ROW_SEAMS for k in ("span", "begins", "ends")}
    assert {(c.ext) for c in cases} == {0, 1}


def test_bytes_hold_every_value_on_both_sides():
    cases = rc.cases("bytes")
    assert {len(c.ref) for c in cases} == {300, 2100}
    for c, (sc, _, cig, _) in zip(cases, rc.expected("bytes")):
        assert set(c.ref) == set(range(256)) and set(c.read) == set(range(256)), c.name
        assert b"X" * 5 in c.read and b"x" * 40 in c.read, c.name
        # the window is found where it stands in the read: most of it in aligned columns, equal and unequal ones
        assert sum(n for n, op in cig if op in "=X") >= 0.75 * len(c.ref) and {"=", "X"} <= {op for _, op in cig}, c.name


def test_mixed_is_one_call_of_every_class_that_the_budget_cuts_up():
    cases = rc.cases("mixed")
    assert 35 <= len(cases) <= 45
    assert {(c.open, c.ext, c.gap_pref) for c in cases} == {(7, 0, 0)}
    assert {rc.geometry(len(c.ref))[:2] for c in cases} == {(4, 1), (8, 1), (16, 1), (32, 1), (32, 2), (32, 3)}
    assert {c.name.split("/")[1] for c in cases} == {"grid", "tracts", "col_seams", "row_seams", "bytes"}
    cut = rc.chunks(cases, rc.MIXED_BUDGET)
    assert len(cut) >= 4 and any(p1 - p0 > 1 for p0, p1 in cut)
    alone = [c for c in cases if rc.trace_bytes(len(c.ref), len(c.read)) > rc.MIXED_BUDGET]
    assert alone, "no pair exceeds the budget alone"
    assert rc.chunks(cases, 16 << 30) == [(0, len(cases))]


def test_bound_cases_are_the_last_taken_and_their_neighbours_the_first_refused():
    inside, outside = rc.cases("bound"), rc.bound_outside()
    assert len(inside) == len(outside) == len(rc.BOUND_EDGES) * (len(rc.BOUND_N2) + 1)
    for c, d in zip(inside, outside):
        assert 0 <= c.ext <= c.open <= 4096 and (d.open, d.ext) == (c.open, c.ext) and len(d.ref) == len(c.ref) + 1
        assert rc.gap_cost_reach(c.open, c.ext, len(c.ref)) < rc.GAP_COST_LIMIT <= rc.gap_cost_reach(d.open, d.ext, len(d.ref)), c.name
    assert {rc.geometry(len(c.ref))[1] for c in inside} == {2, 3}
    assert {len(c.read) for c in inside} >= set(rc.BOUND_N2) and any(len(c.read) > len(c.ref) for c in inside)
    assert {c.gap_pref for c in inside} == {0, 1}


# ---- the kernel's arithmetic without the device (tests/realign_scalar.c) ------------------------------------------------------
@pytest.fixture(scope="module")
def scalar():
    fn = rc.scalar()
    if fn is None:
        pytest.skip("no host C compiler")
    return fn


@pytest.mark.parametrize("cell", rc.CELLS)
def test_scalar_restatement_of_the_kernel_equals_the_oracle_inside_the_bound(scalar, cell):
    cases, exp = rc.cases(cell), rc.expected(cell)
    got = rc._pool_map(lambda c: scalar(c.ref, c.read, c.open, c.ext, c.gap_pref), cases)
    for c, g, (sc, e2, cig, _) in zip(cases, got, exp):
        assert g == (sc, e2, cig), c.name


def test_scalar_restatement_goes_wrong_where_the_derivation_says(scalar):
    """Outside 2*open + (n1 - 2)*extend < 2^24 (strk_realign.h at kRealignNeg) the sentinel stands in for row 0's gap state:
    at the first window length refused its value equals the real one (the scores still agree); it gains `extend` per base
    after that and gives wrong scores once it is above the real H of its column.  With open = extend = 4096 against a
    one-base read (an X: 0 against every base): 4095 is the last length taken, 4096 to 4098 still agree in score, 4099
    does not, nor does anything behind it."""
    rng = np.random.default_rng(7)
    ref = rand_seq(rng, 4700)
    score = lambda fn, n1: fn(ref[:n1], "X", 4096, 4096, 0)[0]   # noqa: E731
    for n1 in (4000, 4094, 4095):
        assert rc.gap_cost_reach(4096, 4096, n1) < rc.GAP_COST_LIMIT
        sc, e2, cg = oracle.realign(ref[:n1], "X", 4096, 4096, 0)
        assert sc == -4096 * (n1 - 1) and scalar(ref[:n1], "X", 4096, 4096, 0) == (sc, e2, tuple(cigar_tuples(cg)))
    for n1 in (4096, 4097, 4098):
        assert rc.gap_cost_reach(4096, 4096, n1) >= rc.GAP_COST_LIMIT
        assert score(scalar, n1) == score(oracle.realign, n1) == -4096 * (n1 - 1)
    for n1 in (4099, 4100, 4552):
        assert score(oracle.realign, n1) == -4096 * (n1 - 1)
        assert score(scalar, n1) == -((1 << 24) + 4096), n1       # the sentinel less one extension: -16 781 312
