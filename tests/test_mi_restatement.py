"""CPU: the oracle of the `mi` tests (mi_restatement.py: the reference's rule over scipy.stats) on the hand cases of
mi_cases.py, each of which is there for one property of the rule."""
import math

import pytest
import scipy.stats as sst

import mi_cases as cases
import mi_restatement as R

HAND = cases.hand_cases()


def kinds(name, widen=0.0):
    return R.respects_mi(HAND[name], widen)


def test_respects_kinds_one_by_one():
    assert kinds("strict")["strict"] and kinds("strict")["pm1"] and kinds("strict")["ci_95"]
    r = kinds("pm1_only")
    assert (r["strict"], r["pm1"], r["ci_95"]) == (False, True, False)
    r = kinds("ci95_only")
    assert (r["strict"], r["pm1"], r["ci_95"]) == (False, False, True)
    assert kinds("strict")["ci_99"] is None and kinds("strict")["seq"] is None and kinds("strict")["sl_pm1"] is None


def test_widen_opens_the_parents_intervals():
    assert kinds("ci95_with_widen")["ci_95"] is False
    assert kinds("ci95_with_widen", widen=0.1)["ci_95"] is True
    assert kinds("ci95_with_widen", widen=0.1)["pm1"] is False      # (pm1 never widens)


def test_sequence_kinds_are_their_own():
    r = kinds("seq_not_strict")
    assert r["seq"] is True and r["strict"] is False
    r = kinds("strict_not_seq")
    assert r["seq"] is False and r["strict"] is True and r["sl"] is True and r["sl_pm1"] is True


def test_touching_intervals_overlap_by_the_epsilon():
    assert R.cis_overlap((10, 11), (8, 10)) and R.cis_overlap((8, 10), (10, 11))
    assert not R.cis_overlap((10.0002, 11), (8, 10)) and R.cis_overlap((10.00005, 11), (8, 10))
    r = kinds("touching")
    assert (r["strict"], r["pm1"], r["ci_95"]) == (False, False, True)


def test_one_bin_chi_square_is_exactly_one():
    assert sst.chi2_contingency([[3], [5]], correction=False)[1] == 1.0
    d = R.de_novo(HAND["one_bin"], "x2")
    assert d["status"] == R.TESTED and d["p"] == 1.0 and d["config"] == 0 and d["mutation_from"] == "none"


@pytest.mark.parametrize("name", ["one_bin", "overlap_first_config_only"])
def test_complete_overlap_is_not_tested_under_wmw_but_under_x2(name):
    assert R.de_novo(HAND[name], "wmw")["status"] == R.OVERLAP and R.de_novo(HAND[name], "wmw-gt")["status"] == R.OVERLAP
    assert R.de_novo(HAND[name], "x2")["status"] == R.TESTED


def test_empty_groups():
    for test in cases.TESTS:
        assert R.de_novo(HAND["empty_parent"], test)["status"] == R.EMPTY_PARENT
        assert R.de_novo(HAND["empty_parent_later"], test)["status"] == R.EMPTY_PARENT
        assert R.de_novo(HAND["empty_child"], test)["status"] == R.EMPTY_CHILD
    d = R.de_novo(HAND["empty_child_group"], "x2")      # a mean of nothing is NaN: neither sum of distances is the larger one
    assert d["status"] == R.TESTED and d["p"] < cases.SIG and d["mutation_from"] == "?" and d["second_ps"] == []


def test_all_tied_second_test_is_nan_and_not_below_the_level():
    assert math.isnan(sst.mannwhitneyu([5, 5, 5], [5, 5], use_continuity=False)[1])
    d = R.de_novo(HAND["all_tied_second"], "x2")
    assert d["p"] < cases.SIG and math.isnan(d["second_ps"][0]) and d["second_ps"][1] == 1.0 and d["mutation_from"] == "?"


def test_equal_distance_sums_give_a_question_mark():
    d = R.de_novo(HAND["equal_distances"], "x2")
    assert d["p"] < cases.SIG and d["second_ps"] == [] and d["mutation_from"] == "?"


def test_of_four_equal_p_values_the_first_wins():
    for test in cases.TESTS:
        d = R.de_novo(HAND["four_equal"], test)
        assert len(set(d["config_ps"])) == 1 and d["config"] == 0 and d["p"] == d["config_ps"][0]


def test_a_de_novo_expansion_of_the_fathers_allele():
    d = R.de_novo(HAND["de_novo_pat"], "x2")
    assert d["p"] < cases.SIG and R.CONFIGS[d["config"]] == (0, 0) and d["mutation_from"] == "pat"
    assert d["second_ps"][0] > cases.SIG > d["second_ps"][1]


def test_method_switch_of_mannwhitneyu_as_installed():
    """exact with a side of at most 8 and no tie, asymptotic otherwise: what strk_mi.h restates"""
    x, y = list(range(0, 16, 2)), list(range(1, 19, 2))
    assert sst.mannwhitneyu(x, y, use_continuity=False)[1] == sst.mannwhitneyu(x, y, use_continuity=False, method="exact")[1]
    x = list(range(0, 18, 2))
    assert sst.mannwhitneyu(x, y, use_continuity=False)[1] == sst.mannwhitneyu(x, y, use_continuity=False, method="asymptotic")[1]
    assert sst.mannwhitneyu([1, 2, 3], [3, 4], use_continuity=False)[1] == sst.mannwhitneyu([1, 2, 3], [3, 4], use_continuity=False, method="asymptotic")[1]
