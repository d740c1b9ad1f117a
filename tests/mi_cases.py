"""The corpus of the `mi` tests and the one comparison they share: loci as mi_restatement.py takes them, in cells
(name -> list of loci), the oracle's answers computed once per (cell, test), and `compare`, which holds a library result
against them under the tolerances of DESIGN.md §16.

Cells: `hand` (the hand cases of test_mi_restatement.py), `d2` .. `d250` (seeded random trios of that many reads per group),
`exact` (groups of distinct integers: the exact Mann-Whitney branch, short sides 1, 2, 8, 9 and long sides 1, 8, 9, 64, 300),
`wide` (copy numbers 0 .. 5000 in one locus), `deep` (disjoint samples over 60 to 1 500 bins: chi-square statistics of 1 420 to
4 000, p of 1e-200 to 1e-300) and `tiny` (disjoint samples over few bins: p down to below 1e-300)."""
import functools

import numpy as np

import mi_restatement as R

TESTS = ("x2", "wmw", "wmw-gt")
SIG = 0.05
P_RTOL = 1e-9          # against the oracle wherever its p >= 1e-300
LENIENT_RTOL = 1e-8    # two p-values, or a p-value and the level, closer than this: either branch is accepted
MAX_LENIENT_SHARE = 0.2


def locus(reads, gt=None, ci95=None, seqs=None):
    reads = [tuple(int(v) for v in g) for g in reads]
    if gt is None:
        gt = [int(round(float(np.mean(g)))) if g else 0 for g in reads]
    if ci95 is None:
        ci95 = [(g - 1, g + 1) for g in gt]
    return {"gt": list(gt), "ci95": [tuple(c) for c in ci95], "ci99": None, "seqs": seqs, "reads": reads}


def hand_cases():
    rd = [(10, 10, 11), (12, 12), (10, 10), (14, 14, 15), (12, 12, 13), (20, 20)]
    out = {
        "strict": locus(rd, gt=[10, 12, 10, 14, 12, 20], ci95=[(10, 10), (12, 12), (10, 10), (14, 14), (12, 12), (20, 20)]),
        "pm1_only": locus(rd, gt=[11, 12, 10, 14, 12, 20], ci95=[(11, 11), (12, 12), (10, 10), (14, 14), (12, 12), (20, 20)]),
        "ci95_only": locus(rd, gt=[13, 12, 10, 16, 12, 20], ci95=[(12, 14), (12, 12), (10, 10), (14, 17), (12, 12), (20, 20)]),
        "ci95_with_widen": locus(rd, gt=[13, 12, 10, 10, 12, 30], ci95=[(13, 13), (12, 12), (10, 10), (11, 12), (12, 12), (30, 30)]),
        "seq_not_strict": locus(rd, gt=[10, 12, 11, 14, 13, 20], seqs=["ACAC", "ACACAC", "ACAC", "ACACACAC", "ACACAC", "AC"]),
        "strict_not_seq": locus(rd, gt=[10, 12, 10, 14, 12, 20], seqs=["ACAC", "ACACAC", "ACAT", "ACACACAC", "ACACAT", "AC"]),
        "touching": locus(rd, gt=[10, 12, 8, 14, 12, 20], ci95=[(10, 11), (12, 12), (8, 10), (14, 14), (12, 12), (20, 20)]),
        "one_bin": locus([(5, 5), (5,), (5, 5), (5,), (5,), (5, 5)]),
        "overlap_first_config_only": locus([(5, 5), (5,), (5, 5), (6,), (5,), (6, 6)]),
        "empty_parent": locus([(5, 6), (7,), (5, 5), (), (6,), (7,)]),
        "empty_parent_later": locus([(5, 6), (7,), (5, 5), (6, 6), (6,), ()]),
        "empty_child": locus([(), (), (5, 5), (6,), (6,), (7,)]),
        "empty_child_group": locus([(30, 31, 32, 30, 31, 32, 30, 31), (), (5, 5, 5, 5), (6, 6, 6), (6, 6, 6), (7, 7, 7)]),
        "all_tied_second": locus([(5, 5), (7, 7, 7, 7, 11, 11, 11, 11), (5, 5, 5), (5, 5, 5), (9,) * 8, (9,) * 8]),
        "equal_distances": locus([(8, 8, 8), (8, 8, 8), (2, 2, 2), (2, 2), (2, 2, 2), (2, 2)]),
        "four_equal": locus([(7, 8, 9), (8, 9, 10), (3, 4), (4, 3), (5, 4), (4, 5)]),
        "de_novo_pat": locus([(10, 10, 10, 11, 10, 10, 10, 10), (17, 18, 18, 18, 18, 19, 18, 18), (10, 10, 10, 10, 9, 10, 10, 10),
                              (12, 12, 12, 12, 13, 12, 12, 12), (15, 15, 15, 14, 15, 15, 15, 16), (20, 20, 21, 20, 20, 20, 20, 20)]),
    }
    return out


def _reads(rng, allele, n):
    return tuple(int(max(0, v)) for v in np.rint(allele + rng.normal(0.0, 0.35 + 0.02 * allele, n)))


def random_trio(rng, depth):
    m, f = sorted(rng.integers(5, 40, 2).tolist()), sorted(rng.integers(5, 40, 2).tolist())
    if rng.random() < 0.2:
        m[1] = m[0]
    c = [m[int(rng.integers(2))], f[int(rng.integers(2))]]
    if rng.random() < 0.35:
        c[int(rng.integers(2))] += int(rng.integers(1, 4)) * (1 if rng.random() < 0.6 else -1)
    sizes = [max(0 if rng.random() < 0.02 else 1, int(depth + rng.integers(-depth // 3, depth // 3 + 1))) for _ in range(6)]
    alleles = c + m + f
    return locus([_reads(rng, a, n) for a, n in zip(alleles, sizes)], gt=alleles)


def exact_locus(rng, child_sizes, parent_sizes, shift):
    """Six groups of distinct integers; `shift` moves the child's values up against the parents'."""
    sizes = list(child_sizes) + list(parent_sizes)
    total = sum(sizes)
    pool = rng.permutation(np.arange(10, 10 + 3 * total))[:total]
    groups, at = [], 0
    for k, n in enumerate(sizes):
        g = np.sort(pool[at:at + n])
        groups.append(g * 2 + (1 + 2 * shift if k < 2 else 0))      # parents even, child odd: no value is tied
        at += n
    return locus(groups)


def deep_tail_locus(n, bins):
    """Child and parents on disjoint values, `bins` distinct values each side, about n reads per group: the chi-square statistic
    of a configuration is then its n1 + n2 (1 420 to 4 000 here) over 2 bins - 1 degrees, a p of 1e-200 to 1e-300, where
    e^(-statistic / 2) alone is denormal or 0.  The parents' groups have sizes of their own, so the four p-values differ; the steps are coprime to
    the numbers of bins used (30, 55, 750), so every group visits every bin."""
    sizes = (n, n + 5, n, n + 10, n + 3, n + 17)
    return locus([[(1000 if g < 2 else 10) + (i * (7, 13, 17, 19, 23, 29)[g] + g) % bins for i in range(m)] for g, m in enumerate(sizes)])


def exact_cases(rng):
    """The two parents' groups get sizes whose four sums differ, so that the four configurations are four different tests: with all
    values distinct a configuration's chi-square statistic is n1 + n2 whatever the values are, and equal sums would make the four
    p-values one number in four orders of summation, whose order in scipy is rounding noise of 3e-16 and no property of the rule."""
    out = []
    for short in (1, 2, 8, 9):
        for long_ in (1, 8, 9, 64, 300):
            h = max(long_ // 2, 1)
            for shift in (0, 3 * long_):
                # the child is the short side of the four first tests; its groups against the parents' are the second ones
                out.append(exact_locus(rng, (short - short // 2, short // 2), (h, h + 1, h, h + 2), shift))
                # the parents are the short side: short, short + 2, short + 1 and short + 3 values (from 2 on)
                a, b = max(short - short // 2, 1), max(short // 2, 1)
                out.append(exact_locus(rng, (h, max(long_ - h, 1)), (a, a + 1, b, b + 2), shift))
    return out


@functools.lru_cache(maxsize=None)
def cells():
    rng = np.random.default_rng(20260222)
    out = {"hand": list(hand_cases().values())}
    for depth, n in ((2, 60), (5, 60), (15, 60), (30, 60), (250, 12)):
        out[f"d{depth}"] = [random_trio(rng, depth) for _ in range(n)]
    out["exact"] = exact_cases(rng)
    wide = rng.integers(0, 5001, 90)
    wide[:2] = (0, 5000)
    out["wide"] = [locus([wide[0:10], wide[10:30], wide[30:45], wide[45:60], wide[60:75], wide[75:90]]),
                   locus([wide[0:40] // 7, wide[40:50], wide[50:60] // 7, wide[60:70], wide[70:80] // 7, wide[80:90]])]
    out["deep"] = [deep_tail_locus(375, 55), deep_tail_locus(400, 55), deep_tail_locus(425, 55), deep_tail_locus(370, 30), deep_tail_locus(1000, 750)]
    out["tiny"] = [locus([[100 + i % 11 for i in range(n)], [104 + i % 7 for i in range(n)], [10 + i % 11 for i in range(n)],
                          [12 + i % 5 for i in range(n)], [14 + i % 3 for i in range(n)], [20 + i % 9 for i in range(n)]]) for n in (125, 250, 350, 400)]
    return out


def all_loci():
    """(loci in one list, the cell's name per locus)"""
    loci, names = [], []
    for name, ls in cells().items():
        loci += ls
        names += [name] * len(ls)
    return loci, names


@functools.lru_cache(maxsize=None)
def oracle(test, sig_level=SIG):
    """The oracle's de_novo per locus of all_loci(), computed once per test and left unchanged."""
    return tuple(R.de_novo(l, test, sig_level) for l in all_loci()[0])


@functools.lru_cache(maxsize=None)
def oracle_respects(widen=0.0):
    return tuple(R.respects_mi(l, widen) for l in all_loci()[0])


def _close(a, b, rtol):
    return a == b or abs(a - b) <= rtol * max(abs(a), abs(b))


def lenient(exp, sig_level=SIG):
    """(either configuration is accepted, either branch at the level is accepted) for one oracle answer."""
    ps = sorted((p for p in exp["config_ps"] if p == p), reverse=True)
    either_config = len(ps) >= 2 and ps[0] != ps[1] and _close(ps[0], ps[1], LENIENT_RTOL)
    deciding = ([exp["p"]] if exp["p"] is not None else []) + [p for p in exp["second_ps"] if p == p]
    either_branch = any(_close(p, sig_level, LENIENT_RTOL) for p in deciding)
    return either_config, either_branch


def lenient_share(test, sig_level=SIG):
    """Per cell the share of loci that use a lenient case, from the oracle alone."""
    _, names = all_loci()
    used, total = {}, {}
    for exp, name in zip(oracle(test, sig_level), names):
        total[name] = total.get(name, 0) + 1
        used[name] = used.get(name, 0) + (1 if any(lenient(exp, sig_level)) else 0)
    return {k: used[k] / total[k] for k in total}


def compare(got, test, sig_level=SIG, widen=0.0):
    """Holds the arrays of mi_trio_batch over all_loci() against the oracle; returns the agreement line.  Discrete outputs are
    compared exactly, p at P_RTOL where the oracle's is >= 1e-300 (below that both are below 1e-299; a NaN meets a NaN)."""
    loci, names = all_loci()
    exp_r = oracle_respects(widen)
    for i, e in enumerate(exp_r):
        want = [-1 if e[k] is None else int(e[k]) for k in R.KINDS]
        assert got["respects"][i].tolist() == want, (names[i], i, got["respects"][i].tolist(), want)
    if test == "none":
        return f"mi none: {len(loci)} loci, 7 kinds equal"
    worst, n_tested, n_lenient = 0.0, 0, 0
    for i, e in enumerate(oracle(test, sig_level)):
        where = (test, names[i], i)
        assert int(got["status"][i]) == e["status"], (where, int(got["status"][i]), e["status"])
        p, cfg, frm = float(got["p"][i]), int(got["config"][i]), R.FROM[int(got["mutation_from"][i])]
        if e["status"] != R.TESTED:
            assert p != p and cfg == -1 and frm == "none", (where, p, cfg, frm)
            continue
        n_tested += 1
        either_config, either_branch = lenient(e, sig_level)
        n_lenient += 1 if either_config or either_branch else 0
        want_p = e["p"]
        if cfg != e["config"]:
            assert either_config, (where, cfg, e["config"], e["config_ps"])
            want_p = e["config_ps"][cfg]
        if want_p >= 1e-300:
            assert _close(p, want_p, P_RTOL), (where, p, want_p)
            worst = max(worst, abs(p - want_p) / want_p)
        else:
            assert 0.0 <= p < 1e-299, (where, p, want_p)
        if cfg == e["config"] and not either_branch:
            assert frm == e["mutation_from"], (where, frm, e["mutation_from"], e["second_ps"])
    return f"mi {test}: {len(loci)} loci, {n_tested} tested, {n_lenient} lenient, worst relative p error {worst:.2e}"
