"""The oracle of the `mi` tests: the reference's rule for one trio locus (strkit/mi/result.py:275-501 with decimal=False,
strkit/utils.py:49-57) written out in plain Python over scipy.stats, and the multiple-testing corrections of its report
(result.py:669-698 through statsmodels' multipletests) from their published definitions in plain loops.  A restatement, not a
copy: it exists so that the library's host function and kernels have something independent to be held against.

A locus is a dict: gt = six called copy numbers (child 0, child 1, mother 0, mother 1, father 0, father 1), ci95 = six (lo, hi),
ci99 = the same or None, seqs = six strings or None, reads = six tuples of per-read copy numbers."""
import math
import warnings

import numpy as np
import scipy.stats as sst

KINDS = ("strict", "pm1", "ci_95", "ci_99", "seq", "sl", "sl_pm1")
CONFIGS = ((0, 0), (0, 1), (1, 0), (1, 1))       # (mother's allele, father's allele)
TESTED, OVERLAP, EMPTY_PARENT, EMPTY_CHILD = range(4)
FROM = ("none", "?", "mat", "pat", "both")
MT_METHODS = ("none", "bonferroni", "sidak", "holm-sidak", "holm", "simes-hochberg", "fdr_bh", "fdr_by")


def cis_overlap(a, b) -> bool:
    epsilon = -0.0001
    return (b[1] - a[0]) > epsilon and (a[1] - b[0]) > epsilon


def _strict(c, m, f) -> bool:
    return (c[0] in m and c[1] in f) or (c[0] in f and c[1] in m)


def _ci(c, m, f, widen) -> bool:
    mw = [(x[0] - x[0] * widen, x[1] + x[1] * widen) for x in m]
    fw = [(x[0] - x[0] * widen, x[1] + x[1] * widen) for x in f]
    for first, second in ((0, 1), (1, 0)):       # which child allele is the mother's
        for a in mw:
            for b in fw:
                if cis_overlap(c[first], a) and cis_overlap(c[second], b):
                    return True
    return False


def _pm1(c, m, f) -> bool:
    return _ci([(x - 1, x + 1) for x in c], [(x, x) for x in m], [(x, x) for x in f], 0.0)


def respects_mi(locus, widen=0.0) -> dict:
    gt = locus["gt"]
    c, m, f = gt[0:2], gt[2:4], gt[4:6]
    out = {"strict": _strict(c, m, f), "pm1": _pm1(c, m, f)}
    ci = locus["ci95"]
    out["ci_95"] = _ci(ci[0:2], ci[2:4], ci[4:6], widen)
    ci = locus.get("ci99")
    out["ci_99"] = None if ci is None else _ci(ci[0:2], ci[2:4], ci[4:6], widen)
    s = locus.get("seqs")
    if s is None:
        out.update(seq=None, sl=None, sl_pm1=None)
    else:
        ln = [len(x) for x in s]
        out["seq"] = _strict(s[0:2], s[2:4], s[4:6])
        out["sl"] = _strict(ln[0:2], ln[2:4], ln[4:6])
        out["sl_pm1"] = _pm1(ln[0:2], ln[2:4], ln[4:6])
    return out


def x2_p(parent, child) -> float:
    lo, hi = min(*parent, *child), max(*parent, *child)
    cf, pf = [0] * (hi - lo + 1), [0] * (hi - lo + 1)
    for v in child:
        cf[v - lo] += 1
    for v in parent:
        pf[v - lo] += 1
    keep = [i for i in range(hi - lo + 1) if cf[i] or pf[i]]
    return float(sst.chi2_contingency(np.array([[cf[i] for i in keep], [pf[i] for i in keep]]), correction=False)[1])


def wmw_p(parent, child, greater=False) -> float:
    with np.errstate(all="ignore"):
        return float(sst.mannwhitneyu(np.array(parent), np.array(child), alternative="greater" if greater else "two-sided",
                                      use_continuity=False)[1])


def _from(mat_p, pat_p, sig) -> str:
    if mat_p < sig and pat_p < sig:
        return "both"
    if mat_p < sig:
        return "mat"
    if pat_p < sig:
        return "pat"
    return "?"


def de_novo(locus, test, sig_level=0.05) -> dict:
    """status, p, config (index into CONFIGS), mutation_from; and, for the tests' two lenient cases, config_ps (the four
    p-values, as far as the loop came) and second_ps (the p-values of the second stage, when it ran)."""
    child = [tuple(locus["reads"][0]), tuple(locus["reads"][1])]
    mother, father = locus["reads"][2:4], locus["reads"][4:6]
    res = {"status": TESTED, "p": None, "config": None, "mutation_from": "none", "config_ps": [], "second_ps": []}
    c_all = child[0] + child[1]
    if not c_all:
        res["status"] = EMPTY_CHILD      # this project's own: the reference fails here
        return res
    c_set = set(c_all)
    best_p, best = 0.0, 0
    for k, (a, b) in enumerate(CONFIGS):
        mat, pat = tuple(mother[a]), tuple(father[b])
        parent = mat + pat
        if len(c_set) == 1 and c_set == set(parent) and test.startswith("wmw"):
            res["status"] = OVERLAP
            return res
        if not mat or not pat:
            res["status"] = EMPTY_PARENT
            return res
        p = x2_p(parent, c_all) if test == "x2" else wmw_p(parent, c_all, greater=test == "wmw-gt")
        res["config_ps"].append(p)
        if p > best_p:
            best_p, best = p, k
    res["p"], res["config"] = best_p, best
    if best_p < sig_level:
        mat, pat = tuple(mother[CONFIGS[best][0]]), tuple(father[CONFIGS[best][1]])
        with np.errstate(all="ignore"), warnings.catch_warnings():
            warnings.simplefilter("ignore")          # (the mean of an empty child group is NaN, and then neither sum is larger)
            c0, c1 = np.mean(child[0]), np.mean(child[1])
            d1 = np.abs(c0 - np.mean(mat)) + np.abs(c1 - np.mean(pat))
            d2 = np.abs(c1 - np.mean(mat)) + np.abs(c0 - np.mean(pat))
        if d2 > d1:
            res["second_ps"] = [wmw_p(mat, child[0]), wmw_p(pat, child[1])]
            res["mutation_from"] = _from(*res["second_ps"], sig_level)
        elif d1 > d2:
            res["second_ps"] = [wmw_p(mat, child[1]), wmw_p(pat, child[0])]
            res["mutation_from"] = _from(*res["second_ps"], sig_level)
        else:
            res["mutation_from"] = "?"
    return res


# ---- multiple testing (Bonferroni 1936, Sidak 1967, Holm 1979, Hochberg 1988, Benjamini-Hochberg 1995, Benjamini-Yekutieli 2001)
def _sidak(x, k):
    return 1.0 if x >= 1.0 else -math.expm1(k * math.log1p(-x))


def multipletests(pvals, alpha, method):
    """(rejected, adjusted p) in the caller's order.  Step-down: running maximum over ascending p; step-up: running minimum from the
    largest p down; adjusted p clipped at 1; a step-down method stops rejecting at the first p above its threshold, a step-up
    method rejects everything up to the last p at or below its threshold."""
    if method in ("fdr_tsbh", "fdr_tsbky"):
        raise ValueError(f"the two-stage method {method} is not supported")
    p = [float(x) for x in pvals]
    n = len(p)
    if method == "none":
        return [x < alpha for x in p], list(p)
    order = sorted(range(n), key=lambda i: p[i])
    ps = [p[i] for i in order]
    adj, rej = [0.0] * n, [False] * n
    if method == "bonferroni":
        adj = [x * n for x in ps]
        rej = [x <= alpha / n for x in ps]
    elif method == "sidak":
        adj = [_sidak(x, n) for x in ps]
        rej = [x <= 1 - (1 - alpha) ** (1.0 / n) for x in ps]
    elif method in ("holm", "holm-sidak"):
        run, going = 0.0, True
        for i, x in enumerate(ps):
            k = n - i
            raw = x * k if method == "holm" else _sidak(x, k)
            thr = alpha / k if method == "holm" else 1 - (1 - alpha) ** (1.0 / k)
            run = max(run, raw)
            adj[i] = run
            going = going and not x > thr
            rej[i] = going
    elif method in ("simes-hochberg", "fdr_bh", "fdr_by"):
        cm = sum(1.0 / i for i in range(1, n + 1)) if method == "fdr_by" else 1.0
        run, last = math.inf, -1
        for i in range(n - 1, -1, -1):
            if method == "simes-hochberg":
                raw, thr = ps[i] * (n - i), alpha / (n - i)
            else:
                raw, thr = ps[i] * n * cm / (i + 1), alpha * (i + 1) / (n * cm)
            run = min(run, raw)
            adj[i] = run
            if last < 0 and ps[i] <= thr:
                last = i
        rej = [i <= last for i in range(n)]
    else:
        raise ValueError(f"unknown method {method}")
    out_adj, out_rej = [0.0] * n, [False] * n
    for i, o in enumerate(order):
        out_adj[o], out_rej[o] = min(adj[i], 1.0), rej[i]
    return out_rej, out_adj
