"""CPU restatement of the phased allele call that k_phase_group / k_alleles / k_phase_finish run on the device.

Test infrastructure only: the product never imports this file.  It states rule A-F of DESIGN.md §13 (STRkit's
call_alleles_with_haplotags, call_alleles_with_incorporated_snvs, calculate_read_distance and
call_and_filter_useful_snvs, with sklearn's average-linkage clustering written out as scipy's nearest-neighbour chain)
in plain numpy; the per-group single-allele calls of step D are alleles_restatement.call_locus.
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

import alleles_restatement as AR

CALLED, TOO_FEW, EMPTY_PEAK, NOT_PHASED = 0, 1, 2, 3
ASSIGN_NONE, ASSIGN_HP, ASSIGN_SNV, ASSIGN_SNV_DIST = 0, 1, 2, 3
REASON_NONE, REASON_NO_TAGS, REASON_TAG_THRESHOLDS, REASON_FEW_SNV_READS, REASON_GROUP_NOT_CALLED, REASON_NO_SNV_CALLED = range(6)
SNV_NOT_EVALUATED, SNV_CALLED, SNV_ZERO_TOTAL, SNV_ONLY_OUT_OF_RANGE, SNV_CROSS_TALK, SNV_SAME_BASE = -1, 0, 1, 2, 3, 4
OUT_OF_RANGE, GAP = ord("-"), ord("_")


@dataclass(frozen=True)
class PhaseParams:
    min_hp_read_coverage: int = 8
    snv_quality_threshold: int = 20
    many_snvs_quantity: int = 3
    cn_weight_few: float = 0.2
    cn_weight_many: float = 0.1


def unskipped(base: np.ndarray, qual: np.ndarray, thr: int) -> np.ndarray:
    """Cells that take part in a distance: not '-', and a real base only with quality >= thr."""
    return (base != OUT_OF_RANGE) & ((base == GAP) | (qual >= thr))


def real_cells(base: np.ndarray, qual: np.ndarray, thr: int) -> np.ndarray:
    return (base != OUT_OF_RANGE) & (base != GAP) & (qual >= thr)


def distance_matrix(cn, base, qual, pure: bool, pp: PhaseParams = PhaseParams()) -> np.ndarray:
    """calculate_read_distance over the clustered reads (rows of base / qual)."""
    cn = np.asarray(cn, dtype=np.int64)
    u = unskipped(base, qual, pp.snv_quality_threshold)
    both = u[:, None, :] & u[None, :, :]
    d = (both & (base[:, None, :] != base[None, :, :])).sum(axis=2).astype(np.float64)
    if not pure:
        ncomp = both.sum(axis=2)
        wgt = np.where(ncomp >= pp.many_snvs_quantity, pp.cn_weight_many, pp.cn_weight_few)
        d = d + np.abs(cn[:, None] - cn[None, :]).astype(np.float64) * wgt
    np.fill_diagonal(d, 0.0)
    return d


def nn_chain_two_clusters(dm: np.ndarray) -> np.ndarray:
    """Average linkage cut at two clusters by scipy's nearest-neighbour chain.  Returns 0/1 labels, cluster 0 holding
    point 0."""
    m = dm.shape[0]
    D = np.array(dm, dtype=np.float64)
    size = np.ones(m, dtype=np.int64)
    chain: list[int] = []
    mx, my, md = [], [], []
    for _ in range(m - 1):
        if not chain:
            chain.append(int(np.nonzero(size > 0)[0][0]))
        while True:
            x = chain[-1]
            row = np.where(size > 0, D[x], np.inf)
            row[x] = np.inf
            y = int(np.argmin(row))          # the lowest index among the smallest
            cur = float(row[y])
            if len(chain) > 1 and D[x, chain[-2]] <= cur:   # the previous element wins ties
                y = chain[-2]
                cur = float(D[x, y])
            if len(chain) > 1 and y == chain[-2]:
                break
            chain.append(y)
        del chain[-2:]
        if x > y:
            x, y = y, x
        nx, ny = int(size[x]), int(size[y])
        mx.append(x)
        my.append(y)
        md.append(cur)
        size[x] = 0
        size[y] = nx + ny
        live = size > 0
        live[y] = False
        new = (float(nx) * D[live, x] + float(ny) * D[live, y]) / float(nx + ny)
        D[live, y] = new
        D[y, live] = new
    order = np.argsort(np.asarray(md), kind="stable")
    parent = list(range(m))

    def find(a: int) -> int:
        while parent[a] != a:
            parent[a] = parent[parent[a]]
            a = parent[a]
        return a

    for k in order[: m - 2]:
        parent[find(mx[k])] = find(my[k])
    root0 = find(0)
    return np.array([0 if find(i) == root0 else 1 for i in range(m)], dtype=np.int32)


def _most_common(seq):
    """Counter.most_common: by count, ties to the byte seen first."""
    first, count = {}, {}
    for i, b in enumerate(seq):
        first.setdefault(b, i)
        count[b] = count.get(b, 0) + 1
    return sorted(count.items(), key=lambda kv: (-kv[1], first[kv[0]])), count


def call_snvs(base, qual, read_peak, thr: int):
    """Step E.  Returns status [S], call [S, 2], rcs [S, 2]."""
    S = base.shape[1]
    status = np.zeros(S, np.int32)
    call = np.zeros((S, 2), np.uint8)
    rcs = np.zeros((S, 2), np.int32)
    for s in range(S):
        mc, cnt, tot = [], [], []
        for p in range(2):
            ok = (read_peak == p) & ((base[:, s] == GAP) | (qual[:, s] >= thr))
            m, c = _most_common(base[ok, s].tolist())
            mc.append(m)
            cnt.append(c)
            tot.append(int(ok.sum()))
        picked = []
        st = SNV_CALLED
        for a in range(2):
            b = 1 - a
            if tot[a] == 0:
                st = SNV_ZERO_TOTAL
                break
            m = mc[a][0]
            if m[0] == OUT_OF_RANGE:
                if len(mc[a]) < 2:
                    st = SNV_ONLY_OUT_OF_RANGE
                    break
                m = mc[a][1]
            if tot[b] == 0:
                st = SNV_ZERO_TOTAL
                break
            if cnt[b].get(m[0], 0) / tot[b] > cnt[a].get(m[0], 0) / tot[a] / 2:
                st = SNV_CROSS_TALK
                break
            picked.append(m)
        if st == SNV_CALLED and picked[0][0] == picked[1][0]:
            st = SNV_SAME_BASE
        status[s] = st
        if st == SNV_CALLED:
            call[s] = [picked[0][0], picked[1][0]]
            rcs[s] = [picked[0][1], picked[1][1]]
    return status, call, rcs


def _seqsum(a) -> float:
    s = 0.0
    for x in a:
        s = s + float(x)
    return s


def call_locus(cn, w, n_alleles: int, seed: int, hp=None, ps=None, base=None, qual=None, p: AR.Params = AR.Params(),
               pp: PhaseParams = PhaseParams()) -> dict:
    """Rule A-F for one locus.  base / qual: [n, S] uint8 or None."""
    cn = np.asarray(cn, dtype=np.int32)
    w = np.asarray(w, dtype=np.float64)
    n = cn.shape[0]
    S = 0 if base is None else base.shape[1]
    out = dict(status=TOO_FEW, method=ASSIGN_NONE, reason=REASON_NONE, ps=-1, modal_n=0, call=[-1, -1], ci95=[-1] * 4,
               ci99=[-1] * 4, means=[np.nan] * 2, weights=[np.nan] * 2, stdevs=[np.nan] * 2, peak_n_reads=[0, 0],
               read_peak=np.full(n, -1, np.int32), snv_status=np.full(S, SNV_NOT_EVALUATED, np.int32),
               snv_call=np.zeros((S, 2), np.uint8), snv_rcs=np.zeros((S, 2), np.int32), close_means=False, labels=None)
    if n < p.min_reads:
        return out
    out["status"] = NOT_PHASED
    gp = AR.Params(**{**p.__dict__, "min_reads": p.min_allele_reads})

    def call_groups(groups):
        res = []
        for g, idx in enumerate(groups):
            wg = w[idx]
            r = AR.call_locus(cn[idx], wg / _seqsum(wg) if len(idx) else wg, 1, AR.locus_seed(seed, g), gp)
            if r["status"] == TOO_FEW:
                return None
            res.append(r)
        return res

    def combine(res, groups, order):
        k = len(res)
        pad = 2 - k
        rp = np.full(n, -1, np.int32)
        for pk, g in enumerate(order):
            rp[groups[g]] = pk
        rr = [res[g] for g in order]
        out.update(status=CALLED, modal_n=k, call=[r["call"][0] for r in rr] + [-1] * pad,
                   ci95=[x for r in rr for x in r["ci95"][:2]] + [-1, -1] * pad,
                   ci99=[x for r in rr for x in r["ci99"][:2]] + [-1, -1] * pad,
                   means=[r["means"][0] for r in rr] + [np.nan] * pad, weights=[1.0 / k] * k + [np.nan] * pad,
                   stdevs=[r["stdevs"][0] for r in rr] + [np.nan] * pad,
                   peak_n_reads=[len(groups[g]) for g in order] + [0] * pad, read_peak=rp)

    # B. haplotags
    reason = REASON_NO_TAGS
    if hp is not None:
        hp = np.asarray(hp, dtype=np.int32)
        ps = np.asarray(ps, dtype=np.int32)
        tagged = (hp >= 0) & (ps >= 0)
        reason = REASON_TAG_THRESHOLDS
        if tagged.any():
            seen, cnts = [], {}
            for v in ps[tagged].tolist():
                if v not in cnts:
                    seen.append(v)
                cnts[v] = cnts.get(v, 0) + 1
            top = max(seen, key=lambda v: (cnts[v], -seen.index(v)))
            haps = sorted(set(hp[tagged].tolist()))
            if int(tagged.sum()) >= pp.min_hp_read_coverage and len(haps) == n_alleles and cnts[top] >= pp.min_hp_read_coverage:
                groups = [np.nonzero((hp == h) & (ps == top))[0] for h in haps]
                res = call_groups(groups)
                if res is None:
                    reason = REASON_GROUP_NOT_CALLED
                else:
                    combine(res, groups, list(range(len(groups))))
                    out.update(method=ASSIGN_HP, ps=int(top))
                    return out
    # C. SNVs
    if n_alleles == 2 and S >= 1:
        thr = pp.snv_quality_threshold
        nreal = real_cells(base, qual, thr).sum(axis=1)
        n_many, n_one = int((nreal >= 2).sum()), int((nreal >= 1).sum())
        n_none = n - n_one
        pure = n_many + n_none == n
        proceed = (pure and n_many >= min(n * 0.68, 16)) or n_one >= min(n * 0.8, 16)
        if not proceed or n_one < 2:
            reason = REASON_FEW_SNV_READS
        else:
            idx = np.nonzero(nreal >= 1)[0]
            dm = distance_matrix(cn[idx], base[idx], qual[idx], pure, pp)
            lab = nn_chain_two_clusters(dm)
            out["labels"] = lab
            groups = [idx[lab == 0], idx[lab == 1]]
            res = call_groups(groups)
            if res is None:
                reason = REASON_GROUP_NOT_CALLED
            else:
                k0 = (res[0]["means"][0], res[0]["ci95"][0])
                k1 = (res[1]["means"][0], res[1]["ci95"][0])
                order = [1, 0] if k1 < k0 else [0, 1]
                m0, m1 = k0[0], k1[0]
                close = m0 != m1 and abs(m0 - m1) <= 1e-6 * max(abs(m0), abs(m1))
                rp = np.full(n, -1, np.int32)
                for pk, g in enumerate(order):
                    rp[groups[g]] = pk
                st, sc, rc = call_snvs(base, qual, rp, thr)
                out.update(snv_status=st, close_means=close)
                if not (st == SNV_CALLED).any():
                    reason = REASON_NO_SNV_CALLED
                else:
                    combine(res, groups, order)
                    out.update(method=ASSIGN_SNV if pure else ASSIGN_SNV_DIST, snv_call=sc, snv_rcs=rc)
                    return out
    out["reason"] = reason
    return out
