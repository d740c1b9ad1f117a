"""Loci for the tests of the phased allele calls: one generator, and the corpus that the device tests compare against
tests/phase_restatement.py.  Test infrastructure only."""
from __future__ import annotations

import numpy as np

import alleles_restatement as AR
import phase_restatement as PR

BASES = np.frombuffer(b"ACGT", np.uint8)
LDS_CUT = 80   # kPhaseLdsReads of strk_phase.h
SIZES = (0, 1, 2, 3, 4, 7, 8, 9, 15, 16, 17, 30, 63, 64, 65, LDS_CUT, LDS_CUT + 1, 250)
SNV_COUNTS = (0, 1, 2, 3, 63, 64)
TAG_KINDS = ("none", "clean", "three_ps", "three_hp", "sparse", "one_hp", "split_top")
CELL_KINDS = ("clean", "noisy", "out_of_range_rows", "gap_rows", "at_threshold", "identical", "few_real")


def make_locus(rng, n: int, S: int, n_alleles: int, tag_kind: str, cell_kind: str):
    """One locus: cn, w [n]; hp, ps [n]; base, qual [n, S]."""
    hap = rng.integers(0, 2, size=n)
    a, b = int(rng.integers(5, 40)), int(rng.integers(5, 40))
    if n_alleles == 1:
        b = a
    cn = (np.where(hap == 0, a, b) + rng.integers(-1, 2, size=n) * (rng.random(n) < 0.3)).astype(np.int32)
    w = rng.uniform(0.2, 2.0, size=n)
    hp = np.full(n, -1, np.int32)
    ps = np.full(n, -1, np.int32)
    if tag_kind != "none" and n:
        tagged = rng.random(n) < (0.3 if tag_kind == "sparse" else 0.9)
        hp[tagged] = (1 + hap[tagged]) if tag_kind != "one_hp" else 1
        ps[tagged] = 7
        if tag_kind == "three_ps":
            ps[tagged] = rng.choice([7, 3, 11], size=int(tagged.sum()))
        if tag_kind == "split_top":   # two phase sets of (nearly) the same size: the one met first wins a tie
            idx = np.nonzero(tagged)[0]
            ps[idx[::2]] = 9
        if tag_kind == "three_hp":
            idx = np.nonzero(tagged)[0]
            if idx.size:
                hp[idx[-1]] = 3
        some = rng.random(n) < 0.05   # a tag without its partner does not count
        ps[some] = -1
    base = np.zeros((n, S), np.uint8)
    qual = np.zeros((n, S), np.uint8)
    if S and n:
        alleles = np.stack([rng.permutation(BASES)[:2] for _ in range(S)])   # [S, 2]
        base[:] = alleles[np.arange(S)[None, :], hap[:, None]]
        qual[:] = rng.choice([30, 40, 60], size=(n, S))
        if cell_kind in ("noisy", "out_of_range_rows", "gap_rows", "few_real"):
            err = rng.random((n, S)) < 0.08
            base[err] = rng.choice(BASES, size=int(err.sum()))
            base[rng.random((n, S)) < 0.06] = PR.OUT_OF_RANGE
            base[rng.random((n, S)) < 0.06] = PR.GAP
            qual[rng.random((n, S)) < 0.15] = rng.choice([0, 10, 19])
        if cell_kind == "out_of_range_rows":
            base[rng.random(n) < 0.2] = PR.OUT_OF_RANGE
        if cell_kind == "gap_rows":
            base[rng.random(n) < 0.2] = PR.GAP
        if cell_kind == "at_threshold":
            qual[:] = rng.choice([19, 20, 21], size=(n, S))
        if cell_kind == "identical":
            base[:] = base[0]
            qual[:] = 40
        if cell_kind == "few_real":
            base[rng.random(n) < 0.5] = PR.OUT_OF_RANGE
    return dict(cn=cn, w=w, n_alleles=n_alleles, hp=hp, ps=ps, base=base, qual=qual)


def pack(loci, seeds, with_tags=True, with_snvs=True):
    """The loci as the arrays of one call."""
    read_off = np.concatenate(([0], np.cumsum([len(x["cn"]) for x in loci]))).astype(np.int32)
    cat = lambda k, dt: np.concatenate([x[k] for x in loci]).astype(dt) if loci else np.zeros(0, dt)
    out = dict(read_off=read_off, cns=cat("cn", np.int32), weights=cat("w", np.float64),
               n_alleles=np.array([x["n_alleles"] for x in loci], np.int32), seeds=np.asarray(seeds, np.uint64))
    if with_tags:
        out.update(hp=cat("hp", np.int32), ps=cat("ps", np.int32))
    if with_snvs:
        out.update(snv_off=np.concatenate(([0], np.cumsum([x["base"].shape[1] for x in loci]))).astype(np.int32),
                   snv_base=np.concatenate([x["base"].ravel() for x in loci]).astype(np.uint8),
                   snv_qual=np.concatenate([x["qual"].ravel() for x in loci]).astype(np.uint8))
    return out


def corpus(seed: int = 20, n_loci: int = 2000):
    """About n_loci loci over every size, SNV count, tag kind and cell kind, the sizes either side of the LDS / workspace
    cut, one locus of 1 024 reads, and a block of everyday loci (30 reads, 4 SNVs)."""
    rng = np.random.default_rng(seed)
    loci = []
    combos = [(n, S) for n in SIZES for S in SNV_COUNTS]
    i = 0
    while len(loci) < n_loci - 1:
        n, S = combos[i % len(combos)]
        if n == 250 and i >= 4 * len(combos):   # the large ones a few times only
            n = 30
        if S >= 63 and i >= 6 * len(combos):
            S = 4
        tag_kind = TAG_KINDS[(i // 3) % len(TAG_KINDS)] if i % 3 else "none"
        cell_kind = CELL_KINDS[(i // 5) % len(CELL_KINDS)]
        n_alleles = 1 if i % 7 == 3 else 2
        loci.append(make_locus(rng, n, S, n_alleles, tag_kind, cell_kind))
        i += 1
    loci.insert(len(loci) // 2, make_locus(rng, 1024, 5, 2, "none", "noisy"))
    seeds = [AR.locus_seed(seed, t) for t in range(len(loci))]
    return loci, seeds


def restate(loci, seeds, p=AR.Params(), pp=PR.PhaseParams(), tags=True, snvs=True):
    return [PR.call_locus(x["cn"], x["w"], x["n_alleles"], s, x["hp"] if tags else None, x["ps"] if tags else None,
                          x["base"] if snvs else None, x["qual"] if snvs else None, p, pp) for x, s in zip(loci, seeds)]


def _locus(cn, hp=None, ps=None, cells=None, quals=None, n_alleles=2):
    """A hand-written locus: cells is one string per read (one character per SNV), quals one list per read or one number."""
    n = len(cn)
    S = len(cells[0]) if cells else 0
    base = np.array([list(r.encode()) for r in cells], np.uint8).reshape(n, S) if cells else np.zeros((n, 0), np.uint8)
    qual = np.full((n, S), 40, np.uint8)
    if quals is not None:
        qual[:] = np.asarray(quals, np.uint8)
    return dict(cn=np.asarray(cn, np.int32), w=np.ones(n), n_alleles=n_alleles,
                hp=np.asarray(hp if hp is not None else [-1] * n, np.int32),
                ps=np.asarray(ps if ps is not None else [-1] * n, np.int32), base=base, qual=qual)


def hand_vectors():
    """(name, locus, tags given, SNVs given, expected fields).  Copy numbers of the two haplotypes are far apart, so the means
    of the groups are distinct."""
    X, Y = [10, 10, 11, 10], [20, 21, 20, 20]
    v = []
    v.append(("no_tags", _locus(X + Y), False, False, dict(status=PR.NOT_PHASED, method=PR.ASSIGN_NONE, reason=PR.REASON_NO_TAGS)))
    v.append(("too_few_reads", _locus([10, 11, 12], hp=[1, 2, 1], ps=[4, 4, 4]), True, False,
              dict(status=PR.TOO_FEW, method=PR.ASSIGN_NONE, reason=PR.REASON_NONE)))
    # seven tagged reads: one short of min_hp_read_coverage
    v.append(("tag_thresholds", _locus(X + Y, hp=[1, 1, 1, 1, 2, 2, 2, -1], ps=[4] * 8), True, False,
              dict(status=PR.NOT_PHASED, reason=PR.REASON_TAG_THRESHOLDS)))
    v.append(("three_hp_values", _locus(X + Y + X, hp=[1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3], ps=[4] * 12), True, False,
              dict(status=PR.NOT_PHASED, reason=PR.REASON_TAG_THRESHOLDS)))
    v.append(("hp_group_of_one", _locus(X + X + [20, 10], hp=[1] * 8 + [2, 1], ps=[4] * 10), True, False,
              dict(status=PR.NOT_PHASED, reason=PR.REASON_GROUP_NOT_CALLED)))
    # peaks stay in ascending HP order: HP 1 carries the LARGER copy numbers
    v.append(("hp_order_kept", _locus(Y + X, hp=[1] * 4 + [2] * 4, ps=[4] * 8), True, False,
              dict(status=PR.CALLED, method=PR.ASSIGN_HP, ps=4, call=[20, 10], peak_n_reads=[4, 4], modal_n=2,
                   read_peak=[0, 0, 0, 0, 1, 1, 1, 1], weights=[0.5, 0.5])))
    # phase sets 9 and 5 carry eight reads each; 9 is met first
    v.append(("top_phase_set_tie", _locus(X + Y + X + Y, hp=[1] * 4 + [2] * 4 + [1] * 4 + [2] * 4, ps=[9, 5] * 8), True, False,
              dict(status=PR.CALLED, method=PR.ASSIGN_HP, ps=9, peak_n_reads=[4, 4],
                   read_peak=[0, -1, 0, -1, 1, -1, 1, -1, 0, -1, 0, -1, 1, -1, 1, -1])))
    v.append(("one_allele_hp", _locus(X + X, hp=[1] * 8, ps=[2] * 8, n_alleles=1), True, False,
              dict(status=PR.CALLED, method=PR.ASSIGN_HP, ps=2, modal_n=1, call=[10, -1], peak_n_reads=[8, 0], weights=[1.0, np.nan])))
    # ten reads, three of them with a real base
    v.append(("few_snv_reads", _locus(X + Y + [10, 20], cells=["AT", "AT", "TA"] + ["--"] * 7), False, True,
              dict(status=PR.NOT_PHASED, reason=PR.REASON_FEW_SNV_READS)))
    # one SNV, so copy numbers join the distance; both clusters carry 'A'
    v.append(("no_snv_survives", _locus(X + Y, cells=["A"] * 8), False, True,
              dict(status=PR.NOT_PHASED, method=PR.ASSIGN_NONE, reason=PR.REASON_NO_SNV_CALLED, snv_status=[PR.SNV_CROSS_TALK])))
    v.append(("snv_cluster_of_one", _locus(X + Y, cells=["AA"] * 7 + ["TT"]), False, True,
              dict(status=PR.NOT_PHASED, reason=PR.REASON_GROUP_NOT_CALLED)))
    # SNVs 0 and 1 separate the haplotypes; 2: most-common tie (C met first); 3: '-' most common; 4: only '-';
    # 5: cross-talk; 6: the same byte in both peaks, which the cross-talk test meets first (a byte that both peaks call is in
    # each at more than half its share of the other, so the reference's degenerate-call skip behind it is never reached);
    # 7: no cell of the first peak counts (quality 10)
    cells = ["AACA-ACA", "AAA--ACC", "AAA--GCG", "AACA-GCT",
             "TTGG-GCA", "TTGG-GCA", "TTGG-ACA", "TTGG-ACA"]
    quals = [[40] * 7 + [10]] * 4 + [[40] * 8] * 4
    v.append(("snv_calls", _locus(X + Y, cells=cells, quals=quals), False, True,
              dict(status=PR.CALLED, method=PR.ASSIGN_SNV, ps=-1, call=[10, 20], peak_n_reads=[4, 4], read_peak=[0] * 4 + [1] * 4,
                   snv_status=[PR.SNV_CALLED, PR.SNV_CALLED, PR.SNV_CALLED, PR.SNV_CALLED, PR.SNV_ONLY_OUT_OF_RANGE,
                               PR.SNV_CROSS_TALK, PR.SNV_CROSS_TALK, PR.SNV_ZERO_TOTAL],
                   snv_call=[list(b"AT"), list(b"AT"), list(b"CG"), list(b"AG"), [0, 0], [0, 0], [0, 0], [0, 0]],
                   snv_rcs=[[4, 4], [4, 4], [2, 4], [2, 4], [0, 0], [0, 0], [0, 0], [0, 0]])))
    # the groups come out of the clustering as (large, small): the peaks are re-ordered by mean
    v.append(("snv_peaks_sorted", _locus(Y + X, cells=["TT"] * 4 + ["AA"] * 4), False, True,
              dict(status=PR.CALLED, method=PR.ASSIGN_SNV, call=[10, 20], read_peak=[1] * 4 + [0] * 4, snv_call=[list(b"AT"), list(b"AT")])))
    # every read has one real base only: copy numbers join the distance
    v.append(("snv_and_dist", _locus(X + Y, cells=["A-"] * 4 + ["T-"] * 4), False, True,
              dict(status=PR.CALLED, method=PR.ASSIGN_SNV_DIST, call=[10, 20], snv_status=[PR.SNV_CALLED, PR.SNV_ONLY_OUT_OF_RANGE])))
    return v


def check_expected(name, got: dict, exp: dict):
    for k, want in exp.items():
        have = np.asarray(got[k])
        want = np.asarray(want)
        assert have.shape == want.shape, (name, k, have, want)
        if want.dtype.kind == "f":
            assert np.array_equal(have, want, equal_nan=True), (name, k, have, want)
        else:
            assert np.array_equal(have, want), (name, k, have, want)
