#!/usr/bin/env python3
"""Cost model of k_dp_band's chunks on the bench's own input (no GPU needed): what an order of the band items, a band geometry
or a step form is worth in instructions, before anything is built.

A wave runs the 8 (4) items of a chunk in lock step.  A pass costs max(rows) + G - 1 steps (rounded up to a pair); every step
costs its D cells (two instructions each), D / 4 v_perm and D / 4 v_alignbyte, four for edges and addresses and, unless the
step is test-free, one for the fork-row test; the fork block (LDS reads, D adds, D / 2 v_max3, an LDS atomic: D + D / 2 + 8)
runs at every step from the earliest fork row of any group of the wave to the latest; a chunk costs 1 600 instructions of
staging and search.  The fork-row test is priced at ONE instruction per step (its v_cmp; the s_and_saveexec and the branch behind
it are scalar and not counted), so a test-free step is discounted by one: that price was never set against a measured
instruction count of the test-free steps, which may come out differently (profiles/r15_band_order.txt has the measurement).
Calibration (round 4, BASELINE config 2 at 10 000 loci): 20 410 scored reads and 536 M wave-instructions per launch measured,
20 410 items and ~500 M modelled — good for ratios.

The model follows the library: the dedupe (byte-identical reads of a locus), k_plan's window rule at +-6 (+-8 for motifs of
1-2 bases), band_geometry with BandTune's inner span, k_plan's block-local (class, bin of the rows, read) order.

Parameters of the block-local order: the sort scope (reads one block of k_plan orders; 0: the whole call), the row bins of its
counting sort (rows >> shift per layout class; None: exact rows) and the largest window of layout class 0 (448: the LDS layout
of rounds 4-18; 512 since round 19: what a band of 128 diagonals can hold).  The last table sweeps them.

    python tools/band_order_model.py [n_loci]        # default 1000 loci of config 2; figures scale linearly
"""
import os
import sys
from collections import Counter

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from strkit_amd.synth import make_config

MAX_DB = (512, 1024, 4096, 12288)
MAX_COL = (320, 512, 1024, 1536)
ROW_SLACK, NARROW_SLACK, CHUNK_COST = 96, 22, 1600


def band_wd(c):
    return (8 << (c & 3)) * (12 if c >= 4 else 16)


BIN_SHIFT = (2, 3, 6, 7)   # strk_plan_order.h: plan_bin_shift per layout class
SCOPE = 2048               # strk_plan_order.h: kPlanScope (calls of 32 768 reads and more; smaller ones: 512)


def band_class(nfl, ntr, nfr, m, lo, n, span_w, max_db0=None):
    """strk_search.h: band_geometry's class (-1: not eligible); span_w = 64 is the whole table."""
    max_db = (max_db0 or MAX_DB[0],) + MAX_DB[1:]
    ndb = nfl + ntr + nfr
    t = max((n - 1) // 2 - span_w, 0)
    c_lo, c_hi = lo + t, lo + n - 1 - t
    span_lo, span_hi = min(ntr - c_hi * m, 0), max(ntr - c_lo * m, 0)
    smin = max(ndb >> 5, 12)
    rows = nfl + (lo + n - 1) * m
    for k in range(8):
        c = (k >> 1) + (0 if k & 1 else 4)
        w = band_wd(c)
        slack = NARROW_SLACK if (c >= 4 and smin < NARROW_SLACK) else smin
        if span_hi - span_lo + 1 + 2 * slack > w:
            continue
        if ndb > max_db[c & 3] or (n - 1) * m + w > MAX_COL[c & 3] or rows > max_db[c & 3] + ROW_SLACK:
            continue
        if (c & 3) >= 1 and w * 5 > (ndb + 1) * 4:
            return -1
        return c
    return -1


def items_of(b):
    """(read, locus, nfl, ntr, nfr, m, lo, n) of every read that is the first of its copies."""
    out, dups = [], 0
    for l in range(b.n_loci):
        r0, r1 = int(b.read_off[l]), int(b.read_off[l + 1])
        m = int(b.motif_off[l + 1] - b.motif_off[l])
        seen = set()
        for r in range(r0, r1):
            key = (bytes(b.seqs[int(b.seq_off[r]):int(b.seq_off[r + 1])]), int(b.nfl[r]), int(b.ntr[r]), int(b.est_cn[r]))
            if key in seen:
                dups += 1
                continue
            seen.add(key)
            est = int(b.est_cn[r])
            w = (8 if m <= 2 else 6) + min(max(est, 0) >> 7, 7)
            lo = max(est - w, 0)
            out.append((r, l, int(b.nfl[r]), int(b.ntr[r]), int(b.nfr[r]), m, lo, max(est + w, lo) - lo + 1))
    return out, dups


ORDERS = {   # per class: the key the items of a class are listed by (None: k_plan's order inside each block of `scope` reads)
    "block-local (today)": None,          # (scope, bins, class-0 limit: model()'s parameters)
    "call-wide by rows": lambda x: (x[1],),
    "buckets of 4 rows": lambda x: (x[1] >> 2, x[5]),
    "buckets of 8 rows": lambda x: (x[1] >> 3, x[5]),
    "buckets of 16 rows": lambda x: (x[1] >> 4, x[5]),
}


def model(items, span_w, order, test_free, scope=SCOPE, bins=BIN_SHIFT, max_db0=None):
    recs = []   # (class, rows, fork0, nfr, m, read)
    for (r, l, nfl, ntr, nfr, m, lo, n) in items:
        c = band_class(nfl, ntr, nfr, m, lo, n, span_w if m <= 6 else 64, max_db0)
        if c >= 0 and c & 3 < 2:   # k_dp_band's classes
            recs.append((c, nfl + (lo + n - 1) * m, nfl + lo * m, nfr, m, r))
    per = {}
    if ORDERS[order] is None:
        blocks = {}
        for x in recs:
            blocks.setdefault((x[5] // scope if scope else 0, x[0]), []).append(x)
        for (_, c), v in sorted(blocks.items()):
            sh = bins[c & 3] if bins else 0
            per.setdefault(c, []).extend(sorted(v, key=lambda x: (x[1] >> sh, x[5])))
    else:
        for x in recs:
            per.setdefault(x[0], []).append(x)
        for v in per.values():
            v.sort(key=ORDERS[order])
    instr = steps = fork_steps = 0
    for c, v in per.items():
        D, G = (12 if c >= 4 else 16), 8 << (c & 3)
        step_cost, fork_cost = 2 * D + 2 * (D // 4) + 4 + 1, D + D // 2 + 8
        for i in range(0, len(v), 64 // G):
            ch = v[i:i + 64 // G]
            t_fwd = (max(x[1] for x in ch) + G) & ~1
            t_bwd = (max(x[3] for x in ch) + G) & ~1
            f0, f1 = min(x[2] - 1 for x in ch), max(x[1] - 1 + G - 1 for x in ch)
            cost = (t_fwd + t_bwd) * step_cost + (f1 - f0 + 1) * fork_cost + CHUNK_COST
            if test_free:   # no test in front of the first fork row (forward) and of the first last row (backward)
                cost -= (f0 & ~1) + ((min(x[3] for x in ch) - 1) & ~1)
            instr += cost
            steps += t_fwd + t_bwd
            fork_steps += f1 - f0 + 1
    return Counter(x[0] for x in recs), instr, steps, fork_steps


def main():
    n_loci = int(sys.argv[1]) if len(sys.argv) > 1 else 1000
    b = make_config(2, n_loci=n_loci)
    items, dups = items_of(b)
    print(f"config 2, {n_loci} loci: {b.n_reads} reads, {dups} copies, {len(items)} items")
    base = None
    for span_w in (64, 4):
        for test_free in (False, True):
            print(f"-- band around {'the whole table' if span_w == 64 else 'the inner +-%d sizes (motifs <= 6)' % span_w}, "
                  f"{'test-free steps in front of the first event' if test_free else 'a fork-row test at every step'}")
            for order in ORDERS:
                classes, instr, steps, fork_steps = model(items, span_w, order, test_free)
                base = base or instr
                cl = " ".join(f"{(8 << (c & 3))}x{12 if c >= 4 else 16}:{k}" for c, k in sorted(classes.items()))
                print(f"   {order:22s} items {cl}   wave-steps {steps:9d}   fork-block steps {fork_steps:8d}   "
                      f"instructions {instr / 1e6:7.2f} M   x {instr / base:.3f}")
    # the block-local order by sort scope, row bins and class-0 window limit (whole table, test-free steps); 1.000 = 256 reads,
    # exact rows, 448 bases: the tree of rounds 15-18
    ref = model(items, 64, "block-local (today)", True, 256, None, 448)[1]
    print("-- block-local order: sort scope x row bins x largest class-0 window (band around the whole table, test-free steps)")
    print(f"   {'scope (reads)':14s} {'exact rows, 448':>16s} {'bins, 448':>10s} {'exact rows, 512':>16s} {'bins, 512':>10s}")
    for scope in (256, 1024, 2048, 4096, 0):
        row = [model(items, 64, "block-local (today)", True, scope, b, db0)[1] / ref for db0 in (448, 512) for b in (None, BIN_SHIFT)]
        print(f"   {str(scope) if scope else 'whole call':14s} {row[0]:16.3f} {row[1]:10.3f} {row[2]:16.3f} {row[3]:10.3f}")
    over = [x for x in items if x[2] + x[3] + x[4] > 448]
    print(f"   items with windows over 448 bases: {len(over)} of {len(items)} ({sum(1 for x in over if x[2] + x[3] + x[4] > 512)} over 512)")


if __name__ == "__main__":
    main()
