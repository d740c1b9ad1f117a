"""Seam corpus of the exact scoring path: k_plan's classify, then one of the 17 classes of k_dp_all, k_dp_ref, k_dp_long or
k_dp_generic.  Deterministic (fixed seeds for the noise) and built from score_constants() and strk_classify, so that it
follows the kernels as built.  A case is one read of a locus of its own: a name, the motif and (fl, tr, fr), the candidate
window [lo, lo + n), the list it claims for every chunk of kTableMax candidates (`route`), and the edge it sits on with
the side of that edge (`edge`, `side`).  Most edges hold two reads, a clean tract and a noisy one (ACGT plus wildcards).
Families a-j: see DESIGN.md, "Exact path: seam corpus".  CPU half: test_exact_cases.py, GPU half: test_gpu_exact_cases.py.
"""
from __future__ import annotations

import functools
from concurrent.futures import ThreadPoolExecutor
from dataclasses import dataclass

import numpy as np

import oracle
from helpers import ALPHA_WC, hifi_motif, noisy_tract, rand_seq
from oracle import py_restatement as py
from strkit_amd.batch import classify, score_constants
from strkit_amd.synth import LocusBatch

K = score_constants()
CAPS, LANES = K["caps"], K["lanes"]
NC, TM, RS, T = K["kNumClasses"], K["kTableMax"], K["kRowSlack"], K["kLongTile"]
FF, LF, MM, SG = K["kFastFlankMax"], K["kLongFlankMax"], K["kMotifMax"], K["kStairMinG"]
LONG, GENERIC = NC, NC + 1
LANE_COUNTS = sorted(set(LANES))
FIRST_OF = {g: LANES.index(g) for g in LANE_COUNTS}                  # first and last class of each lane count
LAST_OF = {g: NC - 1 - LANES[::-1].index(g) for g in LANE_COUNTS}
CELL_CAP = 4 * 10 ** 9


def py_classify(nfl, ntr, nfr, m, lo, n, force_generic=False, ref_mode=False):
    """classify() of strk_kernels.h, restated: a change to it has to be made twice."""
    slots, rows = nfl + ntr + nfr + 1, nfl + (lo + n - 1) * m
    if force_generic or nfl < 1 or (nfr < 1 and not ref_mode) or n > TM or m > MM:
        return GENERIC
    for c in range(NC - 1 if ref_mode else 0, NC):
        if slots <= CAPS[c] and rows <= CAPS[c] + RS and (nfr <= FF or ref_mode):
            return c
    tiled = not ref_mode and nfl <= LF and nfr <= LF and slots <= T * K["kLongMaxTiles"] and rows <= 1 << 20
    return LONG if tiled else GENERIC


@dataclass(frozen=True)
class Case:
    name: str
    family: str
    edge: str          # the seam
    side: str          # which side of it (or which of its listed values)
    motif: str
    fl: str
    tr: str
    fr: str
    lo: int
    n: int
    route: tuple       # claimed list of every chunk of kTableMax candidates
    handover: bool = False   # more than eight symbols: every chunk is also counted in the generic list
    ref: bool = False        # reference side (score_ref_table)

    @property
    def ndb(self):
        return len(self.fl) + len(self.tr) + len(self.fr)

    def chunks(self):
        return [(k0, min(TM, self.n - k0)) for k0 in range(0, self.n, TM)]

    def classified(self, force_generic=False):
        return tuple(classify(len(self.fl), len(self.tr), len(self.fr), len(self.motif), self.lo + k0, nn, force_generic, self.ref)
                     for k0, nn in self.chunks())

    def rows(self, k0=0):
        return len(self.fl) + (self.lo + min(self.n, k0 + TM) - 1) * len(self.motif)

    def cells(self):
        """DP cells the oracle spends on the case at one end-flag setting: |db| x candidate length, per candidate."""
        tail = 0 if self.ref else len(self.fr)
        return sum(self.ndb * (len(self.fl) + (self.lo + k) * len(self.motif) + tail) for k in range(self.n))


def _factor(p):
    """(m, lo) with m * lo == p, the motif at most 12 bases where p allows it."""
    for m in range(12, 1, -1):
        if p % m == 0:
            return m, p // m
    return p, 1


class _Builder:
    def __init__(self):
        self.rng = np.random.default_rng(2501)
        self.cases: list[Case] = []
        self.calls: dict[str, list[str]] = {}

    def motif(self, m):
        return hifi_motif(self.rng, m) if m > 1 else "ACGT"[int(self.rng.integers(4))]

    def tract(self, motif, ntr, noisy):
        """Exactly ntr bases: the motif repeated and cut; noisy: edits from ACGT plus wildcards, then cut or padded to length."""
        m = len(motif)
        clean = (motif * (ntr // m + 2))
        if not noisy or ntr == 0:
            return clean[:ntr]
        tr = (noisy_tract(self.rng, motif, ntr // m + 1, 2 + ntr // 40, ALPHA_WC) + clean)[:ntr]
        return tr[:ntr // 2] + "X" + tr[ntr // 2 + 1:]             # (at least one wildcard, whatever the edits drew)

    def flank(self, n, noisy):
        s = rand_seq(self.rng, n)
        if noisy and n > 4:
            i = int(self.rng.integers(1, n - 1))
            s = s[:i] + "N" + s[i + 1:]
        return s

    def add(self, family, name, edge, side, motif, fl, tr, fr, lo, n, route=None, handover=False, ref=False):
        if route is None:
            route = tuple(py_classify(len(fl), len(tr), len(fr), len(motif), lo + k0, min(TM, n - k0), False, ref) for k0 in range(0, n, TM))
        elif isinstance(route, int):
            route = (route,) * ((n + TM - 1) // TM)
        assert name not in {c.name for c in self.cases}, name
        self.cases.append(Case(name, family, edge, side, motif, fl, tr, fr, int(lo), int(n), tuple(route), handover, ref))
        return name

    def pair(self, family, name, edge, side, m, nfl, ntr, nfr, lo, n, route=None, motif=None, ref=False):
        """The clean and the noisy read of an edge; lo < 0: that many sizes below the tract's own copy number."""
        motif = motif or self.motif(m)
        if lo < 0:
            lo = max(0, ntr // len(motif) + lo)
        return [self.add(family, f"{name}/{kind}", edge, side, motif, self.flank(nfl, noisy), self.tract(motif, ntr, noisy), self.flank(nfr, noisy),
                         lo, n, route, ref=ref) for kind, noisy in (("clean", False), ("noisy", True))]


def _fast_for(slots):
    return next(c for c in range(NC) if slots <= CAPS[c])


def _family_a(b):
    """Capacity edges: |db| + 1 == capacity stays, + 1 moves on (the last class to the tiled kernel); rows stay small."""
    for c in range(NC):
        for side, d in (("in", 0), ("out", 1)):
            f = 20 if CAPS[c] < 400 else 60
            b.pair("a", f"a/cap[{c}]/{side}", f"cap[{c}]", side, 1 + c % 6, f, CAPS[c] - 1 + d - 2 * f, f, -2, 5,
                   route=c if d == 0 else (c + 1 if c + 1 < NC else LONG))


def _family_b(b):
    """Row edges: rows == capacity + kRowSlack and + 1 on a short window, by a window far above the tract."""
    for g in LANE_COUNTS:
        for c in sorted({FIRST_OF[g], LAST_OF[g]}):
            for side, d in (("in", 0), ("out", 1)):
                m, n = 1 + c % 2, 3
                rows = CAPS[c] + RS + d
                nfl = 20 + (rows - 20) % m
                lo = (rows - nfl) // m - (n - 1)
                assert nfl + (lo + n - 1) * m == rows
                b.pair("b", f"b/rows[{c}]/{side}", f"rows[{c}]", side, m, nfl, 30, 20, lo, n, route=c if d == 0 else (c + 1 if c + 1 < NC else LONG))


def _family_c(b):
    """Flank edges: the right flank at the fast and the tiled kernel's limits, the left flank at the tiled kernel's, and
    empty flanks (generic kernel) around its 64-column blocks."""
    for nfr in (FF, FF + 1, LF, LF + 1):
        b.pair("c", f"c/nfr{nfr}", "nfr", str(nfr), 3, 30, 60, nfr, -2, 5,
               route=_fast_for(30 + 60 + nfr + 1) if nfr <= FF else (LONG if nfr <= LF else GENERIC))
    for nfl in (1, LF, LF + 1):
        b.pair("c", f"c/nfl{nfl}", "nfl", str(nfl), 4, nfl, T + 8 - nfl, 100, -2, 3, route=LONG if nfl <= LF else GENERIC)
    for ndb in (63, 64, 65, 128, 129, T + 9):
        for which, nfl, nfr in (("nfl0", 0, 20), ("nfr0", 20, 0), ("both0", 0, 0)):
            b.pair("c", f"c/{which}/ndb{ndb}", which, str(ndb), 3, nfl, ndb - nfl - nfr, nfr, -2, 4, route=GENERIC)


def _family_d(b):
    """Motif edges: kMotifMax in the narrowest and the widest class, the lane counts, motifs longer than the flank / the tract."""
    for m in (MM - 1, MM, MM + 1):
        # class 0 holds no whole copy of such a motif: the tract is the motif's END, so that its last bases are on the best path
        motif = b.motif(m)
        tr = motif[-80:]
        for kind, noisy, t in (("clean", False, tr), ("noisy", True, tr[:40] + "X" + tr[42:] + "N")):
            b.add("d", f"d/m{m}/c0/{kind}", "motif[0]", str(m), motif, b.flank(20, noisy), t, b.flank(20, noisy), 0, 2, route=0 if m <= MM else GENERIC)
        b.pair("d", f"d/m{m}/c{NC - 1}", f"motif[{NC - 1}]", str(m), m, 70, 5 * m, 70, 4, 4, route=NC - 1 if m <= MM else GENERIC)
    for g in LANE_COUNTS:
        c = FIRST_OF[g]
        for m in (g - 1, g, g + 1):
            b.pair("d", f"d/lanes{g}/m{m}", f"motif-lanes[{g}]", str(m - g), m, 30, CAPS[c] - 61, 30, -1, 3, route=c)
    b.pair("d", "d/m-over-nfl", "motif-over-nfl", "m7-nfl3", 7, 3, 70, 30, -2, 5)
    b.pair("d", "d/m-over-tract", "motif-over-tract", "m9-ntr4", 9, 25, 4, 25, 0, 3)


def _family_e(b):
    """Staircase switch: lo * m at G - 2, G - 1, G in classes that fold fork rows along a staircase; two calls in which one
    item below the threshold shares its wave with items above it."""
    names = {}
    for g in [x for x in LANE_COUNTS if x >= SG]:
        c = FIRST_OF[g]
        for side, p in (("G-2", g - 2), ("G-1", g - 1), ("G", g)):
            m, lo = _factor(p)
            names[g, side] = b.pair("e", f"e/stair[{c}]/{side}", f"stair[{g}]", side, m, 40, CAPS[c] - 81, 40, lo, 4, route=c)
            # ... and with the left flank reaching into the group's last lane, whose step of the staircase lies G - 1 rows above
            # the fork row: only there does the best path cross the rows that must all be motif rows for the fold to be exact
            cl = CAPS[c] // g
            motif = b.motif(m)
            fl = b.flank((g - 1) * cl + 3, False)
            if fl[-1] == motif[m - 1 - (g - 2) % m]:                # the flank's last base is not the motif's continuation
                fl = fl[:-1] + next(ch for ch in "ACGT" if ch not in (fl[-1], fl[-2]))
            for kind, noisy in (("clean", False), ("noisy", True)):
                b.add("e", f"e/stair[{c}]/{side}/corner/{kind}", f"stair-corner[{g}]", side, motif, fl, b.tract(motif, cl - 10, noisy),
                      b.flank(6, False), lo, 4, route=c)
    if (32, "G") in names:
        b.calls["e/ballot32"] = [names[32, "G"][0], names[32, "G-2"][1]]
    if (16, "G") in names:
        b.calls["e/ballot16"] = names[16, "G"] + [names[16, "G-1"][1], names[16, "G-2"][0]]


def _family_f(b):
    """Group occupancy: partly filled waves of an 8-, a 16- and a 32-lane class."""
    for g, c, counts in ((8, 2, (1, 7, 8, 9)), (16, FIRST_OF[16], (1, 4, 5)), (32, FIRST_OF[32], (1, 2, 3))):
        assert LANES[c] == g
        names = []
        for k in range(max(counts)):
            motif = b.motif(2 + k % 4)
            names.append(b.add("f", f"f/lanes{g}/{k}", f"occupancy[{g}]", str(k), motif, b.flank(30 + k, True), b.tract(motif, CAPS[c] - 75 - k, True),
                               b.flank(30, True), max(0, (CAPS[c] - 75 - k) // len(motif) - 3), 6, route=c))
        for k in counts:
            b.calls[f"f/lanes{g}x{k}"] = names[:k]


def _family_g(b):
    """Table chunks: n around kTableMax and twice that on a fast class and on the tiled kernel, degenerate windows, and reads
    whose two chunks classify differently."""
    for n in (1, TM - 1, TM, TM + 1, 2 * TM, 2 * TM + 1):
        b.pair("g", f"g/fast/n{n}", "n-fast", str(n), 3, 40, 150, 40, 20, n, route=_fast_for(231))
        b.pair("g", f"g/long/n{n}", "n-long", str(n), 5, 70, T - 120, 70, (T - 120) // 5 - 40, n, route=LONG)
    b.pair("g", "g/lo0-n1", "degenerate", "lo0-n1", 3, 25, 30, 25, 0, 1)
    b.pair("g", "g/ntr0", "degenerate", "ntr0", 3, 20, 0, 20, 0, 4)
    lo = (CAPS[NC - 1] + RS - 22) // 10 - (TM - 1) - 1             # chunk 0 under the last class's row limit, chunk 1 over it
    b.pair("g", "g/split/fast-long", "split", "fast-long", 10, 22, 60, 30, lo, 2 * TM, route=(NC - 1, LONG))
    lo = CAPS[2] + RS - 20 - (TM - 1) - 5
    b.pair("g", "g/split/class-next", "split", "class-next", 1, 20, 40, 20, lo, 2 * TM, route=(2, 3))


def _family_h(b):
    """Tiles of k_dp_long: the tile count, one tile reached by rows or by the right flank alone, the 64-step blocks of the
    forward pass, fork rows on every step of a block, edits on the seam between two tiles, candidates far from the window."""
    for side, slots, route in (("T", T, NC - 1), ("T+1", T + 1, LONG), ("2T", 2 * T, LONG), ("2T+1", 2 * T + 1, LONG)):
        b.pair("h", f"h/slots/{side}", "tiles", side, 4, 70, slots - 1 - 140, 70, -2, 5, route=route)
    b.pair("h", "h/nt1/by-rows", "nt1", "rows", 1, 30, 40, 30, CAPS[NC - 1] + RS + 1 - 30 - 2, 3, route=LONG)
    b.pair("h", "h/nt1/by-nfr", "nt1", "nfr", 3, 30, 60, FF + 1, -2, 5, route=LONG)
    for k in (0, 1, 2):                                            # rowsP = nfl + lo + n - 1 with m == 1
        b.pair("h", f"h/rowsP-mod64/{k}", "rowsP-mod64", str(k), 1, 70, T + 60, 70, 30 * 64 + k - 70 - 4, 5, route=LONG)
    for k in (0, 32):
        b.pair("h", f"h/fork-step/{k}", "fork-step", str(k), 1, 70, T + 60, 70, 29 * 64 + k - 70, TM, route=LONG)
    motif = "ACGT"                                                 # (every base differs from the one three places on)
    fl, fr, tr = b.flank(70, False), b.flank(70, False), b.tract(motif, 2 * T - 400, False)
    for col in (T - 1, T, T + 1):
        p = col - len(fl)                                          # the edit's place in the tract: window column `col`
        sub = "ACGT"[("ACGT".index(tr[p]) + 1) % 4]
        for kind, t2 in (("sub", tr[:p] + sub + tr[p + 1:]), ("del3", tr[:p] + tr[p + 3:]), ("ins3", tr[:p] + 3 * sub + tr[p:])):
            b.add("h", f"h/seam-edit/{kind}@{col}", "seam-edit", f"{kind}@{col - T:+d}", motif, fl, t2, fr, len(tr) // 4 - 2, 5, route=LONG)
    # With one end of the window free the best path can cross the column between two tiles in the FIRST rows of a pass, where the
    # boundary column is handed over apart from the 64-row blocks.  fwd: the window holds a second copy of the left flank that
    # begins d columns from the tile edge, so with the window's begin free the candidate is the window's end, row 0 at that column.
    # bwd: a copy of the right flank ends d columns from the tile edge, so with the window's end free the candidate is the
    # window's beginning and its last row (the backward pass's first) lies there.
    motif, fl, fr = b.motif(3), b.flank(70, False), b.flank(70, False)
    for d in (-4, -3, -2, -1, 0):                                  # (d = -2: row 1 of the forward pass's boundary column)
        b.add("h", f"h/edge-row/fwd{d:+d}", "edge-row-fwd", f"{d:+d}", motif, fl, b.tract(motif, T + d - 70, False) + fl + motif * 80, fr, 78, 5, route=LONG)
    m = 4 if (T - 140) % 4 == 0 else 1
    motif = b.motif(m)
    for d in (-3, -2, -1, 0, 1):                                   # (d = -1: row 1 of the backward pass's)
        fl = b.flank(70 + d + 2, False)
        b.add("h", f"h/edge-row/bwd{d:+d}", "edge-row-bwd", f"{d:+d}", motif, fl, motif * ((T - 140) // m) + fr + motif * (400 // m), fr,
              (T - 140) // m - 2, 5, route=LONG)
    ntr = T + 200
    b.pair("h", "h/cand/short", "cand-length", "quarter", 4, 70, ntr, 70, (ntr + 140) // 16 - 20, 5, route=LONG)
    b.pair("h", "h/cand/long", "cand-length", "triple", 4, 70, ntr, 70, 3 * (ntr + 140) // 4 - 20, 5, route=LONG)


def _family_i(b):
    """Symbols: exactly eight distinct symbols stay, a ninth in the last base of the window hands the item to the generic
    kernel in mid-kernel (fast class and two-tile window)."""
    for where, ntr, route in (("fast", 150, _fast_for(231)), ("tiled", T + 300, LONG)):
        motif = b.motif(3)
        fl = "ACGTRYSW" + rand_seq(b.rng, 32)                      # A C G T R Y S W: eight symbols
        tr = b.tract(motif, ntr, False)
        fr = rand_seq(b.rng, 39)
        b.add("i", f"i/{where}/8", f"symbols-{where}", "8", motif, fl, tr, fr + "W", ntr // 3 - 2, 5, route=route)
        b.add("i", f"i/{where}/9", f"symbols-{where}", "9", motif, fl, tr, fr + "K", ntr // 3 - 2, 5, route=route, handover=True)


def ref_last_row(db, cand):
    """The last row of the reference-side DP, row by row in numpy: H(|cand|, j), j = 1 .. |db|, of the candidate against
    db[:j] with both begins fixed and linear gaps (the row whose maximum and first column strk_score_ref_table returns)."""
    M = np.array(py.dna_matrix, np.int64)
    a, d = py._enc(cand), np.array(py._enc(db), np.int64)
    g, idx = py.indel_penalty, np.arange(len(d) + 1, dtype=np.int64)
    H = -g * idx
    for i, sym in enumerate(a, 1):
        t = np.empty_like(H)
        t[0] = -g * i
        t[1:] = np.maximum(H[:-1] + M[sym][d], H[1:] - g)
        H = np.maximum.accumulate(t + g * idx) - g * idx
    return H[1:]


def tie_columns(c: Case, last_column=False):
    """Per candidate of a reference-side case: in how many columns the last DP row holds its maximum (last_column: whether
    the last column is one of them)."""
    out = []
    for k in range(c.n):
        row = ref_last_row(c.fl + c.tr + c.fr, c.fl + c.motif * (c.lo + k))
        out.append(bool(row[-1] == row.max()) if last_column else int((row == row.max()).sum()))
    return out


def _family_j(b):
    """Reference side (one class, then the generic kernel): its capacity and row edges, and small windows in which the last
    DP row's maximum lies in two or more columns (the end-column rule)."""
    last = NC - 1
    for side, d in (("in", 0), ("out", 1)):
        b.pair("j", f"j/cap/{side}", "ref-cap", side, 3, 70, CAPS[last] - 1 + d - 140, 70, -2, 5, route=last if d == 0 else GENERIC, ref=True)
        b.pair("j", f"j/rows/{side}", "ref-rows", side, 1, 30, 60, 30, CAPS[last] + RS + d - 30 - 2, 3, route=last if d == 0 else GENERIC, ref=True)
    rng, found = np.random.default_rng(2502), 0
    for _ in range(400):
        motif = rand_seq(rng, int(rng.integers(1, 5)))
        cn = int(rng.integers(3, 12))
        tr = noisy_tract(rng, motif, cn, int(rng.integers(1, 4)), ALPHA_WC)
        c = Case(f"j/tie/{found}", "j", "ref-tie", str(found), motif, rand_seq(rng, int(rng.integers(8, 30))), tr,
                 noisy_tract(rng, motif, int(rng.integers(0, 3)), 1, ALPHA_WC) + rand_seq(rng, int(rng.integers(5, 30))), max(0, cn - 2), 5, (last,), ref=True)
        if c.ndb <= 200 and max(tie_columns(c)) >= 2:
            b.cases.append(c)
            found += 1
            if found == 8:
                break
    found = 0
    for _ in range(4000):                                          # ... and ties between the last column and an earlier one
        motif = rand_seq(rng, int(rng.integers(1, 5)))
        cn = int(rng.integers(3, 10))
        c = Case(f"j/tie-last/{found}", "j", "ref-tie-last", str(found), motif, rand_seq(rng, int(rng.integers(8, 20))),
                 noisy_tract(rng, motif, cn, int(rng.integers(1, 4)), ALPHA_WC), noisy_tract(rng, motif, 1, 1, ALPHA_WC)[:int(rng.integers(0, 3))],
                 max(0, cn - 2), 5, (last,), ref=True)
        if any(x >= 2 and at_end for x, at_end in zip(tie_columns(c), tie_columns(c, last_column=True))):
            b.cases.append(c)
            found += 1
            if found == 4:
                break


@functools.lru_cache(maxsize=None)
def corpus():
    b = _Builder()
    for fam in (_family_a, _family_b, _family_c, _family_d, _family_e, _family_f, _family_g, _family_h, _family_i, _family_j):
        fam(b)
    return tuple(b.cases), b.calls


def cases(family=None, ref=False):
    return [c for c in corpus()[0] if c.ref == ref and (family is None or c.family in family)]


def by_name(names):
    idx = {c.name: c for c in corpus()[0]}
    return [idx[n] for n in names]


def calls():
    return corpus()[1]


def reduced():
    """The cases of the all-end-flags run: one per lane count, a two-tile window, one tile reached by rows, two generic."""
    return by_name([f"a/cap[{FIRST_OF[g]}]/in/noisy" for g in LANE_COUNTS]
                   + ["h/slots/T+1/noisy", "h/nt1/by-rows/noisy", "c/nfl0/ndb65/noisy", f"d/m{MM + 1}/c0/noisy"])


def edge_rows():
    """... and the cases whose seam shows only with one end of the window free."""
    return [c for c in corpus()[0] if c.edge.startswith("edge-row")]


def batch(cs, est=None):
    return LocusBatch.from_reads([(c.motif, [(c.fl, c.tr, c.fr)]) for c in cs], None if est is None else [[int(e)] for e in est])


def windows(cs):
    return np.array([c.lo for c in cs], np.int32), np.array([c.n for c in cs], np.int32)


def route_histogram(cs, force_generic=False):
    """Lengths of the class lists a call over these cases leaves (strk_class_counts): every chunk in the list it is classified
    to, and the chunks of a handed-over item in the generic list as well."""
    h = np.zeros(NC + 2, np.int32)
    for c in cs:
        for r in (GENERIC,) * len(c.route) if force_generic else c.route:
            h[r] += 1
            if c.handover and r != GENERIC:
                h[GENERIC] += 1
    return h


_EXPECTED: dict = {}   # (case name, flags) -> what the oracle says, computed once and shared by the tests


def _oracle_case(c: Case, flags):
    if c.ref:
        got = [oracle.score_ref_boundaries(c.fl + c.tr + c.fr, c.fl, c.fr, c.motif, c.lo + k, len(c.tr))[0] for k in range(c.n)]
        return (np.array([s for s, _ in got], np.int32), np.array([a - 1 + len(c.fl) + len(c.tr) for _, a in got], np.int32))   # (score, end_query)
    return np.array([oracle.candidate_score(c.tr, c.fl, c.fr, c.motif, c.lo + k, flags) for k in range(c.n)], np.int32)


def prefetch(cs, flag_settings):
    """Fills the table of expectations for the cases at each of the end-flag settings, most expensive first over 16 threads
    (the oracle is a C library that keeps no state between calls and runs without the interpreter lock)."""
    oracle.lib()
    todo = sorted(((c, f) for c in cs for f in flag_settings if (c.name, f) not in _EXPECTED), key=lambda cf: -cf[0].cells())
    if todo:
        with ThreadPoolExecutor(min(16, len(todo))) as pool:
            for (c, f), v in zip(todo, pool.map(lambda cf: _oracle_case(*cf), todo)):
                _EXPECTED[c.name, f] = v


def expected(cs, flags=15):
    """The oracle's score table of each case (reference side: scores and end_query)."""
    prefetch(cs, [flags])
    return [_EXPECTED[c.name, flags] for c in cs]
