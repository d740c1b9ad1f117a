"""CPU half of the exact path's seam corpus (exact_cases.py): every case's claimed route against strk_classify, both sides of
every listed edge, the oracle-cell cap, the tie condition of the reference-side cases, strk_classify against its Python
restatement around every capacity, and the C oracle against the Python restatement on the small cases.  Loads the library;
needs no device."""
import itertools

import numpy as np

import exact_cases as X
import oracle
from oracle import py_restatement as py
from strkit_amd.batch import classify

ALL = X.corpus()[0]
BY = {c.name: c for c in ALL}


def _sides(edge):
    return {c.side for c in ALL if c.edge == edge}


def _pair(name):
    """Both reads of an edge: the clean tract and the noisy one."""
    a, b = BY[name + "/clean"], BY[name + "/noisy"]
    assert (a.fl, a.tr, a.fr) != (b.fl, b.tr, b.fr) and (len(a.fl), len(a.tr), len(a.fr), a.lo, a.n) == (len(b.fl), len(b.tr), len(b.fr), b.lo, b.n), name
    assert set(b.tr) - set("ACGT") or set(b.fl + b.fr) - set("ACGT"), name      # the noise brings wildcards
    return a, b


def test_names_are_unique_and_routes_match_classify():
    assert len(BY) == len(ALL) > 300
    for c in ALL:
        assert len(c.route) == len(c.chunks()) and c.n >= 1 and c.lo >= 0 and c.motif, c.name
        assert c.route == c.classified(), (c.name, c.edge, c.side, c.route, c.classified())
        assert set(c.classified(force_generic=True)) == {X.GENERIC}, c.name
    hist = X.route_histogram(X.cases())
    assert (hist > 0).all(), hist.tolist()            # every fast class, the tiled kernel and the generic kernel
    print("items per class list:", hist.tolist())


def test_capacity_and_row_edges():
    for c in range(X.NC):
        nxt = c + 1 if c + 1 < X.NC else X.LONG
        for side, d, route in (("in", 0, c), ("out", 1, nxt)):
            for k in _pair(f"a/cap[{c}]/{side}"):
                assert k.ndb + 1 == X.CAPS[c] + d and k.route == (route,) and k.rows() <= X.CAPS[0] + X.RS + k.ndb, k.name
    row_classes = sorted({X.FIRST_OF[g] for g in X.LANE_COUNTS} | {X.LAST_OF[g] for g in X.LANE_COUNTS})
    assert X.LANE_COUNTS == [8, 16, 32, 64] and row_classes[0] == 0 and row_classes[-1] == X.NC - 1
    for c in row_classes:
        nxt = c + 1 if c + 1 < X.NC else X.LONG
        for side, d, route in (("in", 0, c), ("out", 1, nxt)):
            for k in _pair(f"b/rows[{c}]/{side}"):
                assert k.rows() == X.CAPS[c] + X.RS + d and k.route == (route,) and k.ndb + 1 <= X.CAPS[0], k.name
                assert k.lo > 4 * (len(k.tr) // len(k.motif)), k.name             # a window far above the tract
    assert BY[f"b/rows[{X.NC - 1}]/out/clean"].ndb < 100                          # the tiled kernel on a short window


def test_flank_and_motif_edges():
    for nfr, kind in ((X.FF, "fast"), (X.FF + 1, X.LONG), (X.LF, X.LONG), (X.LF + 1, X.GENERIC)):
        for k in _pair(f"c/nfr{nfr}"):
            assert len(k.fr) == nfr and (k.route[0] < X.NC if kind == "fast" else k.route == (kind,)), k.name
    for nfl, route in ((1, X.LONG), (X.LF, X.LONG), (X.LF + 1, X.GENERIC)):
        for k in _pair(f"c/nfl{nfl}"):
            assert len(k.fl) == nfl and k.route == (route,) and k.ndb + 1 > X.CAPS[-1], k.name   # only the tiled kernel would take it
    sizes = [63, 64, 65, 128, 129]
    for which in ("nfl0", "nfr0", "both0"):
        got = sorted(int(s) for s in _sides(which))
        assert got[:5] == sizes and 1750 <= got[5] <= 1850, (which, got)
        for s in got:
            for k in _pair(f"c/{which}/ndb{s}"):
                assert k.ndb == s and k.route == (X.GENERIC,), k.name
                assert (len(k.fl) == 0 or which == "nfr0") and (len(k.fr) == 0 or which == "nfl0"), k.name
    for cls in (0, X.NC - 1):
        for m in (X.MM - 1, X.MM, X.MM + 1):
            for k in _pair(f"d/m{m}/c{cls}"):
                assert len(k.motif) == m and k.route == ((cls,) if m <= X.MM else (X.GENERIC,)), k.name
                assert k.motif[-30:] in k.tr, k.name                             # the motif's last bases are in the window
    for g in X.LANE_COUNTS:
        assert _sides(f"motif-lanes[{g}]") == {"-1", "0", "1"}
        for m in (g - 1, g, g + 1):
            for k in _pair(f"d/lanes{g}/m{m}"):
                assert len(k.motif) == m and X.LANES[k.route[0]] == g, k.name
    for k in _pair("d/m-over-nfl"):
        assert len(k.motif) > len(k.fl) >= 1 and k.route[0] < X.NC
    for k in _pair("d/m-over-tract"):
        assert len(k.motif) > len(k.tr) > 0 and k.route[0] < X.NC


def test_staircase_and_occupancy_calls():
    calls = X.calls()
    stair_lanes = [g for g in X.LANE_COUNTS if g >= X.SG]
    assert stair_lanes == [16, 32, 64]
    for g in stair_lanes:
        for side, p in (("G-2", g - 2), ("G-1", g - 1), ("G", g)):
            for k in _pair(f"e/stair[{X.FIRST_OF[g]}]/{side}") + _pair(f"e/stair[{X.FIRST_OF[g]}]/{side}/corner"):
                assert k.lo * len(k.motif) == p and X.LANES[k.route[0]] == g, k.name
            for k in _pair(f"e/stair[{X.FIRST_OF[g]}]/{side}/corner"):      # the flank ends in the columns of the group's last lane
                assert len(k.fl) > (g - 1) * (X.CAPS[k.route[0]] // g) and k.ndb + 1 <= X.CAPS[k.route[0]], k.name
    for name, g, n_items in (("e/ballot32", 32, 2), ("e/ballot16", 16, 4)):
        items = X.by_name(calls[name])
        assert len(items) == n_items == 64 // g and len({k.route for k in items}) == 1 and X.LANES[items[0].route[0]] == g
        assert sum(k.lo * len(k.motif) < g - 1 for k in items) == 1, name         # one item turns the fold off for the wave
    for g, counts in ((8, (1, 7, 8, 9)), (16, (1, 4, 5)), (32, (1, 2, 3))):
        for n in counts:
            items = X.by_name(calls[f"f/lanes{g}x{n}"])
            assert len(items) == n and len({k.route for k in items}) == 1 and X.LANES[items[0].route[0]] == g
            assert len({(k.fl, k.tr, k.fr) for k in items}) == n


def test_chunk_tile_and_symbol_edges():
    ns = [1, X.TM - 1, X.TM, X.TM + 1, 2 * X.TM, 2 * X.TM + 1]
    assert ns == [1, 31, 32, 33, 64, 65]
    for n in ns:
        for k in _pair(f"g/fast/n{n}"):
            assert k.n == n and len(set(k.route)) == 1 and k.route[0] < X.NC, k.name
        for k in _pair(f"g/long/n{n}"):
            assert k.n == n and set(k.route) == {X.LONG} and k.ndb + 1 > X.T, k.name
    for k in _pair("g/lo0-n1"):
        assert (k.lo, k.n) == (0, 1)
    for k in _pair("g/ntr0"):
        assert len(k.tr) == 0 and k.route[0] < X.NC
    for k in _pair("g/split/fast-long"):
        assert k.route == (X.NC - 1, X.LONG)
    for k in _pair("g/split/class-next"):
        assert len(k.route) == 2 and k.route[1] == k.route[0] + 1 < X.NC
    nt = lambda k: (k.ndb + 1 + X.T - 1) // X.T                                   # noqa: E731
    for side, slots, tiles, route in (("T", X.T, 1, X.NC - 1), ("T+1", X.T + 1, 2, X.LONG), ("2T", 2 * X.T, 2, X.LONG), ("2T+1", 2 * X.T + 1, 3, X.LONG)):
        for k in _pair(f"h/slots/{side}"):
            assert k.ndb + 1 == slots and nt(k) == tiles and k.route == (route,), k.name
    for k in _pair("h/nt1/by-rows"):
        assert nt(k) == 1 and k.route == (X.LONG,) and len(k.fr) <= X.FF and k.rows() == X.CAPS[-1] + X.RS + 1
    for k in _pair("h/nt1/by-nfr"):
        assert nt(k) == 1 and k.route == (X.LONG,) and len(k.fr) == X.FF + 1 and k.rows() <= X.CAPS[0] + X.RS + k.ndb
    for r in (0, 1, 2):
        for k in _pair(f"h/rowsP-mod64/{r}"):
            assert k.rows() % 64 == r and nt(k) == 2 and k.route == (X.LONG,), k.name
    for r in (0, 32):
        for k in _pair(f"h/fork-step/{r}"):
            assert len(k.motif) == 1 and k.n == 32 and (len(k.fl) + k.lo) % 64 == r and k.route == (X.LONG,), k.name
    assert _sides("seam-edit") == {f"{kind}@{d:+d}" for kind in ("sub", "del3", "ins3") for d in (-1, 0, 1)}
    base = None
    for k in (c for c in ALL if c.edge == "seam-edit"):
        assert nt(k) == 2 and k.route == (X.LONG,), k.name
        kind, col = k.side.split("@")[0], X.T + int(k.side.split("@")[1])
        clean = (k.motif * (len(k.tr) // len(k.motif) + 2))
        db = k.fl + k.tr + k.fr
        ref = k.fl + clean
        assert db[:col] == ref[:col] and db[col] != ref[col], k.name              # the first base that differs is window column `col`
        base = base or (k.fl, k.fr)
        assert (k.fl, k.fr) == base
    for d in (-4, -3, -2, -1, 0):
        k = BY[f"h/edge-row/fwd{d:+d}"]                                         # the window's end IS the middle candidate, from column T + d on
        db, cand = k.fl + k.tr + k.fr, k.fl + k.motif * (k.lo + 2) + k.fr
        assert nt(k) == 2 and db.endswith(cand) and k.ndb - len(cand) == X.T + d and k.route == (X.LONG,), k.name
    for d in (-3, -2, -1, 0, 1):
        k = BY[f"h/edge-row/bwd{d:+d}"]                                         # the window's beginning IS the middle candidate, up to column T + d + 2
        db, cand = k.fl + k.tr + k.fr, k.fl + k.motif * (k.lo + 2) + k.fr
        assert nt(k) == 2 and db.startswith(cand) and len(cand) == X.T + d + 2 and k.route == (X.LONG,), k.name
    assert len(X.edge_rows()) == 10
    for side, lo_f, hi_f in (("short", 0.2, 0.3), ("long", 2.9, 3.1)):
        for k in _pair(f"h/cand/{side}"):
            assert lo_f * k.ndb <= k.rows() <= hi_f * k.ndb and nt(k) == 2 and k.route == (X.LONG,), k.name
    for where, kind in (("fast", "fast"), ("tiled", X.LONG)):
        k8, k9 = BY[f"i/{where}/8"], BY[f"i/{where}/9"]
        sym = lambda s: {oracle.encode(ch) for ch in s}                           # noqa: E731
        db8, db9 = k8.fl + k8.tr + k8.fr, k9.fl + k9.tr + k9.fr
        assert len(sym(db8)) == 8 and len(sym(db9)) == 9 and len(sym(db9[:-1])) == 8 and db8[:-1] == db9[:-1]
        assert not k8.handover and k9.handover and k8.route == k9.route
        assert (k8.route[0] < X.NC) if kind == "fast" else (k8.route == (X.LONG,) and nt(k8) == 2)


def test_reference_side_edges_and_ties():
    last = X.NC - 1
    for side, d, route in (("in", 0, last), ("out", 1, X.GENERIC)):
        for k in _pair(f"j/cap/{side}"):
            assert k.ref and k.ndb + 1 == X.CAPS[last] + d and k.route == (route,), k.name
        for k in _pair(f"j/rows/{side}"):
            assert k.ref and k.rows() == X.CAPS[last] + X.RS + d and k.route == (route,), k.name
    ties = [c for c in ALL if c.edge == "ref-tie"]
    at_end = [c for c in ALL if c.edge == "ref-tie-last"]
    assert len(ties) >= 6 and len(at_end) >= 4 and all(c.ref and c.ndb <= 200 and c.route == (last,) for c in ties + at_end)
    for c in ties + at_end:
        cols = X.tie_columns(c)
        assert max(cols) >= 2, (c.name, cols)
        assert c in ties or any(x >= 2 and e for x, e in zip(cols, X.tie_columns(c, last_column=True))), c.name
        # ... and the restated row is the oracle's: its maximum and the first column that holds it
        for k in range(c.n):
            row = X.ref_last_row(c.fl + c.tr + c.fr, c.fl + c.motif * (c.lo + k))
            (s, adj), _ = oracle.score_ref_boundaries(c.fl + c.tr + c.fr, c.fl, c.fr, c.motif, c.lo + k, len(c.tr))
            assert (int(row.max()), int(np.argmax(row))) == (s, adj - 1 + len(c.fl) + len(c.tr)), (c.name, k)


def test_cell_cap_holds():
    read_side = sum(c.cells() for c in X.cases())
    ref_side = sum(c.cells() for c in X.cases(ref=True))
    print(f"oracle cells at one end-flag setting: {read_side:,} read side + {ref_side:,} reference side (cap {X.CELL_CAP:,})")
    assert read_side + ref_side <= X.CELL_CAP


def test_classify_agrees_with_its_restatement_around_every_capacity():
    n_checked = 0
    for c in range(X.NC):
        cap = X.CAPS[c]
        for slots, rows, nfr, nfl0 in itertools.product(range(cap - 1, cap + 3), range(cap + X.RS - 1, cap + X.RS + 3),
                                                        (0, 1, X.FF, X.FF + 1, X.LF, X.LF + 1), (0, 1, 17, X.LF, X.LF + 1)):
            for m, n in ((1, 1), (1, X.TM), (1, X.TM + 1), (2, 3), (X.MM, 1), (X.MM + 1, 1)):
                nfl = nfl0 + (rows - nfl0) % m                     # rows = nfl + (lo + n - 1) * m
                lo = (rows - nfl) // m - (n - 1)
                ntr = slots - 1 - nfl - nfr
                if lo < 0 or ntr < 0:
                    continue
                for force, ref in ((0, 0), (0, 1), (1, 0)):
                    assert classify(nfl, ntr, nfr, m, lo, n, force, ref) == X.py_classify(nfl, ntr, nfr, m, lo, n, force, ref), \
                        (nfl, ntr, nfr, m, lo, n, force, ref)
                    n_checked += 1
    for ndb, rows in ((X.T * X.K["kLongMaxTiles"] - 1, 100), (X.T * X.K["kLongMaxTiles"], 100), (3000, 1 << 20), (3000, (1 << 20) + 1)):
        assert classify(50, ndb - 100, 50, 1, rows - 50, 1, 0, 0) == X.py_classify(50, ndb - 100, 50, 1, rows - 50, 1)
    assert n_checked > 10000


def test_c_oracle_agrees_with_python_restatement_on_small_cases():
    """The corpus's expectations do not rest on the C oracle alone: the first candidate of every case of up to 300 bases with
    all ends free, and where the DP is small also the last candidate and both end-flag settings of the whole-corpus run
    (a Python loop runs about a million cells per second; the windows far above a short tract, whose candidates run to
    thousands of rows, are left to the C oracle); on the reference side (score, end)."""
    n_checked = n_cells = 0
    for c in ALL:
        if c.ndb > 300 or c.ndb == 0:
            continue
        db = c.fl + c.tr + c.fr
        for k in sorted({0, c.n - 1}):
            i = c.lo + k
            cells = c.ndb * (len(c.fl) + i * len(c.motif))
            if cells > (40000 if k == 0 else 16000):
                continue
            if c.ref:
                fwd, _ = py.score_ref_boundaries(db, c.motif * i, c.fl, c.fr, len(c.tr))
                assert fwd == oracle.score_ref_boundaries(db, c.fl, c.fr, c.motif, i, len(c.tr))[0], (c.name, i)
            else:
                cand = c.fl + c.motif * i + c.fr
                for flags in (15, 0) if cells <= 16000 else (15,):
                    got = py.sg_align(db, cand, 5, 5, bool(flags & 1), bool(flags & 2), bool(flags & 4), bool(flags & 8))[0]
                    assert got == oracle.candidate_score(c.tr, c.fl, c.fr, c.motif, i, flags), (c.name, i, flags)
            n_checked += 1
            n_cells += cells
    print(f"{n_checked} candidates, {n_cells:,} cells per end-flag setting")
    assert n_checked >= 150
