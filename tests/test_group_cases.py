"""CPU half of the group kernels' seam corpus (tests/group_cases.py): every case is on the side of its seam that it claims, by
the Python model of the routing; the model against the restatements where they overlap; hand-written expectations through
the restatements on the smallest cases.  No device.  GPU half: test_gpu_group_cases.py."""
import numpy as np
import pytest

import consensus_restatement as BR
import group_cases as G
import kmers_restatement as KR
import poa_restatement as P

CASES = G.cases()
ROUTES = G.routes()


def test_names_are_unique_and_every_seam_has_all_its_sides():
    names = [c.name for c in CASES]
    assert len(set(names)) == len(names)
    have = {}
    for c in CASES:
        have.setdefault(c.seam, set()).add(c.side)
    assert {s: set(v) for s, v in G.SEAMS.items()} == have
    assert {c.family for c in CASES} == set("abcdefgh")


def test_limits_of_the_calls_and_of_the_python_restatements():
    for c in CASES:
        assert len(c.group) <= G.MAX_GROUP and max(map(len, c.group)) <= G.MAX_LEN, c.name
        assert c.k is not None or c.cons, c.name
        if c.cons:                                      # Levenshtein and POA in Python
            assert max(map(len, c.group)) <= 300, c.name
    assert len(G.cons_cases()) >= 40 and len(G.kmer_cases()) >= 100


def _plain_hash(s: bytes) -> int:
    h = 0
    for p, b in enumerate(s):
        h = (h + (b + 1) * ((p * 2654435761 + 0x9E3779B9) & G.M32)) & G.M32
    return h


def test_dedup_hash_is_the_kernels_and_is_two_sums():
    rng = np.random.default_rng(1)
    for n in (0, 1, 3, 64, 300, 5000):
        s = G.rand(rng, bytes(range(256)), n)
        assert G.dedup_hash(s) == _plain_hash(s)
    assert G.dedup_hash(b"AGA") == G.dedup_hash(b"CCC") == _plain_hash(b"AGA")
    assert G.dedup_hash(b"AGA") != G.dedup_hash(b"AGC")
    # equal sums, equal hash: 20 000 random 40-mers have hundreds of colliding pairs, each one of the sums' (a 32-bit hash
    # would give 0.05 on average)
    strs = [G.rand(rng, b"ACGT", 40) for _ in range(20000)]
    sums = {}
    for s in strs:
        b = np.frombuffer(s, np.uint8).astype(np.int64) + 1
        sums.setdefault((int(b.sum()), int((b * np.arange(40)).sum())), set()).add(G.dedup_hash(s))
    assert all(len(v) == 1 for v in sums.values())
    assert len({G.dedup_hash(s) for s in strs}) == len(sums) <= len(set(strs)) - 100


@pytest.mark.parametrize("case", [c for c in CASES if c.family == "a"], ids=lambda c: c.name)
def test_dedup_cases_visit_the_colliders_they_claim(case):
    rep, failed = G.dedup_trace(case.group)
    assert sum(r == i for i, r in enumerate(rep)) == case.claim["d"] == len(set(case.group))
    assert {i: failed[i] for i in case.claim["failed"]} == case.claim["failed"]
    assert {i: rep[i] for i in case.claim.get("rep", {})} == case.claim.get("rep", {})
    first = {}
    for i, s in enumerate(case.group):
        assert rep[i] == first.setdefault(s, i)                       # the model's dedup is the restatements'
    if case.side != "no collision":
        assert sum(failed) > 0
    if case.seam == "dedup compare passes":                           # the pair differs in its last three bytes and nowhere else
        x, y = case.group[0], case.group[1]
        assert len(x) == len(y) == int(case.side.split()[1]) and x[:-3] == y[:-3] and x[-1] != y[-1]


def test_all_collide_group_has_one_hash_and_no_equal_pair():
    g = G.by_name("a/all-collide").group
    assert len({G.dedup_hash(s) for s in g}) == 1 and len(set(g)) == len(g) == 70 and len({len(s) for s in g}) == 1
    g = G.by_name("a/collider-3-dup-70").group
    assert G.dedup_hash(g[3]) == G.dedup_hash(g[70]) and g[3] != g[70] and g[70] == g[71] and g[72] == g[3]


def test_alphabet_cases_have_the_sigma_they_claim():
    seen = set()
    for c in CASES:
        if "sigma" not in c.claim:
            continue
        sigma, bits, cmap = G.code_map(c.group)
        assert sigma == c.claim["sigma"] and bits == c.claim.get("bits", bits), c.name
        if c.family == "b" and c.cons:
            values = sorted(set(b"".join(c.group)))
            seen.add((sigma, values[0] >= 0xF7))
            if c.name.endswith("/part"):                              # pairs over a part of the values
                assert len(set(c.group[0] + c.group[1])) < sigma and len(set(c.group[3] + c.group[4])) == 2
                assert c.group[3][0] == values[0] and c.group[4][0] == values[-1]
                if sigma == 9:                                        # the two values that `& 7` would fold together
                    assert (int(cmap[values[0]]) & 7) == (int(cmap[values[-1]]) & 7)
    assert seen == {(s, high) for s in (7, 8, 9) for high in (False, True)}
    lens = {len(c.group[0]) for c in CASES if c.family == "b" and c.cons and not c.name.endswith("/part")}
    assert lens == {1, 63, 64, 65, 130}


@pytest.mark.parametrize("case", G.kmer_cases(), ids=lambda c: c.name)
def test_kmer_cases_go_where_they_claim(case):
    r = ROUTES[case.name]
    for key in ("state", "table", "windows", "distinct", "sigma", "bits", "ones"):
        if key in case.claim:
            assert getattr(r, key) == case.claim[key], (case.name, key)
    assert r.windows == KR.n_windows(case.group, case.k)
    if case.seam.startswith("code width"):
        want = int(case.side.split()[0])
        assert case.k * r.bits == want and (r.state == G.GENERAL) == (want > 64)
    if r.state == G.HASHED:
        assert r.distinct <= r.table - r.table // 4
    if r.state == G.SPILLED:
        assert r.table == G.LARGE_T and r.distinct > 1536 and case.k * r.bits <= 64
    if case.seam in ("run of 8", "second round"):
        assert len(case.group[0]) - case.k + 1 == int(case.side.split()[0])
    if case.seam in ("sort padding", "sort stretches"):
        assert r.windows == int(case.side.split()[1]) and r.sorted


def test_every_state_and_table_is_in_the_corpus():
    have = {(r.state, r.table) for r in ROUTES.values()}
    assert have >= {(G.HASHED, G.SMALL_T), (G.HASHED, G.LARGE_T), (G.SPILLED, G.LARGE_T), (G.GENERAL, G.SMALL_T), (G.GENERAL, G.LARGE_T)}
    assert max(G.pow2_above(r.windows) for r in ROUTES.values() if r.sorted) == 65536     # the largest single sort


def test_capacity_cases_sit_on_the_capacity():
    r = ROUTES
    assert (r["c/small/384"].windows, r["c/small/384"].distinct, r["c/small/384"].table) == (384, 384, 512)
    assert (r["c/small/385"].windows, r["c/small/385"].table, r["c/small/385"].state) == (385, 2048, G.HASHED)
    assert (r["c/large/1536"].distinct, r["c/large/1536"].state) == (1536, G.HASHED)
    assert (r["c/large/1537"].distinct, r["c/large/1537"].state) == (1537, G.SPILLED)
    for name, d, state in (("c/ones/1536", 1536, G.HASHED), ("c/ones/1537", 1537, G.SPILLED)):
        c = G.by_name(name)
        assert c.k * r[name].bits == 64 and (r[name].distinct, r[name].ones > 0, r[name].state) == (d, True, state)
        entries = KR.count_group(c.group, c.k)
        assert len(entries) == d + 1 and entries[-1][0] == b"T" * 32 and entries[-1][1] == r[name].ones      # all ones: last


@pytest.mark.parametrize("case", [c for c in CASES if c.family == "d"], ids=lambda c: c.name)
def test_probe_cases_wrap_and_chain(case):
    r = ROUTES[case.name]
    T = r.table
    keys = np.concatenate(G.packed_keys(case.group, case.k))
    lay = G.probe_layout(keys, T)
    assert len(lay["slots"]) == r.distinct and sorted(set(lay["slots"].values())) == sorted(lay["slots"].values())
    if case.seam == "probe wrap":
        homes = G.home_slot(np.array(list(lay["slots"]), np.uint64), T)
        assert {T - 4, T - 3, T - 2, T - 1} <= set(homes.tolist())
        assert lay["wraps"] >= case.claim["wraps"] and min(lay["slots"].values()) == 0
    else:
        assert lay["chain"] >= case.claim["chain"] >= 64 and lay["longest"] >= 63
    # the other order holds the same windows: the same entries but for the places
    other = G.by_name(case.name[:-3] + ("rev" if case.name.endswith("fwd") else "fwd"))
    assert other.group == case.group[::-1]
    assert KR.count_dict(other.group, other.k) == KR.count_dict(case.group, case.k)
    # the words are windows of the strings: FILLER-separated, every ninth offset
    assert all((len(s) + 1) % 9 == 0 for s in case.group if len(s) >= case.k)


def test_key_order_is_byte_order_and_entry_counts_are_the_restatements():
    """The model against the restatement where both speak: entries = distinct keys (+ 1 with all-ones windows), and the keys
    ascend in the restatement's order of the windows."""
    n = 0
    for c in G.kmer_cases():
        r = ROUTES[c.name]
        if r.state not in (G.HASHED, G.SPILLED) or r.windows > 5000:
            continue
        entries = KR.count_group(c.group, c.k)
        assert len(entries) == r.distinct + (r.ones > 0), c.name
        keys = G.packed_keys(c.group, c.k)
        first = [int(keys[si][i]) for _w, _c, (si, i) in entries]
        assert first == sorted(first) and len(set(first)) == len(first), c.name
        n += 1
    assert n >= 60


def test_place_cases_have_their_first_occurrence_at_the_far_end():
    s = G.by_name("h/long/k1").group[0]
    assert len(s) == 65535 and s.index(b"T") == 65534
    for name, idx in (("h/str249/hashed", 249), ("h/str249/spilled", 249), ("h/str249/general", 249)):
        c = G.by_name(name)
        assert len(c.group) == 250
        others = {w for t in c.group[:idx] for w in KR.windows(t, c.k)}
        assert any(w not in others for w in KR.windows(c.group[idx], c.k)), name
    c = G.by_name("g/general/prefix")
    assert len({s[:c.k - 1] for s in c.group[:5]}) == 1 and len({s[c.k - 1] for s in c.group[:5]}) == 4
    c = G.by_name("g/spilled/twice")
    assert all(e[1] == 2 for e in KR.count_group(c.group, c.k))
    c = G.by_name("g/general/equal")
    counts = [e[1] for e in KR.count_group(c.group, c.k)]
    assert max(counts) >= 4 and min(counts) == 1


def test_cap_call_is_cut_into_at_least_three_pieces():
    cs = [G.by_name(n) for n in G.CAP_CALL]
    states = [ROUTES[c.name].state for c in cs]
    assert {G.HASHED, G.SPILLED, G.GENERAL} == set(states)
    pow2 = [G.pow2_above(ROUTES[c.name].windows) for c in cs if ROUTES[c.name].sorted]
    pieces = G.sort_pieces(pow2, G.CAP_WS_BYTES)
    assert len(pieces) >= 3 and pieces[0] == (0, 1)
    assert G.sort_pieces([4, 4, 8, 1, 1, 16, 2], 8 * G.ELEM_BYTES) == [(0, 2), (2, 3), (3, 5), (5, 6), (6, 7)]


def test_hand_written_expectations_through_the_restatements():
    g = G.by_name("a/AGA-CCC").group
    assert g == (b"AGA", b"CCC", b"AGA", b"CCC", b"CCC")
    assert KR.count_group(g, 3) == [(b"AGA", 2, (0, 0)), (b"CCC", 3, (1, 0))]
    assert KR.count_group(g, 2) == [(b"AG", 2, (0, 0)), (b"CC", 6, (1, 0)), (b"GA", 2, (0, 1))]
    assert BR.best_representative(g) == (1, "best_rep", 6)              # lev 3: D(AGA) = 3 * 3, D(CCC) = 2 * 3
    assert P.consensus(g) == (-1, "poa", b"CCC", False)
    assert BR.best_representative([b"AGA", b"CCC"]) == (0, "best_rep", 3)
    # nine values: the smallest against the largest
    lo, hi = b"A" * 5, b"Y" * 5
    assert BR.best_representative([lo, hi, hi]) == (1, "best_rep", 5)
    # the tail pair: one distance of 3 (three substitutions), the third string one more
    c = G.by_name("a/tail/L64")
    x, y, z = c.group[0], c.group[1], c.group[4]
    assert BR.lev(x, y) == 3 and BR.lev_plain(x[-8:], y[-8:]) == 3 and BR.lev(x, z) <= 3
    # the tandem of 9 windows: CAG, AGC, GCA three times each, and ACGT's two windows
    c = G.by_name("e/tandem/9")
    assert KR.count_dict(c.group, 3) == {b"ACG": 1, b"AGC": 3, b"CAG": 3, b"CGT": 1, b"GCA": 3}
    c = G.by_name("h/str249/hashed")
    assert [(w, n, p) for w, n, p in KR.count_group(c.group, 3)] == [
        (b"AGC", 249, (0, 1)), (b"AGT", 1, (249, 1)), (b"CAG", 499, (0, 0)), (b"GCA", 249, (0, 2)), (b"GTT", 1, (249, 2)),
        (b"TTT", 1, (249, 3))]
