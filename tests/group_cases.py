"""Seam corpus of the kernels that work on packed sequence groups: k_kmers_hash / k_kmers_sort (strk_kmers.h, host side
strk_host_kmers.inc), k_best_rep (strk_consensus.h) and the copy of its dedup at the head of k_poa (strk_poa.h).
Deterministic: fixed seeds or construction.  A case is one group of byte strings, a window length k where the k-mer call takes
part, the seam it aims at with the side of that seam, and what it claims about where the group goes (`claim`).  The claims are
checked against a small Python model of the routing, restated from the kernel text (every function names the lines it
restates: a change there has to be made twice); the GPU half ties the model to the library through the call's statistics.
Expected values never come from here: they are those of kmers_restatement, consensus_restatement and poa_restatement.
Families a-h: see DESIGN.md, "Group kernels: seam corpus".  CPU half: test_group_cases.py, GPU half: test_gpu_group_cases.py.
"""
from __future__ import annotations

import functools
from dataclasses import dataclass, field

import numpy as np

M32 = (1 << 32) - 1
SMALL_T, LARGE_T = 512, 2048                   # kKmerSmallSlots, kKmerLargeSlots
MAX_GROUP, MAX_LEN = 250, 65535                # kKmerMaxGroup / kConsMaxGroup, kKmerMaxLen / kConsMaxLen
ELEM_BYTES = 16                                # sizeof(KmerElem)
HASHED, SPILLED, GENERAL, NO_WINDOWS = "hashed", "spilled", "general", "no windows"
ONES = np.uint64(0xFFFFFFFFFFFFFFFF)           # kKmerEmpty: the key that lives outside the table


# ---------------------------------------------------------------------------------------------
# The model
# ---------------------------------------------------------------------------------------------
def _u8(s) -> np.ndarray:
    return np.frombuffer(bytes(s), np.uint8)


def dedup_hash(s) -> int:
    """k_best_rep step 1 (strk_consensus.h, `h += (b + 1u) * ((uint32_t)p * 2654435761u + 0x9E3779B9u)`) and the same line of
    k_poa: linear in the bytes, so it is a function of sum(b + 1) and sum((b + 1) * p) alone."""
    b = _u8(s).astype(np.uint64)
    p = np.arange(b.shape[0], dtype=np.uint64)
    w = (p * np.uint64(2654435761) + np.uint64(0x9E3779B9)) & np.uint64(M32)
    return int(((b + np.uint64(1)) * w).sum() & np.uint64(M32))            # (256 * 2^32 * 65 535 < 2^64)


def dedup_trace(group) -> tuple[list[int], list[int]]:
    """k_best_rep step 2 / k_poa step 1: for every string its first equal predecessor (itself if none) and the number of
    byte comparisons that failed on the way: predecessors of equal hash and length, in ascending order, until one is equal."""
    g = [bytes(s) for s in group]
    h = [dedup_hash(s) for s in g]
    rep, failed = [], []
    for i, s in enumerate(g):
        r, f = i, 0
        for j in range(i):
            if h[j] == h[i] and len(g[j]) == len(s):
                if g[j] == s:
                    r = j
                    break
                f += 1
        rep.append(r)
        failed.append(f)
    return rep, failed


def code_map(group) -> tuple[int, int, np.ndarray]:
    """kmer_code_bits (strk_kmers.h): (sigma, bits, map) with a byte's code its rank in the group's set of byte values and
    bits = max(1, ceil(log2 sigma)).  k_best_rep builds the same set; it switches planes at sigma <= 8."""
    present = np.zeros(256, bool)
    for s in group:
        present[_u8(s)] = True
    sigma = int(present.sum())
    cmap = np.where(present, np.cumsum(present) - 1, 0).astype(np.uint64)
    return sigma, max(1, (sigma - 1).bit_length()), cmap


def n_windows(group, k: int) -> int:
    return sum(max(len(s) - k + 1, 0) for s in group)


def packed_keys(group, k: int) -> list[np.ndarray]:
    """The 64-bit key of every window, one array per string (k * bits <= 64): the first byte in the highest bits, masked to
    k * bits (k_kmers_hash: `key = ((key << bits) | s_map[s[i + k - 1]]) & mask`)."""
    _sigma, bits, cmap = code_map(group)
    kb = k * bits
    assert kb <= 64
    mask = ONES if kb == 64 else np.uint64((1 << kb) - 1)
    out = []
    for s in group:
        nw = max(len(s) - k + 1, 0)
        codes = cmap[_u8(s)]
        key = np.zeros(nw, np.uint64)
        for j in range(k if nw else 0):
            key = (key << np.uint64(bits)) | codes[j:j + nw]
        out.append(key & mask)
    return out


def home_slot(keys, T: int) -> np.ndarray:
    """k_kmers_hash: `(uint32_t)((key * 0x9E3779B97F4A7C15ull) >> 40) & (T - 1)`."""
    keys = np.asarray(keys, np.uint64)
    with np.errstate(over="ignore"):
        return ((keys * np.uint64(0x9E3779B97F4A7C15)) >> np.uint64(40)).astype(np.int64) & (T - 1)


def table_of(n_win: int) -> int:
    """count_kmers_impl (strk_host_kmers.inc): `w > kKmerSmallSlots - kKmerSmallSlots / 4` goes to the large table."""
    return SMALL_T if n_win <= SMALL_T - SMALL_T // 4 else LARGE_T


@dataclass(frozen=True)
class Route:
    windows: int
    sigma: int
    bits: int
    table: int | None          # None: no window, no workgroup
    state: str
    distinct: int | None       # distinct packed keys without the all-ones key (None on the general path)
    ones: int                  # windows that pack to all ones

    @property
    def sorted(self) -> bool:
        return self.state in (SPILLED, GENERAL)


def route(group, k: int) -> Route:
    """Where strk_count_kmers sends a group: the table by its window count, general with k * bits > 64, spilled with more than
    3T/4 distinct keys in the table (`atomicAdd(&s_d, 1) + 1 > kCap`; the all-ones key is counted outside s_d)."""
    sigma, bits, _ = code_map(group)
    w = n_windows(group, k)
    if w == 0:
        return Route(0, sigma, bits, None, NO_WINDOWS, None, 0)
    T = table_of(w)
    if k * bits > 64:
        return Route(w, sigma, bits, T, GENERAL, None, 0)
    keys = np.concatenate(packed_keys(group, k))
    ones = int((keys == ONES).sum())
    d = int(np.unique(keys[keys != ONES]).shape[0])
    return Route(w, sigma, bits, T, SPILLED if d > T - T // 4 else HASHED, d, ones)


def probe_layout(keys_in_order, T: int) -> dict:
    """Linear probing as k_kmers_hash does it, the keys claimed in the given order: the slot of every distinct key, whether a
    probe sequence wraps from slot T - 1 to slot 0, the longest probe and the largest number of keys with one home slot."""
    slot_of: dict[int, int] = {}
    used = [False] * T
    wraps, longest = 0, 0
    per_home: dict[int, int] = {}
    keys = [int(x) for x in keys_in_order if int(x) != int(ONES)]
    homes = home_slot(np.array(keys, np.uint64), T).tolist() if keys else []
    for key, h0 in zip(keys, homes):
        if key in slot_of:
            continue
        per_home[h0] = per_home.get(h0, 0) + 1
        h, n = h0, 0
        while used[h]:
            h, n = (h + 1) & (T - 1), n + 1
        used[h] = True
        slot_of[key] = h
        wraps += h < h0
        longest = max(longest, n)
    return dict(slots=slot_of, wraps=wraps, longest=longest, chain=max(per_home.values(), default=0))


def sort_pieces(pow2_elems, ws_bytes: int) -> list[tuple[int, int]]:
    """strk_groups::cut_piece over the sorted groups (count_kmers_impl): [p0, p1) of every launch of k_kmers_sort; items in
    order while their padded element counts fit ws_bytes / sizeof(KmerElem), always at least one."""
    budget = max(1, ws_bytes // ELEM_BYTES)
    out, p0 = [], 0
    while p0 < len(pow2_elems):
        used, p1 = 0, p0
        while p1 < len(pow2_elems) and not (p1 > p0 and used + pow2_elems[p1] > budget):
            used += pow2_elems[p1]
            p1 += 1
        out.append((p0, p1))
        p0 = p1
    return out


def pow2_above(w: int) -> int:
    p = 1
    while p < w:
        p <<= 1
    return p


# ---------------------------------------------------------------------------------------------
# Cases
# ---------------------------------------------------------------------------------------------
# seam -> the sides a corpus must hold
SEAMS = {
    "dedup collision": ("collider in block", "collider block 0, duplicate block 1", "three colliders", "all collide",
                        "no collision"),
    "dedup compare passes": ("len 63", "len 64", "len 65", "len 66", "len 67"),
    "best_rep planes": ("sigma 7", "sigma 8", "sigma 9"),
    "small table capacity": ("384 windows", "385 windows"),
    "large table capacity": ("1536 distinct", "1537 distinct"),
    "all-ones beside a full table": ("1536 + ones", "1537 + ones"),
    "probe wrap": ("T 512", "T 2048"),
    "probe chain": ("T 512", "T 2048"),
    "run of 8": ("1 window", "7 windows", "8 windows", "9 windows"),
    "second round": ("2047 windows", "2048 windows", "2049 windows", "4097 windows"),
    "code width 2": ("62 bits", "64 bits", "66 bits general"),
    "code width 3": ("63 bits", "66 bits general"),
    "code width 4": ("64 bits", "68 bits general"),
    "code width 5": ("60 bits", "65 bits general"),
    "code width 8": ("64 bits", "72 bits general"),
    "sort padding": ("W 1", "W 2", "W 3", "W 1023", "W 1024", "W 1025"),
    "sort stretches": ("W 2047", "W 2048", "W 2049"),
    "sort runs": ("shared prefix", "equal across strings", "every window twice"),
    "place i": ("i 65534 k 1", "i 65533 k 2", "two windows", "one window", "sorted packed", "sorted general"),
    "place string": ("hashed 249", "spilled 249", "general 249"),
}


@dataclass(frozen=True)
class Case:
    name: str
    family: str
    seam: str
    side: str
    group: tuple               # of bytes
    k: int | None              # None: no k-mer call
    cons: bool                 # takes part in the best-representative and the consensus call (strings of at most 300 bytes)
    claim: dict = field(compare=False, hash=False)   # state, table, distinct, windows, sigma, ... (test_group_cases.py)


def rand(rng, alpha: bytes, n: int) -> bytes:
    return _u8(alpha)[rng.integers(0, len(alpha), n)].tobytes()


def mutate(rng, s: bytes, rate: float, alpha: bytes, indel: float = 0.5) -> bytes:
    """Every position is hit with probability `rate`: a deletion, an insertion before it (share `indel`, half each) or a
    substitution by a letter of `alpha`."""
    out = bytearray()
    hit = rng.random(len(s)) < rate
    for i, ch in enumerate(s):
        if not hit[i]:
            out.append(ch)
            continue
        r = rng.random()
        if r < indel / 2:
            continue
        out.append(alpha[int(rng.integers(0, len(alpha)))])
        if r < indel:
            out.append(ch)
    return bytes(out)


def distinct_run(rng, alpha: bytes, k: int, n_win: int) -> bytes:
    """A string of n_win windows of length k, all distinct (redrawn until they are: deterministic under the seed)."""
    while True:
        s = rand(rng, alpha, n_win + k - 1)
        if len({s[i:i + k] for i in range(n_win)}) == n_win:
            return s


class _Builder:
    def __init__(self):
        self.cases: list[Case] = []

    def add(self, family, name, seam, side, group, k=None, cons=False, **claim):
        assert name not in {c.name for c in self.cases}, name
        assert seam in SEAMS and side in SEAMS[seam], (seam, side)
        group = tuple(bytes(s) for s in group)
        assert len(group) <= MAX_GROUP and all(len(s) <= MAX_LEN for s in group), name
        assert not cons or all(len(s) <= 300 for s in group), name
        self.cases.append(Case(name, family, seam, side, group, k, cons, claim))


# Two equal-length strings collide when sum(b + 1) and sum((b + 1) * p) agree.  "AGA" and "CCC" do at any offset:
# 66 + 72 + 66 = 3 * 68 and 72 + 2 * 66 = 68 * (1 + 2).  A string with n such blocks has 2^n colliding variants.  One differing
# byte cannot collide (the weight of a position below 65 536 has at most 17 trailing zero bits), nor do two adjacent bytes among
# the first 70 positions, so three bytes are the shortest difference at the tail of a string.
SWAP = (b"AGA", b"CCC")


def variants(parts, n: int) -> list[bytes]:
    """n colliding strings: `parts` joined by AGA or CCC, the choice at joint j being bit j of the variant's number."""
    assert n <= 1 << (len(parts) - 1)
    return [b"".join(p + (SWAP[(v >> j) & 1] if j < len(parts) - 1 else b"") for j, p in enumerate(parts)) for v in range(n)]


def _family_a(b):
    """Dedup on a hash collision: the `while (cand)` loop on candidates whose bytes differ."""
    rng = np.random.default_rng(3301)
    parts = [rand(rng, b"ACGT", 5) for _ in range(8)]                # 7 joints: 128 variants of 61 bytes
    v = variants(parts, 128)
    others = [rand(rng, b"ACGT", len(v[0])) for _ in range(80)]
    F, K3 = "a", 3
    b.add(F, "a/collider-then-dup", "dedup collision", "collider in block", [v[1], v[0], v[0], v[1], others[0]], K3, True,
          d=3, failed={2: 1, 3: 0}, rep={2: 1, 3: 0})
    g = others[:3] + [v[5]] + others[3:69] + [v[0], v[0], v[5]]       # collider at 3, the string at 70, its duplicate at 71
    b.add(F, "a/collider-3-dup-70", "dedup collision", "collider block 0, duplicate block 1", g, K3, True,
          d=71, failed={70: 1, 71: 1, 72: 0}, rep={71: 70, 72: 3})
    b.add(F, "a/three-colliders", "dedup collision", "three colliders", [v[1], v[2], v[4], v[0], others[1], v[0], v[4]], K3, True,
          d=5, failed={3: 3, 5: 3, 6: 2}, rep={5: 3, 6: 2})
    b.add(F, "a/all-collide", "dedup collision", "all collide", v[:70], K3, True, d=70, failed={69: 69, 64: 64, 1: 1})
    b.add(F, "a/no-collision", "dedup collision", "no collision", [others[0], others[1], others[0], others[2], others[1]], K3, True,
          d=3, failed={2: 0, 4: 0}, rep={2: 0, 4: 1})
    b.add(F, "a/AGA-CCC", "dedup collision", "collider in block", [b"AGA", b"CCC", b"AGA", b"CCC", b"CCC"], K3, True,
          d=2, failed={1: 1, 2: 0, 3: 1, 4: 1}, rep={2: 0, 3: 1, 4: 1})
    for L in (63, 64, 65, 66, 67):      # the pair differs in its last three bytes only: the comparison's first or second pass
        base = rand(rng, b"ACGT", L - 3)
        x, y = base + SWAP[0], base + SWAP[1]
        b.add(F, f"a/tail/L{L}", "dedup compare passes", f"len {L}", [x, y, x, y, base + b"TTT", y], K3, True,
              d=3, failed={1: 1, 2: 0, 3: 1, 5: 1}, rep={2: 0, 3: 1, 5: 1})


ALPHA9 = {"ascii": b"ACGKMNRTY", "high": bytes(range(0xF7, 0x100))}


def _family_b(b):
    """The alphabet of k_best_rep: `s_sigma <= 8` chooses three planes of `sigma & 7` codes or eight planes of raw bytes."""
    rng = np.random.default_rng(3302)
    for kind, a9 in ALPHA9.items():
        for sigma in (7, 8, 9):
            alpha = a9[9 - sigma:] if kind == "high" else a9[:sigma]
            for L in (1, 63, 64, 65, 130):
                base = rand(rng, alpha, L)
                g = [base, mutate(rng, base, 0.1, alpha), mutate(rng, base, 0.25, alpha), mutate(rng, base, 0.1, alpha, indel=0.0),
                     alpha, rand(rng, alpha, L), base]
                b.add("b", f"b/{kind}/s{sigma}/L{L}", "best_rep planes", f"sigma {sigma}", g, 5, True, sigma=sigma)
            # pairs over a part of the values inside a group that uses all of them; the smallest value against the largest (the
            # two that `& 7` would fold together at sigma 9)
            lo, hi = alpha[:1], alpha[-1:]
            g = [rand(rng, alpha[:4], 70), rand(rng, alpha[:4], 70), rand(rng, alpha[-3:], 66), lo * 65, hi * 65, lo * 33 + hi * 32,
                 alpha]
            b.add("b", f"b/{kind}/s{sigma}/part", "best_rep planes", f"sigma {sigma}", g, 5, True, sigma=sigma)
        a8, a9_ = (a9[1:], a9) if kind == "high" else (a9[:8], a9)
        for alpha, bits, ks in ((a8, 3, ((21, "63 bits"), (22, "66 bits general"))), (a9_, 4, ((16, "64 bits"), (17, "68 bits general")))):
            for k, side in ks:
                g = [rand(rng, alpha, 200), alpha, alpha[-1:] * (k + 3), rand(rng, alpha, k), rand(rng, alpha, k - 1)]
                g.append(g[0][50:150])
                b.add("b", f"b/{kind}/kmers/b{bits}/k{k}", f"code width {bits}", side, g, k, False, sigma=len(alpha), bits=bits,
                      state=GENERAL if "general" in side else HASHED)


def _family_c(b):
    """Table capacity: 3T/4 distinct keys fit, one more spills; the all-ones key is counted beside the table."""
    rng = np.random.default_rng(3303)
    s = distinct_run(rng, b"ACGT", 12, 385)
    b.add("c", "c/small/384", "small table capacity", "384 windows", [s[:-1]], 12, state=HASHED, table=SMALL_T, windows=384, distinct=384)
    b.add("c", "c/small/385", "small table capacity", "385 windows", [s], 12, state=HASHED, table=LARGE_T, windows=385, distinct=385)
    s = distinct_run(rng, b"ACGT", 12, 1537)
    b.add("c", "c/large/1536", "large table capacity", "1536 distinct", [s[:700], s[:-1], s[300:900]], 12,
          state=HASHED, table=LARGE_T, distinct=1536)
    b.add("c", "c/large/1537", "large table capacity", "1537 distinct", [s[:700], s, s[300:900]], 12,
          state=SPILLED, table=LARGE_T, distinct=1537)
    s = distinct_run(rng, b"ACGT", 32, 1537)                              # k * bits = 64: TTT...T packs to all ones
    ones = [b"T" * 40, b"T" * 32]
    b.add("c", "c/ones/1536", "all-ones beside a full table", "1536 + ones", [s[:-1]] + ones + [s[100:200]], 32,
          state=HASHED, table=LARGE_T, distinct=1536, ones=10)
    b.add("c", "c/ones/1537", "all-ones beside a full table", "1537 + ones", [s] + ones + [s[100:200]], 32,
          state=SPILLED, table=LARGE_T, distinct=1537, ones=10)


PROBE_ALPHA, PROBE_K, FILLER = b"ACGNT", 8, b"N"     # five values, three bits: 8-mers are 24-bit keys; N separates them


@functools.lru_cache(None)
def _probe_words():
    """All 5^8 8-mers over ACGNT as packed keys (codes 0..4 in 3-bit fields), with their digits."""
    idx = np.arange(5 ** PROBE_K, dtype=np.int64)
    digits = np.stack([(idx // 5 ** (PROBE_K - 1 - j)) % 5 for j in range(PROBE_K)], axis=1)
    keys = np.zeros(idx.shape[0], np.uint64)
    for j in range(PROBE_K):
        keys = (keys << np.uint64(3)) | digits[:, j].astype(np.uint64)
    return keys, digits.astype(np.uint8)


def _words_with_home(T: int, home: int, n: int) -> list[bytes]:
    """n 8-mers whose keys have the home slot `home` in a table of T slots (a table of 2 048 slots has only 32 such words
    without the filler, so a word may hold it)."""
    keys, digits = _probe_words()
    rows = np.flatnonzero(home_slot(keys, T) == home)[:n]
    assert rows.shape[0] == n
    return [_u8(PROBE_ALPHA)[digits[r]].tobytes() for r in rows]


def _embed(words, per: int) -> list[bytes]:
    """`per` words per string, separated by the filler (which takes part in the alphabet, so the codes stay three bits)."""
    return [FILLER.join(words[i:i + per]) for i in range(0, len(words), per)]


def _family_d(b):
    """Probe chains: a cluster that wraps from slot T - 1 to slot 0, and 64 keys with one home slot; two string orders."""
    for T, per in ((SMALL_T, 1), (LARGE_T, 8)):
        words = [w for slot in range(T - 4, T) for w in _words_with_home(T, slot, 3)]
        pad = _words_with_home(T, T // 2, 0 if per == 1 else 48)   # (the large table needs more than 384 windows)
        g = [PROBE_ALPHA] + _embed(words + pad, per)
        for order, grp in (("fwd", g), ("rev", g[::-1])):
            b.add("d", f"d/wrap/T{T}/{order}", "probe wrap", f"T {T}", grp, PROBE_K, state=HASHED, table=T, wraps=8, sigma=5)
        words = _words_with_home(T, 37, 64) + _words_with_home(T, 38, 8)
        pad = _words_with_home(T, T // 2, 0 if per == 1 else 8)
        g = [PROBE_ALPHA] + _embed(words + pad, per)
        for order, grp in (("fwd", g), ("rev", g[::-1])):
            b.add("d", f"d/chain/T{T}/{order}", "probe chain", f"T {T}", grp, PROBE_K, state=HASHED, table=T, chain=64, sigma=5)


def _family_e(b):
    """A lane rolls through kKmerRun = 8 windows; 256 lanes cover 2 048 windows of a string per round."""
    rng = np.random.default_rng(3305)
    for nw in (1, 7, 8, 9, 2047, 2048, 2049, 4097):
        seam = "run of 8" if nw < 10 else "second round"
        side = f"{nw} window" + ("s" if nw > 1 else "")
        tandem = (b"CAG" * (nw // 3 + 2))[:nw + 2]
        b.add("e", f"e/tandem/{nw}", seam, side, [tandem, b"ACGT"], 3, state=HASHED, windows=nw + 2)
        noise = rand(rng, b"ACGT", nw + 4)                                   # k = 5: at most 1 024 distinct keys
        b.add("e", f"e/random/{nw}", seam, side, [noise, b"ACGT"], 5, state=HASHED, windows=nw)


def _family_f(b):
    """Code widths of 2, 5 and 8 bits around k * bits = 64 (3 and 4 bits: family b)."""
    rng = np.random.default_rng(3306)
    a17, a129 = bytes(range(0x40, 0x51)), bytes(range(0x60, 0xE1))
    for alpha, bits, ks in ((b"ACG", 2, ((31, "62 bits"), (32, "64 bits"), (33, "66 bits general"))),
                            (a17, 5, ((12, "60 bits"), (13, "65 bits general"))),
                            (a129, 8, ((8, "64 bits"), (9, "72 bits general")))):
        for k, side in ks:
            base = rand(rng, alpha, 180)
            g = [base, alpha, alpha[-1:] * (k + 2), base[40:140], rand(rng, alpha, k), rand(rng, alpha, k - 1),
                 mutate(rng, base, 0.05, alpha)]
            b.add("f", f"f/b{bits}/k{k}", f"code width {bits}", side, g, k, sigma=len(alpha), bits=bits,
                  state=GENERAL if "general" in side else HASHED)


def _family_g(b):
    """k_kmers_sort: padding to a power of two, stretches of ceil(W / 1024) elements, runs."""
    rng = np.random.default_rng(3307)
    K = 33                                                                    # two bits per code: general
    for W in (1, 2, 3, 1023, 1024, 1025):
        b.add("g", f"g/general/W{W}", "sort padding", f"W {W}", [distinct_run(rng, b"ACGT", K, W)], K, state=GENERAL, windows=W)
    for W in (2047, 2048, 2049):
        b.add("g", f"g/spilled/W{W}", "sort stretches", f"W {W}", [distinct_run(rng, b"ACGT", 16, W)], 16,
              state=SPILLED, windows=W, distinct=W)
    p = rand(rng, b"ACGT", K - 1)
    g = [p + b"G", p + b"A", p + b"T", p + b"C", p + b"A", b"T" + p, b"A" + p]
    b.add("g", "g/general/prefix", "sort runs", "shared prefix", g, K, state=GENERAL, windows=7)
    s = distinct_run(rng, b"ACGT", K, 300)
    g = [s[100:], s, s[:250], rand(rng, b"ACGT", 90), s[40:140], s]
    b.add("g", "g/general/equal", "sort runs", "equal across strings", g, K, state=GENERAL)
    s = distinct_run(rng, b"ACGT", 16, 2000)
    b.add("g", "g/spilled/twice", "sort runs", "every window twice", [s, s], 16, state=SPILLED, windows=4000, distinct=2000)


def _family_h(b):
    """place = string index << 16 | i: the largest i and the largest string index, on the table and on the sort path."""
    rng = np.random.default_rng(3308)
    s = rand(rng, b"ACG", MAX_LEN - 1) + b"T"                                 # T only at i = 65 534
    b.add("h", "h/long/k1", "place i", "i 65534 k 1", [s], 1, state=HASHED, table=LARGE_T, windows=MAX_LEN, distinct=4)
    b.add("h", "h/long/k2", "place i", "i 65533 k 2", [s], 2, state=HASHED, table=LARGE_T, windows=MAX_LEN - 1)
    b.add("h", "h/long/k65534", "place i", "two windows", [s], MAX_LEN - 1, state=GENERAL, table=SMALL_T, windows=2)
    b.add("h", "h/long/k65535", "place i", "one window", [s], MAX_LEN, state=GENERAL, table=SMALL_T, windows=1)
    b.add("h", "h/long/k16", "place i", "sorted packed", [s], 16, state=SPILLED, windows=MAX_LEN - 15)
    b.add("h", "h/long/k33", "place i", "sorted general", [s], 33, state=GENERAL, windows=MAX_LEN - 32)
    g = [b"CAGCAG"] * 249 + [b"CAGTTT"]
    b.add("h", "h/str249/hashed", "place string", "hashed 249", g, 3, state=HASHED, table=LARGE_T, windows=1000, distinct=6)
    g = [rand(rng, b"ACGT", 20) for _ in range(250)]
    b.add("h", "h/str249/spilled", "place string", "spilled 249", g, 12, state=SPILLED, windows=2250)
    g = [rand(rng, b"ACGT", 40) for _ in range(250)]
    b.add("h", "h/str249/general", "place string", "general 249", g, 33, state=GENERAL, windows=2000)


@functools.lru_cache(None)
def cases() -> tuple[Case, ...]:
    b = _Builder()
    for fam in (_family_a, _family_b, _family_c, _family_d, _family_e, _family_f, _family_g, _family_h):
        fam(b)
    return tuple(b.cases)


def by_name(name: str) -> Case:
    return next(c for c in cases() if c.name == name)


def kmer_cases() -> list[Case]:
    return [c for c in cases() if c.k is not None]


def cons_cases() -> list[Case]:
    return [c for c in cases() if c.cons]


@functools.lru_cache(None)
def routes() -> dict[str, Route]:
    return {c.name: route(c.group, c.k) for c in kmer_cases()}


# The call of the cap-and-retry test: hashed, spilled and general groups in this order (the test adds one without a window)
CAP_CALL = ("e/tandem/9", "g/spilled/W2047", "c/small/385", "g/general/W1025", "a/AGA-CCC", "g/spilled/W2049", "g/general/W1",
            "c/ones/1536", "g/general/prefix")
CAP_WS_BYTES = 2048 * ELEM_BYTES      # one group of 2 048 padded elements per launch of the sort kernel
