"""Shared by tests/test_snv_discover_rule.py, test_snv_discover_host.py (CPU) and test_gpu_snv_discover.py: a corpus of
hand-made loci written with write_bam, each aimed at one place where the pileup of strk_snv_discover.h can go wrong (window
and tile edges, operations against tiles and wave passes, CIGAR content, base codes and qualities, counts at the thresholds,
the nearest-1 024 rule), and what frontend/snv_discovery.py (the readable statement of the rule) gives for it.  One contig,
37 loci, at most 65 reads a locus, reads of at most 3 kb; windows of 8 192 (two whole tiles a side) and 5 000 (a whole tile and
a part of one) run over the same file.  Built once per process."""
import functools

import numpy as np

from strkit_amd.frontend import phase_inputs as pi
from strkit_amd.frontend import snv_discovery as sd
from strkit_amd.frontend.bam import AlignedSegment

CONTIG = ("chr1", 900000)
WINDOWS = (8192, 5000)
MIN_BASE_QUAL = 20
MIN_ALLELE_READS = 2
LOCUS_LEN = 60
_REF = np.random.default_rng(20250117).choice(list("ACGT"), CONTIG[1])
_OPS = "MIDNSHP=X"


def alt_base(p: int) -> str:
    return {"A": "C", "C": "G", "G": "T", "T": "A"}[_REF[p]]


def third_base(p: int) -> str:
    return {"A": "G", "C": "T", "G": "A", "T": "C"}[_REF[p]]


def make_read(name: str, start: int, cigar, over=None, quals=None, drop: int = 0, qual=True) -> dict:
    """A record along `cigar` from `start`: reference bases under the aligned operations except over[p], quality 30 except
    quals[p]; inserted bases are the ALT of the next reference position (a walk that is off by the insertion reads an ALT),
    clipped bases G.  drop: bases left off the end (a CIGAR longer than its sequence)."""
    over, quals = over or {}, quals or {}
    seq, q, r = [], [], start
    for ln, op in cigar:
        if op in "M=X":
            for p in range(r, r + ln):
                seq.append(over.get(p, _REF[p]))
                q.append(quals.get(p, 30))
        elif op == "I":
            seq.extend(alt_base(r) * ln)
            q.extend([30] * ln)
        elif op == "S":
            seq.extend("G" * ln)
            q.extend([30] * ln)
        if op in "MDN=X":
            r += ln
    if drop:
        seq, q = seq[:-drop], q[:-drop]
    return {"name": name, "flag": 0, "contig": CONTIG[0], "pos": int(start), "mapq": 60, "cigar": list(cigar), "seq": "".join(seq),
            "qual": np.array(q, np.uint8) if qual else None, "tags": b""}


def pile(prefix: str, start: int, cigar, n: int, sites=None, qsites=None, **kw) -> list[dict]:
    """n reads of one alignment; sites[p] = the n bases the reads carry at p (None: the reference base), qsites[p] = their qualities."""
    sites, qsites = sites or {}, qsites or {}
    return [make_read(f"{prefix}_{j}", start, cigar, {p: b[j] for p, b in sites.items() if b[j] is not None},
                      {p: v[j] for p, v in qsites.items()}, **kw) for j in range(n)]


def het(p: int, n: int, k: int, extra: int = 0) -> list:
    """k of n reads carry the ALT at p (the first k), `extra` more a third base, the rest the reference base."""
    return [alt_base(p)] * k + [third_base(p)] * extra + [None] * (n - k - extra)


def op_starts(start: int, cigar) -> list[int]:
    out, r = [], start
    for ln, op in cigar:
        out.append(r)
        r += ln if op in "MDN=X" else 0
    return out


def many_ops(n_ops: int) -> list:
    """6M 1I 6M 1D ... : n_ops operations, the even ones aligned"""
    return [(6, "M") if k % 2 == 0 else (1, "ID"[(k // 2) % 2]) for k in range(n_ops)]


@functools.lru_cache(maxsize=None)
def corpus() -> dict:
    loci: list[dict] = []

    def locus(name, left, reads, want=None, kept=None, allowed=True, alt=None, right=None):
        loci.append({"name": name, "left": left, "right": left + LOCUS_LEN if right is None else right, "reads": reads, "want": want,
                     "kept": list(range(len(reads))) if kept is None else kept, "allowed": allowed, "alt": alt or {}})

    base = iter(range(20000, CONTIG[1], 20000))
    M = lambda ln: [(ln, "M")]  # noqa: E731

    # -- window and tile edges ------------------------------------------------------------------------------------------------
    # a window cut at position 0: left = 3000, sites at 0 and 5 (and the locus's left window is [0, 3000) under both windows)
    L = 3000
    locus("cut_at_0", L, pile("cut0", 0, M(300), 10, {0: het(0, 10, 5), 5: het(5, 10, 4), 299: het(299, 10, 2)}), want={8192: [0, 5, 299], 5000: [0, 5, 299]})
    # the far edge of either window on the left: left - w - 1 is outside, left - w inside
    L = next(base)
    a, b = L - 8192, L - 5000
    locus("left_far", L, pile("lf8", a - 150, M(300), 10, {a - 1: het(a - 1, 10, 5), a: het(a, 10, 5)})
          + pile("lf5", b - 150, M(300), 10, {b - 1: het(b - 1, 10, 5), b: het(b, 10, 5)}), want={8192: [a, b - 1, b], 5000: [b]})
    # around the flanked locus: left - 1 and right are candidates, nothing in [left, right) is
    L = next(base)
    R = L + LOCUS_LEN
    s = {p: het(p, 10, 5) for p in (L - 700, L - 1, L, L + 30, R - 1, R, R + 700)}
    locus("near", L, pile("near", L - 1500, M(3000), 10, s), want={w: [L - 700, L - 1, R, R + 700] for w in WINDOWS})
    # the far edge on the right: right + w - 1 inside, right + w outside
    L = next(base)
    R = L + LOCUS_LEN
    a, b = R + 8192, R + 5000
    locus("right_far", L, pile("rf8", a - 150, M(300), 10, {a - 1: het(a - 1, 10, 5), a: het(a, 10, 5)})
          + pile("rf5", b - 150, M(300), 10, {b - 1: het(b - 1, 10, 5), b: het(b, 10, 5)}), want={8192: [b - 1, b, a - 1], 5000: [b - 1]})
    # tile seams, an aligned operation across each: 8 192: left - 4097 | left - 4096; 5 000: left - 905 | left - 904 (the second
    # tile of that window has 904 positions: a window that is no multiple of the tile)
    L = next(base)
    a, b = L - 4096, L - 904
    locus("left_seams", L, pile("ls8", a - 150, M(300), 10, {a - 1: het(a - 1, 10, 5), a: het(a, 10, 4)})
          + pile("ls5", b - 150, M(300), 10, {b - 1: het(b - 1, 10, 4), b: het(b, 10, 5)}), want={w: [a - 1, a, b - 1, b] for w in WINDOWS})
    L = next(base)
    R = L + LOCUS_LEN
    a = R + 4096
    locus("right_seam", L, pile("rs", a - 2000, M(2500), 10, {a - 1: het(a - 1, 10, 5), a: het(a, 10, 5), a + 499: het(a + 499, 10, 5)}),
          want={w: [a - 1, a, a + 499] for w in WINDOWS})

    # -- operations against the switch between one lane and all lanes, and against the passes of 64 operations ------------
    L = next(base)
    cig = [(63, "M"), (1, "D"), (64, "M"), (1, "I"), (65, "M"), (2, "D"), (63, "="), (1, "I"), (64, "X"), (1, "D"), (65, "M")]
    st = op_starts(L - 600, cig)
    sites = {}
    for (ln, op), r0 in zip(cig, st):
        if op in "M=X":
            sites[r0] = het(r0, 10, 5)
            sites[r0 + ln - 1] = het(r0 + ln - 1, 10, 4)
    locus("ops_63_64_65", L, pile("o636465", L - 600, cig, 10, sites), want={w: sorted(sites) for w in WINDOWS})
    for n_ops in (64, 65, 130):
        L = next(base)
        cig = many_ops(n_ops)
        st = op_starts(L - 700, cig)
        sites = {st[k] + 2: het(st[k] + 2, 10, 5) for k in (0, 2, 62, 64, 66, 126, 128) if k < n_ops}
        locus(f"ops_{n_ops}", L, pile(f"ops{n_ops}", L - 700, cig, 10, sites), want={w: sorted(sites) for w in WINDOWS})

    # -- reads against the four waves of a workgroup ------------------------------------------------------------------------
    for n, k, want in ((3, 1, False), (4, 2, True), (5, 2, True)):     # n = 3: a_thr = min_allele_reads = 2 > rint(3 / 5), and 1 < 2
        L = next(base)
        locus(f"reads_{n}", L, pile(f"n{n}", L - 500, M(1000), n, {L - 100: het(L - 100, n, k)}), want={w: [L - 100] if want else [] for w in WINDOWS})
    L = next(base)           # 65 reads: a_thr = 13
    locus("reads_65", L, pile("n65", L - 500, M(1000), 65, {L - 100: het(L - 100, 65, 13), L - 90: het(L - 90, 65, 12)}), want={w: [L - 100] for w in WINDOWS})

    # -- CIGAR content ------------------------------------------------------------------------------------------------------------
    # under D and under N: four reads have the gap at p, and the base behind the gap is p's ALT; one read carries the ALT
    for gap in "DN":
        L = next(base)
        p = L - 200
        plain = pile(f"g{gap}a", L - 500, M(1000), 6, {p: het(p, 6, 1)})
        cig = [(300, "M"), (1, gap), (699, "M")]
        gapped = pile(f"g{gap}b", L - 500, cig, 4, {p + 1: [alt_base(p)] * 4})
        behind = [p + 1] if alt_base(p) != _REF[p + 1] else []      # (that base makes p + 1 a site of its own, unless it is the reference's)
        locus(f"under_{gap}", L, plain + gapped, want={w: behind for w in WINDOWS})
    L = next(base)           # right after an insertion (whose bases are the ALT of the site)
    p = L - 200
    cig = [(300, "M"), (3, "I"), (700, "M")]
    locus("after_I", L, pile("afterI", L - 500, cig, 10, {p: het(p, 10, 5)}), want={w: [p] for w in WINDOWS})
    L = next(base)           # zero-length operations, H in front (the S behind it is then not the first operation: no take-in)
    cig = [(5, "H"), (100, "S"), (0, "M"), (200, "M"), (0, "D"), (0, "I"), (0, "N"), (300, "M"), (0, "M")]
    locus("zero_H", L, pile("zeroH", L - 400, cig, 10, {L - 400: het(L - 400, 10, 5), L - 200: het(L - 200, 10, 5)}), want={w: [L - 400, L - 200] for w in WINDOWS})
    for clip, take in ((100, 250), (99, 0)):
        L = next(base)       # a left clip: lo = start + take
        s0 = L - 650
        sites = {p: het(p, 10, 5) for p in (s0, s0 + 249, s0 + 250)}
        locus(f"clip_left_{clip}", L, pile(f"cl{clip}", s0, [(clip, "S"), (600, "M")], 10, sites), want={w: [p for p in sorted(sites) if p >= s0 + take] for w in WINDOWS})
        L = next(base)       # a right clip: hi = end - take
        s0 = L + LOCUS_LEN
        e = s0 + 600
        sites = {p: het(p, 10, 5) for p in (e - 251, e - 250, e - 1)}
        locus(f"clip_right_{clip}", L, pile(f"cr{clip}", s0, [(600, "M"), (clip, "S")], 10, sites), want={w: [p for p in sorted(sites) if p < e - take] for w in WINDOWS})
    L = next(base)           # substitute alignments: reads 0 .. 3 are walked one base to the right of where their records say
    p = L - 300
    reads = pile("sub", L - 600, M(500), 10, {p: het(p, 10, 4)})
    sub = {j: (np.array([(500 << 4)], np.uint32), L - 599) for j in range(4)}
    locus("substitute", L, reads, alt=sub)
    L = next(base)           # a CIGAR longer than its sequence: the last 100 aligned pairs have no base
    s0 = L - 800
    sites = {p: het(p, 10, 5) for p in (s0 + 599, s0 + 600)}
    locus("long_cigar", L, pile("lc", s0, M(700), 10, sites, drop=100), want={w: [s0 + 599] for w in WINDOWS})

    # -- bases and qualities ------------------------------------------------------------------------------------------------------
    L = next(base)           # 22 reads, a_thr = 4: all sixteen codes at p (A x 4, C x 4, the others once); at p + 7 A x 4 and M x 4
    p = L - 300
    codes = ["A"] * 4 + ["C"] * 4 + list("GT=MRSVWYHKDBN")
    locus("sixteen_codes", L, pile("codes", L - 600, M(500), 22, {p: codes, p + 7: ["A"] * 4 + ["M"] * 4 + ["N"] * 14}), want={w: [p] for w in WINDOWS})
    L = next(base)           # without qualities every A C G T counts
    p = L - 300
    locus("no_qual", L, pile("noq", L - 600, M(500), 10, {p: het(p, 10, 5)}, qual=False), want={w: [p] for w in WINDOWS})
    L = next(base)           # the ALT bases at min_base_qual (counted) and one below (not counted)
    p = L - 300
    locus("qual_edge", L, pile("qe", L - 600, M(500), 10, {p: het(p, 10, 5), p + 9: het(p + 9, 10, 5)},
                               {p: [MIN_BASE_QUAL] * 5 + [30] * 5, p + 9: [MIN_BASE_QUAL - 1] * 5 + [30] * 5}), want={w: [p] for w in WINDOWS})

    # -- counts and thresholds ----------------------------------------------------------------------------------------------------
    L = next(base)           # n = 10, a_thr = 2: 2 / 8; 1 / 9; three bases at the threshold; 1 + 1 / 8
    p = L - 300
    sites = {p: het(p, 10, 2), p + 5: het(p + 5, 10, 1), p + 10: het(p + 10, 10, 2, 2), p + 15: het(p + 15, 10, 1, 1)}
    locus("at_threshold", L, pile("thr", L - 600, M(500), 10, sites), want={w: [p, p + 10] for w in WINDOWS})
    for n, a_thr in ((9, 2), (12, 2), (13, 3)):      # rint(n / 5) = 2, 2, 3
        L = next(base)
        p = L - 300
        sites = {p: het(p, n, a_thr), p + 5: het(p + 5, n, a_thr - 1)}
        locus(f"n_{n}", L, pile(f"cnt{n}", L - 600, M(500), n, sites), want={w: [p] for w in WINDOWS})

    # -- loci -----------------------------------------------------------------------------------------------------------------------
    L = next(base)
    p = L - 300
    locus("no_kept_read", L, pile("nokept", L - 600, M(500), 10, {p: het(p, 10, 5)}), kept=[], want={w: [] for w in WINDOWS})
    L = next(base)
    p = L - 300
    locus("gate", L, pile("gate", L - 600, M(500), 10, {p: het(p, 10, 5)}), allowed=False, want={w: [] for w in WINDOWS})
    L = next(base)           # two loci 400 apart that share their reads; the second's flanked locus hides a site of the first
    reads = pile("shared", L - 1000, M(2500), 10, {p: het(p, 10, 5) for p in (L - 50, L + 420, L + 700)})
    locus("shared_a", L, reads, want={w: [L - 50, L + 420, L + 700] for w in WINDOWS})
    locus("shared_b", L + 400, reads, want={w: [L - 50, L + 700] for w in WINDOWS})
    L = next(base)           # homozygous ALT: every read agrees
    p = L - 300
    locus("hom_alt", L, pile("hom", L - 600, M(500), 10, {p: het(p, 10, 10), p + 5: het(p + 5, 10, 5)}), want={w: [p + 5] for w in WINDOWS})
    # the nearest-1 024 rule: 1 101 heterozygous positions, at distance 1 on the left and at every even distance 2 .. 1 100 on both
    # sides: L1, then pairs at one distance; the 1 024th place goes to the left one of the pair at 1 024
    L = next(base)
    R = L + LOCUS_LEN
    pos = [L - 1] + [L - d for d in range(2, 1101, 2)] + [R - 1 + d for d in range(2, 1101, 2)]
    keep = [L - 1] + [L - d for d in range(2, 1025, 2)] + [R - 1 + d for d in range(2, 1023, 2)]
    locus("nearest_1024", L, pile("near1024", L - 1470, M(3000), 24, {p: het(p, 24, 12) for p in pos}), want={w: sorted(keep) for w in WINDOWS})
    assert len(pos) == 1101 and len(keep) == pi.MAX_CANDIDATES

    # the file is coordinate-sorted; items keep the loci's order (a shared record is an item of both loci)
    by_name: dict[str, dict] = {}
    for lc in loci:
        for r in lc["reads"]:
            by_name.setdefault(r["name"], r)
    records = sorted(by_name.values(), key=lambda r: r["pos"])
    file_index = {r["name"]: k for k, r in enumerate(records)}
    item_locus, item_file, kept_item, kept_n, alt, entries, kept_entries = [], [], [], [], {}, [], []
    for l, lc in enumerate(loci):
        first = len(item_locus)
        segs = [AlignedSegment(r["name"], 0, CONTIG[0], r["pos"], 60, np.array([(ln << 4) | _OPS.index(op) for ln, op in r["cigar"]], np.uint32),
                               r["seq"], r["qual"]) for r in lc["reads"]]
        for j, r in enumerate(lc["reads"]):
            item_locus.append(l)
            item_file.append(file_index[r["name"]])
            if j in lc["alt"]:
                alt[first + j] = lc["alt"][j]
        use = lc["kept"] if lc["allowed"] else []
        kept_item.extend(first + j for j in use)
        kept_n.append(len(use))
        entries.append([(s_, False) for s_ in segs])
        kept_entries.append([(segs[j], lc["alt"].get(j, False)) for j in lc["kept"]])
    return {"records": records, "loci": loci, "n_loci": len(loci), "item_locus": np.array(item_locus, np.int32),
            "item_file_index": np.array(item_file, np.int64), "left": np.array([lc["left"] for lc in loci], np.int64),
            "right": np.array([lc["right"] for lc in loci], np.int64), "kept_off": np.concatenate(([0], np.cumsum(kept_n))).astype(np.int32),
            "kept_item": np.array(kept_item, np.int32), "alt": alt, "entries": entries, "kept_entries": kept_entries}


@functools.lru_cache(maxsize=None)
def expected(window: int) -> tuple[np.ndarray, np.ndarray]:
    """(cand_off, cand_pos) of the rule (frontend/snv_discovery.py) over the corpus."""
    c = corpus()
    per = [sd.discover_candidates(c["entries"][l], c["kept_entries"][l], lc["left"], lc["right"], window, MIN_BASE_QUAL, MIN_ALLELE_READS,
                                  allowed=lc["allowed"]) for l, lc in enumerate(c["loci"])]
    return np.concatenate(([0], np.cumsum([p.size for p in per]))).astype(np.int32), np.concatenate(per).astype(np.int64)


def library(bam, window: int, **kw) -> tuple[np.ndarray, np.ndarray]:
    """The library's function for `bam` (a NativeBam or a DeviceBam of the corpus's file) over the whole corpus."""
    c = corpus()
    return sd.library_discover_snvs(bam, c["item_file_index"], c["item_locus"], c["left"], c["right"], c["kept_off"], c["kept_item"], alt=c["alt"],
                                    window=window, min_base_qual=MIN_BASE_QUAL, min_allele_reads=MIN_ALLELE_READS, **kw)
