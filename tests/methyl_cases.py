"""Shared by tests/test_methyl_rule.py, tests/test_methyl_host.py (CPU) and tests/test_gpu_methyl.py: seeded random reads with
MM / ML tags (well-formed and not), and a corpus of BAM records written with the project's writer, with the shapes at which
k_dbam_methyl can go wrong (taken from the size constants of the library as built).  Built once per process."""
import functools
import struct

import numpy as np

from strkit_amd.frontend import methyl as me
from strkit_amd.frontend.synth_methyl import encode_mm, mm_tags

CONTIG = ("chr1", 4_000_000)
OPS = "MIDNSHP=X"
EDGE_PROBS = (0, 127, 128, 255)


def int_tag(tag: bytes, ty: str, val: int) -> bytes:
    return tag + ty.encode() + struct.pack({"c": "<b", "C": "<B", "s": "<h", "S": "<H", "i": "<i", "I": "<I"}[ty], val)


def cigar_array(ops) -> np.ndarray:
    return np.array([(ln << 4) | OPS.index(op) for ln, op in ops], np.uint32)


def random_seq(rng, n: int) -> str:
    """CpG-rich, with a few bases that are no target (N, S)."""
    return "".join(rng.choice(list("ACGTNS"), n, p=[0.14, 0.34, 0.34, 0.14, 0.02, 0.02]))


def _noise(rng) -> bytes:
    k = int(rng.integers(0, 5))
    if k == 0:
        return b"RGZ" + bytes(rng.integers(65, 91, int(rng.integers(0, 9))).astype(np.uint8)) + b"\0"
    if k == 1:
        cnt = int(rng.integers(0, 7))
        return b"ZBBs" + struct.pack("<I", cnt) + bytes(rng.integers(0, 256, cnt * 2).astype(np.uint8))
    if k == 2:
        return b"MMi" + struct.pack("<i", 7)          # an MM that is no string: passed over
    if k == 3:
        return b"XFf" + struct.pack("<f", 1.5)
    return int_tag(b"NM", "i", int(rng.integers(0, 100)))


def _prob(rng) -> int:
    return int(rng.choice(EDGE_PROBS)) if rng.integers(0, 2) else int(rng.integers(0, 256))


def _decoy(rng) -> tuple[str, list[int], list[int]]:
    head, c = (("A+a", 1), ("C+h", 1), ("C+h.", 1), ("G-m", 1), ("G-m?", 1), ("C+76792", 1), ("T+gc", 2), ("C-m", 1), ("N+n?", 1))[int(rng.integers(9))]
    n = int(rng.integers(0, 6))
    return head, [int(x) for x in rng.integers(0, 12, n)], [_prob(rng) for _ in range(n * c)]


def random_tags(rng, seq: str, flag: int, p_good: float = 0.78) -> tuple[bytes, str]:
    """(auxiliary bytes, what they were built to be: "good", "none", "no_entry", "bad_text", "bad_ml", "past", "clipped")."""
    reverse = bool(flag & 16)
    target = "G" if reverse else "C"
    pos = [p for p in range(len(seq)) if seq[p] == target]
    rate = float(rng.choice([0.0, 0.3, 0.7, 1.0]))
    calls = {p: _prob(rng) for p in pos if rng.random() < rate}
    skips, probs = encode_mm(seq, reverse, calls)
    kind = "good" if rng.random() < p_good else str(rng.choice(["none", "no_entry", "bad_text", "bad_ml", "past", "clipped"]))
    head = "C+" + str(rng.choice(["m", "m", "m", "mh", "hm", "ahm"])) + str(rng.choice(["", ".", "?"]))
    c, j = len(head.rstrip(".?")) - 2, head.index("m") - 2
    if kind == "past":                                       # one more number: its ordinal is the number of targets
        skips, probs = skips + [len(pos) - sum(x + 1 for x in skips)], probs + [1]
    ml = []
    for x in probs:
        cell = [_prob(rng) for _ in range(c)]
        cell[j] = x
        ml += cell
    entries = [_decoy(rng) for _ in range(int(rng.integers(0, 3)) if rng.integers(0, 2) else 0)]
    if kind != "no_entry":
        entries.append((head, skips, ml))
        if rng.integers(0, 4) == 0:
            entries.append(_decoy(rng) if rng.integers(0, 2) else ("C+m", [0] * min(len(pos), 2), [9] * min(len(pos), 2)))   # a second C+m is not taken
    lower = kind == "good" and rng.integers(0, 8) == 0
    tags = mm_tags(entries, final_semicolon=bool(rng.integers(0, 4)), lower=lower)
    if kind == "none":
        tags = b""
    elif kind == "bad_text":
        z = tags.index(b"\0")
        text = tags[3:z]
        how = int(rng.integers(0, 6))
        if how == 0 and text:
            k = int(rng.integers(0, len(text)))
            text = text[:k] + bytes([int(rng.choice(list(b"x+, ;C?.-9")))]) + text[k + 1:]   # (may happen to stay well-formed)
        elif how == 1:
            text = text + b",12345678901"
        elif how == 2:
            text = text + b",2147483648"
        elif how == 3:
            text = b";" + text
        elif how == 4:
            text = text + b";;"
        else:
            text = text + b",-1"
        tags = b"MMZ" + text + b"\0" + tags[z + 1:]
    elif kind == "bad_ml":
        z = tags.index(b"\0") + 1
        cnt = struct.unpack_from("<I", tags, z + 4)[0]
        how = int(rng.integers(0, 3))
        if how == 0:
            tags = tags[:z + 3] + b"c" + tags[z + 4:]
        elif how == 1:
            tags = tags[:z + 4] + struct.pack("<I", cnt + 1) + tags[z + 8:] + b"\x07"
        else:
            tags = tags[:z]                                   # MM without ML
    elif kind == "clipped":
        tags += int_tag(b"MN", "cCsSiI"[int(rng.integers(2, 6))], len(seq) + int(rng.choice([-1, 1, 5])))
    elif rng.integers(0, 5) == 0:
        tags += int_tag(b"MN", "i", len(seq))                 # MN equal to l_seq changes nothing
    if rng.integers(0, 3) == 0 and tags:                      # ML in front of MM
        z = tags.index(b"\0") + 1
        tags = tags[z:] + tags[:z] if tags[:2] in (b"MM", b"Mm") and b"MN" not in tags else tags
    front = b"".join(_noise(rng) for _ in range(int(rng.integers(0, 3))))
    back = b"".join(_noise(rng) for _ in range(int(rng.integers(0, 2))))
    return front + tags + back, kind


# ---- the rule-level corpus: (seq, flag, cigar, tags, q_l, q_r) --------------------------------------------------------------
RULE_LENGTHS = (0, 1, 2, 3, 10, 63, 64, 65, 200)


@functools.lru_cache(maxsize=None)
def rule_corpus(n: int = 4000, seed: int = 20250117) -> list[tuple]:
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n):
        ln = int(rng.choice(RULE_LENGTHS, p=[0.02, 0.02, 0.04, 0.04, 0.16, 0.16, 0.16, 0.16, 0.24]))
        seq = random_seq(rng, ln)
        flag = 16 if rng.integers(0, 2) else 0
        tags, _ = random_tags(rng, seq, flag)
        q_l = int(rng.integers(0, ln + 1))
        q_r = int(rng.integers(q_l, ln + 1)) if rng.integers(0, 3) else ln
        cig = cigar_array([(5, "H"), (ln, "M")] if rng.integers(0, 40) == 0 else [(ln, "M")])
        if rng.integers(0, 50) == 0:
            q_l = q_r = None
        out.append((seq, flag, cig, tags, q_l, q_r))
    return out


# ---- the BAM-level corpus -----------------------------------------------------------------------------------------------------
def _aligned_record(rng, name: str, pos: int, seq: str, flag: int, tags: bytes, tract: tuple[int, int], shape: str) -> tuple[dict, list[int], tuple | None]:
    """A record whose alignment puts the read's [tract) onto a reference tract, the four locus boundaries, and a substitute
    alignment (shape "alt": the record itself is soft-clipped from the middle of the tract)."""
    n = len(seq)
    q_l, q_r = tract
    ins = int(rng.integers(0, 4)) if shape != "plain" and q_r - q_l >= 4 else 0      # bases inserted at the tract's right boundary
    dele = int(rng.integers(0, 4)) if shape != "plain" else 0                          # reference bases deleted inside the right flank
    ops = [(q_l, "M"), (q_r - q_l - ins, "M")] + ([(ins, "I")] if ins else [])
    right = n - q_r
    if dele and right >= 2:
        ops += [(1, "M"), (dele, "D"), (right - 1, "M")]
    else:
        dele = 0
        ops += [(right, "M")]
    lc, rc = pos + q_l, pos + q_r - ins
    ref_end = pos + n - ins + dele
    lfc = max(pos, lc - int(rng.integers(1, 30)))
    rfc = min(ref_end - 1, rc + dele + int(rng.integers(1, 30)))
    if rng.integers(0, 25) == 0:
        rfc = ref_end + 3                                                              # the read does not reach the right flank
    rec = {"name": name, "flag": flag, "contig": CONTIG[0], "pos": pos, "mapq": 60, "cigar": [o for o in ops if o[0] > 0 or o[1] != "M"], "seq": seq,
           "qual": None if rng.integers(0, 10) == 0 else rng.integers(0, 61, n).astype(np.uint8), "tags": tags}
    alt = None
    if shape == "long":
        rec["long_cigar"] = True
    elif shape == "alt":
        alt = (cigar_array(rec["cigar"]), pos)
        keep = q_l + (q_r - q_l) // 2
        rec["cigar"] = [(keep, "M"), (n - keep, "S")] if 0 < keep < n else rec["cigar"]
    elif shape == "hard":
        rec["cigar"] = [(4, "H")] + rec["cigar"]
    return rec, [lfc, lc, rc, rfc], alt


def _cg_read(n: int, at: list[int]) -> str:
    """n As with a CG at every position of `at`."""
    s = ["A"] * n
    for p in at:
        s[p], s[p + 1] = "C", "G"
    return "".join(s)


@functools.lru_cache(maxsize=None)
def corpus() -> dict:
    """records (in file order = item order), coords [n, 4], alt, kinds, and the constants the shapes were made for."""
    k = me.methyl_constants()
    chunk, seq_pass, mm_pass, window = k["chunk_bases"], k["seq_pass_bases"], k["mm_pass_bytes"], k["window"]
    rng = np.random.default_rng(20250118)
    recs, coords, alt, kinds = [], [], {}, []
    pos = 1000

    def add(seq, flag, tags, tract, shape="plain", kind="hand"):
        nonlocal pos
        rec, co, a = _aligned_record(rng, f"m{len(recs)}", pos, seq, flag, tags, tract, shape)
        if a is not None:
            alt[len(recs)] = a
        recs.append(rec)
        coords.append(co)
        kinds.append(kind)
        pos += int(rng.integers(0, 40))

    def all_called(seq, flag, mode="", decoys=()):
        target = "G" if flag & 16 else "C"
        calls = {p: EDGE_PROBS[p % 4] for p in range(len(seq)) if seq[p] == target}
        s, p = encode_mm(seq, bool(flag & 16), calls)
        return mm_tags(list(decoys) + [("C+m" + mode, s, p)])

    # ~400 loci of ~5 random reads
    for locus in range(400):
        for _ in range(int(rng.integers(4, 7))):
            n = int(rng.choice([8, 20, 63, 64, 65, 150, 400]))
            seq = random_seq(rng, n)
            flag = 16 if rng.integers(0, 2) else 0
            tags, kind = random_tags(rng, seq, flag, p_good=0.8)
            if rng.integers(0, 12) == 0:
                tags = b""                                        # a record without auxiliary data
                kind = "none"
            q_l = int(rng.integers(1, max(2, n // 2)))
            q_r = int(rng.integers(q_l, n - 1))
            shape = str(rng.choice(["plain", "indel", "indel", "long", "alt", "hard"], p=[0.3, 0.3, 0.15, 0.1, 0.1, 0.05]))
            add(seq, flag, tags, (q_l, q_r), shape, kind)
    for flag in (0, 16):
        # the bases per sequence pass: l_seq at K - 1, K, K + 1, every target called
        for n in (seq_pass - 1, seq_pass, seq_pass + 1):
            seq = random_seq(rng, n)
            add(seq, flag, all_called(seq, flag), (3, n - 2))
        # a CG whose C ends a lane's chunk, a CG across a pass, a G one past the tract, a C as the last base
        at = [chunk - 1, 3 * chunk - 1, seq_pass - 1, 2 * seq_pass - 1, 2 * seq_pass + 7]
        seq = _cg_read(2 * seq_pass + 40, at)
        for q_r in (2 * seq_pass + 20, 2 * seq_pass, seq_pass, 3 * chunk):          # (the last three end on a C whose G is outside)
            add(seq, flag, all_called(seq, flag, "?"), (1, q_r))
            add(seq, flag, mm_tags([("C+m?", [1, 1], [200, 100])]), (chunk - 1, q_r))
        add(seq[:-1] + "C", flag, all_called(seq[:-1] + "C", flag), (5, len(seq) - 1))
        # the MM pass: a number whose digits cross it, a ';' on its last byte, 0 / 1 / 63 / 64 / 65 / ~1000 numbers
        seq = "CG" * 1100
        target_pos = [p for p in range(len(seq)) if seq[p] == ("G" if flag else "C")]
        for n_num in (0, 1, mm_pass - 1, mm_pass, mm_pass + 1, 1000):
            order = target_pos[::-1] if flag else target_pos
            calls = {p: EDGE_PROBS[i % 4] for i, p in enumerate(order[:n_num])}
            s, p = encode_mm(seq, bool(flag), calls)
            add(seq, flag, mm_tags([("C+m", s, p)]), (2, 2100))
        calls = {p: 255 for p in (target_pos[::-1] if flag else target_pos)[10::11]}    # skips of two digits: ",10" is three bytes
        s, p = encode_mm(seq, bool(flag), calls)
        assert all(x == 10 for x in s)
        add(seq, flag, mm_tags([("C+m", s, p)]), (2, 2100))                             # a ',' on byte 63, its digits on 64 and 65
        pad = (mm_pass - 1 - 3) // 2                                                      # "A+a" + ",0" * pad + ";": the ';' is byte 63
        add(seq, flag, mm_tags([("A+a", [0] * pad, [5] * pad), ("C+m", s, p)]), (2, 2100))
        add(seq, flag, mm_tags([("A+a", [0] * pad, [5] * pad), ("C+m.", [], [])]), (2, 200))   # an entry with no numbers
        add(seq, flag, mm_tags([("C+m?", [], [])], final_semicolon=False), (2, 200))
        # the ordinal window: a tract with K - 1, K, K + 1 targets (and calls on both sides of every window's edge)
        seq = "A" * 37 + "CG" * (2 * window + 50) + "A" * 30
        for n_t in (window - 1, window, window + 1, 2 * window + 3):
            for shift in (0, 5):
                q_l = 37 + 2 * shift
                add(seq, flag, all_called(seq, flag), (q_l, q_l + 2 * n_t))
        calls = {p: 255 for p in (37 + 2 * i + (1 if flag else 0) for i in (0, window - 1, window, window + 1, 2 * window - 1, 2 * window))}
        s, p = encode_mm(seq, bool(flag), calls)
        for mode in ("?", "."):
            add(seq, flag, mm_tags([("C+m" + mode, s, p)]), (37, 37 + 2 * (2 * window + 10)))
    return {"records": recs, "coords": np.array(coords, np.int64), "alt": alt, "kinds": kinds, "constants": k}


@functools.lru_cache(maxsize=None)
def expected() -> dict:
    """The rule (frontend/methyl.py) on every item of the corpus, from the records as written."""
    from strkit_amd.frontend.bam import AlignedSegment
    c = corpus()
    out = {k: np.zeros(len(c["records"]), np.int32) for k in ("status", "sites", "known", "mc")}
    for i, r in enumerate(c["records"]):
        tags = r.get("tags", b"")
        own = cigar_array(r["cigar"])
        seg = AlignedSegment(r["name"], r["flag"], r["contig"], r["pos"], 60, own, r["seq"], r["qual"], tags)
        got = me.segment_methylation(seg, c["coords"][i], c["alt"].get(i))
        for k, v in zip(("status", "sites", "known", "mc"), got):
            out[k][i] = v
    return out


def raw_record(pos: int, cigar: list[int], seq: bytes, l_seq: int, tags: bytes, flag: int = 0, name: bytes = b"r\0") -> bytes:
    """One BAM alignment record (with its block_size) with the packed bases `seq` and quality 30."""
    body = struct.pack("<iiBBHHHIiii", 0, pos, len(name), 60, 4680, len(cigar), flag, l_seq, -1, -1, 0)
    body += name + b"".join(struct.pack("<I", c) for c in cigar) + seq + bytes([30]) * l_seq + tags
    return struct.pack("<i", len(body)) + body
