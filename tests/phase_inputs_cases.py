"""Shared by tests/test_phase_inputs_host.py (CPU) and tests/test_gpu_phase_inputs.py: a seeded corpus of random and
hand-made alignments with candidate SNV positions, written with write_bam, and what frontend/phase_inputs.py (the readable
statement of the rule) gives for it.  Built once per process."""
import functools
import struct

import numpy as np

from strkit_amd.frontend import phase_inputs as pi

CONTIG = ("chr1", 200000)
N_RANDOM = 2100
_CODES = "=ACMGRSVTWYHKDBN"


def int_tag(tag: bytes, ty: str, val: int) -> bytes:
    fmt = {"c": "<b", "C": "<B", "s": "<h", "S": "<H", "i": "<i", "I": "<I"}[ty]
    return tag + ty.encode() + struct.pack(fmt, val)


def _noise_tag(rng) -> bytes:
    k = int(rng.integers(0, 6))
    if k == 0:
        return b"RGZ" + bytes(rng.integers(65, 91, int(rng.integers(0, 9))).astype(np.uint8)) + b"\0"
    if k == 1:
        sub = "cCsSiIf"[int(rng.integers(0, 7))]
        es = {"c": 1, "C": 1, "s": 2, "S": 2}.get(sub, 4)
        cnt = int(rng.integers(0, 7))
        return b"ZBB" + sub.encode() + struct.pack("<I", cnt) + bytes(rng.integers(0, 256, cnt * es).astype(np.uint8))
    if k == 2:
        return b"XAA" + b"Q"
    if k == 3:
        return b"XFf" + struct.pack("<f", 1.5)
    if k == 4:
        return b"MMH" + b"1AE3" + b"\0"
    return int_tag(b"NM", "i", int(rng.integers(0, 100)))


def random_tags(rng, types=None) -> tuple[bytes, tuple[int, int]]:
    """(auxiliary bytes, the (HP, PS) they mean)"""
    parts, want = [], (-1, -1)
    mode = int(rng.integers(0, 5))          # 0 none, 1 HP only, 2 PS only, 3-4 both
    for _ in range(int(rng.integers(0, 3))):
        parts.append(_noise_tag(rng))
    hp = ps = None
    rng_of = {"c": (-5, 100), "C": (0, 255), "s": (-5, 30000), "S": (0, 65535), "i": (-5, 2**31 - 1), "I": (0, 2**32 - 1)}
    if mode in (1, 3, 4):
        ty = types[0] if types else "cCsSiI"[int(rng.integers(0, 6))]
        hp = int(rng.integers(1, 3))
        parts.append(int_tag(b"HP", ty, hp))
    for _ in range(int(rng.integers(0, 2))):
        parts.append(_noise_tag(rng))
    if mode in (2, 3, 4):
        ty = types[1] if types else "cCsSiI"[int(rng.integers(0, 6))]
        lo, hi = rng_of[ty]
        ps = int(rng.integers(max(lo, 0), hi + 1)) if rng.integers(0, 4) else hi
        parts.append(int_tag(b"PS", ty, ps))
        if ps > 2**31 - 1:
            ps = None
    for _ in range(int(rng.integers(0, 2))):
        parts.append(_noise_tag(rng))
    if hp is not None and ps is not None:
        want = (hp, ps)
    return b"".join(parts), want


def random_cigar(rng, n_ops: int) -> list[tuple[int, str]]:
    if n_ops == 0:
        return []
    clip = lambda: int(rng.choice([3, 40, 99, 100, 101, 300]))  # noqa: E731
    ops = []
    body = n_ops
    head, tail = [], []
    if body >= 3 and rng.integers(0, 2):
        head.append((clip(), "S"))
        body -= 1
    if body >= 3 and rng.integers(0, 2):
        tail.append((clip(), "S"))
        body -= 1
    if body >= 3 and rng.integers(0, 8) == 0:
        head.insert(0, (7, "H"))
        body -= 1
    long_m = n_ops <= 8                      # few operations: long matches, so that the clip take-in leaves something
    for k in range(body):
        op = "M" if k % 2 == 0 and rng.integers(0, 4) else "M=XIDNIDP"[int(rng.integers(0, 9))]
        ln = int(rng.integers(0, 2)) if rng.integers(0, 25) == 0 else int(rng.integers(1, 400 if (long_m and op in "M=X") else 25))
        ops.append((ln, op))
    return head + ops + tail


def _record(rng, name: str, pos: int, cigar, tags: bytes, qual="random", long_cigar=False, seq=None) -> dict:
    n_q = sum(ln for ln, op in cigar if op in "MIS=X")
    seq = seq or "".join(_CODES[int(c)] for c in np.where(rng.integers(0, 12, n_q) == 0, rng.integers(0, 16, n_q), rng.choice([1, 2, 4, 8], n_q)))
    q = None if qual is None else rng.integers(0, 61, n_q).astype(np.uint8)
    r = {"name": name, "flag": 0, "contig": CONTIG[0], "pos": int(pos), "mapq": 60, "cigar": cigar, "seq": seq, "qual": q, "tags": tags}
    if long_cigar:
        r["long_cigar"] = True
    return r


def _span(r: dict) -> tuple[int, int]:
    return r["pos"], r["pos"] + sum(ln for ln, op in r["cigar"] if op in "MDN=X")


# hand vectors: every position around the alignment is a candidate, so that the first / last aligned base, the first / last
# base of every operation, D, N, the neighbours of I, odd and even read positions, lo - 1, lo, hi - 1 and hi are all there
HAND_CIGARS = [
    [(100, "S"), (300, "M"), (2, "D"), (300, "M"), (100, "S")],
    [(99, "S"), (300, "M"), (2, "D"), (300, "M"), (99, "S")],
    [(100, "S"), (280, "="), (3, "I"), (5, "X"), (4, "N"), (290, "M"), (99, "S")],
    [(5, "H"), (100, "S"), (600, "M")],                       # the clip is not the first operation: no take-in
    [(3, "D"), (10, "M"), (2, "I"), (7, "M"), (5, "N"), (1, "M"), (4, "D")],   # D before the first and after the last aligned pair
    [(10, "M")], [(10, "S")], [(4, "D")], [],
    [(100, "S"), (200, "M"), (100, "S")],                     # the two take-ins cross: lo > hi
    [(0, "M"), (12, "M"), (0, "D"), (0, "I"), (9, "M")],
]


@functools.lru_cache(maxsize=None)
def corpus() -> dict:
    """records (in file order), item_locus, cand_off, cand_pos, alt, want_tags and the rule's hp / ps / cells."""
    rng = np.random.default_rng(20240611)
    loci: list[tuple[list[dict], np.ndarray]] = []      # (records, candidates)

    def dense(recs, margin=3):
        lo = min(_span(r)[0] for r in recs) - margin
        hi = max(_span(r)[1] for r in recs) + margin
        return np.arange(lo, hi, dtype=np.int64)

    for k, cig in enumerate(HAND_CIGARS):
        recs = [_record(rng, f"hand{k}", 1000 + k, cig, int_tag(b"HP", "C", 1) + int_tag(b"PS", "i", 1000 + k))]
        recs.append(_record(rng, f"hand{k}nq", 1001 + k, cig, b"", qual=None))
        loci.append((recs, dense(recs)))
    # CIGARs of 0, 1, 63, 64, 65, 129 (and 128, 130, 200) operations; a CG-tag long CIGAR; tags behind a Z and a B field
    for k, n_ops in enumerate([0, 1, 63, 64, 65, 128, 129, 130, 200]):
        recs = [_record(rng, f"ops{n_ops}_{j}", 3000 + 10 * k + j, random_cigar(rng, n_ops), random_tags(rng)[0]) for j in range(3)]
        loci.append((recs, dense(recs)[:pi.MAX_CANDIDATES]))
    recs = [_record(rng, f"long{j}", 5000 + j, random_cigar(rng, n), int_tag(b"HP", "s", 2) + int_tag(b"PS", "S", 777), long_cigar=True)
            for j, n in enumerate([5, 64, 70])]
    loci.append((recs, dense(recs)[:pi.MAX_CANDIDATES]))
    want_tags: dict[str, tuple[int, int]] = {}
    recs = []
    for j, (t_hp, t_ps) in enumerate([(a, b) for a in "cCsSiI" for b in "cCsSiI"]):
        tags = (b"RGZgroup\0" + b"ZBBs" + struct.pack("<I", 3) + b"\1\0\2\0\3\0" + int_tag(b"HP", t_hp, 1 + j % 2) + b"XAAx" + int_tag(b"PS", t_ps, 60 + j))
        recs.append(_record(rng, f"types{j}", 6000 + j, [(50, "M")], tags))
        want_tags[f"types{j}"] = (1 + j % 2, 60 + j)
    for j, (tags, want) in enumerate([(int_tag(b"HP", "C", 1), (-1, -1)), (int_tag(b"PS", "i", 5), (-1, -1)), (b"", (-1, -1)),
                                      (int_tag(b"HP", "C", 2) + int_tag(b"PS", "I", 2**31), (-1, -1)),
                                      (int_tag(b"HP", "C", 2) + int_tag(b"PS", "I", 2**31 - 1), (2, 2**31 - 1)),
                                      (b"HPZ1\0" + int_tag(b"PS", "i", 5), (-1, -1)), (b"HPf\0\0\0\0" + int_tag(b"PS", "i", 5), (-1, -1)),
                                      (int_tag(b"HP", "c", 1) + int_tag(b"HP", "c", 2) + int_tag(b"PS", "i", 9), (1, 9))]):
        recs.append(_record(rng, f"tagcase{j}", 6100 + j, [(50, "M")], tags))
        want_tags[f"tagcase{j}"] = want
    loci.append((recs, np.array([6010, 6050, 6120], np.int64)))
    # loci of 1 024, 1 and 0 candidates
    recs = [_record(rng, f"many{j}", 8000 + j, [(700, "M"), (30, "D"), (700, "M")], b"") for j in range(2)]
    loci.append((recs, dense(recs)[100:100 + pi.MAX_CANDIDATES]))
    loci.append(([_record(rng, "one", 9000, [(30, "M")], b"")], np.array([9007], np.int64)))
    loci.append(([_record(rng, "none", 9100, [(30, "M")], b"")], np.zeros(0, np.int64)))
    # two haplotypes that differ at 80 (more than the 64 that are taken) and at 10 positions, twelve reads each way
    for k, n_het in enumerate([80, 10]):
        hap = rng.choice(list("ACGT"), 400)
        other = hap.copy()
        het = rng.choice(400, n_het, replace=False)
        other[het] = [{"A": "C", "C": "G", "G": "T", "T": "A"}[b] for b in hap[het]]
        recs = [_record(rng, f"hap{k}_{j}", 12000 + 1000 * k + j % 3, [(2, "S"), (400 - j % 3, "M")], b"", seq="NN" + "".join((hap, other)[j % 2][j % 3:]))
                for j in range(24)]
        loci.append((recs, dense(recs)))
    # the random part
    n_rand = 0
    pos = 20000
    while n_rand < N_RANDOM:
        recs = []
        for _ in range(int(rng.integers(1, 9))):
            tags, want = random_tags(rng)
            name = f"r{n_rand}"
            recs.append(_record(rng, name, pos + int(rng.integers(0, 200)), random_cigar(rng, int(rng.integers(1, 40))), tags,
                                qual=None if rng.integers(0, 10) == 0 else "random"))
            want_tags[name] = want
            n_rand += 1
        d = dense(recs, margin=12)
        k = int(rng.choice([0, 1, 5, 20, 60, 150]))
        loci.append((recs, np.sort(rng.choice(d, min(k, d.size), replace=False)) if k else np.zeros(0, np.int64)))
        pos += int(rng.integers(0, 60))
    # the file is coordinate-sorted; items keep the loci's order
    flat = [(l, r) for l, (recs, _) in enumerate(loci) for r in recs]
    order = sorted(range(len(flat)), key=lambda i: flat[i][1]["pos"])
    file_index = {flat[i][1]["name"]: k for k, i in enumerate(order)}
    records = [flat[i][1] for i in order]
    items = [r for _, r in flat]
    item_locus = np.array([l for l, _ in flat], np.int32)
    cand_off = np.concatenate(([0], np.cumsum([len(c) for _, c in loci]))).astype(np.int32)
    cand_pos = np.concatenate([c for _, c in loci]).astype(np.int64)
    # substitute alignments for a few items
    alt = {}
    for i in rng.choice(len(items), 40, replace=False):
        cig = random_cigar(rng, int(rng.integers(1, 70)))
        alt[int(i)] = (np.array([(ln << 4) | "MIDNSHP=X".index(op) for ln, op in cig], np.uint32), int(items[int(i)]["pos"] + rng.integers(-20, 50)))
    return {"records": records, "items": items, "item_file_index": np.array([file_index[r["name"]] for r in items], np.int64),
            "item_locus": item_locus, "cand_off": cand_off, "cand_pos": cand_pos, "alt": alt, "want_tags": want_tags, "n_loci": len(loci)}


@functools.lru_cache(maxsize=None)
def expected(with_alt: bool) -> dict:
    """The rule (frontend/phase_inputs.py) over the corpus: hp, ps, and the cells item after item."""
    c = corpus()
    hp, ps, base, qual = [], [], [], []
    for i, r in enumerate(c["items"]):
        h, p = pi.read_tags(r["tags"])            # (write_bam appends the CG tag of a long CIGAR; it carries neither HP nor PS)
        hp.append(h)
        ps.append(p)
        l = int(c["item_locus"][i])
        cand = c["cand_pos"][c["cand_off"][l]:c["cand_off"][l + 1]]
        cig = np.array([(ln << 4) | "MIDNSHP=X".index(op) for ln, op in r["cigar"]], np.uint32)
        start = r["pos"]
        if with_alt and i in c["alt"]:
            cig, start = c["alt"][i]
        b, q = pi.alignment_cells(cig, start, r["seq"], r["qual"], cand)
        base.append(b)
        qual.append(q)
    return {"hp": np.array(hp, np.int32), "ps": np.array(ps, np.int32), "base": np.concatenate(base), "qual": np.concatenate(qual)}


def kept_reads(seed: int = 5) -> tuple[np.ndarray, np.ndarray]:
    """(kept_off, kept_item): per locus a random subset of its items, in item order."""
    c = corpus()
    rng = np.random.default_rng(seed)
    keep = rng.integers(0, 5, c["item_locus"].size) > 0
    kept_item = np.nonzero(keep)[0].astype(np.int32)
    kept_off = np.concatenate(([0], np.cumsum(np.bincount(c["item_locus"][keep], minlength=c["n_loci"])))).astype(np.int32)
    return kept_off, kept_item


def raw_record(pos: int, cigar: list[int], seq_len: int, tags: bytes, name: bytes = b"r\0") -> bytes:
    """One BAM alignment record (with its block_size) of `seq_len` A bases and quality 30."""
    packed = bytes([0x11]) * ((seq_len + 1) // 2)
    body = struct.pack("<iiBBHHHIiii", 0, pos, len(name), 60, 4680, len(cigar), 0, seq_len, -1, -1, 0)
    body += name + b"".join(struct.pack("<I", c) for c in cigar) + packed + bytes([30]) * seq_len + tags
    return struct.pack("<i", len(body)) + body
