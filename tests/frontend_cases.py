"""Shared by tests/test_frontend_cases.py (CPU) and tests/test_gpu_frontend_cases.py: a seeded corpus of hand-made and random
alignment records on several contigs, written with write_bam together with a .bai, (record, four locus boundaries) items over
it, and what frontend/extract.py (the readable statement of the rule) gives for every item.  Built once per process.

What the rule leaves open and this module fixes, for both libraries under test:
* extract.py cuts Python strings, which never fail: when the positions to cut (the flanks shortened to flank_size) are out of
  order or outside the read (a boundary insertion with lfc == lc gives a > b; a substitute alignment may consume more bases
  than the read has), no flank | tract | flank can be cut and the item is "incomplete" (status 1) - strk_host_files.inc and
  strk_dbam.inc say the same at their test ("coordinates outside the read: incomplete");
* the flanks are the last / first `flank_size` bases of what get_sequence_data_for_locus keeps (it keeps ten more)."""
import atexit
import functools
import gzip
import os
import shutil
import struct
import tempfile
from types import SimpleNamespace

import numpy as np

from phase_inputs_cases import HAND_CIGARS, _record, int_tag, random_cigar, random_tags
from strkit_amd.frontend import read_bam, write_bam
from strkit_amd.frontend.extract import CigarIndex, LowMeanBaseQual, get_read_coords_from_cigar, get_sequence_data_for_locus
from strkit_amd.frontend.native import realign_cigar_to_read_alignment
from strkit_amd.frontend.synth_large import write_bai

CONTIGS = [("chrA", 600000), ("chrEmpty", 5000), ("chrB", 400000), ("chrC", 400000)]
PARAMS = [(70, 13, 3), (25, 30, 3), (0, 0, 60), (1, 61, -1)]      # (flank_size, min_avg_phred, wildcard_threshold)
FLANKS = (0, 1, 25, 70)
N_RANDOM = 2000
_OPS = "MIDNSHP=X"
ALL_CODES = "=ACMGRSVTWYHKDBN"

# beyond the hand CIGARs of phase_inputs_cases: a locus wholly inside a deletion / a skipped region, insertions at both tract
# boundaries, an insertion right behind the first and in front of the last aligned pair
EXTRA_HAND = [
    [(90, "M"), (40, "D"), (90, "M")],
    [(90, "="), (40, "N"), (90, "X")],
    [(80, "M"), (6, "I"), (30, "M"), (5, "I"), (80, "M")],
    [(1, "M"), (4, "I"), (150, "M"), (3, "I"), (1, "M")],
    [(3, "S"), (75, "M"), (2, "P"), (1, "D"), (1, "I"), (75, "M"), (2, "H")],
]


def enc(cigar) -> np.ndarray:
    return np.array([(ln << 4) | _OPS.index(op) for ln, op in cigar], np.uint32)


def _ref_len(cigar) -> int:
    return sum(ln for ln, op in cigar if op in "MDN=X")


def _q_len(cigar) -> int:
    return sum(ln for ln, op in cigar if op in "MIS=X")


def _ref_points(cigar, pos: int) -> list[int]:
    """Reference positions around every edge of the alignment: start and end -1 / 0 / +1, the first, middle and last base of
    every operation that consumes reference, the two sides of every insertion."""
    r = pos
    pts = {pos - 1, pos, pos + 1}
    for ln, op in cigar:
        if op in "MDN=X":
            pts |= {r - 1, r, r + 1, r + ln // 2, r + ln - 1, r + ln}
            r += ln
        elif op == "I":
            pts |= {r - 1, r, r + 1}
    pts |= {r - 2, r - 1, r, r + 1}
    return sorted(pts)


def _hand_items(cigar, pos: int) -> list[tuple[int, int, int, int]]:
    out = []
    pts = _ref_points(cigar, pos)
    end = pos + _ref_len(cigar)
    for k, lc in enumerate(pts):
        for j, f in enumerate(FLANKS):
            rc = lc + (0, 1, 4)[(k + j) % 3]
            out.append((lc - f, lc, rc, rc + f))
        for x in (1, 3):                                   # crossed boundaries: the out[1] > out[2] clamp
            out.append((lc - x - 25, lc, lc - x, lc + 25))
            out.append((lc - x - 1, lc, lc - x, lc + 1))
    mid = pos + _ref_len(cigar) // 2
    for rfc in (end - 2, end - 1, end, end + 1):           # the right flank end around the alignment's end ...
        out.append((pos, mid, mid + 2, rfc))
        out.append((pos + 1, mid - 3, mid, rfc))
    for lfc in (pos - 1, pos, pos + 1):                    # ... and the left flank start around its start
        out.append((lfc, mid, mid + 2, end - 1))
    return out


@functools.lru_cache(maxsize=None)
def corpus() -> dict:
    """records (file order), items (`rec`: file index, `coords`), their groups, the substitute alignments."""
    rng = np.random.default_rng(20261020)
    recs: list[dict] = []          # creation order
    items: list[tuple[int, tuple[int, int, int, int]]] = []      # (creation index of the record, boundaries)
    hand_recs, cg_recs = [], []

    def add(r, contig="chrA", flag=0):
        r["contig"], r["flag"] = contig, flag
        r.setdefault("real_cigar", r["cigar"])
        recs.append(r)
        return len(recs) - 1

    def random_items(k, n=2):
        r = recs[k]
        s, e = r["pos"], r["pos"] + _ref_len(r["real_cigar"])
        for _ in range(n):
            f = int(rng.choice(FLANKS))
            if rng.integers(0, 3) == 0:                    # anywhere around the span: incomplete on either side
                lc = int(rng.integers(s - 12, e + 12))
                rc = lc + int(rng.integers(0, 40))
            else:                                          # inside, the flanks mostly spanned
                room = max(e - s - 2 * f, 1)
                lc = s + min(f, (e - s) // 2) + int(rng.integers(0, room))
                rc = min(lc + int(rng.integers(0, 30)), max(lc, e - 1 - f + int(rng.integers(0, 3))))
            items.append((k, (lc - f, lc, rc, rc + f)))

    # the hand CIGARs, each once with and once without qualities, on two contigs
    for k, cig in enumerate(HAND_CIGARS + EXTRA_HAND):
        for nq in (False, True):
            tags = b"" if nq else int_tag(b"HP", "C", 1) + int_tag(b"PS", "i", 1000 + k)
            i = add(_record(rng, f"hand{k}{'nq' if nq else ''}", 1000 + 3 * k + nq, cig, tags, qual=None if nq else "random"),
                    contig="chrA" if k % 2 == 0 else "chrB")
            if not nq and k % 2:                           # every other one with low qualities: its tracts fail the mean
                recs[i]["qual"] = rng.integers(0, 20, len(recs[i]["seq"])).astype(np.uint8)
            hand_recs.append(i)
            items.extend((i, c) for c in _hand_items(cig, recs[i]["pos"]))
    # CIGARs of 0, 1, 63, 64, 65 and 200 operations
    for k, n_ops in enumerate([0, 1, 63, 64, 65, 200]):
        for j in range(3):
            i = add(_record(rng, f"ops{n_ops}_{j}", 3000 + 10 * k + j, random_cigar(rng, n_ops), random_tags(rng)[0]))
            random_items(i, 3)
    # the real CIGAR in the CG tag, behind other tags (write_bam appends it) and in front of them (placeholder and tag by hand)
    for j in range(24):
        cig = random_cigar(rng, [5, 64, 70][j % 3] if j < 6 else int(rng.integers(3, 40)))
        if _q_len(cig) == 0:
            cig = cig + [(30, "M")]
        other = random_tags(rng)[0]
        if j % 2 == 0:
            r = _record(rng, f"cg_behind{j}", 5000 + 7 * j, cig, other, long_cigar=True, qual=None if j % 8 == 0 else "random")
        else:
            c32 = enc(cig)
            r = _record(rng, f"cg_front{j}", 5000 + 7 * j, [(_q_len(cig), "S"), (_ref_len(cig), "N")],
                        b"CGBI" + struct.pack("<I", c32.size) + c32.tobytes() + other, qual=None if j % 8 == 1 else "random")
            r["real_cigar"] = cig
        i = add(r, contig="chrB")
        cg_recs.append(i)
        random_items(i, 4)
    # all sixteen nibble codes at odd and even read positions, odd and even l_seq
    for j, n in enumerate([32, 33, 47, 48]):
        seq = (ALL_CODES * 4)[j % 2:j % 2 + n]
        i = add(_record(rng, f"codes{j}", 7000 + j, [(n, "M")], b"", qual=None if j < 2 else "random", seq=seq), contig="chrC")
        for a in range(0, 9):
            items.append((i, (7000 + j, 7000 + j + 1 + a, 7000 + j + n - 2 - a % 3, 7000 + j + n - 1)))
    # names of 0, 1 and 254 characters; flags
    name_recs = [add(_record(rng, name, 7500 + j, [(40, "M")], b""), contig="chrC") for j, name in enumerate(["", "x", "n" * 254])]
    for i in name_recs:
        random_items(i, 2)
    for j, flag in enumerate([0, 16, 256, 2048, 16 | 2048]):
        i = add(_record(rng, f"flag{flag}", 7600 + j, random_cigar(rng, 6), b""), contig="chrC", flag=flag)
        random_items(i, 2)
    # the random part: groups of reads whose spans interleave, on three contigs; now and then a jump past a 16 kb index window
    n_rand = 0
    qual_kind = []
    for contig, share in (("chrA", 0.4), ("chrB", 0.3), ("chrC", 0.3)):
        pos, upto = 20000, n_rand + int(N_RANDOM * share)
        while n_rand < upto:
            for _ in range(int(rng.integers(1, 9))):
                kind = int(rng.choice([0, 1, 1, 3, 3, 3, 2, 2, 2, 2]))       # no qualities | mean about 13 | 0 .. 60 | mean about 7
                r = _record(rng, f"r{n_rand}", pos + int(rng.integers(0, 200)), random_cigar(rng, int(rng.integers(1, 40))),
                            random_tags(rng)[0], qual=None if kind == 0 else "random")
                if kind in (1, 3):
                    r["qual"] = rng.integers(0, 27 if kind == 1 else 15, len(r["seq"])).astype(np.uint8)
                i = add(r, contig=contig, flag=int(rng.choice([0, 0, 0, 16, 16, 256, 2048])))
                qual_kind.append(kind)
                random_items(i, 2)
                n_rand += 1
            pos += int(rng.integers(0, 60)) if rng.integers(0, 12) else int(rng.integers(16000, 40000))
    # unmapped records at the end of the file, as aligners write them
    unmapped = []
    for j in range(6):
        n = [0, 1, 50, 51, 300, 7][j]
        r = _record(rng, f"unmapped{j}", -1, [], b"", seq="".join(rng.choice(list("ACGT"), n)) if n else None)
        r["qual"] = None if j % 2 else rng.integers(0, 61, n).astype(np.uint8)      # (_record sizes them by the CIGAR: none here)
        unmapped.append(add(r, contig="*", flag=4))
    items.append((unmapped[2], (0, 10, 20, 30)))
    items.append((unmapped[3], (-5, -1, 0, 3)))

    tid_of = {"chrA": 0, "chrEmpty": 1, "chrB": 2, "chrC": 3, "*": 1 << 30}
    order = sorted(range(len(recs)), key=lambda i: (tid_of[recs[i]["contig"]], recs[i]["pos"]))       # (stable)
    file_index = np.empty(len(recs), np.int64)
    file_index[order] = np.arange(len(recs))
    to_file = lambda ks: np.sort(file_index[np.array(ks, np.int64)])  # noqa: E731
    item_rec = file_index[np.array([k for k, _ in items], np.int64)]
    coords = np.array([c for _, c in items], np.int64)
    n_items = len(items)

    # substitute alignments: random CIGARs with shifted starts, the record's own CIGAR shifted (it fits the read), and CIGARs in
    # the orientation of strk_realign turned round by realign_cigar_to_read_alignment
    alt = {}
    for it in rng.choice(n_items, 420, replace=False):
        it = int(it)
        r = recs[items[it][0]]
        kind = int(rng.integers(0, 3))
        if kind == 0:
            cig = enc(random_cigar(rng, int(rng.integers(1, 70))))
        elif kind == 1:
            cig = enc(r["real_cigar"]) if r["real_cigar"] else enc([(len(r["seq"]), "M")])
        else:
            body = [(int(rng.integers(1, 60)), "MMMID=X"[int(rng.integers(0, 7))]) for _ in range(int(rng.integers(1, 12)))]
            cig = realign_cigar_to_read_alignment(enc(([(int(rng.integers(1, 50)), "D")] if rng.integers(0, 2) else []) + body))
        alt[it] = (cig, int(r["pos"] + rng.integers(-20, 50)))
    # a small item set for the call without alt_start: substitute alignments that start at reference position 0
    alt0_rec, alt0_coords, alt0 = [], [], {}
    for j in range(64):
        k = int(rng.integers(0, len(recs) - len(unmapped)))
        r = recs[k]
        alt0_rec.append(int(file_index[k]))
        if j % 4:
            cig = enc([(int(rng.integers(0, 30)), "S"), (int(rng.integers(20, 200)), "M"), (int(rng.integers(0, 9)), "I"), (len(r["seq"]), "M")][j % 2:])
            alt0[j] = (cig, 0)
            lc = int(rng.integers(1, 120))
            f = int(rng.choice(FLANKS))
            alt0_coords.append((lc - f, lc, lc + int(rng.integers(0, 30)), lc + 30 + f))
        else:                                              # (an item without a substitute among them: its own alignment)
            alt0_coords.append(items[int(np.nonzero(item_rec == file_index[k])[0][0])][1])

    return {"records": [recs[i] for i in order], "item_rec": item_rec, "coords": coords, "alt": alt,
            "alt0_rec": np.array(alt0_rec, np.int64), "alt0_coords": np.array(alt0_coords, np.int64), "alt0": alt0,
            "hand": to_file(hand_recs), "cg": to_file(cg_recs), "names": file_index[np.array(name_recs)], "unmapped": to_file(unmapped),
            "no_qual": np.array([i for i, k in enumerate(order) if recs[k]["qual"] is None and len(recs[k]["seq"])], np.int64)}


# ---- the file, its index, and what read_bam says about it ------------------------------------------------------------------
def bgzf_layout(path: str) -> tuple[np.ndarray, np.ndarray, np.ndarray]:
    """(compressed offset, offset in the decompressed stream, decompressed length) of every BGZF block of the file, from the
    block headers (SAM specification 4.1: BSIZE in the BC subfield, ISIZE in the last four bytes)."""
    raw = open(path, "rb").read()
    coff, uoff, ulen = [], [], []
    off = u = 0
    while off < len(raw):
        assert raw[off:off + 4] == b"\x1f\x8b\x08\x04"
        xlen, = struct.unpack_from("<H", raw, off + 10)
        x, bsize = off + 12, None
        while x < off + 12 + xlen:
            si1, si2, slen = struct.unpack_from("<BBH", raw, x)
            if (si1, si2, slen) == (66, 67, 2):
                bsize, = struct.unpack_from("<H", raw, x + 4)
            x += 4 + slen
        isize, = struct.unpack_from("<I", raw, off + bsize + 1 - 4)
        coff.append(off); uoff.append(u); ulen.append(isize)
        off += bsize + 1
        u += isize
    return np.array(coff, np.int64), np.array(uoff, np.int64), np.array(ulen, np.int64)


def record_offsets(stream: bytes) -> np.ndarray:
    """Offsets of the alignment records in a decompressed BAM stream, plus the end of the last one (the block_size chain)."""
    l_text, = struct.unpack_from("<i", stream, 4)
    off = 8 + l_text
    n_ref, = struct.unpack_from("<i", stream, off)
    off += 4
    for _ in range(n_ref):
        l_name, = struct.unpack_from("<i", stream, off)
        off += 8 + l_name
    out = [off]
    while off + 4 <= len(stream):
        off += 4 + struct.unpack_from("<i", stream, off)[0]
        out.append(off)
    return np.array(out, np.int64)


def virtual_offsets(layout, u: np.ndarray) -> np.ndarray:
    """Offsets in the decompressed stream -> BAM virtual offsets (the block that HOLDS the byte: an offset at a block's end is
    written as the start of the next block)."""
    coff, uoff, _ = layout
    k = np.searchsorted(uoff, u, side="right") - 1
    # (empty blocks share their offset with the block behind them: searchsorted right takes the last, which holds the byte)
    return (coff[k].astype(np.uint64) << np.uint64(16)) | (u - uoff[k]).astype(np.uint64)


@functools.lru_cache(maxsize=None)
def corpus_file() -> dict:
    """The corpus written once per process (a temporary directory, removed at exit): path (with its .bai next to it), the
    decompressed stream, the BGZF layout, every record's offset and what read_bam makes of the file."""
    d = tempfile.mkdtemp(prefix="frontend_cases_")
    atexit.register(shutil.rmtree, d, ignore_errors=True)
    path = os.path.join(d, "corpus.bam")
    write_bam(path, CONTIGS, corpus()["records"])
    with gzip.open(path, "rb") as fh:
        stream = fh.read()
    bam = read_bam(path)
    rec_off = record_offsets(stream)
    assert rec_off.size == len(bam.segments) + 1 and rec_off[-1] == len(stream)
    layout = bgzf_layout(path)
    names = [c for c, _ in CONTIGS]
    tid = np.array([names.index(s.contig) if s.contig != "*" else -1 for s in bam.segments], np.int32)
    voff = virtual_offsets(layout, rec_off)
    write_bai(path + ".bai", len(CONTIGS), tid, np.array([s.start for s in bam.segments], np.int64),
              np.array([s.end for s in bam.segments], np.int64), voff[:-1], voff[1:])
    fields = {"rec_off": rec_off[:-1], "tid": tid,
              "pos": np.array([s.start for s in bam.segments], np.int32), "end": np.array([s.end for s in bam.segments], np.int32),
              "flag": np.array([s.flag for s in bam.segments], np.int32), "l_seq": np.array([s.length for s in bam.segments], np.int32),
              "clip_l": np.array([s.soft_clips()[0] for s in bam.segments], np.int32),
              "clip_r": np.array([s.soft_clips()[1] for s in bam.segments], np.int32),
              "l_name": np.array([len(s.name.encode()) + 1 for s in bam.segments], np.int32)}
    return {"path": path, "stream": stream, "layout": layout, "rec_end": rec_off[1:], "voff": voff[:-1], "bam": bam, "fields": fields}


# ---- the rule ------------------------------------------------------------------------------------------------------------
def _item_coords(seg, c4, alt_one):
    """(a, b, c, d) read positions of the boundaries, or None when the rule finds the read incomplete for the locus."""
    view = seg if alt_one is None else SimpleNamespace(cigar=np.asarray(alt_one[0], np.uint32), start=int(alt_one[1]))
    c = get_read_coords_from_cigar(int(c4[0]), int(c4[1]), int(c4[2]), int(c4[3]), view)
    if c.is_incomplete():
        return None
    return c.left_flank_start, c.left_flank_end, c.right_flank_start, c.right_flank_end


def _expect(item_rec, coords, alt, param) -> dict:
    segs = corpus_file()["bam"].segments
    flank, phred, wc = param
    n = len(item_rec)
    status = np.ones(n, np.int32)
    nfl, ntr, nfr = np.zeros(n, np.int32), np.zeros(n, np.int32), np.zeros(n, np.int32)
    cut_a = np.zeros(n, np.int64)
    parts = []
    for it in range(n):
        seg = segs[int(item_rec[it])]
        q = _item_coords(seg, coords[it], alt.get(it) if alt else None)
        if q is None:
            continue
        a, d = max(q[0], q[1] - flank), min(q[3], q[2] + flank)         # what is cut: the flanks are at most `flank` long
        if not (0 <= a <= q[1] <= q[2] <= d <= seg.length):             # (see the module's docstring)
            continue
        lc = SimpleNamespace(left_flank_start=q[0], left_flank_end=q[1], right_flank_start=q[2], right_flank_end=q[3])
        try:
            sd = get_sequence_data_for_locus(seg, lc, flank, phred, wc)
        except LowMeanBaseQual:
            status[it] = 2
            continue
        fl = sd.flank_left_seq_wc[max(0, len(sd.flank_left_seq_wc) - flank):]
        fr = sd.flank_right_seq_wc[:flank]
        status[it], nfl[it], ntr[it], nfr[it] = 0, len(fl), len(sd.tr_seq_wc), len(fr)
        cut_a[it] = q[1] - len(fl)
        parts.append(fl + sd.tr_seq_wc + fr)
    seq_off = np.concatenate(([0], np.cumsum(nfl.astype(np.int64) + ntr + nfr))).astype(np.int64)
    return {"status": status, "nfl": nfl, "ntr": ntr, "nfr": nfr, "cut_a": cut_a, "seq_off": seq_off,
            "seqs": np.frombuffer("".join(parts).encode("ascii"), np.uint8)}


@functools.lru_cache(maxsize=None)
def expected(param: tuple[int, int, int], with_alt: bool) -> dict:
    """The rule (frontend/extract.py) over all items: status, nfl, ntr, nfr, seq_off, the bases, and the first read position cut."""
    c = corpus()
    return _expect(c["item_rec"], c["coords"], c["alt"] if with_alt else None, param)


@functools.lru_cache(maxsize=None)
def expected_alt0(param: tuple[int, int, int]) -> dict:
    c = corpus()
    return _expect(c["alt0_rec"], c["alt0_coords"], c["alt0"], param)


def boundary_kinds(seg, c4) -> set[str]:
    """Where the tract boundaries of an item fall in the record's own alignment: inside a D or N run, right behind an I (the
    first aligned pair at or right of the boundary follows inserted bases), with crossed pair indices (the clamp)."""
    kinds = set()
    r = seg.start
    for c in seg.cigar.tolist():
        op, ln = _OPS[c & 15], c >> 4
        for x in (int(c4[1]), int(c4[2])):
            if op in "DN" and r <= x < r + ln:
                kinds.add(op)
            if op == "I" and ln > 0 and x == r:
                kinds.add("I")
        if op in "MDN=X":
            r += ln
    ix = CigarIndex(seg)
    if ix.n_pairs and ix.first_pair_at_or_after(int(c4[1])) > ix.first_pair_at_or_after(int(c4[2])):
        kinds.add("clamp")
    return kinds


# ---- comparisons and the C ABI called directly --------------------------------------------------------------------------------
def same_segment(a, b) -> None:
    assert (a.name, a.contig, a.start, a.end, a.flag, a.mapq, a.query_sequence, a.tags) == \
        (b.name, b.contig, b.start, b.end, b.flag, b.mapq, b.query_sequence, b.tags), (a.name, b.name)
    assert np.array_equal(a.cigar, b.cigar), a.name
    assert (a.query_qualities is None) == (b.query_qualities is None), a.name
    assert a.query_qualities is None or np.array_equal(a.query_qualities, b.query_qualities), a.name


def same_extraction(got: dict, seqs: np.ndarray, want: dict, lo: int = 0, hi: int | None = None) -> None:
    """status, the three lengths, seq_off and the bases of items [lo, hi) of `want` equal what a library returned for them."""
    hi = len(want["status"]) if hi is None else hi
    for k in ("status", "nfl", "ntr", "nfr"):
        bad = np.nonzero(got[k] != want[k][lo:hi])[0]
        assert bad.size == 0, (k, lo + int(bad[0]), got[k][bad[:6]], want[k][lo:hi][bad[:6]])
    base = int(want["seq_off"][lo])
    assert np.array_equal(got["seq_off"], want["seq_off"][lo:hi + 1] - base)
    w = want["seqs"][base:int(want["seq_off"][hi])]
    assert seqs.size == w.size
    bad = np.nonzero(seqs != w)[0]
    if bad.size:
        it = int(np.searchsorted(got["seq_off"], bad[0], side="right")) - 1
        raise AssertionError(("bases", lo + it, int(bad[0] - got["seq_off"][it]), seqs[bad[:8]].tobytes(), w[bad[:8]].tobytes()))


def malformed_alt(n: int) -> list[tuple[tuple, bytes]]:
    """The substitute-alignment triples of a call of n >= 3 items that strk_extract_reads and strk_dbam_extract refuse before
    they read a record, each with the message of the shared check.  (The offsets alone are read: the operations never are.)"""
    ops = np.full(4, 5 << 4, np.uint32)
    off = np.zeros(n + 1, np.int64)
    off[2:] = 2
    start = np.zeros(n, np.int64)
    both = b"alt_cigar and alt_cigar_off must both be given or both be NULL"
    from1, down, huge = off + 1, off.copy(), off.copy()
    down[2] = 3
    huge[2:] = (1 << 31) + 1
    return [((ops, None, start), both), ((None, off, start), both), ((ops, from1, start), b"alt_cigar_off[0] must be 0"),
            ((ops, down, None), b"item 2: alt_cigar_off is decreasing (or a CIGAR too long)"),
            ((ops, huge, None), b"item 1: alt_cigar_off is decreasing (or a CIGAR too long)")]


def raw_extract(bam, rec_idx, coords, alt, param, alt_start: bool = True, rec_off=None, check: bool = True, alt_raw=None):
    """strk_extract_reads (a host reader) or strk_dbam_extract (a DeviceBam) called directly: (the outputs with `rc`, the bases).
    alt_start=False passes NULL for the substitute alignments' starts; rec_off replaces the offsets of `rec_idx`; alt_raw =
    (alt_cigar, alt_cigar_off, alt_start) as arrays or None goes to the library as it is, in place of `alt`."""
    from strkit_amd import _lib
    L = _lib.load()
    n = len(rec_idx)
    rec_off = np.ascontiguousarray(bam.rec_off[rec_idx] if rec_off is None else rec_off, np.int64)
    coords = np.ascontiguousarray(coords, np.int64).reshape(n, 4)
    out = {k: np.zeros(n, np.int32) for k in ("status", "nfl", "ntr", "nfr")}
    out["seq_off"] = np.zeros(n + 1, np.int64)
    a_cig = a_off = a_start = None
    if alt:
        a_off = np.concatenate(([0], np.cumsum([alt[i][0].size if i in alt else 0 for i in range(n)]))).astype(np.int64)
        a_cig = np.concatenate([np.asarray(alt[i][0], np.uint32) for i in sorted(alt)] + [np.zeros(1, np.uint32)])
        a_start = np.array([alt[i][1] if i in alt else 0 for i in range(n)], np.int64) if alt_start else None
    if alt_raw is not None:
        a_cig, a_off, a_start = alt_raw
    mid = (_lib.ptr(a_cig), _lib.ptr(a_off), _lib.ptr(a_start), *(int(x) for x in param),
           *(_lib.ptr(out[k]) for k in ("status", "nfl", "ntr", "nfr")))
    if hasattr(bam, "_h"):
        import ctypes as C
        name_len = np.zeros(max(n, 1), np.int32)
        d_seqs = C.c_void_p()
        out["rc"] = L.strk_dbam_extract(bam._h, n, _lib.ptr(rec_off), _lib.ptr(coords), *mid, _lib.ptr(out["seq_off"]), _lib.ptr(name_len),
                                        C.byref(d_seqs))
        out["name_len"] = name_len[:n]
        seqs = np.zeros(int(out["seq_off"][-1]) if out["rc"] == 0 else 0, np.uint8)
        if out["rc"] == 0 and seqs.size:
            _lib.check(L.strk_dbam_download_seqs(bam._h, seqs.size, _lib.ptr(seqs)))
    else:
        head = (_lib.ptr(bam.data), bam.data.size, n, _lib.ptr(rec_off), _lib.ptr(coords))
        out["rc"] = L.strk_extract_reads(*head, *mid, None, 0, _lib.ptr(out["seq_off"]))
        seqs = np.zeros(int(out["seq_off"][-1]) if out["rc"] == 0 else 0, np.uint8)
        if out["rc"] == 0:
            out["rc"] = L.strk_extract_reads(*head, *mid, _lib.ptr(seqs) if seqs.size else _lib.ptr(np.zeros(1, np.uint8)), seqs.size,
                                             _lib.ptr(out["seq_off"]))
    if check:
        _lib.check(out["rc"])
    return out, seqs
