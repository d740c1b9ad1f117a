"""Shared by tests/test_frontend.py (CPU: strk_inflate.h compiled for the host, the zlib path, the header walkers),
tests/test_gpu_inflate.py (k_bgzf_inflate) and tools/inflate_asan.sh: one corpus of raw deflate bodies.  Every case is
(name, raw_deflate_body, expected_bytes or None); expected_bytes is what zlib.decompressobj(-15) makes of the body — never
what the code under test or the assembler below thinks it should be — and None marks a body (with its BGZF trailer,
corpus()["trailer"][name]) that must be refused.  Built once per process, seeded.

  zlib_matrix()   payloads x zlib levels / strategies (the runs of every period, the matches of every length and distance
                  class, matches that end `cut` bytes before the block's end, blocks of 1, 7, 8, 9 and 65536 bytes)
  flushed         one compressobj fed in pieces with every flush mode between them: empty stored and fixed blocks in
                  mid-stream, matches that reach back across a deflate-block boundary
  asm/...         streams put together bit by bit (class Deflate): every copy branch of inflate_block by construction,
                  the code shapes zlib never writes but RFC 1951 allows
  refuse/...      one malformed body per error return of inflate_block

What cannot be built: HCLEN = 0 in a legal stream (the first four code-length codes are 16, 17, 18 and 0: no length but 0 can
be written, so there is no end-of-block code; HLIT = 0 / HDIST = 0 therefore come with HCLEN = 1, and HCLEN = 0 is a
refusal), and a code-length code longer than 7 bits (its lengths are three-bit fields)."""
import functools
import struct
import zlib

import numpy as np

# RFC 1951 3.2.5, as data
LBASE = (3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258)
LEXT = (0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0)
DBASE = (1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193,
         12289, 16385, 24577)
DEXT = (0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13)
CL_ORDER = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)
FIXED_LL = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
FIXED_D = [5] * 32

STRATEGIES = ((0, zlib.Z_DEFAULT_STRATEGY, "L0"), (1, zlib.Z_FIXED, "L1fixed"), (1, zlib.Z_DEFAULT_STRATEGY, "L1"),
              (6, zlib.Z_DEFAULT_STRATEGY, "L6"), (9, zlib.Z_DEFAULT_STRATEGY, "L9"), (9, zlib.Z_HUFFMAN_ONLY, "L9huff"),
              (4, zlib.Z_RLE, "L4rle"))
# the block types a strategy can open a body with (level 0 stores; Z_FIXED never sends a code; the others choose the
# smallest of the three forms): the corpus must hold each of them
BTYPES_OF = {"L0": {0}, "L1fixed": {0, 1}, "L1": {0, 1, 2}, "L6": {0, 1, 2}, "L9": {0, 1, 2}, "L9huff": {0, 1, 2}, "L4rle": {0, 1, 2}}
BRANCHES = ("264", "pattern", "128", "32", "8", "byte")
(E_TYPE, E_CODE, E_LENGTHS, E_OVERRUN, E_DISTANCE, E_STORED, E_SIZE, E_CRC) = range(1, 9)   # strk_inf::kErr...


def zlib_inflate(body: bytes):
    """(bytes, whole) of a raw deflate body by zlib; None when zlib raises.  whole: the stream reached its final block's end."""
    d = zlib.decompressobj(-15)
    try:
        out = d.decompress(body) + d.flush()
    except zlib.error:
        return None
    return out, d.eof


# ---- the assembler ---------------------------------------------------------------------------------------------------------
class Bits:
    """LSB-first bit writer (RFC 1951 3.1.1)."""

    def __init__(self):
        self.out, self.acc, self.n = bytearray(), 0, 0

    def put(self, v: int, n: int):          # a number: least significant bit first
        assert 0 <= v < (1 << n) or n == 0
        self.acc |= v << self.n
        self.n += n
        while self.n >= 8:
            self.out.append(self.acc & 255)
            self.acc >>= 8
            self.n -= 8

    def code(self, c: int, n: int):          # a Huffman code: most significant bit first
        self.put(int(format(c, f"0{n}b")[::-1], 2) if n else 0, n)

    def align(self):
        if self.n:
            self.put(0, 8 - self.n)

    @property
    def bit_len(self) -> int:
        return 8 * len(self.out) + self.n

    def bytes(self) -> bytes:
        b = Bits()
        b.out, b.acc, b.n = bytearray(self.out), self.acc, self.n
        b.align()
        return bytes(b.out)


def canonical(lengths) -> dict:
    """symbol -> (code, length) of the canonical code with these lengths (RFC 1951 3.2.2)."""
    codes, code = {}, 0
    for ln in range(1, 16):
        for s, l in enumerate(lengths):
            if l == ln:
                codes[s] = (code, ln)
                code += 1
        code <<= 1
    return codes


def flat_lengths(used, n: int) -> list:
    """n lengths, 0 but for the symbols of `used`, which get a complete code of two neighbouring lengths (one code: one bit)."""
    used = sorted(set(used))
    out = [0] * n
    if len(used) == 1:
        out[used[0]] = 1
        return out
    k = max(1, (len(used) - 1).bit_length())
    short = (1 << k) - len(used)
    for i, s in enumerate(used):
        out[s] = k - 1 if i < short else k
    return out


def skewed_lengths(used, n: int) -> list:
    """lengths 1, 2, 3, ..., 14, 15, 15 over the first sixteen symbols of `used` (a Fibonacci-like code: 15-bit codes)."""
    used = sorted(set(used))
    assert len(used) == 16
    out = [0] * n
    for i, s in enumerate(used):
        out[s] = min(i + 1, 15)
    return out


def rle_plain(seq) -> list:
    return [(l, None) for l in seq]


def rle_greedy(seq) -> list:
    """The code-length sequence with codes 16, 17 and 18 wherever they fit, as (symbol, repeat count or None)."""
    ops, i = [], 0
    while i < len(seq):
        j = i
        while j < len(seq) and seq[j] == seq[i]:
            j += 1
        run = j - i
        if seq[i] == 0:
            while run >= 11:
                r = min(run, 138)
                ops.append((18, r))
                run -= r
            if run >= 3:
                ops.append((17, run))
                run = 0
        else:
            ops.append((seq[i], None))
            run -= 1
            while run >= 3:
                r = min(run, 6)
                ops.append((16, r))
                run -= r
        ops += [(seq[i], None)] * run
        i = j
    return ops


def spell(length: int, dist: int, lsym=None) -> tuple:
    """(length symbol, extra value, distance symbol, extra value); lsym forces a spelling of the length (284 + 31 for 258)."""
    if lsym is None:
        lsym = 285 if length == 258 else 257 + max(k for k in range(28) if LBASE[k] <= length)
    lex = length - LBASE[lsym - 257]
    assert 0 <= lex < (1 << LEXT[lsym - 257]), (length, lsym)
    dsym = max(k for k in range(30) if DBASE[k] <= dist)
    return lsym, lex, dsym, dist - DBASE[dsym]


def _norm(tok):
    """int literal | (length, distance[, length symbol]) | ("sym", lsym, lextra, dsym, dextra) -> the first or the last form."""
    if isinstance(tok, int) or tok[0] == "sym":
        return tok
    return ("sym", *spell(*tok))


class Deflate:
    """A raw deflate stream, block by block.  `blocks` keeps (BTYPE, first bit) of every block written, `ops` the
    code-length operations of the dynamic ones."""

    def __init__(self):
        self.b = Bits()
        self.blocks, self.ops = [], []

    def _head(self, final: bool, btype: int):
        self.blocks.append((btype, self.b.bit_len))
        self.b.put(1 if final else 0, 1)
        self.b.put(btype, 2)

    def stored(self, data: bytes, final: bool, nlen=None, length=None):
        self._head(final, 0)
        self.b.align()
        ln = len(data) if length is None else length
        self.b.put(ln, 16)
        self.b.put((ln ^ 0xffff) if nlen is None else nlen, 16)
        for x in data:
            self.b.put(x, 8)
        return self

    def _tokens(self, tokens, ll: dict, dd: dict, eob: bool):
        for tok in map(_norm, tokens):
            if isinstance(tok, int):
                self.b.code(*ll[tok])
                continue
            _, lsym, lex, dsym, dex = tok
            self.b.code(*ll[lsym])
            if lsym <= 285:
                self.b.put(lex, LEXT[lsym - 257])
            self.b.code(*dd[dsym])
            if dsym <= 29:
                self.b.put(dex, DEXT[dsym])
        if eob:
            self.b.code(*ll[256])

    def fixed(self, tokens, final: bool, eob: bool = True):
        self._head(final, 1)
        self._tokens(tokens, canonical(FIXED_LL), canonical(FIXED_D), eob)
        return self

    def dynamic(self, tokens, ll_lengths=None, d_lengths=None, final: bool = True, hclen=None, rle=rle_greedy, cl_lengths=None,
                hlit=None, hdist=None, eob: bool = True):
        """ll_lengths / d_lengths: the code lengths (default: a flat complete code over what the tokens use); rle: a function
        of the joined length sequence or a ready list of (code-length symbol, repeat or None); hclen / hlit / hdist: the raw
        header fields when they shall differ from what the lengths say."""
        toks = [_norm(t) for t in tokens]
        if ll_lengths is None:
            used = {256} | {t for t in toks if isinstance(t, int)} | {t[1] for t in toks if not isinstance(t, int)}
            ll_lengths = flat_lengths(used, max(257, max(used) + 1))
        if d_lengths is None:
            used_d = {t[3] for t in toks if not isinstance(t, int)}
            d_lengths = flat_lengths(used_d, max(used_d) + 1) if used_d else [0]
        seq = list(ll_lengths) + list(d_lengths)
        ops = rle(seq) if callable(rle) else list(rle)
        if cl_lengths is None:
            used_cl = {s for s, _ in ops}
            if len(used_cl) < 2:
                used_cl |= {0, 8}
            cl_lengths = flat_lengths(used_cl, 19)
        n_cl = max(4, max(i + 1 for i, s in enumerate(CL_ORDER) if cl_lengths[s]))
        self._head(final, 2)
        self.b.put(len(ll_lengths) - 257 if hlit is None else hlit, 5)
        self.b.put(len(d_lengths) - 1 if hdist is None else hdist, 5)
        n_cl = n_cl if hclen is None else hclen + 4
        self.b.put(n_cl - 4, 4)
        for s in CL_ORDER[:n_cl]:
            self.b.put(cl_lengths[s], 3)
        cl = canonical(cl_lengths)
        for s, rep in ops:
            self.b.code(*cl[s])
            if s == 16:
                self.b.put(rep - 3, 2)
            elif s == 17:
                self.b.put(rep - 3, 3)
            elif s == 18:
                self.b.put(rep - 11, 7)
        self.ops.append(ops)
        self._tokens(toks, canonical(ll_lengths), canonical(d_lengths), eob)
        return self

    def body(self) -> bytes:
        return self.b.bytes()


def header_fields(body: bytes) -> tuple:
    """(HLIT, HDIST, HCLEN) of a body that starts with a dynamic block."""
    v = int.from_bytes(body[:3], "little")
    assert (v >> 1) & 3 == 2
    return (v >> 3) & 31, (v >> 8) & 31, (v >> 13) & 15


def out_len_of(tokens) -> int:
    return sum(1 if isinstance(t, int) else (LBASE[t[1] - 257] + t[2]) for t in map(_norm, tokens))


# ---- the copy branches of inflate_block, restated to check that the corpus reaches them (never to make expected bytes) ------
def copy_branches(pos: int, length: int, dist: int, out_len: int) -> list:
    got = []
    while length > 0:
        if dist >= 264 and length > 128 and pos + 264 <= out_len:
            got.append("264"); n = length
        elif dist < 8 and pos + 8 <= out_len:
            got.append("pattern"); n = min(length, 8)
        elif dist >= 128 and length > 32 and pos + 128 <= out_len:
            got.append("128"); n = min(length, 128)
        elif dist >= 32 and length > 8 and pos + 32 <= out_len:
            got.append("32"); n = min(length, 32)
        elif pos + 8 <= out_len:
            got.append("8"); n = min(length, 8)
        else:
            got.append("byte"); n = 1
        pos += n; length -= n
    return got


def first_branches(tokens) -> list:
    """The branch the first trip of every match of `tokens` takes."""
    total, pos, got = out_len_of(tokens), 0, []
    for t in map(_norm, tokens):
        if isinstance(t, int):
            pos += 1
        else:
            ln, dist = LBASE[t[1] - 257] + t[2], DBASE[t[3]] + t[4]
            got.append(copy_branches(pos, ln, dist, total)[0])
            pos += ln
    return got


# ---- payloads ----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def payloads() -> tuple:
    """(name, bytes, incompressible) — the matrix tests/test_frontend.py had, the end-of-block cuts tools/inflate_asan.sh had,
    and blocks of 1, 7, 8, 9 and 65536 bytes."""
    rng = np.random.default_rng(4)
    out = [("empty", b"", False), ("one", b"A", False), ("random40000", bytes(rng.integers(256, size=40000, dtype=np.uint8)), True),
           ("acgt36000", b"ACGT" * 9000, False), ("zeros60000", bytes(60000), False),
           ("qual65000", bytes(rng.integers(33, 74, size=65000, dtype=np.uint8)), False)]
    # runs of every short period and matches of every length at short and long distances, up to the last byte of the block
    # (the copy paths of the decoder: pattern fill from registers, 8 / 32 / 128 / 264 bytes per trip, byte-wise tail)
    runs = bytearray()
    for period in range(1, 41):
        pat = bytes(rng.integers(256, size=period, dtype=np.uint8))
        for reps in (3, 11, 40, 300 // period + 2):
            runs += pat * reps + bytes(rng.integers(256, size=int(rng.integers(1, 9)), dtype=np.uint8))
    far = bytearray(bytes(rng.integers(256, size=3000, dtype=np.uint8)))
    for ln in list(range(3, 40)) + [63, 64, 65, 127, 128, 129, 130, 200, 257, 258, 259, 300, 600]:
        for back in (ln, ln + 1, 31, 32, 33, 127, 128, 129, 263, 264, 265, 2000):
            if 1 <= back <= len(far):
                src = len(far) - back
                far += bytes(far[src + i % back] for i in range(ln))
                far += bytes(rng.integers(256, size=int(rng.integers(0, 4)), dtype=np.uint8))
    out += [("runs", bytes(runs[:65000]), False), ("far65000", bytes(far[:65000]), True), ("far60000_tail", bytes(far[:60000]) + b"\x07" * 300, True),
            ("ab_xyz", b"ab" * 150 + b"xyz" * 100, False)]
    for cut in (1, 2, 7, 8, 9, 31, 33, 127, 129, 263, 265):     # a match that ends exactly `cut` bytes before the block's end
        out.append((f"match_ends_{cut}_before", bytes(far[:50000]) + bytes(far[1000:1300])[:300 - cut], True))
    text = bytes(rng.integers(65, 70, size=16, dtype=np.uint8))
    out += [(f"len{n}", text[:n], False) for n in (7, 8, 9)]
    out += [("zeros65536", bytes(65536), False), ("acgt65536", b"ACGT" * 16384, False)]
    return tuple(out)


@functools.lru_cache(maxsize=None)
def zlib_matrix() -> tuple:
    """(name, body, raw payload, strategy name) of every (payload, strategy) whose block fits 64 KiB; lost_pairs(): the rest."""
    out = []
    for pname, raw, _ in payloads():
        for level, strategy, sname in STRATEGIES:
            co = zlib.compressobj(level, zlib.DEFLATED, -15, 8, strategy)
            body = co.compress(raw) + co.flush()
            if len(body) + 26 <= 65536:
                out.append((f"zlib/{pname}/{sname}", body, raw, sname))
    return tuple(out)


def lost_pairs() -> list:
    have = {m[0] for m in zlib_matrix()}
    return [(p, s) for p, _, _ in payloads() for _, _, s in STRATEGIES if f"zlib/{p}/{s}" not in have]


def _flushed() -> list:
    rng = np.random.default_rng(11)
    base = bytes(rng.integers(65, 85, size=600, dtype=np.uint8))
    pieces = [base[:200], base[100:400], b"", base[:64] * 5, bytes(rng.integers(256, size=300, dtype=np.uint8)), base[300:], b"Q", base[:599]]
    out = []
    for level, strategy, sname in ((1, zlib.Z_DEFAULT_STRATEGY, "L1"), (9, zlib.Z_DEFAULT_STRATEGY, "L9"), (6, zlib.Z_FIXED, "L6fixed"),
                                   (0, zlib.Z_DEFAULT_STRATEGY, "L0")):
        for mname, mode in (("sync", zlib.Z_SYNC_FLUSH), ("full", zlib.Z_FULL_FLUSH), ("partial", zlib.Z_PARTIAL_FLUSH), ("block", zlib.Z_BLOCK)):
            co = zlib.compressobj(level, zlib.DEFLATED, -15, 8, strategy)
            body = b"".join(co.compress(p) + co.flush(mode) for p in pieces) + co.flush()
            out.append((f"flushed/{mname}/{sname}", body))
        co = zlib.compressobj(level, zlib.DEFLATED, -15, 8, strategy)   # all four modes in one stream
        modes = (zlib.Z_SYNC_FLUSH, zlib.Z_BLOCK, zlib.Z_PARTIAL_FLUSH, zlib.Z_FULL_FLUSH)
        body = b"".join(co.compress(p) + co.flush(modes[i % 4]) for i, p in enumerate(pieces)) + co.flush()
        out.append((f"flushed/mixed/{sname}", body))
    return out


# ---- assembled streams -------------------------------------------------------------------------------------------------------
def _lits(rng, n: int, lo: int = 97, hi: int = 123) -> list:
    return [int(x) for x in rng.integers(lo, hi, size=n)]


def _branch_cases() -> list:
    """(name, tokens, branch the match must take first): for every clause of every branch predicate one match that just
    satisfies it and one that just fails it, each once more with distance == position (the match starts at the block's first
    byte)."""
    spec = []   # (name, length, distance, bytes from the match's start to the block's end, branch)
    spec += [("264_holds", 129, 264, 264, "264"), ("264_dist_263", 129, 263, 264, "128"), ("264_len_128", 128, 264, 264, "128"),
             ("264_one_short", 129, 264, 263, "128"), ("264_longest", 258, 300, 264, "264")]
    spec += [("pattern_holds_d7", 8, 7, 8, "pattern"), ("pattern_dist_8", 8, 8, 8, "8"), ("pattern_one_short", 7, 7, 7, "byte")]
    spec += [(f"pattern_d{d}", 30 + d, d, 40 + d, "pattern") for d in range(1, 8)]
    spec += [("128_holds", 33, 128, 128, "128"), ("128_dist_127", 33, 127, 128, "32"), ("128_len_32", 32, 128, 128, "32"),
             ("128_one_short", 33, 128, 127, "32"), ("128_twice", 258, 200, 400, "128")]
    spec += [("32_holds", 9, 32, 32, "32"), ("32_dist_31", 9, 31, 32, "8"), ("32_len_8", 8, 32, 32, "8"), ("32_one_short", 9, 32, 31, "8"),
             ("32_tail", 70, 40, 75, "32")]
    spec += [("8_holds", 3, 20, 8, "8"), ("8_one_short", 3, 20, 7, "byte"), ("byte_to_the_end", 7, 9, 7, "byte"), ("byte_pattern_end", 5, 1, 5, "byte")]
    # one byte nearer than a branch's distance, and longer than its trip: the wider copy would read what it has not written yet
    spec += [("264_dist_263_long", 258, 263, 264, "128"), ("128_dist_127_long", 200, 127, 210, "32"), ("32_dist_31_long", 40, 31, 45, "8"),
             ("pattern_dist_8_long", 30, 8, 40, "8")]
    rng = np.random.default_rng(17)
    out = []
    for name, ln, dist, room, branch in spec:
        for at_start in (False, True):
            pos = dist if at_start else dist + 5
            toks = _lits(rng, pos) + [(ln, dist)] + _lits(rng, room - ln)
            out.append((f"asm/branch/{name}" + ("/from_first_byte" if at_start else ""), toks, branch))
    return out


def _assembled():
    """[(name, body)], {branch: [names]}, [(name, BTYPE)], {name: code-length operations}."""
    rng = np.random.default_rng(23)
    out, reached, btypes, ops = [], {b: [] for b in BRANCHES}, [], {}

    def add(name, d: Deflate, tokens=()):
        out.append((name, d.body()))
        btypes.extend((name, t) for t, _ in d.blocks)
        ops[name] = d.ops
        for b in first_branches(list(tokens)):
            reached[b].append(name)

    for i, (name, toks, branch) in enumerate(_branch_cases()):
        got = first_branches(toks)
        assert got == [branch], (name, got, branch)
        add(name, Deflate().dynamic(toks) if i % 2 else Deflate().fixed(toks, True), toks)
    # several deflate blocks of changing type in one stream; matches reach back across the boundaries, empty blocks between
    head = bytes(rng.integers(97, 123, size=300, dtype=np.uint8))
    t1 = _lits(rng, 40) + [(258, 300), (20, 330), (3, 1)]
    t2 = [(100, 600), 65, (9, 32)] + _lits(rng, 9)
    add("asm/blocks/stored_fixed_dynamic", Deflate().stored(head, False).stored(b"", False).fixed(t1, False).fixed([], False)
        .dynamic(t2, final=False).stored(b"xyz", False).dynamic([(3, 3), (258, 264)], final=False).dynamic([], final=True))
    add("asm/blocks/stored_last", Deflate().fixed(_lits(rng, 13), False).stored(b"", False).stored(head[:77], True))
    # code shapes
    all_ll = flat_lengths(range(286), 286)
    all_d = flat_lengths(range(30), 30)
    toks = _lits(rng, 300, 0, 256) + [(11, 7), (258, 200)]
    add("asm/shape/hlit29_hdist29_hclen15", Deflate().dynamic(toks, all_ll, all_d, rle=rle_plain, cl_lengths=flat_lengths(range(19), 19)), toks)
    toks = _lits(rng, 50, 0, 255)
    ll = [8] * 255 + [0, 8]                                                        # 256 codes of eight bits: literals 0..254 and 256
    add("asm/shape/hlit0_hdist0_hclen1", Deflate().dynamic(toks, ll, [0], rle=rle_plain, cl_lengths=flat_lengths((0, 8), 19)), toks)
    assert header_fields(out[-1][1]) == (0, 0, 1) and header_fields(out[-2][1]) == (29, 29, 15)
    lit16 = sorted(int(x) for x in rng.choice(200, size=10, replace=False))
    ll = skewed_lengths(lit16 + [256, 257, 260, 270, 284, 285], 286)
    dl = skewed_lengths(list(range(14)) + [20, 29], 30)
    toks = []
    for k in range(60):
        toks += [lit16[int(x)] for x in rng.integers(10, size=3)]
        if k > 4:
            toks.append((int(rng.choice((3, 6, 25, 257, 258))), int(rng.choice((1, 2, 5, 10, 12))) if k < 50 else int(rng.integers(1025, 1100))))
    toks += [(258, 50, 284), (257, 1500)]
    add("asm/shape/codes_of_15_bits", Deflate().dynamic(toks, ll, dl), toks)
    ll = [8] * 192 + [0] * 64 + [4] * 4                                          # ... 4 4 4 4 | 4 x 16: code 16 runs across
    toks = _lits(rng, 30, 0, 192) + [(5, 3), (4, 14)]
    add("asm/shape/code16_across_the_boundary", Deflate().dynamic(toks, ll, [4] * 16), toks)
    n, at = 0, None
    for s, rep in ops["asm/shape/code16_across_the_boundary"][0]:
        if s == 16 and n < 260 < n + rep:
            at = n
        n += rep or 1
    assert at is not None, "no code 16 over the end of the literal/length lengths"
    ll = flat_lengths([0, 139, 140, 141] + list(range(145, 257)), 257)          # one length, 138 zeros, three lengths, 3 zeros, ...
    toks = [0, 139, 140, 141, 145, 255] * 3
    add("asm/shape/code18_138_code17_3", Deflate().dynamic(toks, ll, [0]), toks)
    assert (18, 138) in ops["asm/shape/code18_138_code17_3"][0] and (17, 3) in ops["asm/shape/code18_138_code17_3"][0]
    toks = _lits(rng, 40) + [(30, 25), (4, 28), (258, 32)]
    dl = [0] * 9 + [1]                                                             # one distance code (symbol 9), one bit
    add("asm/shape/one_distance_code_of_length_1", Deflate().dynamic(toks, None, dl), toks)
    add("asm/shape/no_distance_code_literals_only", Deflate().dynamic(_lits(rng, 70), None, [0] * 30))
    add("asm/shape/end_of_block_only", Deflate().fixed(_lits(rng, 5), False).dynamic([], flat_lengths([256], 257), [0], final=False).fixed([66], True))
    toks = _lits(rng, 300)
    for sym in range(257, 286):
        e = LEXT[sym - 257]
        for ex in {0, (1 << e) - 1}:
            toks += [("sym", sym, ex, *spell(3, int(rng.integers(1, 290)))[2:]), int(rng.integers(97, 123))]
    add("asm/shape/every_length_symbol", Deflate().dynamic(toks, all_ll, all_d), toks)
    add("asm/shape/every_length_symbol_fixed", Deflate().fixed(toks, True), toks)
    # every distance symbol with its extra bits all zero and all one; 32768 inside a block of 65536 bytes
    d = Deflate().stored(bytes(rng.integers(256, size=32768, dtype=np.uint8)), False)
    toks = []
    for sym in range(30):
        for ex in {0, (1 << DEXT[sym]) - 1}:
            toks += [("sym", *spell(int(rng.integers(3, 259)), 1)[:2], sym, ex), int(rng.integers(256))]
    room = 65536 - 32768 - out_len_of(toks)
    toks += [(258, 32768)] * (room // 258) + ([(room % 258, 32768)] if room % 258 >= 3 else _lits(rng, room % 258))
    add("asm/shape/every_distance_symbol_65536", d.dynamic(toks, None, all_d))
    assert 32768 + out_len_of(toks) == 65536
    return out, reached, btypes, ops


# ---- refusals ----------------------------------------------------------------------------------------------------------------
def _refusals() -> list:
    """(name, body, CRC or None for the CRC of what zlib gives, ISIZE, the error return aimed at or None for any)."""
    rng = np.random.default_rng(31)
    lits = _lits(rng, 40)
    good = Deflate().fixed(lits + [(20, 13), (3, 1)] + lits[:9], True).body()
    n_good = 40 + 23 + 9
    two = flat_lengths((65, 256), 257)
    out = [("btype_3", bytes([0b111]), 0, 4, E_TYPE),
           ("stored_len_nlen", Deflate().stored(b"abcdefgh", True, nlen=0xfff6).body(), 0, 8, E_STORED),
           ("stored_len_past_payload", Deflate().stored(b"abcde", True, length=10).body(), 0, 10, E_STORED),
           ("stored_len_past_out_len", Deflate().stored(b"abcdefghij", True).body(), None, 9, E_STORED),
           ("oversubscribed_literal_set", Deflate().dynamic([65, 66], two[:66] + [1] + [0] * 189 + [1], [0]).body(), 0, 2, E_LENGTHS),
           ("incomplete_literal_set", Deflate().dynamic([65], [2 if x else 0 for x in two], [0]).body(), 0, 1, E_LENGTHS),
           ("incomplete_distance_set_two_codes", Deflate().dynamic([65, 65, 65, (3, 1)], None, [2, 2]).body(), 0, 6, E_LENGTHS),
           ("one_distance_code_of_two_bits", Deflate().dynamic([65, 65, 65, (3, 1)], None, [2]).body(), 0, 6, E_LENGTHS),
           ("one_literal_code_of_two_bits", Deflate().fixed([65], False).dynamic([], [0] * 256 + [2], [0]).body(), 0, 1, E_LENGTHS),
           ("no_end_of_block_code", Deflate().dynamic([65, 66], flat_lengths((65, 66), 257), [0], eob=False).body(), 0, 2, E_LENGTHS),
           ("code_16_first", Deflate().dynamic([65], two, [0], rle=[(16, 3)] + rle_plain(two[3:] + [0])).body(), 0, 1, E_LENGTHS),
           ("run_past_hlit_hdist", Deflate().dynamic([65], two, [0], rle=rle_greedy(two[:66]) + [(18, 138), (18, 55)]).body(), 0, 1, E_LENGTHS),
           ("hclen_0_carries_no_length", Deflate().dynamic([], [0] * 257, [0], rle=[(18, 138), (18, 120)], cl_lengths=flat_lengths((0, 16, 17, 18), 19),
                                                           hclen=0, eob=False).body(), 0, 1, E_LENGTHS)]
    for v in (30, 31):
        out.append((f"hlit_{v}", Deflate().dynamic([65], two, [0], hlit=v).body(), 0, 1, E_LENGTHS))
        out.append((f"hdist_{v}", Deflate().dynamic([65], two, [0], hdist=v).body(), 0, 1, E_LENGTHS))
        out.append((f"fixed_distance_symbol_{v}", Deflate().fixed([65, 66, 67, ("sym", 257, 0, v, 0), 68], True).body(), 0, 7, E_CODE))
        out.append((f"fixed_length_symbol_{256 + v}", Deflate().fixed([65, 66, 67, ("sym", 256 + v, 0, 0, 0), 68], True).body(), 0, 7, E_CODE))
    out += [("unused_code_of_one_distance_code", _unused_distance_code(), 0, 6, E_CODE),
            ("distance_pos_plus_1", Deflate().fixed([65, 66, 67, (3, 4), 68], True).body(), 0, 7, E_DISTANCE),
            ("literal_one_past_isize", good, None, n_good - 1, E_SIZE),
            ("match_one_past_isize", Deflate().fixed(lits + [(20, 13)], True).body(), None, 59, E_SIZE),
            ("stream_one_short_of_isize", good, None, n_good + 1, E_SIZE)]
    # truncated payloads: what the decoder meets behind the cut differs between a padded copy and a file, so any error will do
    dyn = Deflate().dynamic(lits * 3 + [(100, 40), (258, 120)] + lits)
    out.append(("cut_in_the_header", dyn.body()[:9], 0, out_len_of(lits * 4) + 358, None))
    fx = Deflate().fixed(lits + [(258, 40, 284)] * 3 + lits, True).body()        # 3 + 40 x 8 bits, then 8 + 5 + 5 + 4 bits of match
    out.append(("cut_in_a_literal_run", fx[:21], 0, 80 + 3 * 258, None))
    out.append(("cut_in_a_match", fx[:42], 0, 80 + 3 * 258, None))
    out.append(("cut_in_the_end_of_block_code", Deflate().fixed(lits + [66], True).body()[:-1], 0, 41, None))
    out.append(("wrong_crc", good, zlib.crc32(zlib_inflate(good)[0]) ^ 0x10000, n_good, E_CRC))
    return [("refuse/" + n, b, c, i, e) for n, b, c, i, e in out]


def _unused_distance_code() -> bytes:
    """One distance code of one bit (code 0); the stream sends the other bit."""
    d = Deflate()
    toks = [65, 65, 65]
    d.dynamic(toks, flat_lengths((65, 256, 257), 258), [1], eob=False)
    d.b.code(*canonical(flat_lengths((65, 256, 257), 258))[257])
    d.b.put(1, 1)
    d.b.code(*canonical(flat_lengths((65, 256, 257), 258))[256])
    return d.body()


REFUSALS_WANTED = ("btype_3", "stored_len_nlen", "stored_len_past_payload", "stored_len_past_out_len", "oversubscribed_literal_set",
                   "incomplete_literal_set", "incomplete_distance_set_two_codes", "no_end_of_block_code", "code_16_first", "run_past_hlit_hdist",
                   "hlit_30", "hlit_31", "hdist_30", "hdist_31", "distance_pos_plus_1", "fixed_distance_symbol_30", "fixed_distance_symbol_31",
                   "fixed_length_symbol_286", "fixed_length_symbol_287", "literal_one_past_isize", "match_one_past_isize",
                   "stream_one_short_of_isize", "cut_in_the_header", "cut_in_a_literal_run", "cut_in_a_match", "wrong_crc",
                   # beyond the list: shapes zlib refuses that a lenient table builder or overrun check lets through
                   "hclen_0_carries_no_length", "one_distance_code_of_two_bits", "one_literal_code_of_two_bits",
                   "unused_code_of_one_distance_code", "cut_in_the_end_of_block_code")


# refusals whose body is a whole stream that the BGZF trailer contradicts; refusals whose body ends early (zlib's stream
# interface asks for more input there, it does not raise): every other body makes zlib raise
WRONG_ISIZE = ("literal_one_past_isize", "match_one_past_isize", "stream_one_short_of_isize", "stored_len_past_out_len")
TRUNCATED = ("stored_len_past_payload", "cut_in_the_header", "cut_in_a_literal_run", "cut_in_a_match", "cut_in_the_end_of_block_code")


@functools.lru_cache(maxsize=None)
def corpus() -> dict:
    """{"cases": ((name, body, expected or None), ...), "trailer": {refusal name: (crc, isize)}, "aim": {refusal name: error
    return or None}, "btypes": ((name, BTYPE), ...), "reached": {branch: names}} — checked by check_coverage()."""
    cases, trailer, aim = [], {}, {}
    for name, body, raw, _ in zlib_matrix():
        got = zlib_inflate(body)
        assert got == (raw, True), name
        cases.append((name, body, got[0]))
    asm, reached, btypes, _ = _assembled()
    for name, body in _flushed() + asm:
        got = zlib_inflate(body)
        assert got is not None and got[1] and len(got[0]) <= 65536 and len(body) + 26 <= 65536, (name, got and (got[1], len(got[0])))
        cases.append((name, body, got[0]))
    btypes = list(btypes) + [(m[0], (m[1][0] >> 1) & 3) for m in zlib_matrix()]
    for name, body, crc, isize, err in _refusals():
        got = zlib_inflate(body)
        short = name[len("refuse/"):]
        if err == E_CRC:
            assert got is not None and got[1] and len(got[0]) == isize and zlib.crc32(got[0]) != crc
        elif short in WRONG_ISIZE:
            assert got is not None and got[1] and len(got[0]) != isize, name     # a whole stream, not of ISIZE bytes
        elif short in TRUNCATED:
            assert got is not None and not got[1], name                          # zlib waits for the rest of the stream
        else:
            assert got is None, name                                             # zlib raises
        trailer[name] = (zlib.crc32(got[0]) if crc is None else crc, isize)
        aim[name] = err
        cases.append((name, body, None))
    assert len({c[0] for c in cases}) == len(cases)
    return {"cases": tuple(cases), "trailer": trailer, "aim": aim, "btypes": tuple(btypes), "reached": reached}


def cases() -> tuple:
    return corpus()["cases"]


def accepted() -> list:
    return [c for c in cases() if c[2] is not None]


def refusals() -> list:
    return [c for c in cases() if c[2] is None]


def check_coverage() -> dict:
    """Asserts that the corpus holds every block type per zlib strategy, reaches every copy branch, names every refusal and
    lost no more (payload, strategy) pairs to the 64 KiB limit than it may; returns what it counted."""
    c = corpus()
    by_strategy = {s: set() for s in BTYPES_OF}
    for name, body, _, sname in zlib_matrix():
        by_strategy[sname].add((body[0] >> 1) & 3)
    assert by_strategy == BTYPES_OF, by_strategy
    asm_types = {t for n, t in c["btypes"] if n.startswith("asm/")}
    assert asm_types == {0, 1, 2}, asm_types
    missing = [b for b in BRANCHES if not c["reached"][b]]
    assert not missing, f"copy branches never reached: {missing}"
    names = {n[len("refuse/"):] for n, _, e in c["cases"] if e is None}
    assert names == set(REFUSALS_WANTED), (set(REFUSALS_WANTED) - names, names - set(REFUSALS_WANTED))
    # a 65536-byte payload cannot be stored in a block of 65536 bytes; otherwise only incompressible payloads are lost, and
    # only where nothing is matched
    hard = {p for p, _, inc in payloads() if inc}
    for p, s in lost_pairs():
        assert (s in ("L0", "L9huff") and p in hard) or (s == "L0" and p.endswith("65536")), (p, s)
    n_acc = sum(1 for x in c["cases"] if x[2] is not None)
    assert n_acc <= 300, n_acc
    return {"accepted": n_acc, "refusals": len(names), "lost": lost_pairs(), "btypes": {s: sorted(v) for s, v in by_strategy.items()},
            "reached": {b: len(v) for b, v in c["reached"].items()}}


# ---- the BGZF container ------------------------------------------------------------------------------------------------------
def bgzf_block(body: bytes, crc: int, isize: int, before: bytes = b"", after: bytes = b"", mtime: int = 0, xfl: int = 0, os_: int = 0xff,
               bc: bool = True, bsize=None) -> bytes:
    """One BGZF block (SAM specification 4.1): extra subfields `before` and `after` the BC one (each SI1 SI2 SLEN data)."""
    xlen = len(before) + (6 if bc else 0) + len(after)
    total = 12 + xlen + len(body) + 8
    assert total <= 65536
    extra = before + (struct.pack("<BBHH", 66, 67, 2, total - 1 if bsize is None else bsize) if bc else b"") + after
    return struct.pack("<BBBBIBBH", 0x1f, 0x8b, 8, 4, mtime, xfl, os_, xlen) + extra + body + struct.pack("<II", crc, isize)


def subfield(si: bytes, data: bytes) -> bytes:
    return si + struct.pack("<H", len(data)) + data


def block_of(case, **kw) -> bytes:
    name, body, want = case
    crc, isize = (zlib.crc32(want), len(want)) if want is not None else corpus()["trailer"][name]
    return bgzf_block(body, crc, isize, **kw)


def bgzf_file(some_cases) -> tuple:
    """(file bytes, offsets of the blocks in it, offsets of their bytes in the decompressed stream, the decompressed stream)."""
    comp, coff, uoff, raw = bytearray(), [], [], bytearray()
    for c in some_cases:
        coff.append(len(comp))
        uoff.append(len(raw))
        comp += block_of(c)
        raw += c[2] or b""
    return bytes(comp), coff, uoff, bytes(raw)


def shuffled(some_cases, seed: int = 5) -> list:
    """A seeded order in which the lanes of a wave hold stored, fixed and dynamic blocks, long and short streams at once."""
    order = np.random.default_rng(seed).permutation(len(some_cases))
    return [some_cases[int(i)] for i in order]


def small_good(n: int = 100) -> list:
    """n small accepted cases of every kind (the company of a refusal: uploads stay small)."""
    small = [c for c in accepted() if len(c[1]) < 1500 and len(c[2]) < 4000]
    assert len(small) >= n, len(small)
    return small[:n]


HEADER_VARIANTS_OK = {
    "subfield_before_bc": dict(before=subfield(b"XY", b"\x01\x02\x03")),
    "subfield_behind_bc": dict(after=subfield(b"RA", b"")),
    "xlen_above_6_both_sides": dict(before=subfield(b"AB", bytes(40)), after=subfield(b"BD", b"BC\x02\x00\xff\xff")),
    "mtime_xfl_os": dict(mtime=0x5f3759df, xfl=4, os_=3),
}


def header_files() -> dict:
    """{"ok": {name: (file, decompressed bytes)}, "bad": {name: (file, offset of the bad block)}}: five small blocks, the
    third (or all) with the header variant; an empty block in mid-file."""
    good = small_good(5)
    plain = [block_of(c) for c in good]
    raw = b"".join(c[2] for c in good)
    ok = {}
    for name, kw in HEADER_VARIANTS_OK.items():
        ok[name] = (b"".join(plain[:2] + [block_of(good[2], **kw)] + plain[3:]), raw)
        ok[name + "_everywhere"] = (b"".join(block_of(c, **kw) for c in good), raw)
    eof = bgzf_block(b"\x03\x00", 0, 0)
    ok["empty_block_in_mid_file"] = (b"".join(plain[:2] + [eof] + plain[2:4] + [eof, eof] + plain[4:] + [eof]), raw)
    at = len(plain[0]) + len(plain[1])
    c = good[2]
    crc, isize = zlib.crc32(c[2]), len(c[2])
    bad = {
        "no_bc_subfield": bgzf_block(c[1], crc, isize, bc=False, before=subfield(b"XY", b"\x01\x02\x03\x04")),
        "bsize_past_the_file": bgzf_block(c[1], crc, isize, bsize=60000),
        "bsize_trailer_overlaps_header": bgzf_block(c[1], crc, isize, bsize=18),
        "isize_above_65536": bgzf_block(c[1], crc, 65537),
    }
    out_bad = {}
    for name, blk in bad.items():
        tail = b"" if name == "bsize_past_the_file" else b"".join(plain[3:])
        out_bad[name] = (b"".join(plain[:2]) + blk + tail, at)
    return {"ok": ok, "bad": out_bad}
