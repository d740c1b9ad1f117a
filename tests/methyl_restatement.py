"""A second, brute-force statement of the methylation rule, written without looking at frontend/methyl.py's
way of doing it: the stored SEQ is reverse-complemented into the read as sequenced, the skips of the C+m entry are walked
base by base into a per-base probability array, CpG sites are found on the sequenced strand and mapped back to the stored
positions.  tests/test_methyl_rule.py holds the two together."""
from __future__ import annotations

import re
import struct

OK, NOT_SPANNING, NO_TAGS, CLIPPED, MALFORMED, NO_SITES = range(6)
_ENTRY = re.compile(r"\A([ACGTUN])([+-])([a-z]+|[0-9]+)([.?]?)((?:,[0-9]{1,10})*)\Z")
_SIZES = {"A": 1, "c": 1, "C": 1, "s": 2, "S": 2, "i": 4, "I": 4, "f": 4}
_INTS = {"c": "<b", "C": "<B", "s": "<h", "S": "<H", "i": "<i", "I": "<I"}
_COMP = str.maketrans("ACGT", "TGCA")


def aux_fields(tags: bytes) -> list[tuple[bytes, str, bytes]]:
    """Every field as (tag, type, value bytes); ValueError for a chain that does not end where the record ends."""
    out, t = [], 0
    while t < len(tags):
        if t + 3 > len(tags):
            raise ValueError("truncated")
        ty = chr(tags[t + 2])
        if ty in _SIZES:
            size = _SIZES[ty]
        elif ty in "ZH":
            size = tags.index(b"\0", t + 3) - (t + 3) + 1          # (ValueError without a NUL)
        elif ty == "B":
            if t + 8 > len(tags) or chr(tags[t + 3]) not in "cCsSiIf":
                raise ValueError("bad array")
            size = 5 + struct.unpack_from("<I", tags, t + 4)[0] * _SIZES[chr(tags[t + 3])]
        else:
            raise ValueError("unknown type")
        if t + 3 + size > len(tags):
            raise ValueError("runs past the end")
        out.append((tags[t:t + 2], ty, tags[t + 3:t + 3 + size]))
        t += 3 + size
    return out


def brute(seq: str, flag: int, cigar, tags: bytes, q_l, q_r, threshold: int = 127) -> tuple[int, int, int, int]:
    fields = aux_fields(tags)
    if q_l is None:
        return NOT_SPANNING, 0, 0, 0

    def first(tag, types):
        return next((v for t, ty, v in fields if t == tag and ty in types), None)
    mm, ml = first(b"MM", "Z"), first(b"ML", "B")
    if mm is None and ml is None:
        mm, ml = first(b"Mm", "Z"), first(b"Ml", "B")
    if mm is None:
        return NO_TAGS, 0, 0, 0
    mn = next(((ty, v) for t, ty, v in fields if t == b"MN" and ty in _INTS), None)
    if any(int(c) % 16 == 5 for c in cigar) or (mn is not None and struct.unpack(_INTS[mn[0]], mn[1])[0] != len(seq)):
        return CLIPPED, 0, 0, 0
    text = mm[:-1].decode("latin-1")
    if text.endswith(";"):
        text = text[:-1]
        if text == "":
            return MALFORMED, 0, 0, 0
    entries = []
    for part in (text.split(";") if text else []):
        m = _ENTRY.match(part)
        if not m:
            return MALFORMED, 0, 0, 0
        nums = [int(x) for x in m.group(5).split(",")[1:]]
        if any(x > 2**31 - 1 for x in nums):
            return MALFORMED, 0, 0, 0
        codes = list(m.group(3)) if m.group(3).isalpha() else [m.group(3)]
        entries.append((m.group(1) + m.group(2), codes, m.group(4), nums))
    ml_sub, ml_bytes = ("C", b"") if ml is None else (chr(ml[0]), ml[5:])
    if ml_sub != "C" or sum(len(c) * len(n) for _, c, _, n in entries) != len(ml_bytes):
        return MALFORMED, 0, 0, 0
    off = 0
    for head, codes, mode, nums in entries:
        if head == "C+" and "m" in codes and codes[0].isalpha():
            break
        off += len(codes) * len(nums)
    else:
        return NO_TAGS, 0, 0, 0
    stride, j = len(codes), codes.index("m")
    reverse = bool(flag & 16)
    n = len(seq)
    read = seq[::-1].translate(_COMP) if reverse else seq          # the read as sequenced
    prob = [None] * n                                              # per base of the sequenced read
    i = 0
    for t, d in enumerate(nums):
        left = d
        while True:
            if i >= n:
                return MALFORMED, 0, 0, 0
            if read[i] == "C":
                if left == 0:
                    prob[i] = ml_bytes[off + t * stride + j]
                    i += 1
                    break
                left -= 1
            i += 1
    sites = known = mc = 0
    for i in range(n - 1):
        if read[i] != "C" or read[i + 1] != "G":
            continue
        p = n - 2 - i if reverse else i                            # the stored position of the site's C
        if not q_l <= p < q_r:
            continue
        sites += 1
        if prob[i] is not None:
            known += 1
            mc += prob[i] > threshold
        elif mode != "?":
            known += 1
    return (OK if known else NO_SITES), sites, known, mc
