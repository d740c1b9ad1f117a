"""5-methyl CpG calls of a read inside a locus's tract, from its MM / ML tags, stated readably.

The reference has this in compiled Rust (STRkitAlignedSegment.get_methylation_prop(locus, 127, 0.0) of strkit_rust_ext; call
site strkit/call/call_locus.py:1301-1305, per-allele means 1621-1640) that is not in its tree, so the rule here is this
project's own and UNPINNED.  It is built from the SAM tags specification (MM, ML, MN) and the three things the
reference's tree does say: a probability threshold of 127, the name "5-methyl CpG sites", and an alpha of 0.0 (not a
parameter here).  Plain Python and numpy, no call into the library: `read_methylation` is what the Python block path runs and
what tests compare the library's host function (strk_methyl) and device kernel (k_dbam_methyl) against.  `methyl` binds those
two for the readers of frontend/native.py.

The order in which an item is judged: a broken auxiliary chain (ValueError; STRK_E_INVALID in the library), a tract that
extraction would not give (NOT_SPANNING), no MM (NO_TAGS), hard clips (CLIPPED), MM's grammar and ML's length (MALFORMED), no
C+m entry (NO_TAGS), a skip past the last target (MALFORMED), then the sites (OK, or NO_SITES when none is known).
"""
from __future__ import annotations

import struct

import numpy as np

from .. import _lib
from .._lib import (STRK_METHYL_CLIPPED, STRK_METHYL_MALFORMED, STRK_METHYL_NO_SITES, STRK_METHYL_NO_TAGS,
                    STRK_METHYL_NOT_SPANNING, STRK_METHYL_OK)

__all__ = ["METHYL_THRESHOLD", "STATUS_NAMES", "MalformedMM", "find_tags", "parse_mm", "read_methylation", "segment_methylation",
           "methyl", "methyl_constants", "allele_means", "record_values", "methyl_row", "tract_of"]

METHYL_THRESHOLD = 127   # call_locus.py:1303
STATUS_NAMES = ("OK", "NOT_SPANNING", "NO_TAGS", "CLIPPED", "MALFORMED", "NO_SITES")
_FIXED = {"A": 1, "c": 1, "C": 1, "s": 2, "S": 2, "i": 4, "I": 4, "f": 4}
_INT_TYPES = {"c": "<b", "C": "<B", "s": "<h", "S": "<H", "i": "<i", "I": "<I"}


class MalformedMM(ValueError):
    pass


# ---- tags -------------------------------------------------------------------------------------------------------------------
def find_tags(tags: bytes, want: dict[bytes, str]) -> dict[bytes, tuple[str, int, int]]:
    """The auxiliary fields of a record, walked to their end: per wanted two-letter tag the (type letter, offset of the value,
    bytes of the value) of its FIRST occurrence whose type is of the wanted class ("int", "Z" or "B").  A chain that runs past
    the end of the record, a Z without its NUL, a B that does not fit, or a type the format does not know raises ValueError."""
    t, n = 0, len(tags)
    found: dict[bytes, tuple[str, int, int]] = {}
    while t < n:
        if t + 3 > n:
            raise ValueError("auxiliary fields: truncated tag")
        tag, ty = tags[t:t + 2], chr(tags[t + 2])
        v = t + 3
        if ty in _FIXED:
            size = _FIXED[ty]
        elif ty in "ZH":
            z = tags.find(b"\0", v)
            if z < 0:
                raise ValueError("auxiliary fields: string without its NUL")
            size = z - v + 1
        elif ty == "B":
            if v + 5 > n:
                raise ValueError("auxiliary fields: truncated array")
            sub = chr(tags[v])
            if sub not in _FIXED or sub == "A":
                raise ValueError("auxiliary fields: unknown array type")
            size = 5 + struct.unpack_from("<I", tags, v + 1)[0] * _FIXED[sub]
        else:
            raise ValueError("auxiliary fields: unknown type")
        if v + size > n:
            raise ValueError("auxiliary fields: value runs past the end of the record")
        cls = "int" if ty in _INT_TYPES else ty
        if tag in want and tag not in found and want[tag] == cls:
            found[tag] = (ty, v, size)
        t = v + size
    return found


# ---- the MM string ----------------------------------------------------------------------------------------------------------
def parse_mm(mm: bytes) -> list[dict]:
    """The entries of an MM string, in order: {"base", "strand", "codes" (a list: the letters, or one ChEBI number as a
    string), "mode" ('.', '?' or ''), "skips" (a list of ints)}.  Entries are separated by ';', the last ';' may be missing, an
    empty string has no entries.  An entry is one base letter of ACGTUN, '+' or '-', one or more lower-case letters or a
    decimal number, an optional '.' or '?', then zero or more ",<decimal>" of 1-10 digits and a value <= 2^31 - 1.  Anything
    else raises MalformedMM."""
    text = mm.decode("latin-1")
    if not text:
        return []
    parts = text.split(";")
    if parts[-1] == "":
        parts.pop()
    out = []
    for part in parts:
        head, *nums = part.split(",")
        if len(head) < 3 or head[0] not in "ACGTUN" or head[1] not in "+-":
            raise MalformedMM(f"entry head {head!r}")
        body, mode = (head[2:-1], head[-1]) if head[-1] in ".?" else (head[2:], "")
        if body and all("a" <= ch <= "z" for ch in body):
            codes = list(body)
        elif body and all("0" <= ch <= "9" for ch in body):
            codes = [body]
        else:
            raise MalformedMM(f"entry head {head!r}")
        skips = []
        for x in nums:
            if not (1 <= len(x) <= 10 and all("0" <= ch <= "9" for ch in x)) or int(x) > 2**31 - 1:
                raise MalformedMM(f"number {x!r}")
            skips.append(int(x))
        out.append({"base": head[0], "strand": head[1], "codes": codes, "mode": mode, "skips": skips})
    return out


# ---- one read -----------------------------------------------------------------------------------------------------------------
def read_methylation(seq: str, flag: int, cigar: np.ndarray, tags: bytes, q_l: int | None, q_r: int | None,
                     threshold: int = METHYL_THRESHOLD) -> tuple[int, int, int, int]:
    """(status, sites, known, mc) of one read.  seq = the stored SEQ, cigar = the record's own CIGAR (for its hard clips),
    [q_l, q_r) = the tract in positions of SEQ: the bases extraction returns as `tr` (None: it would not extract the read).

    MM:Z and ML:B,C at their first occurrence (Mm / Ml where the record has neither MM nor ML).  The entry taken is the first
    with base C, strand + and the code m among its letter codes, at index j of c codes; an entry of n numbers and c codes owns
    n * c bytes of ML, in entry order, and the t-th number's probability is ML[off + t * c + j].  The t-th number d_t gives the
    ordinal o_t = o_(t-1) + d_t + 1 (o_(-1) = -1) among the target bases of the read AS SEQUENCED: the stored Cs counted from
    SEQ[0] upward for a forward read, the stored Gs counted from SEQ[l_seq - 1] downward for a reverse one.  A site is a stored
    position p in [q_l, q_r) with SEQ[p] = C and SEQ[p + 1] = G (which may lie one past the tract); its call base is p on a
    forward read, p + 1 on a reverse one, its ordinal the number of targets in front of that base in the direction of
    counting.  A site whose ordinal is some o_t is known with that probability; otherwise it is known with probability 0 (mode
    '.' or none) or unknown (mode '?').  mc = the known sites with probability > threshold."""
    found = find_tags(tags, {b"MM": "Z", b"ML": "B", b"Mm": "Z", b"Ml": "B", b"MN": "int"})
    if q_l is None or q_r is None:
        return STRK_METHYL_NOT_SPANNING, 0, 0, 0
    k_mm, k_ml = (b"Mm", b"Ml") if b"MM" not in found and b"ML" not in found else (b"MM", b"ML")
    if k_mm not in found:
        return STRK_METHYL_NO_TAGS, 0, 0, 0
    if any(int(c) & 15 == 5 for c in cigar):
        return STRK_METHYL_CLIPPED, 0, 0, 0
    if b"MN" in found:
        ty, v, _ = found[b"MN"]
        if struct.unpack_from(_INT_TYPES[ty], tags, v)[0] != len(seq):
            return STRK_METHYL_CLIPPED, 0, 0, 0
    _, v, size = found[k_mm]
    try:
        entries = parse_mm(tags[v:v + size - 1])
    except MalformedMM:
        return STRK_METHYL_MALFORMED, 0, 0, 0
    ml, ml_sub = b"", "C"
    if k_ml in found:
        _, v, size = found[k_ml]
        ml_sub, ml = chr(tags[v]), tags[v + 5:v + size]
    if ml_sub != "C" or sum(len(e["skips"]) * len(e["codes"]) for e in entries) != len(ml):
        return STRK_METHYL_MALFORMED, 0, 0, 0
    off, taken = 0, None
    for e in entries:
        if e["base"] == "C" and e["strand"] == "+" and "m" in e["codes"] and not e["codes"][0].isdigit():
            taken = e
            break
        off += len(e["skips"]) * len(e["codes"])
    if taken is None:
        return STRK_METHYL_NO_TAGS, 0, 0, 0
    c, j = len(taken["codes"]), taken["codes"].index("m")
    reverse = bool(flag & 0x10)
    n = len(seq)
    # the stored positions of the targets, in the order the read was sequenced
    targets = [p for p in range(n - 1, -1, -1) if seq[p] == "G"] if reverse else [p for p in range(n) if seq[p] == "C"]
    prob_at: dict[int, int] = {}
    o = -1
    for t, d in enumerate(taken["skips"]):
        o += d + 1
        if o >= len(targets):
            return STRK_METHYL_MALFORMED, 0, 0, 0
        prob_at[targets[o]] = ml[off + t * c + j]
    sites = known = mc = 0
    for p in range(max(q_l, 0), min(q_r, n - 1)):
        if seq[p] != "C" or seq[p + 1] != "G":
            continue
        sites += 1
        call_base = p + 1 if reverse else p
        if call_base in prob_at:
            known += 1
            mc += prob_at[call_base] > threshold
        elif taken["mode"] != "?":
            known += 1
    return (STRK_METHYL_OK if known else STRK_METHYL_NO_SITES), sites, known, mc


def tract_of(seg, coords, alt=None) -> tuple[int, int] | tuple[None, None]:
    """[q_l, q_r) of a segment for the four locus boundaries: the read positions extraction cuts the tract at, through the
    record's alignment or the substitute one (`alt` = (read-alignment CIGAR, reference start)); (None, None) where extraction
    would not extract the read, whatever its flank size, for a reason other than base quality: the four positions are not in
    order, or the tract ends past the record's bases (an alignment longer than its sequence)."""
    from .extract import get_read_coords_from_cigar

    class _Alt:
        pass
    walked = seg
    if alt is not None:
        walked = _Alt()
        walked.cigar, walked.start = np.asarray(alt[0], np.uint32), int(alt[1])
    rc = get_read_coords_from_cigar(int(coords[0]), int(coords[1]), int(coords[2]), int(coords[3]), walked)
    if rc.is_incomplete():
        return None, None
    a, b, c, d = rc.left_flank_start, rc.left_flank_end, rc.right_flank_start, rc.right_flank_end
    if not (0 <= a <= b <= c <= d and c <= len(seg.query_sequence)):
        return None, None
    return b, c


def segment_methylation(seg, coords, alt=None, threshold: int = METHYL_THRESHOLD) -> tuple[int, int, int, int]:
    """read_methylation of an AlignedSegment for a locus's boundaries."""
    q_l, q_r = tract_of(seg, coords, alt)
    return read_methylation(seg.query_sequence, seg.flag, seg.cigar, seg.tags, q_l, q_r, threshold)


# ---- the library's functions ------------------------------------------------------------------------------------------------
def methyl_constants() -> dict[str, int]:
    """The size constants of k_dbam_methyl as built."""
    out = np.zeros(4, np.int32)
    _lib.load().strk_methyl_constants(out.ctypes.data_as(_lib._i32p))
    return dict(zip(("chunk_bases", "seq_pass_bases", "mm_pass_bytes", "window"), out.tolist()))


def methyl(bam, rec: np.ndarray, coords: np.ndarray, alt: dict[int, tuple[np.ndarray, int]] | None = None,
           threshold: int = METHYL_THRESHOLD, piece_items: int = 0) -> dict:
    """status / sites / known / mc (int32 arrays) of items (record index, four locus boundaries) of a reader of
    frontend/native.py; `alt` maps item number to (read-alignment CIGAR, reference start) for realigned reads.  A DeviceBam
    runs k_dbam_methyl over the file in HBM, a host reader strk_methyl over its buffer."""
    from .native import DeviceBam, alt_arrays
    L = _lib.load()
    n = int(len(rec))
    rec_off = np.ascontiguousarray(bam.rec_off[np.asarray(rec, np.int64)], np.int64)
    coords = np.ascontiguousarray(coords, np.int64).reshape(n, 4)
    a_cig, a_off, a_start = alt_arrays(n, alt)
    out = {k: np.zeros(n, np.int32) for k in ("status", "sites", "known", "mc")}
    outs = [_lib.ptr(out[k]) for k in ("status", "sites", "known", "mc")]
    if isinstance(bam, DeviceBam):
        _lib.check(L.strk_dbam_methyl(bam._h, n, _lib.ptr(rec_off), _lib.ptr(coords), _lib.ptr(a_cig), _lib.ptr(a_off), _lib.ptr(a_start),
                                      int(threshold), int(piece_items), *outs))
    else:
        _lib.check(L.strk_methyl(_lib.ptr(bam.data), int(bam.data.size), n, _lib.ptr(rec_off), _lib.ptr(coords), _lib.ptr(a_cig), _lib.ptr(a_off),
                                 _lib.ptr(a_start), int(threshold), *outs))
    return out


# ---- rows -------------------------------------------------------------------------------------------------------------------
def record_values(status: int, known: int, mc: int) -> tuple[float | None, int | None]:
    """(m, mc) of a read record: m = mc / known, one float64 division; (None, None) unless the status is OK."""
    return (int(mc) / int(known), int(mc)) if int(status) == STRK_METHYL_OK else (None, None)


def methyl_row(row: dict, recs: list[dict]) -> None:
    """peaks.am / peaks.amc of a called locus from its read records (which carry `p`, `m` and `mc`), where every peak has a
    read with a value."""
    peaks = row.get("peaks")
    if not peaks or not row.get("call"):
        return
    means = allele_means([r.get("p") for r in recs], [r.get("m") for r in recs], [r.get("mc") for r in recs], int(peaks["modal_n"]))
    if means is not None:
        peaks["am"], peaks["amc"] = means


# ---- per allele -------------------------------------------------------------------------------------------------------------
def allele_means(peak_of_read, m, mc, n_peaks: int) -> tuple[list[float], list[float]] | None:
    """(am, amc) of a called locus (call_locus.py:1621-1640): per peak the mean of m, and of mc, over its reads that have a
    value (m is not None), in read order.  Each is a float64 sum, one rounding per addition, divided once by the number of
    values; the reference's statistics.mean rounds once for the whole sum, so the two may differ in the last place.  None when
    any peak has no read with a value (call_locus.py:1624: the locus then has neither)."""
    sums = [[0.0, 0.0, 0] for _ in range(n_peaks)]
    for p, x, y in zip(peak_of_read, m, mc):
        if x is None or p is None or not 0 <= int(p) < n_peaks:
            continue
        s = sums[int(p)]
        s[0] += float(x)
        s[1] += float(y)
        s[2] += 1
    if n_peaks == 0 or any(s[2] == 0 for s in sums):
        return None
    return [s[0] / s[2] for s in sums], [s[1] / s[2] for s in sums]
