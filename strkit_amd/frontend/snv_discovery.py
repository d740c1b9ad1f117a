"""Candidate SNVs of a locus from a pileup of its own reads (`--discover-snvs`), stated readably: a position
of a window on either side of the flanked locus is a candidate when two of the four bases A C G T each occur there in enough
of the locus's kept reads.  It stands where a run with `--incorporate-snvs` asks a VCF for its candidates; everything after the
candidate list (the cells, the useful SNVs, the phased call) is unchanged.

The reference has no such step: its candidates come from a VCF, and the discovery of its earlier pure-Python releases was
replaced by compiled code that is not in its tree.  The rule here is this project's own and UNPINNED, as the rules of
frontend/phase_inputs.py are.  It never looks at the reference sequence, as useful_snvs does not: a site at which all reads
carry the same non-reference base (homozygous ALT) is not a candidate, because it cannot tell two haplotypes apart.

Plain Python and numpy, no call into the library in the first half: discover_candidates is what the Python block path runs
and what tests compare the library's host function (strk_discover_snvs) and kernels (k_snv_pileup, k_snv_pick) against.  The
second half binds those library functions for the readers of frontend/native.py."""
from __future__ import annotations

import numpy as np

from .. import _lib
from . import phase_inputs as pi

__all__ = ["DEFAULT_WINDOW", "MAX_WINDOW", "MAX_KEPT_READS", "DiscoveredSnvs", "window_positions", "window_bytes", "discover_candidates",
           "library_discover_snvs"]

DEFAULT_WINDOW = 8192          # a default of the option, not a measured threshold: about half a 15 kb read, two tiles a side
MAX_WINDOW = 65536             # strk_sd::kMaxWindow
MAX_KEPT_READS = 65535         # strk_sd::kMaxKept: the kernel's counts have 16 bits
_ACGT = np.frombuffer(b"ACGT", np.uint8)


def window_positions(left_flank_coord: int, right_flank_coord: int, window: int) -> np.ndarray:
    """The reference positions p >= 0 with left - window <= p < left or right <= p < right + window, ascending."""
    left = np.arange(max(left_flank_coord - window, 0), max(left_flank_coord, 0), dtype=np.int64)
    right = np.arange(max(right_flank_coord, 0), max(right_flank_coord + window, 0), dtype=np.int64)
    return np.concatenate((left, right))


def window_bytes(cigar: np.ndarray, start: int, seq: str, qual: np.ndarray | None, p0: int, p1: int,
                 clip_threshold: int = pi.SIGNIFICANT_CLIP_THRESHOLD, take_in: int = pi.SIGNIFICANT_CLIP_SNV_TAKE_IN) -> tuple[np.ndarray, np.ndarray]:
    """phase_inputs.alignment_cells(cigar, start, seq, qual, arange(p0, p1)) operation by operation instead of cell by cell
    (tests hold the two together): the same s / e, lo / hi with the clip take-in, '_' inside D, '-' inside N and outside
    [lo, hi), nothing for a read position beyond the bases."""
    n = max(p1 - p0, 0)
    base, q_out = np.full(n, ord("-"), np.uint8), np.zeros(n, np.uint8)
    ops = [(int(c) & 15, int(c) >> 4) for c in cigar]
    if not ops or n == 0:
        return base, q_out
    clip_l = ops[0][1] if ops[0][0] == 4 else 0
    clip_r = ops[-1][1] if ops[-1][0] == 4 else 0
    r, q, runs, s, e = int(start), 0, [], None, None
    for op, ln in ops:
        if op in (0, 7, 8) and ln > 0:
            s = r if s is None else s
            e = r + ln
        runs.append((op, ln, r, q))
        r += ln if op in (0, 2, 3, 7, 8) else 0
        q += ln if op in (0, 1, 4, 7, 8) else 0
    if s is None:
        return base, q_out
    lo = max(s + (take_in if clip_l >= clip_threshold else 0), p0)
    hi = min(e - (take_in if clip_r >= clip_threshold else 0), p1)
    seq_b = np.frombuffer(seq.encode("ascii"), np.uint8)
    for op, ln, r0, q0 in runs:
        a, b = max(r0, lo), min(r0 + ln, hi)
        if ln == 0 or a >= b or op not in (0, 2, 7, 8):
            continue
        if op == 2:
            base[a - p0:b - p0] = ord("_")
            continue
        b = min(b, r0 + len(seq_b) - q0)           # (a CIGAR longer than its bases)
        if a < b:
            base[a - p0:b - p0] = seq_b[q0 + a - r0:q0 + b - r0]
            if qual is not None:
                q_out[a - p0:b - p0] = qual[q0 + a - r0:q0 + b - r0]
    return base, q_out


def _alignment_of(entry):
    """(cigar, start, segment) a kept read is walked along.  entry = (segment, realigned[, ...]); `realigned` False / None: the
    record's own alignment; a (CIGAR, start) pair: that substitute alignment, as segment_cells takes it; True: a realigned read
    whose substitute alignment the caller does not have: it spans only the flanked locus, where no window position lies, so it
    counts as a kept read and contributes nothing."""
    seg, re_ = entry[0], entry[1]
    if isinstance(re_, tuple):
        return np.asarray(re_[0], np.uint32), int(re_[1]), seg
    if re_:
        return np.zeros(0, np.uint32), 0, seg
    return seg.cigar, seg.start, seg


def discover_candidates(entries, kept, left_flank_coord: int, right_flank_coord: int, window: int = DEFAULT_WINDOW, min_base_qual: int = 20,
                        min_allele_reads: int = 2, clip_threshold: int = pi.SIGNIFICANT_CLIP_THRESHOLD,
                        take_in: int = pi.SIGNIFICANT_CLIP_SNV_TAKE_IN, allowed: bool = True) -> np.ndarray:
    """The candidate SNV positions of one locus, ascending int64.  `entries`: the (segment, realigned) pairs fetched for the
    locus (their span bounds the candidates, as it bounds those of a VCF); `kept`: its kept reads, (segment, realigned, ...)
    each (_alignment_of), n of them: the reads useful_snvs counts over, so one pair of thresholds serves both steps.
    `allowed`: phase_inputs.snv_step_allowed of the locus; a locus that is turned away, or has no kept read, has no candidate.

    At a window position p (window_positions) a kept read contributes the cell alignment_cells gives at p; it counts iff that
    byte is one of A C G T and the read has no qualities or its quality there is >= min_base_qual ('=', 'N', the IUPAC codes,
    '_' and '-' never count).  p is a candidate iff at least two of the four counts are >= a_thr =
    useful_thresholds(n, min_allele_reads)[0]; t_thr is not applied here (useful_snvs applies it later, over the cells).
    Beyond MAX_CANDIDATES, locus_candidates' rule keeps the nearest to the flanked locus."""
    n = len(kept)
    if n == 0 or not allowed or not entries:
        return np.zeros(0, np.int64)
    a_thr = pi.useful_thresholds(n, min_allele_reads)[0]
    sides = [(max(left_flank_coord - window, 0), max(left_flank_coord, 0)), (max(right_flank_coord, 0), max(right_flank_coord + window, 0))]
    found = []
    for p0, p1 in sides:
        counts = np.zeros((4, max(p1 - p0, 0)), np.int64)
        for entry in kept:
            cigar, start, seg = _alignment_of(entry)
            b, q = window_bytes(cigar, start, seg.query_sequence, seg.query_qualities, p0, p1, clip_threshold, take_in)
            good = np.ones(b.size, bool) if seg.query_qualities is None else q >= min_base_qual
            for k in range(4):
                counts[k] += (b == _ACGT[k]) & good
        found.append(p0 + np.nonzero((counts >= a_thr).sum(axis=0) >= 2)[0])
    positions = np.concatenate(found).astype(np.int64)
    span = (min(e[0].start for e in entries), max(e[0].end for e in entries))
    return positions[pi.locus_candidates(positions, span[0], span[1], left_flank_coord, right_flank_coord)]


class DiscoveredSnvs:
    """The candidates of one locus in the shape of snv_vcf.ContigSnvs, as phase_row and snv_id read it: `pos` the discovered
    positions, `ids` empty strings (snv_id then names a site <contig>_<1-based position>), `ref` the reference base at each
    position (read from the FASTA for these positions only; "N" where the contig ends or no reference is given)."""

    def __init__(self, contig: str, pos: np.ndarray, ref=None):
        self.contig = contig
        self.pos = np.asarray(pos, np.int64)
        self.ids = [""] * self.pos.size
        self.ref = [_ref_base(ref, contig, int(p)) for p in self.pos]


def _ref_base(ref, contig: str, p: int) -> str:
    if ref is None:
        return "N"
    try:
        return ref.fetch(contig, p, p + 1).upper() or "N"
    except (KeyError, IndexError):
        return "N"


# ---- the library's functions --------------------------------------------------------------------------------------------------
def library_discover_snvs(bam, rec_idx: np.ndarray, item_locus: np.ndarray, left_coord: np.ndarray, right_coord: np.ndarray,
                          kept_off: np.ndarray, kept_item: np.ndarray, alt: dict | None = None, window: int = DEFAULT_WINDOW,
                          min_base_qual: int = 20, min_allele_reads: int = 2, clip_threshold: int = pi.SIGNIFICANT_CLIP_THRESHOLD,
                          take_in: int = pi.SIGNIFICANT_CLIP_SNV_TAKE_IN, piece_items: int = 0) -> tuple[np.ndarray, np.ndarray]:
    """(cand_off, cand_pos) of items (record index, locus) of a reader of frontend/native.py: k_snv_span / k_snv_pileup /
    k_snv_pick for a DeviceBam, strk_discover_snvs on the host's cores otherwise.  A locus that is to have no candidates (its
    gate) is given no kept read."""
    from .native import DeviceBam, alt_arrays
    L = _lib.load()
    n = int(len(rec_idx))
    rec_off = np.ascontiguousarray(bam.rec_off[np.asarray(rec_idx, np.int64)], np.int64)
    item_locus = np.ascontiguousarray(item_locus, np.int32)
    left_coord, right_coord = np.ascontiguousarray(left_coord, np.int64), np.ascontiguousarray(right_coord, np.int64)
    kept_off, kept_item = np.ascontiguousarray(kept_off, np.int32), np.ascontiguousarray(kept_item, np.int32)
    n_loci = int(left_coord.size)
    a_cig, a_off, a_start = alt_arrays(n, alt)
    cand_off = np.zeros(n_loci + 1, np.int32)
    cand_pos = np.zeros(0, np.int64)

    def call(cap):
        tail = (int(clip_threshold), int(take_in), int(window), int(min_base_qual), int(min_allele_reads))
        if isinstance(bam, DeviceBam):
            return L.strk_dbam_discover_snvs(bam._h, n, _lib.ptr(rec_off), _lib.ptr(item_locus), n_loci, _lib.ptr(left_coord), _lib.ptr(right_coord),
                                             _lib.ptr(kept_off), _lib.ptr(kept_item), _lib.ptr(a_cig), _lib.ptr(a_off), _lib.ptr(a_start), *tail,
                                             int(piece_items), _lib.ptr(cand_off), _lib.ptr(cand_pos), cap)
        return L.strk_discover_snvs(_lib.ptr(bam.data), int(bam.data.size), n, _lib.ptr(rec_off), _lib.ptr(item_locus), n_loci, _lib.ptr(left_coord),
                                    _lib.ptr(right_coord), _lib.ptr(kept_off), _lib.ptr(kept_item), _lib.ptr(a_cig), _lib.ptr(a_off), _lib.ptr(a_start),
                                    *tail, _lib.ptr(cand_off), _lib.ptr(cand_pos), cap)

    # room for 64 candidates a locus serves almost every block in one call; a block with more asks once more, at the size it was told
    cap = 64 * n_loci
    for _ in range(2):
        cand_pos = np.zeros(max(cap, 1), np.int64)
        tot = int(call(cap))
        if tot < 0:
            _lib.check(tot)
        if tot <= cap:
            return cand_off, cand_pos[:tot]
        cap = tot
    raise AssertionError("strk_discover_snvs: the size it asked for did not suffice")
