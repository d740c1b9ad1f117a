"""What the phased allele call needs from an alignment file, stated readably: per read its haplotags, per read and candidate
SNV position the base under the read's alignment (a "cell"), per locus the choice of the useful SNVs.

The reference has this in compiled Rust (process_read_snvs_for_locus_and_calculate_useful_snvs, STRkitAlignedSegment.hp / .ps
of strkit_rust_ext; call sites strkit/call/call_locus.py:1147-1260) that is not in its tree, so the rule here is this
project's own and UNPINNED, as the combination rule of DESIGN.md §13 is.  Plain Python and numpy, no call into the library:
the functions of the first half are what the Python block path runs and what tests compare the library's host functions
(strk_phase_cells, strk_useful_snvs) and device kernels (k_dbam_phase_cells, k_snv_useful) against.  The second half binds
those library functions for the readers of frontend/native.py.
"""
from __future__ import annotations

import bisect
import struct

import numpy as np

from .. import _lib

__all__ = ["MAX_CANDIDATES", "MAX_USEFUL_SNVS", "SIGNIFICANT_CLIP_THRESHOLD", "SIGNIFICANT_CLIP_SNV_TAKE_IN", "MANY_REALIGNS_THRESHOLD",
           "read_tags", "locus_candidates", "alignment_cells", "segment_cells", "useful_thresholds", "useful_snvs", "pack_cells",
           "snv_step_allowed", "PhaseSetRemap", "phase_cells", "library_useful_snvs"]

MAX_CANDIDATES = 1024                 # candidate positions of a locus
MAX_USEFUL_SNVS = 64                  # the limit of k_phase_group
SIGNIFICANT_CLIP_THRESHOLD = 100      # strkit/call/params.py:61
SIGNIFICANT_CLIP_SNV_TAKE_IN = 250    # strkit/call/call_locus.py:88
MANY_REALIGNS_THRESHOLD = 2           # strkit/call/call_locus.py:86
_INT_TYPES = {"c": "<b", "C": "<B", "s": "<h", "S": "<H", "i": "<i", "I": "<I"}
_FIXED = {"A": 1, "c": 1, "C": 1, "s": 2, "S": 2, "i": 4, "I": 4, "f": 4}
_ALIGNED, _DEL = (0, 7, 8), 2
_CONSUMES_QUERY, _CONSUMES_REF = (0, 1, 4, 7, 8), (0, 2, 3, 7, 8)


# ---- tags ---------------------------------------------------------------------------------------------------------------------
def read_tags(tags: bytes) -> tuple[int, int]:
    """(HP, PS) of a record's auxiliary fields.  HP and PS count when their type is one of c C s S i I and the value fits an
    int32 (so a PS:I above 2^31 - 1 does not count); the first occurrence that counts is taken.  A read is tagged only with
    both, otherwise (-1, -1).  A chain that runs past the end of the record (or a type the format does not know) raises
    ValueError."""
    t, n = 0, len(tags)
    found: dict[bytes, int] = {}
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
        if tag in (b"HP", b"PS") and ty in _INT_TYPES and tag not in found:
            val = struct.unpack_from(_INT_TYPES[ty], tags, v)[0]
            if val <= 2**31 - 1:
                found[tag] = val
        t = v + size
    if b"HP" in found and b"PS" in found:
        return found[b"HP"], found[b"PS"]
    return -1, -1


# ---- candidates ---------------------------------------------------------------------------------------------------------------
def locus_candidates(positions: np.ndarray, span_start: int, span_end: int, left_flank_coord: int, right_flank_coord: int,
                     limit: int = MAX_CANDIDATES) -> np.ndarray:
    """Indices into `positions` (the 0-based, ascending SNV positions of the candidate file on the locus's contig) of the
    locus's candidates: inside [span_start, span_end) = [min pos, max end) of the locus's fetched records, outside
    [left_flank_coord, right_flank_coord), ascending; beyond `limit`, the `limit` nearest to the flanked locus (distance
    left_flank_coord - p on the left, p - (right_flank_coord - 1) on the right; ties to the left), still ascending."""
    positions = np.asarray(positions, np.int64)
    lo, hi = np.searchsorted(positions, [span_start, span_end], side="left")
    idx = np.arange(lo, max(lo, hi))
    p = positions[idx]
    idx = idx[(p < left_flank_coord) | (p >= right_flank_coord)]
    if idx.size > limit:
        p = positions[idx]
        left = p < left_flank_coord
        dist = np.where(left, left_flank_coord - p, p - (right_flank_coord - 1))
        order = np.lexsort((~left, dist))          # by distance, the left one first among equals
        idx = np.sort(idx[order[:limit]])
    return idx


# ---- cells --------------------------------------------------------------------------------------------------------------------
def alignment_cells(cigar: np.ndarray, start: int, seq: str, qual: np.ndarray | None, cand: np.ndarray,
                    clip_threshold: int = SIGNIFICANT_CLIP_THRESHOLD, take_in: int = SIGNIFICANT_CLIP_SNV_TAKE_IN) -> tuple[np.ndarray, np.ndarray]:
    """(bytes, qualities) of one alignment at the ascending candidate positions `cand`.
    s / e = reference coordinate of the first aligned pair (ops M = X) and one past that of the last; the soft clips are the
    first / last operation when it is S (strk_fe::cigar_span); lo = s + (take_in if clip_l >= clip_threshold), hi likewise.
    c outside [lo, hi): ('-', 0).  Inside an aligned op at offset d: the read's base and quality at q0 + d (quality 0 without
    qualities; a read position beyond the bases leaves ('-', 0)).  Inside D: ('_', 0).  Inside N: ('-', 0)."""
    cand = [int(c) for c in cand]
    base = np.full(len(cand), ord("-"), np.uint8)
    q_out = np.zeros(len(cand), np.uint8)
    ops = [(int(c) & 15, int(c) >> 4) for c in cigar]
    if not ops:
        return base, q_out
    clip_l = ops[0][1] if ops[0][0] == 4 else 0
    clip_r = ops[-1][1] if ops[-1][0] == 4 else 0
    # first pass: where every operation starts, s and e
    r, q, runs, s, e = int(start), 0, [], None, None
    for op, ln in ops:
        if op in _ALIGNED and ln > 0:
            s = r if s is None else s
            e = r + ln
        runs.append((op, ln, r, q))
        r += ln if op in _CONSUMES_REF else 0
        q += ln if op in _CONSUMES_QUERY else 0
    if s is None:
        return base, q_out
    lo = s + (take_in if clip_l >= clip_threshold else 0)
    hi = e - (take_in if clip_r >= clip_threshold else 0)
    for op, ln, r0, q0 in runs:
        if ln == 0 or not (op in _ALIGNED or op == _DEL):
            continue
        for k in range(bisect.bisect_left(cand, max(r0, lo)), bisect.bisect_left(cand, min(r0 + ln, hi))):
            if op == _DEL:
                base[k] = ord("_")
                continue
            qi = q0 + cand[k] - r0
            if qi < len(seq):
                base[k] = ord(seq[qi])
                q_out[k] = 0 if qual is None else int(qual[qi])
    return base, q_out


def segment_cells(seg, cand: np.ndarray, alt: tuple[np.ndarray, int] | None = None, clip_threshold: int = SIGNIFICANT_CLIP_THRESHOLD,
                  take_in: int = SIGNIFICANT_CLIP_SNV_TAKE_IN) -> tuple[np.ndarray, np.ndarray]:
    """alignment_cells of an AlignedSegment; `alt` = (read-alignment CIGAR, reference start) of a realigned read, which is
    then walked instead of the record's own alignment (it spans only the flanked locus, where no candidate lies)."""
    cigar, start = (np.asarray(alt[0], np.uint32), int(alt[1])) if alt is not None else (seg.cigar, seg.start)
    return alignment_cells(cigar, start, seg.query_sequence, seg.query_qualities, cand, clip_threshold, take_in)


# ---- useful SNVs --------------------------------------------------------------------------------------------------------------
def useful_thresholds(n: int, min_allele_reads: int) -> tuple[int, int]:
    """float64, round half to even: n = 10 gives 6 and n = 30 gives 16 for the second."""
    return max(int(np.rint(n / 5.0)), int(min_allele_reads)), max(int(np.rint(n * 0.55)), 5)


def useful_snvs(base: np.ndarray, min_allele_reads: int, limit: int = MAX_USEFUL_SNVS) -> np.ndarray:
    """Candidate indices of the useful SNVs of a locus from the bytes of its kept reads' cells, `base` [n reads, candidates]:
    per candidate the bytes other than '-' and '_' are counted (no quality filter); useful iff at least two distinct bytes
    each have count >= a_thr and the counted cells number >= t_thr; ascending, the first `limit`."""
    base = np.asarray(base, np.uint8)
    n = base.shape[0]
    a_thr, t_thr = useful_thresholds(n, min_allele_reads)
    out = []
    for c in range(base.shape[1] if base.ndim == 2 else 0):
        col = base[:, c]
        col = col[(col != ord("-")) & (col != ord("_"))]
        counts = np.bincount(col, minlength=256)
        if int((counts >= a_thr).sum()) >= 2 and int(col.size) >= t_thr:
            out.append(c)
            if len(out) == limit:
                break
    return np.asarray(out, np.int32)


def pack_cells(base: list[np.ndarray], qual: list[np.ndarray], sel: list[np.ndarray]) -> tuple[np.ndarray, np.ndarray, np.ndarray]:
    """(snv_off, snv_base, snv_qual) as strk_call_alleles_phased takes them, from per locus the kept reads' cells
    [n, candidates] and the chosen candidate indices: read-major per locus, loci back to back."""
    snv_off = np.concatenate(([0], np.cumsum([len(s) for s in sel]))).astype(np.int32)
    take = lambda x, s: np.asarray(x, np.uint8)[:, s].ravel() if len(x) and len(s) else np.zeros(0, np.uint8)  # noqa: E731
    b = [take(x, s) for x, s in zip(base, sel)]
    q = [take(x, s) for x, s in zip(qual, sel)]
    cat = lambda xs: np.concatenate(xs).astype(np.uint8) if xs else np.zeros(0, np.uint8)  # noqa: E731
    return snv_off, cat(b), cat(q)


def snv_step_allowed(n_alleles: int, n_realigned_kept: int, have_rare_realigns: bool) -> bool:
    """The locus gates: no SNV step for a locus whose n_alleles != 2, with MANY_REALIGNS_THRESHOLD or more realigned kept
    reads, or with a "rare realign" (get_have_rare_realigns, call_locus.py:961-971)."""
    return n_alleles == 2 and n_realigned_kept < MANY_REALIGNS_THRESHOLD and not have_rare_realigns


class PhaseSetRemap:
    """Original PS values renumbered 1, 2, ... in order of first appearance (block order, locus order, read order); one object
    per run (the reference's counter starts at 1, call_sample.py:379).  Untagged (-1) stays -1.  With a `counter` (an object
    with take(): phase_sets.PhaseSets, which numbers the SNV calls' sets from the same sequence) a new value takes its number
    from there, and clear() forgets the values of a finished contig."""

    def __init__(self, counter=None):
        self._ids: dict[int, int] = {}
        self._counter = counter

    def __call__(self, ps: np.ndarray, hp: np.ndarray | None = None) -> np.ndarray:
        ps = np.asarray(ps, np.int32)
        out = np.full(ps.shape, -1, np.int32)
        tagged = (ps != -1) if hp is None else (np.asarray(hp) != -1) | (ps != -1)
        for i in np.nonzero(tagged.ravel())[0]:
            key = int(ps.ravel()[i])
            if key not in self._ids:
                self._ids[key] = len(self._ids) + 1 if self._counter is None else self._counter.take()
            out.ravel()[i] = self._ids[key]
        return out

    def __len__(self) -> int:
        return len(self._ids)

    def clear(self) -> None:
        self._ids.clear()

    def originals(self) -> dict[int, int]:
        """{number handed out: the original value it stands for (-1: HP without PS)}."""
        return {number: value for value, number in self._ids.items()}

    def snapshot(self) -> dict:
        """The ids handed out so far; restore() puts them back (a block that failed is run again and numbers its phase sets anew)."""
        return dict(self._ids)

    def restore(self, ids: dict) -> None:
        self._ids = dict(ids)


# ---- the library's functions ----------------------------------------------------------------------------------------------
def phase_cells(bam, rec_idx: np.ndarray, item_locus: np.ndarray, cand_off: np.ndarray, cand_pos: np.ndarray,
                alt: dict[int, tuple[np.ndarray, int]] | None = None, clip_threshold: int = SIGNIFICANT_CLIP_THRESHOLD,
                take_in: int = SIGNIFICANT_CLIP_SNV_TAKE_IN, piece_items: int = 0, download: bool = False) -> dict:
    """Tags and cells of items (record index, locus) of a reader of frontend/native.py.  A DeviceBam runs k_dbam_phase_cells and
    keeps the cells in HBM (download=True copies them back too); a host reader runs strk_phase_cells and returns them."""
    from .native import DeviceBam, alt_arrays
    L = _lib.load()
    n = int(len(rec_idx))
    rec_off = np.ascontiguousarray(bam.rec_off[np.asarray(rec_idx, np.int64)], np.int64)
    item_locus = np.ascontiguousarray(item_locus, np.int32)
    cand_off = np.ascontiguousarray(cand_off, np.int32)
    cand_pos = np.ascontiguousarray(cand_pos, np.int64)
    n_loci = int(cand_off.size) - 1
    hp, ps = np.full(n, -1, np.int32), np.full(n, -1, np.int32)
    a_cig, a_off, a_start = alt_arrays(n, alt)
    n_cells = int((cand_off[item_locus + 1] - cand_off[item_locus]).sum()) if n else 0
    out = {"hp": hp, "ps": ps, "n_cells": n_cells, "item_locus": item_locus, "cand_off": cand_off}
    if isinstance(bam, DeviceBam):
        _lib.check(L.strk_dbam_phase_cells(bam._h, n, _lib.ptr(rec_off), _lib.ptr(item_locus), n_loci, _lib.ptr(cand_off), _lib.ptr(cand_pos),
                                           _lib.ptr(a_cig), _lib.ptr(a_off), _lib.ptr(a_start), int(clip_threshold), int(take_in),
                                           int(piece_items), _lib.ptr(hp), _lib.ptr(ps)))
        out["device"] = bam
        if download:
            out["base"], out["qual"] = np.empty(n_cells, np.uint8), np.empty(n_cells, np.uint8)
            _lib.check(L.strk_dbam_download_cells(bam._h, n_cells, _lib.ptr(out["base"]), _lib.ptr(out["qual"])))
        return out
    base, qual = np.empty(n_cells, np.uint8), np.empty(n_cells, np.uint8)
    _lib.check(L.strk_phase_cells(_lib.ptr(bam.data), int(bam.data.size), n, _lib.ptr(rec_off), _lib.ptr(item_locus), n_loci, _lib.ptr(cand_off),
                                  _lib.ptr(cand_pos), _lib.ptr(a_cig), _lib.ptr(a_off), _lib.ptr(a_start), int(clip_threshold), int(take_in),
                                  _lib.ptr(hp), _lib.ptr(ps), _lib.ptr(base), _lib.ptr(qual), n_cells))
    out["base"], out["qual"] = base, qual
    return out


def library_useful_snvs(cells: dict, kept_off: np.ndarray, kept_item: np.ndarray, min_allele_reads: int) -> dict:
    """The useful SNVs of every locus over the cells of a phase_cells call: snv_off, snv_cand (per useful SNV its index among
    the locus's candidates) and the packed snv_base / snv_qual (k_snv_useful + k_snv_gather for a DeviceBam's cells,
    strk_useful_snvs otherwise)."""
    L = _lib.load()
    kept_off = np.ascontiguousarray(kept_off, np.int32)
    kept_item = np.ascontiguousarray(kept_item, np.int32)
    n_loci = int(kept_off.size) - 1
    snv_off = np.zeros(n_loci + 1, np.int32)
    snv_cand = np.zeros(max(MAX_USEFUL_SNVS * n_loci, 1), np.int32)
    n_kept = np.diff(kept_off).astype(np.int64)
    n_cand = np.diff(cells["cand_off"]).astype(np.int64)
    cap = int((n_kept * np.minimum(n_cand, MAX_USEFUL_SNVS)).sum())
    base, qual = np.empty(max(cap, 1), np.uint8), np.empty(max(cap, 1), np.uint8)
    if "device" in cells:
        tot = L.strk_dbam_useful_snvs(cells["device"]._h, n_loci, _lib.ptr(kept_off), _lib.ptr(kept_item), int(min_allele_reads),
                                      _lib.ptr(snv_off), _lib.ptr(snv_cand), _lib.ptr(base), _lib.ptr(qual), cap)
    else:
        tot = L.strk_useful_snvs(int(cells["item_locus"].size), _lib.ptr(cells["item_locus"]), n_loci, _lib.ptr(cells["cand_off"]),
                                 _lib.ptr(cells["base"]), _lib.ptr(cells["qual"]), _lib.ptr(kept_off), _lib.ptr(kept_item),
                                 int(min_allele_reads), _lib.ptr(snv_off), _lib.ptr(snv_cand), _lib.ptr(base), _lib.ptr(qual), cap)
    if tot < 0:
        _lib.check(int(tot))
    return {"snv_off": snv_off, "snv_cand": snv_cand[:int(snv_off[-1])], "snv_base": base[:int(tot)], "snv_qual": qual[:int(tot)]}
