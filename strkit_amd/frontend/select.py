"""Which of the records fetched for a locus are used: the skip flags, one record per read name, the read cap,
and the reads that are chimeric in the region.  `select_segments` is the readable statement of the rule over AlignedSegments
(the python block path); `select_reads` is the same rule over the item list of the native block paths, made by the library:
strk_select_reads over a host stream, strk_dbam_select_reads (kernels k_select_small / k_select_large) over a file resident on
the device, where the names never come to the host.

Stands where the reference builds a locus's segments (block_segments.get_segments_for_locus of strkit_rust_ext, not in its
tree; call sites strkit/call/call_locus.py:1044-1057,1277-1285): the rule is this project's own statement."""
from __future__ import annotations

import numpy as np

from .. import _lib

__all__ = ["RULE_SKIP_SUPPLEMENTARY", "RULE_SKIP_SECONDARY", "RULE_UNIQUE", "CHIMERIC", "rules_of", "select_segments", "select_items",
           "select_reads", "select_constants"]

RULE_SKIP_SUPPLEMENTARY, RULE_SKIP_SECONDARY, RULE_UNIQUE = 1, 2, 4
KEPT, SUPPLEMENTARY, SECONDARY, DUPLICATE, OVER_CAP = range(5)
CHIMERIC = 3                    # the status of a name that has a supplementary and a non-supplementary record over the locus
NO_CAP = (1 << 31) - 1          # max_reads of a fetch that select_reads caps afterwards


def rules_of(opts) -> int:
    """The `rules` bit set of an options object (any options type may be asked; 0: read selection is off)."""
    return ((RULE_SKIP_SUPPLEMENTARY if getattr(opts, "skip_supplementary", False) else 0)
            | (RULE_SKIP_SECONDARY if getattr(opts, "skip_secondary", False) else 0)
            | (RULE_UNIQUE if getattr(opts, "unique_reads", False) else 0))


def select_segments(segs: list, rules: int, max_reads: int) -> tuple[list, list[int]]:
    """The rule over the segments of one locus, in the order `fetch` yields them: (the kept segments, the status of each).
    `name` may be str or bytes."""
    status: dict = {}
    for seg in segs:                                    # 1. the status of a name: over all its records, whatever becomes of them
        status[seg.name] = status.get(seg.name, 0) | (2 if seg.flag & 0x800 else 1)
    kept, seen = [], set()
    for seg in segs:
        if rules & RULE_SKIP_SUPPLEMENTARY and seg.flag & 0x800:      # 2. flag skips
            continue
        if rules & RULE_SKIP_SECONDARY and seg.flag & 0x100:
            continue
        if rules & RULE_UNIQUE:                                       # 3. an earlier record of the name that was not flag-skipped
            if seg.name in seen:
                continue
            seen.add(seg.name)
        if len(kept) < max_reads:                                     # 4. the cap
            kept.append(seg)
    return kept, [status[seg.name] for seg in kept]


def select_constants() -> dict:
    """The size constants of the kernels as built (strk_select_constants)."""
    out = np.zeros(4, np.int32)
    _lib.load().strk_select_constants(out.ctypes.data_as(_lib._i32p))
    return dict(zip(("small_items", "small_slots", "threads", "compare_step"), out.tolist()))


def select_items(bam, rec_off: np.ndarray, item_off: np.ndarray, rules: int, max_reads: int) -> tuple[np.ndarray, np.ndarray, np.ndarray]:
    """(reason, status) per item and the number kept per locus, by the library: on the device for a DeviceBam (whole or the
    resident span of a streamed one), on the host cores for a reader that has its stream in `data`."""
    from .native import DeviceBam
    rec_off = np.ascontiguousarray(rec_off, np.int64)
    item_off = np.ascontiguousarray(item_off, np.int64)
    n_loci = int(item_off.size) - 1
    n = int(rec_off.size)
    reason, status = np.zeros(max(n, 1), np.uint8), np.zeros(max(n, 1), np.uint8)
    n_kept = np.zeros(max(n_loci, 1), np.int32)
    L = _lib.load()
    if isinstance(bam, DeviceBam):
        rc = L.strk_dbam_select_reads(bam._h, n_loci, item_off.ctypes.data, rec_off.ctypes.data, int(rules), int(max_reads),
                                      reason.ctypes.data, status.ctypes.data, n_kept.ctypes.data)
    else:
        rc = L.strk_select_reads(bam.data.ctypes.data, bam.data.size, n_loci, item_off.ctypes.data, rec_off.ctypes.data, int(rules),
                                 int(max_reads), reason.ctypes.data, status.ctypes.data, n_kept.ctypes.data)
    _lib.check(rc)
    return reason[:n], status[:n], n_kept[:n_loci]


def select_reads(bam, rec: np.ndarray, counts: np.ndarray, rules: int, max_reads: int) -> tuple[np.ndarray, np.ndarray, np.ndarray]:
    """The item list of a block (`rec`: record index per item, `counts`: items per locus, as fetch_many yields them without a
    cap) cut down to the kept items: (rec, counts, status per kept item)."""
    rec = np.asarray(rec, np.int64)
    item_off = np.concatenate(([0], np.cumsum(np.asarray(counts, np.int64)))).astype(np.int64)
    reason, status, n_kept = select_items(bam, bam.rec_off[rec], item_off, rules, max_reads)
    keep = reason == KEPT
    return rec[keep], n_kept.astype(np.int64), status[keep]
