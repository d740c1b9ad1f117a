"""Phase sets across loci for SNV calls ("Phase sets across loci"): the reference's
_determine_snv_call_phase_set (call_locus.py:291-444) with the filter in front of it (snvs.py:148-157), the demotion of a
locus that keeps no SNV (call_locus.py:680) and the fix-up at the end of a contig (call_sample.py:377-388, 424-465, 496-498),
as the reference runs them with one process.  Plain Python over a handful of integers per locus: the rule is a serial chain
over a contig's loci (every locus reads what the loci before it wrote), so there is nothing for a kernel to do in parallel.

`PhaseSets` is the state and the rule; `resolve_block` applies it to the arrays of a block's phased allele call before the
consensus, k-mer and methylation stages read them; `PhaseSets.finish_contig` is the fix-up and the renumbering over a
contig's rows."""
from __future__ import annotations

import time
from dataclasses import dataclass, field

import numpy as np

from ..alleles import CALLED
from ..phasing import ASSIGN_NONE, ASSIGN_SNV, ASSIGN_SNV_DIST, SNV_CALLED

__all__ = ["SNV_CACHE_MISMATCH", "Resolution", "PhaseSets", "resolve_block", "flip_row", "PEAK_LISTS"]

SNV_CACHE_MISMATCH = 100      # snv_status of an SNV that the filter dropped (the library's statuses are -1 .. 4)
# the per-peak lists of a row's `peaks` (call_sample.py:454-465)
PEAK_LISTS = ("means", "weights", "stdevs", "n_reads", "kmers", "seqs", "start_anchor_seqs", "am", "amc")
# what a flip swaps in the arrays of a block's allele call (per locus, the first two slots)
_AL_KEYS = ("call", "ci95", "ci99", "means", "weights", "stdevs", "peak_n_reads")


@dataclass
class Resolution:
    """What the rule says about one locus.  `kept`: per SNV handed in whether it passed the filter; `demoted`: none did, the
    locus takes the plain call; `ps`: its provisional phase set (None: demoted, or refused); `flip`: its two peaks are to be
    swapped."""
    kept: list = field(default_factory=list)
    demoted: bool = False
    ps: int | None = None
    flip: bool = False


class PhaseSets:
    """One object per run.  `counter`: the next provisional id, from 1, never reset; the renumbering of the reads' own PS tags
    (`remap`, a phase_inputs.PhaseSetRemap made with this object as its counter) draws from it too, so that HP and SNV sets
    never share a number.  Per contig `cache`: SNV id -> (base of peak 0, base of peak 1, ps) and `syn`: ps -> (ps', flip), "ps
    is ps', turned over where flip".  `next_final`: the next number the renumbering hands out."""

    def __init__(self, remap=None):
        self.counter = 1
        self.cache: dict[str, tuple[str, str, int]] = {}
        self.syn: dict[int, tuple[int, bool]] = {}
        self.contig: str | None = None
        self.last_index: int | None = None      # locus_index of the contig's last resolved locus (the order check)
        self.next_final = 1
        self.remap = remap
        self.seconds = 0.0
        self._log: list | None = None

    def take(self) -> int:
        self.counter += 1
        return self.counter - 1

    # ---- a failed block is run again locus by locus: everything it wrote is taken back --------------------------------------
    # cache and syn are not copied (a contig's cache holds every SNV cached so far; a copy per block would cost the square of a
    # contig): what is written after a snapshot is noted in a log, and restore() of the LATEST snapshot takes it back.
    def snapshot(self):
        self._log = []
        return (self._log, self.counter, self.contig, self.last_index, self.next_final,
                None if self.remap is None else self.remap.snapshot())

    def restore(self, snap) -> None:
        log, self.counter, self.contig, self.last_index, self.next_final, ids = snap
        if log is not self._log:
            raise ValueError("phase sets: only the latest snapshot can be restored")
        for table, key, old in reversed(log):
            if old is None:
                del table[key]
            else:
                table[key] = old
        del log[:]
        if self.remap is not None:
            self.remap.restore(ids)

    def _write(self, table: dict, key, value) -> None:
        if self._log is not None:
            self._log.append((table, key, table.get(key)))
        table[key] = value

    # ---- the rule ---------------------------------------------------------------------------------------------------------
    def enter(self, contig: str, locus_index: int | None = None) -> None:
        """A locus of `contig` is about to be resolved.  The loci of a contig come in catalog order and a contig is finished
        (finish_contig) before the next begins: anything else is the caller's error, not resolved in the order it came."""
        if self.contig is not None and contig != self.contig:
            raise ValueError(f"phase sets: a locus of {contig} before {self.contig} was finished (finish_contig)")
        if locus_index is not None and self.contig is not None and self.last_index is not None and locus_index <= self.last_index:
            raise ValueError(f"phase sets: locus {locus_index} of {contig} after locus {self.last_index}: the rule needs a "
                             "contig's loci in catalog order")
        self.contig = contig
        if locus_index is not None:
            self.last_index = locus_index

    def resolve(self, snvs) -> Resolution:
        """One locus.  `snvs`: its called SNVs as (id, (c0, c1)), one base per peak."""
        res = Resolution()
        # 1. filter (snvs.py:151-157): cached with another SET of bases -> not useful after all
        res.kept = [not (i in self.cache and set(self.cache[i][:2]) != set(c)) for i, c in snvs]
        left = [(i, tuple(c)) for (i, c), k in zip(snvs, res.kept) if k]
        if not left:                          # 2. demotion (call_locus.py:680)
            res.demoted = True
            return res
        # 3. hits (call_locus.py:325-328): the sets of the cached SNVs, with whether the cached pair is the call reversed
        hits = sorted({(self.cache[i][2], self.cache[i][:2] != c and self.cache[i][:2] == c[::-1]) for i, c in left if i in self.cache})
        if not hits:                          # 4. create (call_locus.py:337-354): EVERY remaining SNV is cached
            res.ps = self.take()
            for i, c in left:
                self._write(self.cache, i, (c[0], c[1], res.ps))
            return res
        # 5. join (call_locus.py:365-440).  One raw set with both orientations is refused here whether or not a synonym
        # exists (the reference's outcome there hangs on the iteration order of a set of tuples).
        raw = [p for p, _ in hits]
        if len(set(raw)) < len(raw):
            return res
        t, f = hits[0]
        while t in self.syn:
            t, r = self.syn[t]
            f ^= r
        if any(p == t for p in raw[1:]):      # (call_locus.py:391-398, the "self-flip")
            return res
        for p, pf in hits[1:]:
            self._write(self.syn, p, (t, f ^ pf))
        res.ps, res.flip = t, f               # (a joining locus does not cache its SNVs: call_locus.py:346-348 writes on creation only)
        return res

    def root(self, ps: int) -> tuple[int, bool]:
        flip = False
        while ps in self.syn:
            ps, r = self.syn[ps]
            flip ^= r
        return ps, flip

    # ---- end of a contig (call_sample.py:427-465, 496-498) ----------------------------------------------------------------------
    def finish_contig(self, rows) -> None:
        """`rows`: the contig's rows.  In locus_index order: every row's `ps` is followed to its root and the row turned over
        where the way there says so (its reads' `ps` follow: the reference leaves the old number on them); then all phase-set
        ids of the contig, HP and SNV alike, on reads and rows, are renumbered in order of first appearance (within a row its
        reads in order, then the row), on from the last contig's last number.  Then the contig's state is cleared."""
        t0 = time.perf_counter()
        rows = sorted(rows, key=lambda r: r["locus_index"])
        for row in rows:
            ps = row.get("ps")
            if ps is None or ps not in self.syn:
                continue
            new, flip = self.root(ps)
            row["ps"] = new
            for r in (row.get("reads") or {}).values():
                if r.get("ps") == ps and r.get("p") is not None:
                    r["ps"] = new
            if flip and row.get("call"):
                flip_row(row)
        final: dict[int, int] = {}
        for row in rows:
            for r in (row.get("reads") or {}).values():
                if r.get("ps", -1) > 0:
                    r["ps"] = self._final(final, r["ps"])
            if row.get("ps") is not None:
                row["ps"] = self._final(final, row["ps"])
        self.cache.clear()
        self.syn.clear()
        if self.remap is not None:
            self.remap.clear()
        self.contig = self.last_index = self._log = None
        self.seconds += time.perf_counter() - t0

    def _final(self, final: dict, ps: int) -> int:
        if ps not in final:
            final[ps] = self.next_final
            self.next_final += 1
        return final[ps]


def flip_row(row: dict) -> None:
    """Everything of a row that is per peak, turned over (call_sample.py:437-465)."""
    row["call"] = row["call"][::-1]
    for k in ("call_95_cis", "call_99_cis"):
        if row.get(k):
            row[k] = row[k][::-1]
    for r in (row.get("reads") or {}).values():
        if r.get("p") is not None and r["p"] in (0, 1):
            r["p"] = 1 - r["p"]
    for s in row.get("snvs") or []:
        s["call"], s["rcs"] = s["call"][::-1], s["rcs"][::-1]
    peaks = row.get("peaks")
    if peaks:
        for k in PEAK_LISTS:
            if peaks.get(k):
                peaks[k] = peaks[k][::-1]


def resolve_block(sets: PhaseSets, loci, al: dict, phase, snv_ids) -> np.ndarray:
    """The rule over the loci of a block, in their order, on the arrays of the block's phased allele call `al` (with read_off
    and the whole block's read_peak): filtered SNVs get snv_status SNV_CACHE_MISMATCH, a locus that is to be turned over has
    the first two entries of call, ci95, ci99, means, weights, stdevs and peak_n_reads swapped, its reads' peaks 0 <-> 1 and
    the two columns of its SNVs' snv_call / snv_rcs swapped; al["snv_ps"] [L] gets the provisional phase set (-1: none).
    `snv_ids(l, s)`: the id of SNV s (an index into snv_status) of locus l.  Returns the loci that are demoted; the caller
    gives them the plain call."""
    t0 = time.perf_counter()
    n_loci = len(loci)
    al["snv_ps"] = np.full(n_loci, -1, np.int64)
    demoted = []
    for l, locus in enumerate(loci):
        if int(al["method"][l]) not in (ASSIGN_SNV, ASSIGN_SNV_DIST) or int(al["status"][l]) != CALLED:
            continue      # (only a row with a call can carry a phase set)
        s0, s1 = int(phase.snv_off[l]), int(phase.snv_off[l + 1])
        called = [s for s in range(s0, s1) if int(al["snv_status"][s]) == SNV_CALLED]
        sets.enter(locus.contig, locus.t_idx)
        res = sets.resolve([(snv_ids(l, s), tuple(chr(int(b)) for b in al["snv_call"][s])) for s in called])
        for s, k in zip(called, res.kept):
            if not k:
                al["snv_status"][s] = SNV_CACHE_MISMATCH
        if res.demoted:
            demoted.append(l)
            continue
        if res.flip:
            for k in _AL_KEYS:
                al[k][l, :2] = al[k][l, 1::-1].copy()
            a, b = int(al["read_off"][l]), int(al["read_off"][l + 1])
            rp = al["read_peak"][a:b]
            rp[(rp == 0) | (rp == 1)] ^= 1
            al["snv_call"][s0:s1] = al["snv_call"][s0:s1, ::-1].copy()
            al["snv_rcs"][s0:s1] = al["snv_rcs"][s0:s1, ::-1].copy()
        if res.ps is not None:
            al["snv_ps"][l] = res.ps
    sets.seconds += time.perf_counter() - t0
    return np.array(demoted, np.int64)


def demote(al: dict, rest: np.ndarray, sub: dict, reads: np.ndarray) -> None:
    """The plain call `sub` of the demoted loci `rest` (their reads: `reads`, indices into the block's read_peak) put where
    their phased call was; they are then what a locus without a phased call is (method ASSIGN_NONE)."""
    for k in ("status", "modal_n", *_AL_KEYS):
        if al[k].ndim > 1 and al[k].shape[1] > sub[k].shape[1]:       # (a block with rows at the wider stride)
            al[k][rest] = np.nan if al[k].dtype.kind == "f" else -1
            al[k][rest, :sub[k].shape[1]] = sub[k]
        else:
            al[k][rest] = sub[k]
    al["read_peak"][reads] = sub["read_peak"]
    al["method"][rest] = ASSIGN_NONE
