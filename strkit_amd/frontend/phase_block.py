"""Phasing inside a block of loci: what the two block paths hand to the phased allele call and what comes
back into the rows.  The native path reads tags and SNV cells through the library (phase_inputs.phase_cells /
library_useful_snvs: kernels for a DeviceBam, their host twins otherwise); the readable path runs the rule of
phase_inputs.py on AlignedSegment.tags / .cigar.  Both end in the same BlockPhase."""
from __future__ import annotations

import time
from dataclasses import dataclass, field

import numpy as np

from ..alleles import AlleleParams
from ..phasing import ASSIGN_HP, ASSIGN_NAMES, ASSIGN_NONE, ASSIGN_SNV, ASSIGN_SNV_DIST, SNV_CALLED
from . import phase_inputs as pi
from .genotype import n_alleles_of
from .options import allele_counts
from .phase_sets import PhaseSets
from .snv_discovery import DiscoveredSnvs, discover_candidates, library_discover_snvs
from .snv_vcf import IndexedSnvVcf, open_snv_candidates

MAX_CELLS = (512 << 20) // 2      # cells (a base and a quality byte each) of one phase_cells call: DESIGN.md §9's 512 MB

__all__ = ["PhaseRun", "BlockPhase", "native_block_phase", "python_block_phase", "phase_row"]


class PhaseRun:
    """What one run keeps across its blocks: the candidate SNVs (a file with a tabix index: opened, then asked block by block,
    on the device when `device` is given, as the alignment file's reader is; any other file: read once), the renumbering of the
    phase sets and, with snv_phase_sets, the phase sets of the SNV calls (`sets`, a phase_sets.PhaseSets; the renumbering then
    counts with it).  With discover_snvs there is no file: `discover` is set, the block paths ask the discovery
    (frontend/snv_discovery.py) for every block's candidates, and `ref` (the run's Fasta) gives their reference bases."""

    def __init__(self, opts, device: int | None = None, ref=None):
        t0 = time.perf_counter()
        self.discover = bool(getattr(opts, "discover_snvs", False))
        self.ref = ref
        self.snvs = (open_snv_candidates(opts.snv_vcf, "host" if device is None else "device", device or 0) if opts.snv_vcf else None)
        self.open_s = time.perf_counter() - t0
        self.sets = PhaseSets() if getattr(opts, "snv_phase_sets", False) else None
        self.remap = pi.PhaseSetRemap(self.sets)
        if self.sets is not None:
            self.sets.remap = self.remap

    @property
    def has_snvs(self) -> bool:
        """Whether the run groups reads by SNVs: it has a candidate file, or discovers its candidates."""
        return self.snvs is not None or self.discover

    def close(self, tm: dict | None = None) -> None:
        """Gives the indexed reader's device object back; its stage times (only it has any) go into `tm`."""
        if isinstance(self.snvs, IndexedSnvVcf):
            if tm is not None:
                tm["snv_candidates_s"] = self.open_s + self.snvs.seconds
                tm["snv_vcf_compressed_mb"] = round(self.snvs.compressed_bytes / 1e6, 4)
                if self.snvs.front_end == "device":
                    tm["snv_vcf_device_s"] = self.snvs.kernel_s()
            self.snvs.close()

    def snapshot(self):
        """What a block may change; restore() puts it back (a block that failed is run again locus by locus)."""
        return self.remap.snapshot() if self.sets is None else self.sets.snapshot()

    def restore(self, snap) -> None:
        if self.sets is None:
            self.remap.restore(snap)
        else:
            self.sets.restore(snap)


@dataclass
class BlockPhase:
    """Per kept read of the block hp / ps (ps renumbered; None without use_hp); per locus the useful SNVs (snv_off) with, per
    useful SNV, its index among the contig's candidate records (snv_rec), and the packed cells of the kept reads."""
    hp: np.ndarray | None
    ps: np.ndarray | None
    snv_off: np.ndarray | None = None
    snv_rec: np.ndarray | None = None
    snv_base: np.ndarray | None = None
    snv_qual: np.ndarray | None = None
    contigs: list = field(default_factory=list)       # per locus its ContigSnvs (or None)

    def without(self, bad_locus: np.ndarray, n_kept: np.ndarray) -> "BlockPhase":
        """The same with the reads and cells of the loci in `bad_locus` taken out (they are not called); snv_off keeps its length."""
        if not bad_locus.any():
            return self
        sel = ~np.repeat(bad_locus, n_kept)
        out = BlockPhase(None if self.hp is None else self.hp[sel], None if self.ps is None else self.ps[sel], contigs=self.contigs)
        if self.snv_off is not None:
            s = np.diff(self.snv_off)
            cell_sel = ~np.repeat(bad_locus, n_kept * s)
            out.snv_off, out.snv_rec = self.snv_off, self.snv_rec
            out.snv_base, out.snv_qual = self.snv_base[cell_sel], self.snv_qual[cell_sel]
        return out


def _candidates(run: PhaseRun, loci, spans):
    """Per locus the indices of its candidates among its contig's records -> (contig records per locus, index arrays, cand_off, cand_pos)."""
    contigs, idx = [], []
    # one query per contig of the block, over [min lo, max hi) of its loci with reads (the reference's per-block query,
    # call_sample.py:124); a file read whole answers with the whole contig
    of_contig: dict = {}
    if run.snvs is not None:
        for name in dict.fromkeys(locus.contig for locus in loci):
            with_reads = [(lo, hi) for locus, (lo, hi) in zip(loci, spans) if locus.contig == name and hi > lo]
            of_contig[name] = (run.snvs.window(name, min(lo for lo, _ in with_reads), max(hi for _, hi in with_reads))
                               if with_reads else None)
    for locus, (lo, hi) in zip(loci, spans):
        c = of_contig.get(locus.contig)
        contigs.append(c)
        idx.append(pi.locus_candidates(c.pos, lo, hi, locus.left_flank_coord, locus.right_flank_coord)
                   if c is not None and hi > lo else np.zeros(0, np.int64))
    cand_off = np.concatenate(([0], np.cumsum([len(i) for i in idx]))).astype(np.int32)
    cand_pos = np.concatenate([c.pos[i] for c, i in zip(contigs, idx) if c is not None] + [np.zeros(0, np.int64)]).astype(np.int64)
    return contigs, idx, cand_off, cand_pos


def _gates(loci, opts, kept_locus, realigned, cn) -> np.ndarray:
    """Per locus whether the SNV step is allowed (phase_inputs.snv_step_allowed)."""
    ok = np.zeros(len(loci), bool)
    counts = allele_counts(opts)
    for l, locus in enumerate(loci):
        m = kept_locus == l
        re_, cns = realigned[m], cn[m]
        rare = any(not (cns[~re_] == c).any() for c in cns[re_])
        ok[l] = pi.snv_step_allowed(n_alleles_of(counts, locus.contig), int(re_.sum()), rare)
    return ok


def _discovered(run: PhaseRun, loci, cand_off, cand_pos):
    """The discovered positions of a block in the shape _candidates gives a file's: per locus an object of ContigSnvs' shape that
    holds that locus's positions alone, and the indices of all of them."""
    contigs = [DiscoveredSnvs(locus.contig, cand_pos[cand_off[l]:cand_off[l + 1]], run.ref) for l, locus in enumerate(loci)]
    idx = [np.arange(c.pos.size, dtype=np.int64) for c in contigs]
    return contigs, idx, np.ascontiguousarray(cand_off, np.int32), np.ascontiguousarray(cand_pos, np.int64)


def native_block_phase(run: PhaseRun, opts, loci, bam, rec, item_locus, alt, kept_item, kept_locus, cn_kept, tm) -> BlockPhase:
    """The native path: `rec` / `item_locus` = record and locus of every item, `alt` the substitute alignments, kept_item /
    kept_locus / cn_kept = item, locus and copy number of every kept read (in read order)."""
    t_a = time.perf_counter()
    n_loci = len(loci)
    spans = []
    first = np.concatenate(([0], np.cumsum(np.bincount(item_locus, minlength=n_loci))))
    for l in range(n_loci):
        r = rec[first[l]:first[l + 1]]
        spans.append((int(bam.pos[r].min()), int(bam.end[r].max())) if r.size else (0, 0))
    mar = (opts.allele_params or AlleleParams()).min_allele_reads
    realigned = np.array([int(i) in alt for i in kept_item], bool) if alt else np.zeros(len(kept_item), bool)
    allowed = (_gates(loci, opts, kept_locus, realigned, cn_kept)[kept_locus] if len(kept_item) and run.has_snvs
               else np.zeros(len(kept_item), bool))
    if run.discover:
        # the candidates come from the kept reads of the loci whose gate is open (a closed one gets no kept read, so no candidate)
        t_b, k_b = time.perf_counter(), bam.kernel_s() if hasattr(bam, "kernel_s") else None
        found = library_discover_snvs(bam, rec, item_locus, [l.left_flank_coord for l in loci], [l.right_flank_coord for l in loci],
                                      np.concatenate(([0], np.cumsum(np.bincount(kept_locus[allowed], minlength=n_loci)))), kept_item[allowed],
                                      alt=alt or None, window=opts.snv_discover_window, min_base_qual=opts.snv_min_base_qual, min_allele_reads=mar,
                                      clip_threshold=opts.significant_clip_threshold)
        contigs, idx, cand_off, cand_pos = _discovered(run, loci, *found)
        tm["snv_discover_s"] = tm.get("snv_discover_s", 0.0) + time.perf_counter() - t_b
        if k_b is not None:
            tm["snv_discover_device_s"] = tm.get("snv_discover_device_s", 0.0) + bam.kernel_s() - k_b
    else:
        contigs, idx, cand_off, cand_pos = _candidates(run, loci, spans)
    bp = BlockPhase(None, None, contigs=contigs)
    # The cells of one call stay within MAX_CELLS: the loci are cut into pieces (a locus is never cut; one locus alone has at most
    # max_reads x 1 024 cells) and every piece makes its own pair of calls.  The result does not depend on the cut.
    per_locus = np.bincount(item_locus, minlength=n_loci).astype(np.int64) * np.diff(cand_off)
    pieces, l0, acc = [], 0, 0
    for l in range(n_loci):
        if l > l0 and acc + per_locus[l] > MAX_CELLS:
            pieces.append((l0, l))
            l0, acc = l, 0
        acc += per_locus[l]
    pieces.append((l0, n_loci))
    hp, ps = np.full(len(kept_item), -1, np.int32), np.full(len(kept_item), -1, np.int32)
    parts = []
    for l0, l1 in pieces:
        i0, i1 = int(first[l0]), int(first[l1])
        t_b = time.perf_counter()
        cells = pi.phase_cells(bam, rec[i0:i1], item_locus[i0:i1] - l0, cand_off[l0:l1 + 1] - cand_off[l0], cand_pos[cand_off[l0]:cand_off[l1]],
                               alt={k - i0: v for k, v in alt.items() if i0 <= k < i1} if alt else None,
                               clip_threshold=opts.significant_clip_threshold)
        tm["phase_cells_s"] = tm.get("phase_cells_s", 0.0) + time.perf_counter() - t_b
        mine = (kept_locus >= l0) & (kept_locus < l1)
        hp[mine], ps[mine] = cells["hp"][kept_item[mine] - i0], cells["ps"][kept_item[mine] - i0]
        if run.has_snvs:
            t_b = time.perf_counter()
            use = mine & allowed
            kept_off = np.concatenate(([0], np.cumsum(np.bincount(kept_locus[use] - l0, minlength=l1 - l0)))).astype(np.int32)
            parts.append(pi.library_useful_snvs(cells, kept_off, kept_item[use] - i0, mar))
            tm["useful_snvs_s"] = tm.get("useful_snvs_s", 0.0) + time.perf_counter() - t_b
    if opts.use_hp:
        bp.hp, bp.ps = hp, run.remap(ps, hp)
    if run.has_snvs:
        bp.snv_off = np.concatenate(([0], np.cumsum(np.concatenate([np.diff(u["snv_off"]) for u in parts])))).astype(np.int32)
        bp.snv_base, bp.snv_qual = (np.concatenate([u[k] for u in parts]) for k in ("snv_base", "snv_qual"))
        snv_cand = np.concatenate([u["snv_cand"] for u in parts])
        owner = np.repeat(np.arange(n_loci), np.diff(bp.snv_off))
        bp.snv_rec = np.array([idx[l][c] for l, c in zip(owner, snv_cand)], np.int64)
    tm["phase_inputs_s"] = tm.get("phase_inputs_s", 0.0) + time.perf_counter() - t_a
    return bp


def python_block_phase(run: PhaseRun, opts, loci, entries_of, kept_of, tm) -> BlockPhase:
    """The readable path.  entries_of[l] = the (segment, realigned) pairs fetched for locus l; kept_of[l] = per kept read of
    the locus (segment, realigned, copy number), in read order."""
    t_a = time.perf_counter()
    spans = [((min(s.start for s, _ in e), max(s.end for s, _ in e)) if e else (0, 0)) for e in entries_of]
    mar = (opts.allele_params or AlleleParams()).min_allele_reads
    if run.discover:
        t_b = time.perf_counter()
        found = []
        for locus, entries, kept in zip(loci, entries_of, kept_of):
            ok = bool(kept) and _gates([locus], opts, np.zeros(len(kept), np.int64), np.array([k[1] for k in kept], bool),
                                       np.array([k[2] for k in kept], np.int64))[0]
            found.append(discover_candidates(entries, kept, locus.left_flank_coord, locus.right_flank_coord, opts.snv_discover_window,
                                             opts.snv_min_base_qual, mar, opts.significant_clip_threshold, allowed=ok))
        contigs, idx, cand_off, cand_pos = _discovered(run, loci, np.concatenate(([0], np.cumsum([f.size for f in found]))),
                                                       np.concatenate(found + [np.zeros(0, np.int64)]))
        tm["snv_discover_s"] = tm.get("snv_discover_s", 0.0) + time.perf_counter() - t_b
    else:
        contigs, idx, cand_off, cand_pos = _candidates(run, loci, spans)
    hp, ps, bases, quals, sels = [], [], [], [], []
    for l, (locus, kept) in enumerate(zip(loci, kept_of)):
        cand = cand_pos[cand_off[l]:cand_off[l + 1]]
        for seg, _re, _cn in kept:
            h, p = pi.read_tags(seg.tags)
            hp.append(h)
            ps.append(p)
        if not run.has_snvs:
            continue
        cells = [pi.alignment_cells(np.zeros(0, np.uint32), 0, "", None, cand) if re_ else
                 pi.segment_cells(seg, cand, clip_threshold=opts.significant_clip_threshold) for seg, re_, _cn in kept]
        b = np.array([c[0] for c in cells], np.uint8).reshape(len(kept), len(cand))
        q = np.array([c[1] for c in cells], np.uint8).reshape(len(kept), len(cand))
        re_ = np.array([k[1] for k in kept], bool)
        cns = np.array([k[2] for k in kept], np.int64)
        ok = _gates([locus], opts, np.zeros(len(kept), np.int64), re_, cns)[0]
        bases.append(b)
        quals.append(q)
        sels.append(pi.useful_snvs(b, mar) if ok and len(kept) else np.zeros(0, np.int32))
    bp = BlockPhase(None, None, contigs=contigs)
    if opts.use_hp:
        bp.hp = np.array(hp, np.int32)
        bp.ps = run.remap(np.array(ps, np.int32), bp.hp)
    if run.has_snvs:
        bp.snv_off, bp.snv_base, bp.snv_qual = pi.pack_cells(bases, quals, sels)
        bp.snv_rec = np.concatenate([idx[l][s] for l, s in enumerate(sels)] + [np.zeros(0, np.int64)]).astype(np.int64)
    tm["phase_inputs_s"] = tm.get("phase_inputs_s", 0.0) + time.perf_counter() - t_a
    return bp


def phase_row(row: dict, al: dict, li: int, recs: list[dict], locus) -> None:
    """After genotype.genotype_row: the fields of a phased call on the row of locus `li` and on its read records.  Per tagged
    read `hp` / `ps`; for an `hp` call assign_method and the locus `ps`; for an SNV call assign_method, `snvs` (the called SNVs)
    and per read `snvu`, its bases at them and, with snv_phase_sets, `ps` on the row and on its reads with a peak."""
    bp: BlockPhase = al["phase"]
    a = int(al["read_off"][li])
    if bp.hp is not None:
        for k, r in enumerate(recs):
            if bp.hp[a + k] != -1 or bp.ps[a + k] != -1:
                r["hp"], r["ps"] = int(bp.hp[a + k]), int(bp.ps[a + k])
    method = int(al["method"][li])
    if not row.get("call") or method == ASSIGN_NONE:
        return
    row["assign_method"] = ASSIGN_NAMES[method]
    if method == ASSIGN_HP:
        row["ps"] = int(al["ps"][li])
    if method in (ASSIGN_SNV, ASSIGN_SNV_DIST):
        s0, s1 = int(bp.snv_off[li]), int(bp.snv_off[li + 1])
        called = [s for s in range(s0, s1) if int(al["snv_status"][s]) == SNV_CALLED]
        c = bp.contigs[li]
        snvs = []
        for s in called:
            k = int(bp.snv_rec[s])
            snvs.append({"id": snv_id(bp, li, s, locus.contig), "ref": c.ref[k], "pos": int(c.pos[k]),
                         "call": [chr(int(b)) for b in al["snv_call"][s]], "rcs": [int(x) for x in al["snv_rcs"][s]]})
        row["snvs"] = snvs
        n_s = s1 - s0
        cell0 = int(al["cell_off"][li])
        for k, r in enumerate(recs):
            r["snvu"] = [chr(int(al["snv_base"][cell0 + k * n_s + (s - s0)])) for s in called]
        # snv_phase_sets (phase_sets.resolve_block): the locus's phase set on the row and on every read with a peak, in the
        # place of the one its tag gave it (call_locus.py:423-438)
        if "snv_ps" in al and int(al["snv_ps"][li]) != -1:
            row["ps"] = int(al["snv_ps"][li])
            for r in recs:
                if r.get("p") is not None and r["p"] >= 0:
                    r["ps"] = row["ps"]


def snv_id(bp: BlockPhase, li: int, s: int, contig: str) -> str:
    """The id of useful SNV `s` of locus `li` of the block: its record's, else contig_position (snvs.py:148)."""
    c, k = bp.contigs[li], int(bp.snv_rec[s])
    return c.ids[k] or f"{contig}_{int(c.pos[k]) + 1}"
