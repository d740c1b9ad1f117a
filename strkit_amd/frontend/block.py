"""One block of loci -> its report rows (strkit/call/call_locus.py:837-1613), by two paths with one genotype tail: the readable
path through bam.py / extract.py (any `BamFile`) and the native path over the records of a NativeBam / IndexedBam / DeviceBam."""
from __future__ import annotations

import time
from dataclasses import dataclass
from typing import Callable

import numpy as np

from ..batch import count_loci, filter_reads
from ..realign import _gate as realign_gate, realign_pairs, realign_reads
from ..segment import calculate_seq_with_wildcards
from ..synth import LocusBatch
from .bam import BamFile
from .extract import LowMeanBaseQual, get_read_coords_from_cigar, get_read_coords_from_matched_pairs, get_sequence_data_for_locus
from .genotype import block_consensus, block_kmers, call_block_alleles, call_block_alleles_phased, genotype_row, kmers_row
from .loci import Locus
from .methyl import methyl, methyl_row, read_methylation, record_values
from .native import extract_raw_slices, extract_reads, realign_cigar_to_read_alignment
from .options import VCF_ANCHOR_SIZE, CallOptions
from .output import block_read_weights, read_weights
from .phase_block import native_block_phase, phase_row, python_block_phase
from .select import CHIMERIC, NO_CAP, rules_of, select_reads, select_segments


def _locus_dict(locus: Locus) -> dict:
    """STRkitLocus.to_dict() + the always-present call keys (call_locus.py:1013-1017, json_report.py:69-74)."""
    return {"locus_index": locus.t_idx, "locus_id": locus.locus_id, "contig": locus.contig, "start": locus.left_coord,
            "end": locus.right_coord, "motif": locus.motif, "annotations": [], "assign_method": None, "call": None,
            "call_95_cis": None, "call_99_cis": None}


def _locus_row(locus: Locus, rd: dict, reads: dict, opts: CallOptions) -> dict:
    row = _locus_dict(locus)
    row["ref_cn"] = int(rd["ref_cn"])
    if not opts.respect_ref:
        row["start_adj"], row["end_adj"] = rd["left_coord_adj"], rd["right_coord_adj"]
    row["ref_start_anchor"] = rd["ref_left_flank_seq"][-VCF_ANCHOR_SIZE:].upper()      # call_locus.py:1350
    row["ref_seq"] = rd["ref_seq"]                                                      # call_locus.py:1351 (case kept)
    # the record without a call (genotype.genotype_row adds one when allele calling is on and the locus has enough reads)
    row["peaks"], row["read_peaks_called"] = None, False
    row["reads"] = reads
    return row


def _count(batch: LocusBatch, opts: CallOptions, ctx, tm=None):
    if not batch.n_reads:
        return ({k: np.zeros(0, np.int32) for k in ("cn", "score", "n_iters", "start")},
                {"sc": np.zeros(0), "keep": np.zeros(0, bool), "locus_ok": np.ones(batch.n_loci, bool)})
    res = count_loci(batch, opts.rc_params, ctx=ctx, tie_rule=opts.tie_rule, end_flags=opts.end_flags, narrowing=opts.narrowing, with_stats=tm is not None)
    if tm is not None and isinstance(res, tuple):
        res, st = res
        tm["count_device_s"] = tm.get("count_device_s", 0.0) + st["kernel_ms"] / 1e3      # HIP-event time of the device work
    return res, filter_reads(batch, res, opts.min_read_align_score)


def _genotype_tail(loci, n_kept, cn, ws, slices, opts: CallOptions, ctx, tm, phase=None, sets=None):
    """The genotype tail of both block paths -> (al, cons, kmers), None for what is off: allele calls of the live `loci` over
    their kept reads (locus l owns the next n_kept[l] entries of `cn` / `ws`) and, with `consensus` or `count_kmers`, allele
    sequences and k-mer counts.  `slices()` is asked only then, and once: (tract_start, tract_len, anchor_start, anchor_len) of
    every kept read inside one buffer, and that buffer as the keywords of genotype.block_consensus (`seqs`, or `d_seqs` ...).
    `phase()` (with a switch of PhasedCallOptions on: call_blocks then hands its PhaseRun to the block paths): the block's phase_block.BlockPhase; the calls are then the phased ones,
    and the consensus and k-mer stages take their read peaks unchanged.  `sets` (snv_phase_sets): the run's phase_sets.PhaseSets;
    the SNV calls are then fitted into phase sets, peaks turned over where need be, before those stages."""
    want_kmers = opts.count_kmers != "none"
    al = cons = kmers = None
    if opts.call_alleles:
        al = (call_block_alleles_phased(loci, n_kept, cn, ws, opts, ctx, tm, phase(), sets) if phase is not None
              else call_block_alleles(loci, n_kept, cn, ws, opts, ctx, tm))
    if (opts.consensus or want_kmers) and len(cn):      # (no kept read: nothing to cut, and both stages would return nothing)
        t_start, t_len, a_start, a_len, where = slices()
        if opts.consensus:
            cons = block_consensus(al, t_start, t_len, a_start, a_len, opts, ctx, tm, **where)
        if want_kmers:
            locus_k = np.array([len(l.motif) for l in loci], np.int32)
            kmers = block_kmers(opts.count_kmers, al, t_start, t_len, np.repeat(locus_k, n_kept), locus_k, opts, ctx, tm, **where)
    return al, cons, kmers


def _call_block_python(block, bam: BamFile, opts: CallOptions, ctx, tm, ref_data, phase_run=None):
    """One block through bam.py / extract.py (the readable statement of the front end): (rows, reads kept).  `ref_data`: the
    reference side of every locus of the block (refside.get_loci_with_ref_data)."""
    flank_size = opts.flank_size
    want_raw = opts.consensus or opts.count_kmers != "none"
    use_methyl = getattr(opts, "use_methyl", False)
    rules = rules_of(opts)            # read selection (select.py); 0: the first max_reads records, as ever
    chimeric: list[set[int]] = []     # per prepared locus: id() of its kept segments that are chimeric in ITS region (the same
                                      # segment object serves every locus it overlaps: the mark is the locus's, not the segment's)
    results: list[dict] = []
    prepared = []                     # (locus, ref data, [[segment, the pairs of its new alignment or None] ...])
    realign_jobs = []                 # (locus, ref data, entry) of the soft-clipped reads
    for locus, rd in zip(block, ref_data):
        if rd is None:
            results.append(_locus_dict(locus))    # SkipLocus: locus fields + empty call (call_locus.py:1032-1036)
            continue
        segs = bam.fetch(locus.contig, locus.left_flank_coord, locus.right_flank_coord)
        if rules:
            t_a = time.perf_counter()
            segs, seg_status = select_segments(segs, rules, opts.max_reads)
            chimeric.append({id(seg) for seg, st_ in zip(segs, seg_status) if st_ == CHIMERIC})
            tm["select_s"] = tm.get("select_s", 0.0) + time.perf_counter() - t_a
        else:
            segs = segs[:opts.max_reads]
            chimeric.append(set())
        entries = [[seg, None] for seg in segs]
        if opts.realign:
            realign_jobs += [(locus, rd, e) for e in entries if e[0].soft_clip_overlaps_locus(locus)]
        prepared.append((locus, rd, entries))
    t_a = time.perf_counter()
    if realign_jobs:                  # every soft-clipped read of the block in one device call (realign.py:75-154)
        refs_ = [rd["ref_total_seq"] for _, rd, _ in realign_jobs]
        reads_ = [calculate_seq_with_wildcards(e[0].query_sequence, e[0].query_qualities, 3) for _, _, e in realign_jobs]
        lfcs = [locus.left_flank_coord for locus, _, _ in realign_jobs]
        for (_, _, e), ac in zip(realign_jobs, realign_reads(refs_, reads_, lfcs, flank_size, context=ctx)):
            if ac is not None:
                e[1] = (ac.query_coords, ac.ref_coords)
    tm["realign_s"] += time.perf_counter() - t_a
    t_a = time.perf_counter()
    # triples of every read of the block -> one batched device call
    loci_reads, meta = [], []
    raw: list[tuple[str, str]] = []      # per extracted read of the block, in batch order
    for locus, rd, entries in prepared:
        triples, names = [], []
        for seg, pairs in entries:
            if pairs is not None:     # realigned: the pairs of the new alignment
                coords = get_read_coords_from_matched_pairs(locus.left_flank_coord, rd["left_coord_adj"],
                                                            rd["right_coord_adj"], locus.right_flank_coord, *pairs)
            else:
                coords = get_read_coords_from_cigar(locus.left_flank_coord, rd["left_coord_adj"],
                                                    rd["right_coord_adj"], locus.right_flank_coord, seg)
            if coords.is_incomplete():
                continue
            try:
                sd = get_sequence_data_for_locus(seg, coords, flank_size, opts.min_avg_phred)
            except LowMeanBaseQual:
                continue
            triples.append((sd.flank_left_seq_wc[-flank_size:], sd.tr_seq_wc, sd.flank_right_seq_wc[:flank_size]))
            names.append((seg.name, seg.strand, pairs is not None, len(sd.tr_seq), seg, coords))
            if want_raw:   # the raw tract and the raw read bases in front of it (no wildcards), call_locus.py:1296-1299
                raw.append((sd.tr_seq, seg.query_sequence[max(coords.left_flank_start, coords.left_flank_end - VCF_ANCHOR_SIZE):
                                                          coords.left_flank_end]))
        loci_reads.append((locus.motif, triples))
        meta.append(names)
    if not prepared:
        return results, 0
    batch = LocusBatch.from_reads(loci_reads)
    tm["extract_s"] += time.perf_counter() - t_a
    t_a = time.perf_counter()
    res, flt = _count(batch, opts, ctx)
    tm["count_s"] += time.perf_counter() - t_a
    recs_of, pairs, kept_of = [], [], []
    seg_of = [{e[0].name: e for e in entries} for _, _, entries in prepared] if phase_run is not None else None
    for li, (locus, rd, _) in enumerate(prepared):
        r0, r1 = int(batch.read_off[li]), int(batch.read_off[li + 1])
        kept = [r for r in range(r0, r1) if flt["keep"][r]]
        reads, raws = {}, {}             # (a read name that occurs twice keeps one record, as the reference's read_dict)
        # read weights (call_locus.py:1254-1259): from the lengths of ALL segments fetched for the locus
        lens_sorted = np.sort(np.array([e[0].length for e in prepared[li][2]], np.int64))
        tlwf = (batch.nfl[r0:r1] + batch.ntr[r0:r1] + batch.nfr[r0:r1]).astype(np.int64)
        ws = read_weights(lens_sorted, tlwf)
        for r in kept:
            name, strand, realigned, sl, seg, rc = meta[li][r - r0]
            sc = float(flt["sc"][r])
            reads[name] = {"s": strand, "cn": int(res["cn"][r]), "w": float(ws[r - r0]),
                           "sc": None if np.isnan(sc) else sc, "sl": sl, **({"realn": True} if realigned else {}),
                           **({"chimeric_in_region": True} if id(seg) in chimeric[li] else {})}
            if use_methyl:     # the rule itself (methyl.py) on the tract extraction cut
                a, b, c, d = rc.left_flank_start, rc.left_flank_end, rc.right_flank_start, rc.right_flank_end
                q = (b, c) if 0 <= a <= b <= c <= d and c <= seg.length else (None, None)
                st_m, _, known, mc = read_methylation(seg.query_sequence, seg.flag, seg.cigar, seg.tags, *q, opts.methyl_threshold)
                reads[name]["m"], reads[name]["mc"] = record_values(st_m, known, mc)
            if want_raw:
                raws[name] = raw[r]
        if not flt["locus_ok"][li]:
            reads, raws = {}, {}
        results.append(_locus_row(locus, rd, reads, opts))
        recs_of.append(list(reads.values()))     # calls and k-mer counts are made from the records of the row
        if seg_of is not None:
            kept_of.append([(seg_of[li][name][0], bool(r.get("realn")), r["cn"]) for name, r in reads.items()])
        pairs.extend(raws.values())

    def slices():      # (raw anchor | raw tract) of every record, in row order, in one host buffer, as the native path has them
        t_len = np.array([len(tr_raw) for tr_raw, _ in pairs], np.int64)
        a_len = np.array([len(anchor) for _, anchor in pairs], np.int64)
        a_start = np.concatenate(([0], np.cumsum(a_len + t_len)[:-1]))
        text = "".join(anchor + tr_raw for tr_raw, anchor in pairs)
        return a_start + a_len, t_len, a_start, a_len, {"seqs": np.frombuffer(text.encode("ascii"), np.uint8)}

    al, cons, km = _genotype_tail([p[0] for p in prepared], np.array([len(x) for x in recs_of], np.int64),
                                  np.array([r["cn"] for x in recs_of for r in x], np.int32),
                                  np.array([r["w"] for x in recs_of for r in x], np.float64), slices, opts, ctx, tm,
                                  phase=(lambda: python_block_phase(phase_run, opts, [p[0] for p in prepared],
                                                                    [[(e[0], e[1] is not None) for e in p[2]] for p in prepared], kept_of, tm))
                                  if phase_run is not None else None, sets=getattr(phase_run, "sets", None))
    first = 0
    for li, row in enumerate(results[-len(prepared):]):
        if al is not None:
            genotype_row(row, al, li, recs_of[li], cons)
            if "phase" in al:
                phase_row(row, al, li, recs_of[li], prepared[li][0])
            if use_methyl:
                methyl_row(row, recs_of[li])
        if km is not None:
            kmers_row(row, km, li, recs_of[li], first)
        first += len(recs_of[li])
    return results, sum(len(x) for x in recs_of)


@dataclass
class BlockState:
    # What the device stage of the native path leaves for the report stage.  Item = a fetched record at a locus; read = an
    # item whose extraction succeeded; kept = a read that passed the filters.
    live: list                    # (locus, reference data) of the loci that are called
    rec: np.ndarray               # record index per item
    ok_items: np.ndarray          # item per read
    read_locus: np.ndarray
    kept: np.ndarray              # read per kept read
    names: list
    minus: np.ndarray
    cn: np.ndarray                # per read, as sc / ntr
    sc: np.ndarray
    ntr: np.ndarray
    alt: dict | None              # substitute alignments of realigned items
    weigh: Callable[[], np.ndarray]     # -> the weights of the kept reads
    ws: np.ndarray | None = None  # ... where they were needed ahead of the report (allele calls)
    al: dict | None = None
    cons: dict | None = None
    kmers: dict | None = None
    methyl: dict | None = None    # status / known / mc per kept read (use_methyl)
    chimeric: np.ndarray | None = None     # per kept read: chimeric in the region (read selection on)


def _call_block_native(block, bam, opts: CallOptions, ctx, tm, ref_data, phase_run=None):
    """One block over the records of a NativeBam / an IndexedBam region / a DeviceBam, with no Python per read before the report:
    one vectorised interval query (`fetch_many`), ONE extraction call, one device call that counts, numpy filters
    (_block_device_stage); only the rows of the report are built read by read (_block_report_stage): (rows, reads kept)."""
    results = [_locus_dict(locus) for locus, rd in zip(block, ref_data) if rd is None]
    live = [(locus, rd) for locus, rd in zip(block, ref_data) if rd is not None]
    if not live:
        return results, 0
    rows, n_kept = _block_report_stage(_block_device_stage(live, bam, opts, ctx, tm, phase_run), opts, tm)
    return results + rows, n_kept


def _block_device_stage(live, bam, opts: CallOptions, ctx, tm, phase_run=None) -> BlockState:
    """Everything of a block's live loci that touches the reader and the device: interval query, extraction, counting, filters,
    the names of the reads that are kept, and the genotype tail."""
    flank_size = opts.flank_size
    t_a = time.perf_counter()
    lfc = np.array([l.left_flank_coord for l, _ in live], np.int64)
    rfc = np.array([l.right_flank_coord for l, _ in live], np.int64)
    lca = np.array([rd["left_coord_adj"] for _, rd in live], np.int64)
    rca = np.array([rd["right_coord_adj"] for _, rd in live], np.int64)
    rules = rules_of(opts)                   # read selection (select.py): the fetch is then made without a cap
    fetch_cap = NO_CAP if rules else opts.max_reads
    if len({l.contig for l, _ in live}) == 1:
        rec, counts = bam.fetch_many(live[0][0].contig, lfc, rfc, fetch_cap)
    else:                                    # a hand-made block that mixes contigs
        parts = [bam.fetch_indices(l.contig, int(a), int(b))[:fetch_cap] for (l, _), a, b in zip(live, lfc, rfc)]
        rec = np.concatenate(parts) if parts else np.zeros(0, np.int64)
        counts = np.array([len(x) for x in parts], np.int64)
    item_status = None
    if rules:                                # from here on nothing sees a record that is left out
        t_s = time.perf_counter()
        rec, counts, item_status = select_reads(bam, rec, counts, rules, opts.max_reads)
        tm["select_s"] = tm.get("select_s", 0.0) + time.perf_counter() - t_s
        t_a += time.perf_counter() - t_s     # (not extract_s's)
    item_locus = np.repeat(np.arange(len(live)), counts)
    coords = np.stack((lfc, lca, rca, rfc), axis=1)[item_locus]
    tm["extract_s"] += time.perf_counter() - t_a
    alt = None
    if opts.realign and rec.size:     # soft-clipped reads of the whole block in one device call (realign.py:75-154)
        t_a = time.perf_counter()
        lf, rf = lfc[item_locus], rfc[item_locus]
        left = (bam.clip_l[rec] > 0) & (bam.pos[rec] >= lf) & (bam.pos[rec] <= rf)
        right = (bam.clip_r[rec] > 0) & (bam.end[rec] >= lf) & (bam.end[rec] <= rf)
        cand = np.nonzero(left | right)[0]
        if cand.size:
            refs_, reads_ = [], []
            for it in cand:
                seg = bam.segment(int(rec[it]))
                refs_.append(live[int(item_locus[it])][1]["ref_total_seq"])
                reads_.append(calculate_seq_with_wildcards(seg.query_sequence, seg.query_qualities, 3))
            gate = realign_gate(flank_size)
            alt = {}
            for it, (sc, _e, cg) in zip(cand, realign_pairs(refs_, reads_, context=ctx)):
                if sc >= gate:
                    alt[int(it)] = (realign_cigar_to_read_alignment(cg), int(lf[it]))
        tm["realign_s"] += time.perf_counter() - t_a
    t_a = time.perf_counter()
    ex = extract_reads(bam, rec, coords, flank_size, opts.min_avg_phred, 3, alt)
    ok = ex["status"] == 0
    motifs = [l.motif.encode() for l, _ in live]
    mlen = np.array([len(m) for m in motifs], np.int64)
    ntr_ok = ex["ntr"][ok]
    batch = LocusBatch(
        seqs=ex["seqs"], seq_off=np.concatenate(([0], ex["seq_off"][1:][ok])).astype(np.int64),
        nfl=ex["nfl"][ok], ntr=ntr_ok, nfr=ex["nfr"][ok],
        est_cn=np.rint(ntr_ok / mlen[item_locus[ok]]).astype(np.int32),      # round(len(tr) / motif_size), half to even
        read_off=np.concatenate(([0], np.cumsum(np.bincount(item_locus[ok], minlength=len(live))))).astype(np.int32),
        motifs=np.frombuffer(b"".join(motifs), np.uint8).copy(),
        motif_off=np.concatenate(([0], np.cumsum(mlen))).astype(np.int32))
    if "d_seqs" in ex:
        batch.d_seqs = ex["d_seqs"]          # extracted on the device: counted where they are
    tm["extract_s"] += time.perf_counter() - t_a
    t_a = time.perf_counter()
    res, flt = _count(batch, opts, ctx, tm)
    tm["count_s"] += time.perf_counter() - t_a
    t_a = time.perf_counter()
    ok_items, read_locus = np.nonzero(ok)[0], item_locus[ok]
    kept = np.nonzero(flt["keep"] & flt["locus_ok"][read_locus])[0]
    kept_rec = rec[ok_items[kept]]
    lens_all = bam.l_seq[rec].astype(np.int64)
    st = BlockState(live=live, rec=rec, ok_items=ok_items, read_locus=read_locus, kept=kept, names=bam.names(kept_rec),
                    minus=(bam.flag[kept_rec] & 16) != 0, cn=res["cn"], sc=flt["sc"], ntr=batch.ntr, alt=alt,
                    weigh=lambda: block_read_weights(counts, item_locus, lens_all, read_locus[kept],
                                                     batch.nfl[kept].astype(np.int64) + batch.ntr[kept] + batch.nfr[kept]))
    if item_status is not None:
        st.chimeric = item_status[ok_items[kept]] == CHIMERIC
    tm["names_s"] = tm.get("names_s", 0.0) + time.perf_counter() - t_a
    if getattr(opts, "use_methyl", False):     # one library call over the kept items: the records are read where they lie
        t_a = time.perf_counter()
        items = ok_items[kept]
        st.methyl = methyl(bam, rec[items], coords[items], {k: alt[it] for k, it in enumerate(items.tolist()) if it in alt} if alt else None,
                           opts.methyl_threshold)
        tm["methyl_s"] = tm.get("methyl_s", 0.0) + time.perf_counter() - t_a
    if opts.call_alleles or opts.count_kmers != "none":
        if opts.call_alleles:
            st.ws = st.weigh()
        # the raw tract and start anchor of every kept read: a second extraction, made only when the tail asks for it
        st.al, st.cons, st.kmers = _genotype_tail(
            [l for l, _ in live], np.bincount(read_locus[kept], minlength=len(live)), st.cn[kept], st.ws,
            lambda: extract_raw_slices(st, bam, coords, VCF_ANCHOR_SIZE, opts.min_avg_phred, tm), opts, ctx, tm,
            phase=(lambda: native_block_phase(phase_run, opts, [l for l, _ in live], bam, rec, item_locus.astype(np.int32), alt,
                                              ok_items[kept], read_locus[kept], st.cn[kept], tm)) if phase_run is not None else None,
            sets=getattr(phase_run, "sets", None))
    return st


def _block_report_stage(st: BlockState, opts: CallOptions, tm):
    """Report rows of a block (call_locus.py:1279-1288,1340-1352) from what _block_device_stage left: Python and numpy only."""
    t_a = time.perf_counter()
    results, live = [], st.live
    kept, names, alt, al, cons, km = st.kept, st.names, st.alt, st.al, st.cons, st.kmers     # (locals: no attribute look-up per row)
    strands = np.where(st.minus, "-", "+").tolist()
    cns = st.cn[kept].tolist()
    scs = [None if x != x else x for x in st.sc[kept].tolist()]
    sls = st.ntr[kept].tolist()
    ws = (st.ws if st.ws is not None else st.weigh()).tolist()
    first = np.concatenate(([0], np.cumsum(np.bincount(st.read_locus[kept], minlength=len(live))))).tolist()
    # the read records of the whole block in one comprehension (values as locals: no indexing), then a dict per locus
    recs = [{"s": s_, "cn": c_, "w": w_, "sc": q_, "sl": l_} for s_, c_, w_, q_, l_ in zip(strands, cns, ws, scs, sls)]
    if alt:
        for k, it in enumerate(st.ok_items[kept].tolist()):
            if it in alt:
                recs[k]["realn"] = True
    if st.chimeric is not None:
        for k in np.nonzero(st.chimeric)[0].tolist():
            recs[k]["chimeric_in_region"] = True
    if st.methyl is not None:
        for r, s_, k_, m_ in zip(recs, st.methyl["status"].tolist(), st.methyl["known"].tolist(), st.methyl["mc"].tolist()):
            r["m"], r["mc"] = record_values(s_, k_, m_)
    for li, (locus, rd) in enumerate(live):
        a, b = first[li], first[li + 1]
        row = _locus_row(locus, rd, dict(zip(names[a:b], recs[a:b])), opts)
        if al is not None:
            genotype_row(row, al, li, recs[a:b], cons)
            if "phase" in al:
                phase_row(row, al, li, recs[a:b], locus)
            if st.methyl is not None:
                methyl_row(row, recs[a:b])
        if km is not None:
            kmers_row(row, km, li, recs[a:b], a)
        results.append(row)
    tm["report_s"] = tm.get("report_s", 0.0) + time.perf_counter() - t_a
    return results, int(len(kept))
