"""Genotypes of a block of loci: allele calls (strkit_amd.alleles) and allele sequences (strkit_amd.consensus) over the kept
reads of all live loci, one library call each per block, and the row fields they become (call_locus.py:1490-1640,
json_report.py:90).  Shared by the native block path and the readable one; opt-in (CallOptions.call_alleles / consensus).
"""
from __future__ import annotations

import math
import time

import numpy as np

from ..alleles import CALLED, MAX_ALLELES, TOO_FEW, AlleleParams, call_alleles_batch, call_alleles_n_batch, call_data_from_batch, locus_seeds
from ..consensus import METHOD_NAMES, best_representatives_packed, consensus_packed
from ..kmers import count_kmers_packed, dicts_of
from .options import allele_counts

__all__ = ["n_alleles_of", "call_block_alleles", "call_block_alleles_phased", "peak_groups", "block_consensus", "genotype_row", "block_kmers", "kmers_row"]


def n_alleles_of(n_alleles, contig: str) -> int:
    """`n_alleles`: one number for every contig, a dict per contig (2 where a contig is not named), or a ploidy configuration
    (options.allele_counts; 0 for a contig that it leaves out)."""
    if hasattr(n_alleles, "n_of"):
        return int(n_alleles.n_of(contig) or 0)
    if isinstance(n_alleles, dict):
        return int(n_alleles.get(contig, n_alleles.get(contig[3:] if contig.startswith("chr") else "chr" + contig, 2)))
    return int(n_alleles)


def call_block_alleles(loci, n_kept: np.ndarray, cns: np.ndarray, ws: np.ndarray, opts, ctx, tm) -> dict:
    """Allele calls of all loci of a block.  `loci`: the live loci; locus l owns the next n_kept[l] entries of cns / ws
    (the kept reads, in read order).  The weights are divided by their per-locus sum (call_locus.py:190-192); a locus with
    a weight that is not a positive finite number (no fetched read is long enough, output.read_weights) is not called.
    Returns call_alleles_batch's arrays plus `n_alleles` [L] and `read_off` [L + 1]; read_peak covers every kept read."""
    t_a = time.perf_counter()
    n_loci = len(loci)
    n_kept = np.asarray(n_kept, np.int64)
    owner = np.repeat(np.arange(n_loci), n_kept)
    w = np.asarray(ws, np.float64)
    good = np.isfinite(w) & (w > 0)
    bad_locus = np.bincount(owner[~good], minlength=n_loci) > 0
    sel = ~bad_locus[owner]
    sums = np.bincount(owner[sel], weights=w[sel], minlength=n_loci)
    n_sel = np.where(bad_locus, 0, n_kept)
    counts = allele_counts(opts)
    nal = np.array([n_alleles_of(counts, l.contig) for l in loci], np.int32)
    seeds = locus_seeds(opts.seed, np.array([l.t_idx for l in loci], np.int64))
    batch = call_alleles_n_batch if n_loci and int(nal.max()) > 2 else call_alleles_batch     # (wider rows)
    out, st = batch(np.concatenate(([0], np.cumsum(n_sel))).astype(np.int32), np.asarray(cns, np.int32)[sel],
                    w[sel] / sums[owner[sel]], nal, seeds, opts.allele_params or AlleleParams(), ctx, with_stats=True)
    rp = np.full(owner.shape[0], -1, np.int32)
    rp[sel] = out["read_peak"]
    out["read_peak"] = rp
    out["n_alleles"] = nal
    out["read_off"] = np.concatenate(([0], np.cumsum(n_kept))).astype(np.int64)
    tm["alleles_s"] = tm.get("alleles_s", 0.0) + time.perf_counter() - t_a
    tm["alleles_device_s"] = tm.get("alleles_device_s", 0.0) + st["kernel_ms"] / 1e3
    return out


def call_block_alleles_phased(loci, n_kept: np.ndarray, cns: np.ndarray, ws: np.ndarray, opts, ctx, tm, phase, sets=None) -> dict:
    """call_block_alleles with the reads grouped by haplotags or SNVs where that applies: the same
    normalisation of the weights, the same seeds, ONE call_alleles_phased_batch(..., fallback=True).  `phase`: the block's
    phase_block.BlockPhase (hp / ps per kept read when use_hp, the useful SNVs' cells when snv_vcf).  Returns what
    call_block_alleles returns plus method, reason, ps, the SNV outputs, `phase`, and `snv_base` / `cell_off` (the cells as the
    call took them and the cells in front of every locus).  `sets` (snv_phase_sets): the run's phase_sets.PhaseSets; the SNV
    calls are then fitted into phase sets across loci (`snv_ps` [L], -1 = none; peaks turned over where the set asks for it),
    and the loci that lose every SNV to the filter take the plain call."""
    from ..phasing import PhaseParams, call_alleles_phased_batch
    t_a = time.perf_counter()
    n_loci = len(loci)
    n_kept = np.asarray(n_kept, np.int64)
    owner = np.repeat(np.arange(n_loci), n_kept)
    w = np.asarray(ws, np.float64)
    good = np.isfinite(w) & (w > 0)
    bad_locus = np.bincount(owner[~good], minlength=n_loci) > 0
    sel = ~bad_locus[owner]
    sums = np.bincount(owner[sel], weights=w[sel], minlength=n_loci)
    n_sel = np.where(bad_locus, 0, n_kept)
    counts = allele_counts(opts)
    nal = np.array([n_alleles_of(counts, l.contig) for l in loci], np.int32)
    seeds = locus_seeds(opts.seed, np.array([l.t_idx for l in loci], np.int64))
    # a locus of more than two alleles is never phased: it sits out the phased call (as a locus without reads) and takes the
    # plain call below
    wide = np.flatnonzero((nal > 2) & ~bad_locus)
    if wide.size:
        bad_locus = bad_locus | (nal > 2)
        sel = ~bad_locus[owner]
        n_sel = np.where(bad_locus, 0, n_kept)
    used = phase.without(bad_locus, n_kept)
    pp = opts.phase_params or PhaseParams()
    if pp.snv_quality_threshold != opts.snv_min_base_qual:
        import dataclasses
        pp = dataclasses.replace(pp, snv_quality_threshold=int(opts.snv_min_base_qual))
    out, st = call_alleles_phased_batch(np.concatenate(([0], np.cumsum(n_sel))).astype(np.int32), np.asarray(cns, np.int32)[sel],
                                        w[sel] / sums[owner[sel]], np.minimum(nal, 2), seeds, hp=used.hp, ps=used.ps, snv_off=used.snv_off,
                                        snv_base=used.snv_base, snv_qual=used.snv_qual, params=opts.allele_params or AlleleParams(),
                                        phase_params=pp, fallback=True, ctx=ctx, with_stats=True)
    rp = np.full(owner.shape[0], -1, np.int32)
    rp[sel] = out["read_peak"]
    out["read_peak"] = rp
    if wide.size:
        reads = np.flatnonzero(np.isin(owner, wide))
        sub, sub_st = call_alleles_n_batch(np.concatenate(([0], np.cumsum(n_kept[wide]))).astype(np.int32), np.asarray(cns, np.int32)[reads],
                                           w[reads] / sums[owner[reads]], nal[wide], seeds[wide], opts.allele_params or AlleleParams(), ctx,
                                           with_stats=True)
        for k in ("call", "ci95", "ci99", "means", "weights", "stdevs"):      # the block's rows at the wider stride
            row = np.full((n_loci, MAX_ALLELES) + out[k].shape[2:], np.nan if out[k].dtype.kind == "f" else -1, out[k].dtype)
            row[:, :2] = out[k]
            row[wide] = sub[k]
            out[k] = row
        for k in ("status", "modal_n", "peak_n_reads"):
            out[k][wide] = sub[k]
        rp[reads] = sub["read_peak"]
        st["kernel_ms"] += sub_st["kernel_ms"]
    out["n_alleles"] = nal
    out["read_off"] = np.concatenate(([0], np.cumsum(n_kept))).astype(np.int64)
    out["phase"] = phase
    if used.snv_off is not None:
        out["snv_base"] = used.snv_base
        out["cell_off"] = np.concatenate(([0], np.cumsum(n_sel * np.diff(used.snv_off)))).astype(np.int64)
        if sets is not None:
            # snv_phase_sets: the rule of phase_sets.py over the block's SNV calls, here, before the consensus, k-mer and
            # methylation stages read the peaks; the loci it demotes take the plain call, ONE call over all of them, with
            # the arguments of call_alleles_phased_batch's fallback
            from .phase_block import snv_id
            from .phase_sets import demote, resolve_block
            rest = resolve_block(sets, loci, out, phase, lambda l, s: snv_id(phase, l, s, loci[l].contig))
            if rest.size:
                reads = np.flatnonzero(np.isin(owner, rest))
                sub, sub_st = call_alleles_batch(np.concatenate(([0], np.cumsum(n_kept[rest]))).astype(np.int32), np.asarray(cns, np.int32)[reads],
                                                 w[reads] / sums[owner[reads]], np.minimum(nal[rest], 2), seeds[rest],
                                                 opts.allele_params or AlleleParams(), ctx, with_stats=True)
                demote(out, rest, sub, reads)
                st["kernel_ms"] += sub_st["kernel_ms"]
    tm["alleles_s"] = tm.get("alleles_s", 0.0) + time.perf_counter() - t_a
    tm["alleles_device_s"] = tm.get("alleles_device_s", 0.0) + st["kernel_ms"] / 1e3
    return out


def peak_groups(al: dict, tract_len: np.ndarray, opts):
    """The read groups whose sequences are wanted: per called locus and peak, in locus and peak order, the kept reads
    assigned to the peak in read order.  Returns (group_locus [G], group_peak [G], tract_reads, tract_off [G + 1],
    anchor_reads, anchor_off [G + 1]) with the reads as indices into the block's kept reads.  A peak whose first tract is
    longer than large_consensus_length keeps its first max_n_large_consensus_reads reads for the tract group
    (call_locus.py:1606-1609); anchor groups are never cut."""
    n_loci = al["status"].shape[0]
    owner = np.repeat(np.arange(n_loci), np.diff(al["read_off"]))
    called = al["status"] == CALLED
    modal = np.where(called & (al["modal_n"] <= 2), al["modal_n"], 0).astype(np.int64)   # (more peaks: no read has one)
    g_first = np.concatenate(([0], np.cumsum(modal)))            # first group of every locus
    n_groups = int(g_first[-1])
    group_locus = np.repeat(np.arange(n_loci), modal)
    group_peak = np.arange(n_groups) - g_first[:-1][group_locus]
    rp = al["read_peak"]
    take = np.flatnonzero(called[owner] & (rp >= 0))
    gid = g_first[:-1][owner[take]] + rp[take]
    order = np.argsort(gid, kind="stable")
    reads, gid = take[order], gid[order]
    sizes = np.bincount(gid, minlength=n_groups)
    off = np.concatenate(([0], np.cumsum(sizes)))
    pos = np.arange(reads.shape[0]) - off[:-1][gid]
    big = np.zeros(n_groups, bool)
    nz = sizes > 0
    big[nz] = tract_len[reads[off[:-1][nz]]] > opts.large_consensus_length
    keep = ~(big[gid] & (pos >= opts.max_n_large_consensus_reads))
    t_sizes = np.bincount(gid[keep], minlength=n_groups)
    return group_locus, group_peak, reads[keep], np.concatenate(([0], np.cumsum(t_sizes))), reads, off


def block_consensus(al: dict, tract_start, tract_len, anchor_start, anchor_len, opts, ctx, tm, seqs=None, d_seqs=None,
                    n_seq_bytes=None, fetch=None) -> dict:
    """Allele sequences of a block: one strk_best_representatives call (opts.consensus_method "best_rep") or one strk_consensus
    call ("poa") over the tract groups and the anchor groups of all called peaks.  The four arrays address every kept read's raw
    tract and raw start anchor inside one buffer (host `seqs`, or device `d_seqs` with `fetch()` returning its host copy for
    the few strings that are reported; strk_consensus returns the strings themselves, so nothing is fetched).  Returns
    {locus: ([[sequence, method] per peak], [[anchor, method] per peak])}."""
    t_a = time.perf_counter()
    tract_start, tract_len = np.asarray(tract_start, np.int64), np.asarray(tract_len, np.int32)
    anchor_start, anchor_len = np.asarray(anchor_start, np.int64), np.asarray(anchor_len, np.int32)
    g_locus, _g_peak, t_reads, t_off, a_reads, a_off = peak_groups(al, tract_len, opts)
    n_groups = g_locus.shape[0]
    if n_groups == 0:
        return {}
    starts = np.concatenate((tract_start[t_reads], anchor_start[a_reads]))
    lens = np.concatenate((tract_len[t_reads], anchor_len[a_reads]))
    group_off = np.concatenate((t_off, t_off[-1] + a_off[1:])).astype(np.int32)
    if opts.consensus_method == "poa":
        out, st = consensus_packed(group_off, starts, lens, seqs=seqs, d_seqs=d_seqs, n_seq_bytes=n_seq_bytes,
                                   max_mdn_poa_length=opts.max_mdn_poa_length, ctx=ctx, with_stats=True)
        tm["consensus_device_s"] = tm.get("consensus_device_s", 0.0) + st["kernel_ms"] / 1e3
        text, off, meth = out["seqs"].tobytes(), out["seq_off"].tolist(), out["method"].tolist()
        res = {}
        for g in range(n_groups):
            t, a = res.setdefault(int(g_locus[g]), ([], []))
            for k, dest in ((g, t), (n_groups + g, a)):
                dest.append([None if meth[k] == 0 else text[off[k]:off[k + 1]].decode("ascii"), METHOD_NAMES[meth[k]]])
        tm["consensus_s"] = tm.get("consensus_s", 0.0) + time.perf_counter() - t_a
        return res
    out, st = best_representatives_packed(group_off, starts, lens, seqs=seqs, d_seqs=d_seqs, n_seq_bytes=n_seq_bytes, ctx=ctx,
                                          with_stats=True)
    tm["consensus_device_s"] = tm.get("consensus_device_s", 0.0) + st["kernel_ms"] / 1e3
    t_b = time.perf_counter()
    host = np.asarray(seqs, np.uint8) if seqs is not None else fetch()
    tm["consensus_fetch_s"] = tm.get("consensus_fetch_s", 0.0) + time.perf_counter() - t_b
    first = group_off[:-1].astype(np.int64) + out["index"]
    res: dict[int, tuple[list, list]] = {}
    text = host.tobytes()
    for g in range(n_groups):
        pair = []
        for k in (g, n_groups + g):
            if out["method"][k] == 0:
                pair.append([None, METHOD_NAMES[0]])
                continue
            s0 = int(starts[first[k]])
            pair.append([text[s0:s0 + int(lens[first[k]])].decode("ascii"), METHOD_NAMES[int(out["method"][k])]])
        t, a = res.setdefault(int(g_locus[g]), ([], []))
        t.append(pair[0])
        a.append(pair[1])
    tm["consensus_s"] = tm.get("consensus_s", 0.0) + time.perf_counter() - t_a
    return res


def block_kmers(mode: str, al: dict | None, tract_start, tract_len, read_k, locus_k, opts, ctx, tm, seqs=None, d_seqs=None,
                n_seq_bytes=None, fetch=None) -> dict:
    """Motif-sized k-mer counts of a block (call_locus.py:1287,1526-1593,1635): ONE strk_count_kmers call whose groups are the
    singleton groups of the kept reads (`mode` "read" / "both") followed by the groups of all reads of every called peak ("peak"
    / "both"; the consensus stage's cut of long alleles does not apply).  tract_start / tract_len address every kept read's raw
    tract inside one buffer (host `seqs`, or device `d_seqs` with `fetch()` returning its host copy, from which the strings are
    cut); read_k is the window length per read, locus_k per locus (the catalog motif's length).  Returns
    {"reads": [{kmer: count} per kept read] or None, "peaks": {locus: [{kmer: count} per peak]} or None}."""
    t_a = time.perf_counter()
    tract_start, tract_len = np.asarray(tract_start, np.int64), np.asarray(tract_len, np.int32)
    read_k, locus_k = np.asarray(read_k, np.int32), np.asarray(locus_k, np.int32)
    n_reads = tract_start.shape[0]
    per_read, per_peak = mode in ("read", "both"), mode in ("peak", "both")
    n_single = n_reads if per_read else 0
    starts, lens, offs, ks = [], [], [np.zeros(1, np.int64)], []
    if per_read:
        starts.append(tract_start); lens.append(tract_len); ks.append(read_k)
        offs.append(np.arange(1, n_reads + 1, dtype=np.int64))
    g_locus = np.zeros(0, np.int64)
    if per_peak:
        g_locus, _g_peak, _t_reads, _t_off, reads, off = peak_groups(al, tract_len, opts)
        starts.append(tract_start[reads]); lens.append(tract_len[reads]); ks.append(locus_k[g_locus])
        offs.append(n_single + off[1:])
    res = {"reads": [] if per_read else None, "peaks": {} if per_peak else None}
    n_groups = n_single + g_locus.shape[0]
    if n_groups == 0:
        return res
    ks = np.concatenate(ks)
    out, st = count_kmers_packed(np.concatenate(offs).astype(np.int32), np.concatenate(starts), np.concatenate(lens), ks, seqs=seqs,
                                 d_seqs=d_seqs, n_seq_bytes=n_seq_bytes, ctx=ctx, with_stats=True)
    tm["kmers_device_s"] = tm.get("kmers_device_s", 0.0) + st["kernel_ms"] / 1e3
    host = np.asarray(seqs, np.uint8) if seqs is not None else fetch()
    dicts = dicts_of(out, ks, host.tobytes().decode("latin-1"))
    if per_read:
        res["reads"] = dicts[:n_single]
    for g, d in zip(g_locus.tolist(), dicts[n_single:]):
        res["peaks"].setdefault(g, []).append(d)
    tm["kmers_s"] = tm.get("kmers_s", 0.0) + time.perf_counter() - t_a
    return res


def kmers_row(row: dict, km: dict, li: int, recs: list[dict], first: int) -> None:
    """Adds the k-mer counts of locus `li` of the block to its row: `kmers` on every read record (recs = the block's records
    first .. first + len(recs)), peaks.kmers on a called locus.  An uncalled locus and a nullified call have no peak counts."""
    if km["reads"] is not None:
        for k, r in enumerate(recs):
            r["kmers"] = km["reads"][first + k]
    if km["peaks"] is not None and li in km["peaks"] and row.get("peaks"):
        row["peaks"]["kmers"] = km["peaks"][li]


def genotype_row(row: dict, al: dict, li: int, recs: list[dict], cons: dict | None) -> None:
    """Adds the call of locus `li` of the block to its row (call_locus.py:1490-1640 + CallData.to_dict): `p` on every read
    record, assign_method, call, the intervals, peaks, read_peaks_called, mean_model_align_score.  A locus with too few
    reads keeps the row it has; a call with an empty peak is nullified as the reference does (call_locus.py:1597-1600) and
    its reads keep their peak labels."""
    status = int(al["status"][li])
    if status == TOO_FEW:
        return
    a = int(al["read_off"][li])
    if int(al["modal_n"][li]) <= 2:     # with more peaks no read is labelled (call_locus.py:1536)
        for k, p in enumerate(al["read_peak"][a:a + len(recs)].tolist()):
            recs[k]["p"] = p
        row["read_peaks_called"] = True
    scs = [r["sc"] for r in recs if r["sc"] is not None]
    row["mean_model_align_score"] = math.fsum(scs) / len(scs) if scs else None
    if status != CALLED:
        return
    cd = call_data_from_batch(al, li, int(al["n_alleles"][li]))
    row.update(cd.to_dict())
    if cons is not None and li in cons:
        row["peaks"]["seqs"], row["peaks"]["start_anchor_seqs"] = cons[li]
