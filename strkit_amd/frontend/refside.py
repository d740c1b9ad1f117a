"""The reference side of a block of loci (strkit/call/call_locus.py:700-835): reference window, reference copy number by
the same counter as the reads, boundaries widened by the offsets it found."""
from __future__ import annotations

import time

import numpy as np

from .. import _lib
from ..repeat_count_params import get_reference_rc_params
from ..repeats import get_ref_repeat_counts, get_ref_repeat_counts_packed
from .fasta import Fasta
from .loci import Locus
from .options import DEFAULT_REF_MAX_ITERS, VCF_ANCHOR_SIZE, CallOptions


def _ref_window(locus: Locus, ref: Fasta):
    """Reference window of a locus split into flank / tract / flank, or None where the reference raises SkipLocus /
    InvalidLocus (call_locus.py:765-787)."""
    try:
        total = ref.fetch(locus.contig, locus.left_flank_coord, locus.right_flank_coord + 1)
    except (IndexError, KeyError):
        return None
    off_l, off_r = locus.left_coord - locus.left_flank_coord, locus.right_coord - locus.left_flank_coord
    fl, fr, tr = total[:off_l], total[off_r:-1], total[off_l:off_r]
    if len(fl) < locus.flank_size or len(fr) < locus.flank_size:
        return None                                           # "reference flank size too small"
    n_run = "N" * locus.motif_size
    if fl.endswith(n_run) or fr.startswith(n_run):
        return None                                           # "reference has flanking N[...] sequence"
    return total, fl, tr, fr


def _adjusted(locus: Locus, respect_ref: bool, l_off: int, r_off: int) -> dict:
    return {"left_coord_adj": locus.left_coord if respect_ref else locus.left_coord - max(0, l_off),
            "right_coord_adj": locus.right_coord if respect_ref else locus.right_coord + max(0, r_off)}


def get_loci_with_ref_data(block: list[Locus], ref: Fasta, respect_ref: bool = False, context=None) -> list[dict | None]:
    """call_locus.py:736-835 for a block of loci: reference windows, reference copy numbers by the same counter (all
    loci in one batched library call), boundaries widened by the offsets it found.  None per skipped locus.
    With a `Fasta` the windows of all loci are gathered and handed over as packed arrays (no Python per locus before
    the result records); any other reference object goes through its `fetch`."""
    if isinstance(ref, Fasta) and len(block) > 1:
        return _loci_with_ref_data_packed(block, ref, respect_ref, context)
    windows = [_ref_window(locus, ref) for locus in block]
    jobs, idx = [], []
    for i, (locus, w) in enumerate(zip(block, windows)):
        if w is None:
            continue
        _, fl, tr, fr = w
        est = round(len(tr) / locus.motif_size)
        jobs.append((est, tr, fl, fr, locus.motif, locus.right_coord - locus.left_coord,
                     get_reference_rc_params("repalign", est, DEFAULT_REF_MAX_ITERS)))
        idx.append(i)
    out: list[dict | None] = [None] * len(block)
    for i, ((ref_cn, _), l_off, r_off, _n_is, (fl2, tr2, fr2)) in zip(
            idx, get_ref_repeat_counts(jobs, VCF_ANCHOR_SIZE, respect_ref, context)):
        out[i] = {"ref_cn": ref_cn, "ref_total_seq": windows[i][0], "ref_seq": tr2, "ref_left_flank_seq": fl2,
                  "ref_right_flank_seq": fr2, **_adjusted(block[i], respect_ref, l_off, r_off)}
    return out


def _loci_with_ref_data_packed(block: list[Locus], ref: Fasta, respect_ref: bool, context) -> list[dict | None]:
    n = len(block)
    out: list[dict | None] = [None] * n
    lc = np.array([l.left_coord for l in block], np.int64)
    rc = np.array([l.right_coord for l in block], np.int64)
    fs = np.array([l.flank_size for l in block], np.int64)
    mlen = np.array([l.motif_size for l in block], np.int64)
    lfc = np.maximum(0, lc - fs)
    rfc = rc + fs
    contig_of = [l.contig for l in block]
    arrays = {}
    for c in set(contig_of):
        try:
            arrays[c] = ref.array(c)
        except KeyError:
            arrays[c] = None                                   # "invalid region" (InvalidLocus)
    clen = np.array([-1 if arrays[c] is None else len(arrays[c]) for c in contig_of], np.int64)
    end = np.minimum(rfc + 1, clen)                            # Python slicing of the fetch (call_locus.py:772)
    nfl = lc - lfc
    nfr = (end - 1) - rc                                       # ref_total_seq[off_r:-1]
    ok = (clen >= 0) & (lfc <= clen) & (nfl >= fs) & (nfr >= fs) & (rc > lc)       # "reference flank size too small"
    idx = np.flatnonzero(ok)
    if idx.size == 0:
        return out
    # gather [lfc, end - 1) of every live locus into one flat array (the trailing +1 base is only used by realign)
    lens = (end - 1 - lfc)[idx]
    seq_off = np.concatenate(([0], np.cumsum(lens)))
    seqs = np.empty(int(seq_off[-1]), np.uint8)
    last_base = np.empty(idx.size, np.uint8)                     # the base after each window (ref_total_seq has it)
    by_contig: dict[str, list[int]] = {}
    for k, i in enumerate(idx.tolist()):
        by_contig.setdefault(contig_of[i], []).append(k)
    for c, ks in by_contig.items():
        ks = np.array(ks, np.int64)
        ln = lens[ks]
        src0 = lfc[idx[ks]]
        owner = np.repeat(np.arange(len(ks)), ln)
        within = np.arange(int(ln.sum())) - (np.cumsum(ln) - ln)[owner]
        seqs[seq_off[ks][owner] + within] = arrays[c][src0[owner] + within]
        last_base[ks] = arrays[c][end[idx[ks]] - 1]
    nfl_i, ntr_i, nfr_i = nfl[idx], (rc - lc)[idx], nfr[idx]
    # "reference has flanking N[...] sequence" (call_locus.py:786-787): only loci with an N next to the tract are looked at
    n_code = (ord("N"), ord("n"))
    tr0 = seq_off[:-1] + nfl_i
    sus = np.flatnonzero(np.isin(seqs[tr0 - 1], n_code) | np.isin(seqs[np.minimum(tr0 + ntr_i, len(seqs) - 1)], n_code))
    keep = np.ones(idx.size, bool)
    for k in sus.tolist():
        n_run = "N" * int(mlen[idx[k]])
        a0 = int(tr0[k])
        fl_s = seqs[int(seq_off[k]):a0].tobytes().decode()
        fr_s = seqs[a0 + int(ntr_i[k]):int(seq_off[k + 1])].tobytes().decode()
        keep[k] = not (fl_s.endswith(n_run) or fr_s.startswith(n_run))
    if not keep.all():                       # (rare) the dropped loci leave the gathered arrays; the rest goes on as it is
        seqs, idx, last_base = seqs[np.repeat(keep, lens)], idx[keep], last_base[keep]
        seq_off = np.concatenate(([0], np.cumsum(lens[keep])))
        nfl_i, ntr_i, nfr_i = nfl_i[keep], ntr_i[keep], nfr_i[keep]
        if idx.size == 0:
            return out
    est = np.rint(ntr_i / mlen[idx]).astype(np.int64)           # round(len(ref_seq) / motif_size): half to even
    # get_reference_rc_params (repeat_count_params.py:17-42)
    max_iters = np.where(est >= 2000, 50, np.where(est >= 1000, 150, np.where(est >= 200, 200, DEFAULT_REF_MAX_ITERS)))
    step = np.where(est >= 2000, 15, np.where(est >= 1000, 5, np.where(est >= 200, 3, 1)))
    lsr = np.where(est >= 2000, 1, 3)
    motifs = b"".join(block[i].motif.encode() for i in idx.tolist())
    motif_off = np.concatenate(([0], np.cumsum(mlen[idx])))
    o9 = get_ref_repeat_counts_packed(est, seqs, seq_off, nfl_i, ntr_i, nfr_i, np.frombuffer(motifs, np.uint8), motif_off,
                                      ntr_i, max_iters, lsr, step, VCF_ANCHOR_SIZE, respect_ref, context)
    text = seqs.tobytes().decode("ascii")
    so = seq_off.tolist()
    last_chr = [chr(x) for x in last_base.tolist()]
    for k, (i, (cn, _sc, l_off, r_off, _n1, _n2, a, b, _c)) in enumerate(zip(idx.tolist(), o9.tolist())):
        base, total_end = so[k], so[k + 1]
        # the reference's ref_total_seq carries one more base (call_locus.py:770-772)
        out[i] = {"ref_cn": cn, "ref_total_seq": text[base:total_end] + last_chr[k],
                  "ref_seq": text[base + a:base + a + b], "ref_left_flank_seq": text[base:base + a],
                  "ref_right_flank_seq": text[base + a + b:total_end], **_adjusted(block[i], respect_ref, l_off, r_off)}
    return out


def get_locus_with_ref_data(locus: Locus, ref: Fasta, respect_ref: bool = False, context=None) -> dict | None:
    return get_loci_with_ref_data([locus], ref, respect_ref, context)[0]


def ref_side_of_blocks(blocks, ref: Fasta, opts: CallOptions, ctx, tm: dict) -> dict:
    """Reference side of ALL loci of `blocks`, a few thousand per library call (each of its lock-step rounds is one device launch
    however many loci take part): {id(locus): reference data or None}.  A chunk that fails is left out — call_blocks' per-block
    path computes it again and isolates the locus."""
    ref_cache: dict[int, dict | None] = {}
    flat = [l for blk in blocks for l in blk]
    t_a = time.perf_counter()
    for c0 in range(0, len(flat), 4096):
        chunk = flat[c0:c0 + 4096]
        try:
            ref_cache.update(zip(map(id, chunk), get_loci_with_ref_data(chunk, ref, opts.respect_ref, ctx)))
        except (_lib.StrkError, ValueError):
            pass
    tm["ref_side_s"] = tm.get("ref_side_s", 0.0) + time.perf_counter() - t_a
    return ref_cache
