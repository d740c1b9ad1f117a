"""Phased allele calls on the GPU: reads grouped by their haplotags or by the SNVs they carry (strk_call_alleles_phased,
kernels k_phase_group, k_phase_pack, k_alleles, k_phase_finish).

Stands where STRkit picks the way a locus is genotyped (strkit/call/call_locus.py:1381-1495): reads pre-separated by HP / PS
tags (call_alleles_with_haplotags), else clustered by the SNVs next to the locus (call_alleles_with_incorporated_snvs), else
the bootstrapped GMM over copy numbers alone (alleles.call_alleles_batch).  The rule is DESIGN.md §13.  There is no CPU path.
Tag parsing, candidate SNVs, per-read SNV bases and cross-locus phase sets belong to a file front end and are not in here.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass

import numpy as np

from . import _lib
from ._lib import ptr
from .alleles import (ALLELE_KEYS, ASSIGN_DIST, ASSIGN_SINGLE, CALLED, TOO_FEW, AlleleParams, CallData, batch_inputs, batch_outputs,
                      call_alleles_batch, call_data_from_batch)

NOT_PHASED = 3
ASSIGN_NONE, ASSIGN_HP, ASSIGN_SNV, ASSIGN_SNV_DIST = 0, 1, 2, 3
ASSIGN_NAMES = {ASSIGN_HP: "hp", ASSIGN_SNV: "snv", ASSIGN_SNV_DIST: "snv+dist"}
(REASON_NONE, REASON_NO_TAGS, REASON_TAG_THRESHOLDS, REASON_FEW_SNV_READS, REASON_GROUP_NOT_CALLED,
 REASON_NO_SNV_CALLED) = range(6)
SNV_NOT_EVALUATED, SNV_CALLED, SNV_ZERO_TOTAL, SNV_ONLY_OUT_OF_RANGE, SNV_CROSS_TALK, SNV_SAME_BASE = -1, 0, 1, 2, 3, 4
MAX_READS, MAX_SNVS = 1024, 64


@dataclass(frozen=True)
class PhaseParams:
    """call_locus.py:79 (min_hp_read_coverage), :96-99 (calculate_read_distance's defaults).  piece_loci / ws_budget: loci and
    workspace bytes of one piece of a call (0: the library's); the result does not depend on them."""
    min_hp_read_coverage: int = 8
    snv_quality_threshold: int = 20
    many_snvs_quantity: int = 3
    cn_weight_few: float = 0.2
    cn_weight_many: float = 0.1
    piece_loci: int = 0
    ws_budget: int = 0

    def _c(self) -> _lib.StrkPhaseParams:
        return _lib.StrkPhaseParams(int(self.min_hp_read_coverage), int(self.snv_quality_threshold),
                                    int(self.many_snvs_quantity), int(self.piece_loci), float(self.cn_weight_few),
                                    float(self.cn_weight_many), int(self.ws_budget))


def call_alleles_phased_batch(read_off, cns, weights, n_alleles, seeds, hp=None, ps=None, snv_off=None, snv_base=None,
                              snv_qual=None, params: AlleleParams | None = None, phase_params: PhaseParams | None = None,
                              fallback: bool = True, ctx=None, with_stats: bool = False):
    """One library call for many loci.  Inputs as alleles.call_alleles_batch, plus per read hp / ps (int32, -1 = untagged;
    both or neither) and per locus snv_off [L + 1] with the cells snv_base / snv_qual (uint8; locus l's reads x SNVs cells,
    read-major, behind those of the loci before it; '-' out of range, '_' a gap).

    Returns call_alleles_batch's dict plus method, reason, ps [L] and snv_status [n_snvs], snv_call, snv_rcs [n_snvs, 2].
    With fallback=True the loci without a phased call (method ASSIGN_NONE) are called with call_alleles_batch under the same
    seeds and merged in, so that the result is what call_locus.py:1381-1495 produces; their method stays ASSIGN_NONE (the
    reference's `dist` / `single`) and their reason says why they were not phased."""
    params = params or AlleleParams()
    phase_params = phase_params or PhaseParams()
    ctx = ctx or _lib.default_context()
    read_off, cns, weights, n_alleles, seeds, n_loci = batch_inputs(read_off, cns, weights, n_alleles, seeds)
    n_reads = cns.shape[0]
    if hp is not None:
        hp = np.ascontiguousarray(hp, dtype=np.int32)
    if ps is not None:
        ps = np.ascontiguousarray(ps, dtype=np.int32)
    for name, t in (("hp", hp), ("ps", ps)):
        if t is not None and t.shape != (n_reads,):
            raise ValueError(f"{name} must have one entry per read")
    n_snvs = n_cells = 0
    if snv_off is not None:
        snv_off = np.ascontiguousarray(snv_off, dtype=np.int32)
        if snv_off.shape != (n_loci + 1,):
            raise ValueError("snv_off must have one entry per locus and one more")
        n_snvs = max(int(snv_off[-1]), 0)
    if snv_base is not None:
        snv_base = np.ascontiguousarray(snv_base, dtype=np.uint8).ravel()
        n_cells = snv_base.shape[0]
    if snv_qual is not None:
        snv_qual = np.ascontiguousarray(snv_qual, dtype=np.uint8).ravel()
        if snv_base is not None and snv_qual.shape != snv_base.shape:
            raise ValueError("snv_base and snv_qual must have one byte per cell each")
    out = dict(batch_outputs(n_loci, n_reads),
               method=np.empty(n_loci, np.int32), reason=np.empty(n_loci, np.int32), ps=np.empty(n_loci, np.int32),
               snv_status=np.empty(n_snvs, np.int32), snv_call=np.zeros((n_snvs, 2), np.uint8),
               snv_rcs=np.zeros((n_snvs, 2), np.int32))
    cp, pp = params._c(), phase_params._c()
    st = _lib.StrkStats()
    _lib.check(_lib.load().strk_call_alleles_phased(
        ctx.handle, n_loci, *map(ptr, (read_off, cns, weights, n_alleles, seeds)), C.byref(cp), C.byref(pp),
        *map(ptr, (hp, ps, snv_off, snv_base, snv_qual)), n_cells,
        *[ptr(out[k]) for k in (*ALLELE_KEYS, "read_peak", "method", "reason", "ps", "snv_status", "snv_call", "snv_rcs")],
        C.byref(st)))
    stats = st.as_dict()
    if fallback:
        rest = np.nonzero(out["status"] == NOT_PHASED)[0]
        if rest.size:
            n = np.diff(read_off)
            sub_off = np.concatenate(([0], np.cumsum(n[rest]))).astype(np.int32)
            reads = np.concatenate([np.arange(read_off[l], read_off[l + 1]) for l in rest]) if sub_off[-1] else np.zeros(0, np.int64)
            sub, sub_st = call_alleles_batch(sub_off, cns[reads], weights[reads], n_alleles[rest], seeds[rest], params, ctx,
                                             with_stats=True)
            for k in ALLELE_KEYS:
                out[k][rest] = sub[k]
            out["read_peak"][reads] = sub["read_peak"]
            stats["kernel_ms"] += sub_st["kernel_ms"]
    if with_stats:
        return out, stats
    return out


def phased_call_data(out: dict, l: int, n_alleles: int, snv_off=None):
    """Locus l of a call_alleles_phased_batch result as (CallData | None, called_snvs): the CallData carries the assign
    method (`hp`, `snv`, `snv+dist`, or `dist` / `single` for a locus called by the fallback) and, for `hp`, the phase set as
    `ps`; called_snvs lists (index of the SNV inside the locus, call bytes, read counts) for every SNV that was called."""
    cd = call_data_from_batch(out, l, n_alleles)
    if cd is None or int(out["status"][l]) == NOT_PHASED:
        return None, []
    method = int(out["method"][l])
    cd.ps = None
    if method != ASSIGN_NONE:
        cd.set_assign_method(ASSIGN_NAMES[method])
        if method == ASSIGN_HP:
            cd.ps = int(out["ps"][l])
    else:
        cd.set_assign_method(ASSIGN_DIST if int(n_alleles) > 1 else ASSIGN_SINGLE)
    snvs = []
    if snv_off is not None and method in (ASSIGN_SNV, ASSIGN_SNV_DIST):
        s0, s1 = int(snv_off[l]), int(snv_off[l + 1])
        for s in range(s0, s1):
            if int(out["snv_status"][s]) == SNV_CALLED:
                snvs.append((s - s0, tuple(chr(int(b)) for b in out["snv_call"][s]), out["snv_rcs"][s].tolist()))
    return cd, snvs


def call_locus_phased(cns, weights, n_alleles: int, seed: int, hp=None, ps=None, snv_base=None, snv_qual=None,
                      params: AlleleParams | None = None, phase_params: PhaseParams | None = None, ctx=None):
    """One locus: cns / weights per read, optionally hp / ps per read and snv_base / snv_qual [n_reads, n_snvs].  Returns
    (CallData | None, called_snvs) as phased_call_data, the fallback included; the CallData also carries `read_peaks`."""
    cns = np.asarray(cns, dtype=np.int32).ravel()
    n = cns.shape[0]
    snv_off = None
    if snv_base is not None:
        snv_base = np.asarray(snv_base, dtype=np.uint8).reshape(n, -1)
        snv_qual = np.asarray(snv_qual, dtype=np.uint8).reshape(n, -1)
        snv_off = np.array([0, snv_base.shape[1]], np.int32)
    out = call_alleles_phased_batch(np.array([0, n], np.int32), cns, weights, [int(n_alleles)], [int(seed) & ((1 << 64) - 1)],
                                    hp, ps, snv_off, snv_base, snv_qual, params, phase_params, True, ctx)
    cd, snvs = phased_call_data(out, 0, n_alleles, snv_off)
    if cd is not None:
        cd.read_peaks = out["read_peak"].copy()
    return cd, snvs
