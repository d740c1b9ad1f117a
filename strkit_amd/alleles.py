"""Allele calling on the GPU: bootstrapped GMM genotypes per locus (strk_call_alleles / strk_call_alleles_n, kernel k_alleles_w).

Drop-in for STRkit's call_alleles (strkit/call/allele.py:176-336) plus the distance-based peak assignment of
call_locus.py:1536-1600.  The algorithm is the reference's with one specified random stream instead of numpy's
Generator and sklearn's seeds, so results are deterministic per locus seed.  There is no CPU path.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass

import numpy as np

from . import _lib
from ._lib import ptr

CALLED, TOO_FEW, EMPTY_PEAK = 0, 1, 2
ASSIGN_SINGLE, ASSIGN_DIST = "single", "dist"
MAX_ALLELES = 6   # STRK_MAX_ALLELES: the row stride of call_alleles_n_batch's per-locus outputs


@dataclass(frozen=True)
class AlleleParams:
    """strkit/call/params.py:39-56,166-172 and sklearn's GaussianMixture defaults."""
    min_reads: int = 4
    min_allele_reads: int = 2
    num_bootstrap: int = 100
    n_init: int = 3
    max_iter: int = 100
    filter_factor: int = 3
    force_gm_filter: bool = False
    tol: float = 1e-3
    reg_covar: float = 1e-6
    expansion_ratio: float = 5.0

    def _c(self) -> _lib.StrkAlleleParams:
        return _lib.StrkAlleleParams(int(self.min_reads), int(self.min_allele_reads), int(self.num_bootstrap),
                                     int(self.n_init), int(self.max_iter), int(self.filter_factor),
                                     int(bool(self.force_gm_filter)), 0, float(self.tol), float(self.reg_covar),
                                     float(self.expansion_ratio))


_M64 = (1 << 64) - 1
_GAMMA = 0x9E3779B97F4A7C15


def mix64(z: int) -> int:
    """The finaliser of splitmix64 (the library's random stream uses the same one)."""
    z &= _M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _M64
    return z ^ (z >> 31)


def locus_seed(seed: int, t_idx: int) -> int:
    """Per-locus seed of the front end: mix64(seed + gamma * (locus_index + 1)).  A locus's call then depends on the run
    seed and its own index only, not on its block, the reader or the order of the blocks."""
    return mix64((int(seed) + _GAMMA * (int(t_idx) + 1)) & _M64)


def locus_seeds(seed: int, t_idx) -> np.ndarray:
    """locus_seed for an array of locus indices (uint64, wrapping arithmetic)."""
    with np.errstate(over="ignore"):
        z = np.uint64(int(seed) & _M64) + np.uint64(_GAMMA) * (np.asarray(t_idx).astype(np.uint64) + np.uint64(1))
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return z ^ (z >> np.uint64(31))


ALLELE_KEYS = ("status", "modal_n", "call", "ci95", "ci99", "means", "weights", "stdevs", "peak_n_reads")   # per locus, in C order


def batch_inputs(read_off, cns, weights, n_alleles, seeds):
    """The five inputs of a batched allele call as contiguous arrays of the C types, n_alleles and seeds broadcast to one
    entry per locus: (read_off, cns, weights, n_alleles, seeds, n_loci).  read_off must span cns."""
    read_off = np.ascontiguousarray(read_off, dtype=np.int32)
    cns = np.ascontiguousarray(cns, dtype=np.int32)
    weights = np.ascontiguousarray(weights, dtype=np.float64)
    n_loci = read_off.shape[0] - 1
    if n_loci < 0 or cns.shape != weights.shape or int(read_off[-1]) != cns.shape[0]:
        raise ValueError("read_off must span cns, and cns and weights must have one entry per read")
    n_alleles = np.ascontiguousarray(np.broadcast_to(np.asarray(n_alleles, dtype=np.int32), (n_loci,)))
    seeds = np.ascontiguousarray(np.broadcast_to(np.asarray(seeds, dtype=np.uint64), (n_loci,)))
    return read_off, cns, weights, n_alleles, seeds, n_loci


def batch_outputs(n_loci: int, n_reads: int, width: int = 2) -> dict:
    """The arrays a batched allele call fills: ALLELE_KEYS per locus (`width` allele slots) and read_peak per read."""
    return dict(status=np.empty(n_loci, np.int32), modal_n=np.empty(n_loci, np.int32),
                call=np.empty((n_loci, width), np.int32), ci95=np.empty((n_loci, width, 2), np.int32),
                ci99=np.empty((n_loci, width, 2), np.int32), means=np.empty((n_loci, width)),
                weights=np.empty((n_loci, width)), stdevs=np.empty((n_loci, width)),
                peak_n_reads=np.empty((n_loci, 2), np.int32), read_peak=np.empty(n_reads, np.int32))


def _call_batch(width: int, read_off, cns, weights, n_alleles, seeds, params, ctx, with_stats: bool):
    """One library call for many loci through the entry point whose rows have `width` allele slots."""
    params = params or AlleleParams()
    ctx = ctx or _lib.default_context()
    read_off, cns, weights, n_alleles, seeds, n_loci = batch_inputs(read_off, cns, weights, n_alleles, seeds)
    out = batch_outputs(n_loci, cns.shape[0], width)
    cp = params._c()
    st = _lib.StrkStats()
    entry = _lib.load().strk_call_alleles if width == 2 else _lib.load().strk_call_alleles_n
    _lib.check(entry(ctx.handle, n_loci, *map(ptr, (read_off, cns, weights, n_alleles, seeds)), C.byref(cp),
                     *[ptr(out[k]) for k in (*ALLELE_KEYS, "read_peak")], C.byref(st)))
    if with_stats:
        return out, st.as_dict()
    return out


def call_alleles_batch(read_off, cns, weights, n_alleles, seeds, params: AlleleParams | None = None, ctx=None,
                       with_stats: bool = False):
    """One library call for many loci.  Locus l owns cns/weights[read_off[l]:read_off[l+1]].  Returns a dict of numpy
    arrays: status, modal_n [L]; call, means, weights, stdevs, peak_n_reads [L, 2]; ci95, ci99 [L, 2, 2];
    read_peak [n_reads] (-1: no call).  Slot 1 of a one-allele locus is -1 / NaN."""
    return _call_batch(2, read_off, cns, weights, n_alleles, seeds, params, ctx, with_stats)


def call_alleles_n_batch(read_off, cns, weights, n_alleles, seeds, params: AlleleParams | None = None, ctx=None,
                         with_stats: bool = False):
    """call_alleles_batch for one to MAX_ALLELES alleles per locus (strk_call_alleles_n, kernel k_alleles_n).
    Same arguments; call, means, weights, stdevs are [L, 6] and ci95, ci99 [L, 6, 2], unused slots -1 / NaN;
    peak_n_reads stays [L, 2].  A locus whose modal number of peaks is above 2 has no read peaks (read_peak -1, counts 0).
    For n_alleles <= 2 the first two slots are call_alleles_batch's, byte for byte."""
    return _call_batch(MAX_ALLELES, read_off, cns, weights, n_alleles, seeds, params, ctx, with_stats)


class CallData:
    """What call_locus.py and output/vcf.py read from strkit_rust_ext.CallData."""

    def __init__(self, call, call_95_cis, call_99_cis, means, weights, stdevs, modal_n, n_reads=None,
                 status: int = CALLED):
        self.call = np.asarray(call, dtype=np.int32)
        self.call_95_cis = np.asarray(call_95_cis, dtype=np.int32)
        self.call_99_cis = np.asarray(call_99_cis, dtype=np.int32)
        self.means = np.asarray(means, dtype=np.float64)
        self.weights = np.asarray(weights, dtype=np.float64)
        self.stdevs = np.asarray(stdevs, dtype=np.float64)
        self.modal_n = int(modal_n)
        self.n_reads = None if n_reads is None else np.asarray(n_reads, dtype=np.uint16)
        self.status = int(status)
        self._assign_method = ASSIGN_DIST if self.call.shape[0] > 1 else ASSIGN_SINGLE

    @property
    def peak_means(self):
        return self.means

    @property
    def peak_weights(self):
        return self.weights

    @property
    def peak_stdevs(self):
        return self.stdevs

    @property
    def peak_modal_n(self) -> int:
        return self.modal_n

    def set_assign_method(self, method) -> None:
        self._assign_method = str(getattr(method, "value", method))

    def get_assign_method_str(self) -> str:
        return self._assign_method

    def set_n_reads(self, n_reads) -> None:
        self.n_reads = np.asarray(n_reads, dtype=np.uint16)

    def to_dict(self) -> dict:
        k = self.modal_n
        return {
            "assign_method": self._assign_method,
            "call": self.call.tolist(),
            "call_95_cis": self.call_95_cis.tolist(),
            "call_99_cis": self.call_99_cis.tolist(),
            "peaks": {
                "means": self.means[:k].tolist(),
                "weights": self.weights[:k].tolist(),
                "stdevs": self.stdevs[:k].tolist(),
                "modal_n": k,
                "n_reads": None if self.n_reads is None else self.n_reads[:k].tolist(),
            },
        }


def call_data_from_batch(out: dict, l: int, n_alleles: int) -> CallData | None:
    """Locus l of a call_alleles_batch or call_alleles_n_batch result as CallData (None when it had too few reads).  With
    more than two peaks called no read has a peak, and n_reads is empty."""
    if int(out["status"][l]) == TOO_FEW:
        return None
    a = int(n_alleles)
    k = int(out["modal_n"][l])
    return CallData(out["call"][l, :a], out["ci95"][l, :a], out["ci99"][l, :a], out["means"][l, :a],
                    out["weights"][l, :a], out["stdevs"][l, :a], k,
                    n_reads=out["peak_n_reads"][l, :k if k <= 2 else 0], status=int(out["status"][l]))


def _param(params, name, default):
    if params is None:
        return default
    if hasattr(params, name):
        return getattr(params, name)
    gp = getattr(params, "gmm_params", None)
    return getattr(gp, name, default) if gp is not None else default


def call_alleles(repeats_fwd, repeats_rev, read_weights_fwd, read_weights_rev, params, min_reads: int, n_alleles: int,
                 separate_strands: bool, read_bias_corr_min: int, seed: int | None, logger_=None, debug_str: str = "",
                 ctx=None) -> CallData | None:
    """The reference's signature (strkit/call/allele.py:176-189).  `params` is an AlleleParams or the reference's
    CallParams (num_bootstrap, min_allele_reads, force_gm_filter, gmm_params.{n_init, filter_factor, expansion_ratio});
    `seed` is the locus seed.  The returned CallData also carries the peak assignment of the reads (in the order
    forward then reverse) as `read_peaks`."""
    repeats_fwd = np.asarray(repeats_fwd, dtype=np.int32).ravel()
    repeats_rev = np.asarray(repeats_rev, dtype=np.int32).ravel()
    if separate_strands and repeats_rev.size:
        raise NotImplementedError("separate_strands=True is not supported by the GPU allele caller")
    d = AlleleParams()
    p = AlleleParams(min_reads=int(min_reads), min_allele_reads=int(_param(params, "min_allele_reads", d.min_allele_reads)),
                     num_bootstrap=int(_param(params, "num_bootstrap", d.num_bootstrap)),
                     n_init=int(_param(params, "n_init", d.n_init)), max_iter=int(_param(params, "max_iter", d.max_iter)),
                     filter_factor=int(_param(params, "filter_factor", d.filter_factor)),
                     force_gm_filter=bool(_param(params, "force_gm_filter", d.force_gm_filter)),
                     tol=float(_param(params, "tol", d.tol)), reg_covar=float(_param(params, "reg_covar", d.reg_covar)),
                     expansion_ratio=float(_param(params, "expansion_ratio", d.expansion_ratio)))
    cns = np.concatenate((repeats_fwd, repeats_rev))
    w = np.concatenate((np.asarray(read_weights_fwd, dtype=np.float64).ravel(),
                        np.asarray(read_weights_rev, dtype=np.float64).ravel()))
    if seed is None:
        seed = int(np.random.default_rng().integers(0, 1 << 63))
    batch = call_alleles_n_batch if int(n_alleles) > 2 else call_alleles_batch
    out = batch(np.array([0, cns.shape[0]], np.int32), cns, w, [int(n_alleles)], [int(seed) & ((1 << 64) - 1)], p, ctx)
    cd = call_data_from_batch(out, 0, n_alleles)
    if cd is not None:
        cd.read_peaks = out["read_peak"].copy()
    return cd
