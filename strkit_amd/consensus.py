"""Allele sequences on the GPU: the best representative of every group of reads (strk_best_representatives, kernel k_best_rep).

Stands where the reference calls strkit_rust_ext.consensus_seq (strkit/call/call_locus.py:1602-1613).  Two of its three
methods exist here: `single` (all reads of the allele are identical) and `best_rep` (the read with the smallest summed
Levenshtein distance to all reads of the allele, the first such read on a tie).  Partial-order alignment (`poa`) is not
built: every allele whose reads differ is reported as `best_rep`.  The definition is ours and unpinned
against STRkit, whose consensus code is not in its tree.  There is no CPU path.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib

NONE, SINGLE, BEST_REP = 0, 1, 2
METHOD_NAMES = ("none", "single", "best_rep")
MAX_GROUP = 250
MAX_LEN = 65535


def _ptr(a: np.ndarray) -> C.c_void_p:
    return C.c_void_p(a.ctypes.data)


def best_representatives_packed(group_off, seq_start, seq_len, seqs=None, d_seqs=None, n_seq_bytes: int | None = None,
                                ctx=None, with_stats: bool = False):
    """One library call for many groups.  Group g owns sequences group_off[g]:group_off[g+1]; sequence i is the seq_len[i]
    bytes at offset seq_start[i] of `seqs` (a host buffer: bytes or a uint8 array) or of `d_seqs` (a device address, with
    n_seq_bytes its size).  Returns a dict of numpy arrays over the groups: index (inside the group, -1 for an empty one),
    method (NONE / SINGLE / BEST_REP) and dist_sum."""
    ctx = ctx or _lib.default_context()
    group_off = np.ascontiguousarray(group_off, dtype=np.int32)
    seq_start = np.ascontiguousarray(seq_start, dtype=np.int64)
    seq_len = np.ascontiguousarray(seq_len, dtype=np.int32)
    n_groups = group_off.shape[0] - 1
    if n_groups < 0 or seq_start.shape != seq_len.shape or seq_start.ndim != 1:
        raise ValueError("group_off needs at least one entry, and seq_start and seq_len one entry per sequence")
    if n_groups and int(group_off[-1]) != seq_start.shape[0]:
        raise ValueError("group_off must span seq_start / seq_len")
    if (seqs is None) == (d_seqs is None):
        raise ValueError("exactly one of seqs (host) and d_seqs (device) must be given")
    out = dict(index=np.empty(n_groups, np.int32), method=np.empty(n_groups, np.int32),
               dist_sum=np.empty(n_groups, np.int64))
    st = _lib.StrkStats()
    L = _lib.load()
    tail = (_ptr(seq_start), _ptr(seq_len), _ptr(out["index"]), _ptr(out["method"]), _ptr(out["dist_sum"]), C.byref(st))
    if d_seqs is None:
        buf = np.frombuffer(seqs, dtype=np.uint8) if isinstance(seqs, (bytes, bytearray, memoryview)) else \
            np.ascontiguousarray(seqs, dtype=np.uint8)
        n = buf.shape[0] if n_seq_bytes is None else int(n_seq_bytes)
        if n > buf.shape[0]:
            raise ValueError("n_seq_bytes exceeds the buffer")
        _lib.check(L.strk_best_representatives(ctx.handle, n_groups, _ptr(group_off), _ptr(buf), n, *tail))
    else:
        if n_seq_bytes is None:
            raise ValueError("d_seqs needs n_seq_bytes")
        _lib.check(L.strk_best_representatives_dseqs(ctx.handle, n_groups, _ptr(group_off), C.c_void_p(int(d_seqs)),
                                                     int(n_seq_bytes), *tail))
    if with_stats:
        return out, st.as_dict()
    return out


def _as_bytes(s) -> bytes:
    return s.encode("ascii") if isinstance(s, str) else bytes(s)


def best_representatives(groups, ctx=None) -> list[tuple[str | None, str]]:
    """(sequence, method) per group, method in "single" | "best_rep"; (None, "none") for an empty group — the pair shape of
    peaks.seqs in the reference's JSON report (docs/output_formats.md:151-153).  Strings come back as str, bytes as str
    too (ASCII)."""
    flat = [[_as_bytes(s) for s in g] for g in groups]
    lens = np.fromiter((len(s) for g in flat for s in g), dtype=np.int32, count=sum(len(g) for g in flat))
    starts = np.zeros(lens.shape[0], np.int64)
    if lens.shape[0]:
        np.cumsum(lens[:-1], out=starts[1:])
    group_off = np.zeros(len(flat) + 1, np.int32)
    np.cumsum([len(g) for g in flat], out=group_off[1:])
    buf = np.frombuffer(b"".join(s for g in flat for s in g), dtype=np.uint8)
    out = best_representatives_packed(group_off, starts, lens, seqs=buf, ctx=ctx)
    res: list[tuple[str | None, str]] = []
    for g, idx, meth in zip(flat, out["index"].tolist(), out["method"].tolist()):
        res.append((None, "none") if meth == NONE else (g[idx].decode("ascii"), METHOD_NAMES[meth]))
    return res


def consensus_seq(seqs, logger_=None, max_mdn_poa_length: int = 0, poa: bool = False, ctx=None):
    """The reference's call shape (call_locus.py:1610) for one group: (sequence, method) or None for no reads.
    `logger_`, `max_mdn_poa_length` and `poa` are accepted and ignored: partial-order alignment is not built, an allele
    whose reads differ is always its best representative."""
    seq, method = best_representatives([list(seqs)], ctx=ctx)[0]
    return None if seq is None else (seq, method)
