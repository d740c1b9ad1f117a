"""Allele sequences on the GPU: the best representative of every group of reads (strk_best_representatives, kernel
k_best_rep) and the consensus by partial-order alignment (strk_consensus, kernel k_poa).

Stands where the reference calls strkit_rust_ext.consensus_seq (strkit/call/call_locus.py:1602-1613).  Its three methods:
`single` (all reads of the allele are identical), `best_rep` (the read with the smallest summed Levenshtein distance to all
reads of the allele, the first such read on a tie) and `poa` (the heaviest path through the partial-order graph of the
reads).  best_representatives* never answer `poa`; consensus* do, for every group whose reads differ, whose median length
is at most max_mdn_poa_length and which fits the device limits.  The definitions are ours and unpinned
against STRkit, whose consensus code is not in its tree.  There is no CPU path.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from ._lib import ptr
from ._groups import group_args, pack_groups

NONE, SINGLE, BEST_REP = 0, 1, 2
POA = 3
METHOD_NAMES = ("none", "single", "best_rep", "poa")
MAX_POA_LEN = 4096       # a group with a longer string is not taken by POA
MAX_POA_NODES = 16384    # nor one whose graph grows beyond this
MAX_GROUP = 250
MAX_LEN = 65535


def best_representatives_packed(group_off, seq_start, seq_len, seqs=None, d_seqs=None, n_seq_bytes: int | None = None,
                                ctx=None, with_stats: bool = False):
    """One library call for many groups.  Group g owns sequences group_off[g]:group_off[g+1]; sequence i is the seq_len[i]
    bytes at offset seq_start[i] of `seqs` (a host buffer: bytes or a uint8 array) or of `d_seqs` (a device address, with
    n_seq_bytes its size).  Returns a dict of numpy arrays over the groups: index (inside the group, -1 for an empty one),
    method (NONE / SINGLE / BEST_REP) and dist_sum."""
    ctx = ctx or _lib.default_context()
    group_off, seq_start, seq_len, n_groups, n, h_ptr, d_ptr, _buf = group_args(group_off, seq_start, seq_len, seqs, d_seqs,
                                                                               n_seq_bytes)
    out = dict(index=np.empty(n_groups, np.int32), method=np.empty(n_groups, np.int32),
               dist_sum=np.empty(n_groups, np.int64))
    st = _lib.StrkStats()
    L = _lib.load()
    tail = (n, ptr(seq_start), ptr(seq_len), ptr(out["index"]), ptr(out["method"]), ptr(out["dist_sum"]), C.byref(st))
    if d_seqs is None:
        _lib.check(L.strk_best_representatives(ctx.handle, n_groups, ptr(group_off), h_ptr, *tail))
    else:
        _lib.check(L.strk_best_representatives_dseqs(ctx.handle, n_groups, ptr(group_off), d_ptr, *tail))
    if with_stats:
        return out, st.as_dict()
    return out


def best_representatives(groups, ctx=None) -> list[tuple[str | None, str]]:
    """(sequence, method) per group, method in "single" | "best_rep"; (None, "none") for an empty group — the pair shape of
    peaks.seqs in the reference's JSON report (docs/output_formats.md:151-153).  Strings come back as str, bytes as str
    too (ASCII)."""
    group_off, starts, lens, buf = pack_groups(groups)
    out = best_representatives_packed(group_off, starts, lens, seqs=buf, ctx=ctx)
    res: list[tuple[str | None, str]] = []
    for first, idx, meth in zip(group_off.tolist(), out["index"].tolist(), out["method"].tolist()):
        i = first + idx
        res.append((None, "none") if meth == NONE else
                   (buf[starts[i]:starts[i] + lens[i]].tobytes().decode("ascii"), METHOD_NAMES[meth]))
    return res


def consensus_packed(group_off, seq_start, seq_len, seqs=None, d_seqs=None, n_seq_bytes: int | None = None,
                     max_mdn_poa_length: int = 5000, ctx=None, with_stats: bool = False, node_limit: int = 0,
                     workspace_bytes: int = 0, cap: int | None = None):
    """One strk_consensus call for many groups, addressed as for best_representatives_packed.  Returns a dict of numpy arrays:
    index [G] (inside the group for SINGLE / BEST_REP, -1 for POA / NONE), method [G], seq_off [G + 1] and seqs (uint8: group
    g's sequence is seqs[seq_off[g]:seq_off[g+1]], whatever its method).  node_limit / workspace_bytes: the general form
    (strk_consensus_ws), 0 = the library's defaults.  cap: the size of the byte buffer offered; None asks for the size first.
    With a cap that is too small `seqs` is None and seq_off still tells the size."""
    ctx = ctx or _lib.default_context()
    group_off, seq_start, seq_len, n_groups, n, h_ptr, d_ptr, _buf = group_args(group_off, seq_start, seq_len, seqs, d_seqs,
                                                                               n_seq_bytes)
    out = dict(index=np.empty(n_groups, np.int32), method=np.empty(n_groups, np.int32),
               seq_off=np.zeros(n_groups + 1, np.int64), seqs=None)
    st = _lib.StrkStats()
    L = _lib.load()

    def call(cap_, arr):
        rc = L.strk_consensus_ws(ctx.handle, n_groups, ptr(group_off), h_ptr, d_ptr, n, ptr(seq_start), ptr(seq_len),
                                 int(max_mdn_poa_length), int(cap_), ptr(out["index"]), ptr(out["method"]), ptr(out["seq_off"]),
                                 ptr(arr), int(node_limit), int(workspace_bytes), C.byref(st))
        if rc < 0:
            _lib.check(int(rc))
        return int(rc)

    if cap is None:
        # a consensus has at most as many bytes as its graph has nodes, and the graph at most as many as the group has bytes
        arr = np.empty(max(int(seq_len.sum(dtype=np.int64)), 1), np.uint8)
        total = call(arr.shape[0], arr)
        out["seqs"] = arr[:total]
    else:
        arr = np.empty(max(int(cap), 1), np.uint8) if cap > 0 else None
        total = call(cap, arr)
        out["seqs"] = arr[:total] if arr is not None and total <= cap else (np.empty(0, np.uint8) if total == 0 else None)
    if with_stats:
        return out, st.as_dict()
    return out


def consensus(groups, max_mdn_poa_length: int = 5000, ctx=None) -> list[tuple[str | None, str]]:
    """(sequence, method) per group, method in "single" | "poa" | "best_rep"; (None, "none") for an empty group.  Sequences come
    back as str (latin-1, so that every byte value survives)."""
    group_off, starts, lens, buf = pack_groups(groups)
    out = consensus_packed(group_off, starts, lens, seqs=buf, max_mdn_poa_length=max_mdn_poa_length, ctx=ctx)
    text = out["seqs"].tobytes()
    off = out["seq_off"].tolist()
    return [(None, "none") if meth == NONE else (text[off[g]:off[g + 1]].decode("latin-1"), METHOD_NAMES[meth])
            for g, meth in enumerate(out["method"].tolist())]


def consensus_seq(seqs, logger_=None, max_mdn_poa_length: int = 0, poa: bool = False, ctx=None, method: str = "best_rep"):
    """The reference's call shape (call_locus.py:1610) for one group: (sequence, method) or None for no reads.
    `logger_`, `max_mdn_poa_length` and `poa` are accepted and ignored, as they were before partial-order alignment was built:
    with the default method="best_rep" an allele whose reads differ is its best representative.  method="poa" takes the
    consensus by partial-order alignment (consensus(), with the reference's default max_mdn_poa_length of 5000)."""
    if method == "poa":
        seq, meth = consensus([list(seqs)], ctx=ctx)[0]
    elif method == "best_rep":
        seq, meth = best_representatives([list(seqs)], ctx=ctx)[0]
    else:
        raise ValueError(f"method must be 'best_rep' or 'poa': got {method!r}")
    return None if seq is None else (seq, meth)
