"""K-mer counts on the GPU: the distinct windows of every group of sequences (strk_count_kmers, kernels k_kmers_hash and
k_kmers_sort).

Stands where the reference counts motif-sized k-mers per read (strkit/call/call_locus.py:1287) and per allele
(:1526-1593, :1635).  A group is an ordered list of byte strings with one window length k; the result has one entry per
distinct window s[i : i + k]: its count over all strings of the group and the place of its first occurrence (smallest string
index, then smallest i), the entries in ascending unsigned byte order.  Raw bytes, case-sensitive, exact.  The definition is
ours and unpinned against STRkit, whose counter is not in its tree.  There is no CPU path.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from ._lib import ptr
from ._groups import group_args, pack_groups

MAX_GROUP = 250
MAX_LEN = 65535
EAGER_ENTRIES = 1 << 22     # a-priori bound (all windows) up to which the arrays are allocated at once; beyond: size query first


def count_kmers_packed(group_off, seq_start, seq_len, k, seqs=None, d_seqs=None, n_seq_bytes: int | None = None, ctx=None,
                       with_stats: bool = False, workspace_bytes: int | None = None):
    """One library call for many groups.  Group g owns sequences group_off[g]:group_off[g+1] and the window length k[g];
    sequence i is the seq_len[i] bytes at offset seq_start[i] of `seqs` (a host buffer: bytes or a uint8 array) or of `d_seqs`
    (a device address, with n_seq_bytes its size).  Returns a dict of numpy arrays: entry_off [n_groups + 1], and per entry
    pos (offset into the buffer of the window's first occurrence) and count; the entries of group g are
    entry_off[g]:entry_off[g+1], in ascending byte order of their windows.  `workspace_bytes` bounds the device workspace of one
    launch (None: the library's default); the result does not depend on it."""
    ctx = ctx or _lib.default_context()
    shapes = "group_off needs at least one entry, seq_start and seq_len one entry per sequence, k one per group"
    group_off, seq_start, seq_len, n_groups, n, h_seqs, dev, _buf = group_args(group_off, seq_start, seq_len, seqs, d_seqs,
                                                                               n_seq_bytes, shapes=shapes)
    k = np.ascontiguousarray(k, dtype=np.int32)
    if k.shape != (n_groups,):
        raise ValueError(shapes)
    entry_off = np.zeros(n_groups + 1, np.int64)
    st = _lib.StrkStats()
    L = _lib.load()

    def call(cap: int, pos, count) -> int:
        rc = L.strk_count_kmers_ws(ctx.handle, n_groups, ptr(group_off), h_seqs, dev, n, ptr(seq_start), ptr(seq_len), ptr(k),
                                   cap, ptr(entry_off), ptr(pos), ptr(count), int(workspace_bytes or 0), C.byref(st))
        if rc < 0:
            _lib.check(int(rc))
        return int(rc)

    # every window distinct is the most there can be: allocate that when it is small, else ask first
    k_seq = np.repeat(k, np.diff(group_off)) if n_groups else np.zeros(0, np.int32)
    bound = int(np.maximum(seq_len.astype(np.int64) - k_seq + 1, 0).sum()) if n_groups else 0
    cap = bound if bound <= EAGER_ENTRIES else 0
    pos, count = np.empty(cap, np.int64), np.empty(cap, np.int32)
    n_entries = call(cap, pos if cap else None, count if cap else None)
    kernel_ms, launches = st.kernel_ms, st.n_dp_launches
    if n_entries > cap:
        cap = n_entries
        pos, count = np.empty(cap, np.int64), np.empty(cap, np.int32)
        n_entries = call(cap, pos, count)
        kernel_ms, launches = kernel_ms + st.kernel_ms, launches + st.n_dp_launches
    out = dict(entry_off=entry_off, pos=pos[:n_entries], count=count[:n_entries])
    if with_stats:
        d = st.as_dict()
        d["kernel_ms"], d["n_dp_launches"] = kernel_ms, launches     # both calls of a retry
        return out, d
    return out


def count_kmers(groups, k, ctx=None) -> list[dict[bytes, int]]:
    """{window: count} per group, the keys in ascending byte order.  `groups`: lists of bytes (or ASCII str); `k`: one window
    length for all groups or one per group."""
    group_off, starts, lens, buf = pack_groups(groups)
    ks = np.full(group_off.shape[0] - 1, k, np.int32) if np.isscalar(k) else np.asarray(k, np.int32)
    out = count_kmers_packed(group_off, starts, lens, ks, seqs=buf, ctx=ctx)
    return dicts_of(out, ks, buf.tobytes())


def dicts_of(out: dict, k, text, first: int = 0, last: int | None = None) -> list[dict]:
    """count_kmers_packed's arrays as one {window: count} per group first..last, cut out of the host copy of the buffer
    (`text`: bytes, or their str form, one character per byte, for str keys)."""
    eo = out["entry_off"].tolist()
    last = len(eo) - 1 if last is None else last
    pos, cnt = out["pos"][eo[first]:eo[last]].tolist(), out["count"][eo[first]:eo[last]].tolist()
    base = eo[first]
    res = []
    for g in range(first, last):
        kg = int(k[g])
        a, b = eo[g] - base, eo[g + 1] - base
        res.append({text[p:p + kg]: c for p, c in zip(pos[a:b], cnt[a:b])})
    return res
