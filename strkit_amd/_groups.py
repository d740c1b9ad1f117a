"""Groups of byte strings as best_representatives*, consensus* and count_kmers* take them: group g owns sequences
group_off[g]:group_off[g+1]; sequence i is the seq_len[i] bytes at offset seq_start[i] of one buffer, which lies on the host
(`seqs`) or on the device (`d_seqs`, with n_seq_bytes its size).  Packing lists of strings into that form, and the opening the
three *_packed functions share.  No library call in here."""
from __future__ import annotations

import ctypes as C

import numpy as np


def pack_groups(groups):
    """Lists of bytes (or ASCII str) -> (group_off int32 [G + 1], starts int64 [S], lens int32 [S], buf uint8): the strings laid
    end to end in order."""
    flat = [[s.encode("ascii") if isinstance(s, str) else bytes(s) for s in g] for g in groups]
    lens = np.fromiter((len(s) for g in flat for s in g), dtype=np.int32, count=sum(len(g) for g in flat))
    starts = np.zeros(lens.shape[0], np.int64)
    if lens.shape[0]:
        np.cumsum(lens[:-1], out=starts[1:])
    group_off = np.zeros(len(flat) + 1, np.int32)
    np.cumsum([len(g) for g in flat], out=group_off[1:])
    return group_off, starts, lens, np.frombuffer(b"".join(s for g in flat for s in g), dtype=np.uint8)


SHAPES = "group_off needs at least one entry, and seq_start and seq_len one entry per sequence"


def group_args(group_off, seq_start, seq_len, seqs, d_seqs, n_seq_bytes, shapes: str = SHAPES):
    """The arguments of a *_packed call, coerced and checked: (group_off, seq_start, seq_len, n_groups, n, h_ptr, d_ptr, buf) with
    n the buffer's size in bytes, h_ptr / d_ptr the host and the device address as ctypes pointers (one of them NULL) and buf the
    host buffer as a uint8 array (None with d_seqs), which keeps h_ptr alive.  `shapes`: what a caller with more arrays than
    these three says about a wrong shape."""
    group_off = np.ascontiguousarray(group_off, dtype=np.int32)
    seq_start = np.ascontiguousarray(seq_start, dtype=np.int64)
    seq_len = np.ascontiguousarray(seq_len, dtype=np.int32)
    n_groups = group_off.shape[0] - 1
    if n_groups < 0 or seq_start.shape != seq_len.shape or seq_start.ndim != 1:
        raise ValueError(shapes)
    if n_groups and int(group_off[-1]) != seq_start.shape[0]:
        raise ValueError("group_off must span seq_start / seq_len")
    if (seqs is None) == (d_seqs is None):
        raise ValueError("exactly one of seqs (host) and d_seqs (device) must be given")
    if d_seqs is None:
        buf = np.frombuffer(seqs, dtype=np.uint8) if isinstance(seqs, (bytes, bytearray, memoryview)) else \
            np.ascontiguousarray(seqs, dtype=np.uint8)
        n = buf.shape[0] if n_seq_bytes is None else int(n_seq_bytes)
        if n > buf.shape[0]:
            raise ValueError("n_seq_bytes exceeds the buffer")
        return group_off, seq_start, seq_len, n_groups, n, C.c_void_p(buf.ctypes.data if buf.size else None), C.c_void_p(None), buf
    if n_seq_bytes is None:
        raise ValueError("d_seqs needs n_seq_bytes")
    return group_off, seq_start, seq_len, n_groups, int(n_seq_bytes), C.c_void_p(None), C.c_void_p(int(d_seqs)), None
