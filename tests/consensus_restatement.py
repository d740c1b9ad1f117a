"""The best-representative rule of strk_best_representatives in plain Python / numpy (test infrastructure only).

A group is an ordered list of byte strings.  No string: (-1, "none", 0).  All strings byte-identical: (0, "single", 0).
Otherwise D(i) = sum_j lev(s_i, s_j) over all strings of the group, duplicates counted as often as they occur; the answer is
the smallest i with minimal D(i), method "best_rep", and D(i).  lev: unit-cost Levenshtein distance on raw bytes.
"""
from __future__ import annotations

import numpy as np


def _b(s) -> bytes:
    return s.encode("ascii") if isinstance(s, str) else bytes(s)


def lev_plain(a, b) -> int:
    """The textbook double loop."""
    a, b = _b(a), _b(b)
    prev = list(range(len(b) + 1))
    for i in range(1, len(a) + 1):
        cur = [i] + [0] * len(b)
        for j in range(1, len(b) + 1):
            cur[j] = min(prev[j] + 1, cur[j - 1] + 1, prev[j - 1] + (a[i - 1] != b[j - 1]))
        prev = cur
    return prev[len(b)]


def lev(a, b) -> int:
    """Row by row, each row vectorised: with c[j] the best of the substitution and deletion candidates,
    D[j] = min(c[j], D[j-1] + 1) is minimum.accumulate(c - j) + j."""
    a, b = _b(a), _b(b)
    if len(a) < len(b):
        a, b = b, a   # rows over the longer string, the vector over the shorter one
    n = len(b)
    if n == 0:
        return len(a)
    bv = np.frombuffer(b, dtype=np.uint8)
    idx = np.arange(n + 1, dtype=np.int64)
    row = idx.copy()
    c = np.empty(n + 1, dtype=np.int64)
    for i, ch in enumerate(a, 1):
        c[0] = i
        np.minimum(row[:-1] + (bv != ch), row[1:] + 1, out=c[1:])
        row = np.minimum.accumulate(c - idx) + idx
    return int(row[n])


def best_representative(group, lev_fn=lev) -> tuple[int, str, int]:
    """(index inside the group, method, distance sum)."""
    g = [_b(s) for s in group]
    if not g:
        return -1, "none", 0
    if all(s == g[0] for s in g):
        return 0, "single", 0
    first: dict[bytes, int] = {}
    for i, s in enumerate(g):
        first.setdefault(s, i)
    uniq = sorted(first.values())
    count = {i: sum(1 for s in g if s == g[i]) for i in uniq}
    dist = {i: 0 for i in uniq}
    for x, i in enumerate(uniq):
        for j in uniq[x + 1:]:
            d = lev_fn(g[i], g[j])
            dist[i] += d * count[j]
            dist[j] += d * count[i]
    best = min(uniq, key=lambda i: (dist[i], i))
    return best, "best_rep", dist[best]
