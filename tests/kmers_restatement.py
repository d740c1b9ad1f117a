"""CPU restatement of the k-mer count of a group: what strk_count_kmers must return, word for word.  Test
infrastructure, not part of the package: a Counter over the windows, sorted, with the place of every first occurrence."""
from __future__ import annotations

from collections import Counter


def _b(s) -> bytes:
    return s.encode("latin-1") if isinstance(s, str) else bytes(s)


def windows(s, k: int) -> list[bytes]:
    s = _b(s)
    return [s[i:i + k] for i in range(len(s) - k + 1)]


def n_windows(group, k: int) -> int:
    return sum(max(len(_b(s)) - k + 1, 0) for s in group)


def count_group(group, k: int) -> list[tuple[bytes, int, tuple[int, int]]]:
    """[(window, count, (string index, i) of the first occurrence)] in ascending unsigned byte order of the windows."""
    if k < 1:
        raise ValueError("k must be at least 1")
    count: Counter = Counter()
    first: dict[bytes, tuple[int, int]] = {}
    for si, s in enumerate(group):
        for i, w in enumerate(windows(s, k)):
            count[w] += 1
            first.setdefault(w, (si, i))
    return [(w, count[w], first[w]) for w in sorted(count)]      # bytes compare as unsigned bytes


def count_dict(group, k: int) -> dict[bytes, int]:
    return {w: c for w, c, _ in count_group(group, k)}


def count_packed(group_off, seq_start, seq_len, k, buf) -> tuple[list[int], list[int], list[int]]:
    """The library's three arrays for groups of slices of `buf`: entry_off, pos (offset of the first occurrence), count."""
    buf = bytes(buf)
    entry_off, pos, cnt = [0], [], []
    for g in range(len(group_off) - 1):
        idx = range(int(group_off[g]), int(group_off[g + 1]))
        group = [buf[int(seq_start[i]):int(seq_start[i]) + int(seq_len[i])] for i in idx]
        for _w, c, (si, i) in count_group(group, int(k[g])):
            pos.append(int(seq_start[idx[si]]) + i)
            cnt.append(c)
        entry_off.append(len(pos))
    return entry_off, pos, cnt
