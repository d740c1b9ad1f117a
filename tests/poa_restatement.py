"""The consensus rule of strk_consensus in plain Python / numpy (test infrastructure only).

A group is an ordered list of byte strings.  The method is chosen in this order: no string -> "none"; all strings
byte-identical -> "single", string 0; median length (element n // 2 of the ascending lengths) > max_mdn_poa_length ->
"best_rep" (tests/consensus_restatement.py); the group exceeds a device limit (a string longer than `max_len`, or a graph of
more than `node_limit` nodes) -> "best_rep"; otherwise "poa": the heaviest path through the partial-order graph of the
group's distinct strings, added in order of first occurrence with their multiplicities as weights.

Alignment of a string to the graph: global, linear gaps, match +5, mismatch -4, gap -8, integers.  Every tie is decided by
node ids, so the result does not depend on the topological order the rows are computed in (`order` chooses between two).
"""
from __future__ import annotations

import heapq

import numpy as np

import consensus_restatement as BR

MATCH, MISMATCH, GAP = 5, -4, -8
MAX_LEN, NODE_LIMIT = 4096, 16384


def _b(s) -> bytes:
    return s.encode("ascii") if isinstance(s, str) else bytes(s)


class Graph:
    def __init__(self, order: str = "min"):
        self.byte: list[int] = []
        self.pred: list[dict[int, int]] = []    # in-edges: source -> weight
        self.n_succ: list[int] = []
        self.st: list[int] = []
        self.en: list[int] = []
        self.aligned: list[list[int]] = []      # the other nodes of the column
        self.n_empty = 0
        self.cells = 0
        self.order = order

    def __len__(self) -> int:
        return len(self.byte)

    def _node(self, b: int) -> int:
        self.byte.append(b)
        self.pred.append({})
        self.n_succ.append(0)
        self.st.append(0)
        self.en.append(0)
        self.aligned.append([])
        return len(self.byte) - 1

    def _edge(self, p: int, v: int, c: int) -> None:
        if p not in self.pred[v]:
            self.pred[v][p] = 0
            self.n_succ[p] += 1
        self.pred[v][p] += c

    def topo(self) -> list[int]:
        """Kahn, smallest id first ("min") or largest id first ("max"); asserts that the graph is acyclic."""
        n = len(self)
        sign = 1 if self.order == "min" else -1
        deg = [len(p) for p in self.pred]
        succ: list[list[int]] = [[] for _ in range(n)]
        for v in range(n):
            for p in self.pred[v]:
                succ[p].append(v)
        heap = [sign * v for v in range(n) if deg[v] == 0]
        heapq.heapify(heap)
        out = []
        while heap:
            v = sign * heapq.heappop(heap)
            out.append(v)
            for u in succ[v]:
                deg[u] -= 1
                if deg[u] == 0:
                    heapq.heappush(heap, sign * u)
        assert len(out) == n, "the graph has a cycle"
        return out

    def add(self, s: bytes, c: int) -> None:
        if not s:
            self.n_empty += c
            return
        if not len(self):
            prev = -1
            for b in s:
                v = self._node(b)
                if prev >= 0:
                    self._edge(prev, v, c)
                prev = v
            self.st[0] += c
            self.en[prev] += c
            return
        path = self._align(s)
        prev = -1
        for b, v in zip(s, path):
            if v < 0:
                cur = self._node(b)
            elif self.byte[v] == b:
                cur = v
            else:
                cur = next((u for u in self.aligned[v] if self.byte[u] == b), -1)
                if cur < 0:
                    cur = self._node(b)
                    members = [v] + self.aligned[v]
                    for u in members:
                        self.aligned[u].append(cur)
                    self.aligned[cur] = members
            if prev >= 0:
                self._edge(prev, cur, c)
            else:
                self.st[cur] += c
            prev = cur
        self.en[prev] += c
        self.topo()

    def _align(self, s: bytes) -> list[int]:
        """The node every byte of s is matched to, -1 for an inserted byte."""
        L = len(s)
        sv = np.frombuffer(s, dtype=np.uint8)
        idx = np.arange(L + 1, dtype=np.int64)
        row0 = GAP * idx
        H: dict[int, np.ndarray] = {-1: row0}
        self.cells += len(self) * L
        for v in self.topo():
            preds = sorted(self.pred[v]) or [-1]
            sub = np.where(sv == self.byte[v], MATCH, MISMATCH)
            c = np.full(L + 1, -(1 << 40), dtype=np.int64)
            for p in preds:
                hp = H[p]
                np.maximum(c, hp + GAP, out=c)
                np.maximum(c[1:], hp[:-1] + sub, out=c[1:])
            H[v] = np.maximum.accumulate(c - GAP * idx) + GAP * idx
        sinks = [v for v in range(len(self)) if self.n_succ[v] == 0]
        v = min(sinks, key=lambda u: (-int(H[u][L]), u))
        j = L
        path = [-1] * L
        while v >= 0 or j > 0:
            if v < 0:
                j -= 1
                continue
            h = int(H[v][j])
            preds = sorted(self.pred[v]) or [-1]
            if j > 0:
                sub = MATCH if s[j - 1] == self.byte[v] else MISMATCH
                p = next((p for p in preds if int(H[p][j - 1]) + sub == h), None)
                if p is not None:
                    path[j - 1] = v
                    v, j = p, j - 1
                    continue
            p = next((p for p in preds if int(H[p][j]) + GAP == h), None)
            if p is not None:
                v = p
                continue
            assert j > 0 and int(H[v][j - 1]) + GAP == h
            j -= 1
        return path

    def consensus(self) -> bytes:
        n = len(self)
        score = [0] * n
        back = [-1] * n
        for v in self.topo():
            cands = [(-w, -score[p], p) for p, w in self.pred[v].items()]
            if self.st[v] > 0:
                cands.append((-self.st[v], 0, -1))
            w, sc, p = min(cands)
            score[v] = -w - sc
            back[v] = p
        ends = [(-self.en[v], -score[v], v) for v in range(n) if self.en[v] > 0]
        if self.n_empty > 0:
            ends.append((-self.n_empty, 0, -1))
        v = min(ends)[2]
        out = bytearray()
        while v >= 0:
            out.append(self.byte[v])
            v = back[v]
        return bytes(out[::-1])


def build(group, order: str = "min", node_limit: int | None = None) -> Graph | None:
    """The graph of a group's distinct strings; None once it holds more than node_limit nodes."""
    g = [_b(s) for s in group]
    count: dict[bytes, int] = {}
    for s in g:
        count[s] = count.get(s, 0) + 1
    gr = Graph(order)
    for s, c in count.items():   # dicts keep the order of first insertion
        gr.add(s, c)
        if node_limit is not None and len(gr) > node_limit:
            return None
    return gr


def poa(group, order: str = "min") -> bytes:
    return build(group, order).consensus()


def consensus(group, max_mdn_poa_length: int = 5000, node_limit: int = NODE_LIMIT, max_len: int = MAX_LEN,
              order: str = "min") -> tuple[int, str, bytes | None, bool]:
    """(index inside the group or -1, method, sequence, whether a device limit sent the group to best_rep)."""
    g = [_b(s) for s in group]
    if not g:
        return -1, "none", None, False
    if all(s == g[0] for s in g):
        return 0, "single", g[0], False
    lens = sorted(len(s) for s in g)
    limited = False
    if lens[len(g) // 2] <= max_mdn_poa_length:
        gr = build(g, order, node_limit) if lens[-1] <= max_len else None
        if gr is not None:
            return -1, "poa", gr.consensus(), False
        limited = True
    i = BR.best_representative(g)[0]
    return i, "best_rep", g[i], limited


# ---- shared by the tests: the hand-sized vectors of DESIGN.md §12 and the read-error model
# group, consensus, nodes of the graph (None: not pinned)
VECTORS = [
    ("ACGT ACGT AGGT", "ACGT", None),
    ("AAAA AAAT", "AAAA", None),
    ("AAAT AAAA AAAT AAAA", "AAAT", None),
    ("ACGT ACT AGT", "ACGT", 4),
    ("TACGT ACGT ACGT ACGTT", "ACGT", None),
    ("GATTACA GATCACA GATTACA GACTACA GATTAA", "GATTACA", None),
    ("CAGCAG CAGCAGCAG CAGCAGCAG", "CAGCAGCAG", None),
    ("acgt ACGT ACGT", "ACGT", 8),
    ("AXB AYB AZB", "AXB", None),
]
EMPTY_VECTORS = [([b"", b"A"], b"A"), ([b"", b"", b"A"], b"")]


def mutate(rng, s: bytes, rate: float, indel: float = 0.7, alpha: bytes = b"ACGT") -> bytes:
    """Every position is hit with probability `rate`: a deletion or an insertion before it (share `indel`, half each), or a
    substitution by another letter."""
    out = bytearray()
    hit = rng.random(len(s)) < rate
    for i, ch in enumerate(s):
        if not hit[i]:
            out.append(ch)
            continue
        r = rng.random()
        if r < indel / 2:
            continue
        if r < indel:
            out.append(alpha[int(rng.integers(0, len(alpha)))])
            out.append(ch)
            continue
        others = bytes(b for b in alpha if b != ch) or alpha
        out.append(others[int(rng.integers(0, len(others)))])
    return bytes(out)
