"""CPU: the partial-order-alignment restatement (tests/poa_restatement.py) against the hand-sized vectors of DESIGN.md §12,
its independence of the topological order, and the quality it must reach on noisy reads of a hidden STR haplotype."""
import numpy as np
import pytest

import consensus_restatement as BR
import poa_restatement as P

VECTORS, EMPTY_VECTORS, mutate = P.VECTORS, P.EMPTY_VECTORS, P.mutate


def str_haplotype(rng) -> bytes:
    """An STR tract of 16 .. 240 bases: a motif of 2 .. 6 letters repeated, with an interruption now and then."""
    k = int(rng.integers(2, 7))
    motif = bytes(b"ACGT"[int(x)] for x in rng.integers(0, 4, k))
    while len(set(motif)) == 1:
        motif = bytes(b"ACGT"[int(x)] for x in rng.integers(0, 4, k))
    n = int(rng.integers(16, 241))
    hap = bytearray((motif * (n // k + 1))[:n])
    for _ in range(int(rng.integers(0, 3))):
        hap[int(rng.integers(0, n))] = b"ACGT"[int(rng.integers(0, 4))]
    return bytes(hap)


def read_corpus(seed: int, n_groups: int, depth: int, rate: float):
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n_groups):
        hap = str_haplotype(rng)
        out.append((hap, [mutate(rng, hap, rate) for _ in range(depth)]))
    return out


@pytest.mark.parametrize("group,expect,nodes", VECTORS)
def test_hand_vectors(group, expect, nodes):
    for order in ("min", "max"):
        gr = P.build(group.split(), order)
        assert gr.consensus() == expect.encode()
        assert nodes is None or len(gr) == nodes
    assert P.consensus(group.split())[1:3] == ("poa", expect.encode())


def test_empty_strings_vote():
    for group, expect in EMPTY_VECTORS:
        assert P.poa(group) == expect
        assert P.consensus(group) == (-1, "poa", expect, False)


def test_method_choice():
    assert P.consensus([]) == (-1, "none", None, False)
    assert P.consensus([b"CAG", b"CAG"]) == (0, "single", b"CAG", False)
    g = [b"CAGCAG", b"CAGCAT", b"CAGCAT", b"CAG"]                 # ascending lengths 3 6 6 6: the median is 6
    assert P.consensus(g, max_mdn_poa_length=6)[1] == "poa"
    assert P.consensus(g, max_mdn_poa_length=5) == (1, "best_rep", b"CAGCAT", False)
    assert P.consensus([b"CAG"] * 3, max_mdn_poa_length=0)[1] == "single"       # identical strings come first
    assert len(P.build(g)) == 7                                    # CAGCA, then G and T in one column
    assert P.consensus(g, node_limit=7) == (-1, "poa", P.poa(g), False)
    assert P.consensus(g, node_limit=6) == (1, "best_rep", b"CAGCAT", True)
    assert P.consensus([b"ACGT", b"TTTTTTTT"], node_limit=5) == (0, "best_rep", b"ACGT", True)
    assert P.consensus([b"ACGT", b"ACGA"], max_len=3) == (0, "best_rep", b"ACGT", True)


def test_topological_order_does_not_matter_and_graphs_are_acyclic():
    rng = np.random.default_rng(77)
    for k in range(120):
        alpha = (b"A", b"AC", b"ACGT", b"ACGTN", bytes(range(256)))[k % 5]
        n = int(rng.integers(2, 12))
        if k % 2:
            base = bytes(alpha[int(x)] for x in rng.integers(0, len(alpha), int(rng.integers(1, 60))))
            group = [mutate(rng, base, 0.15, 0.6, alpha) for _ in range(n)]
        else:
            group = [bytes(alpha[int(x)] for x in rng.integers(0, len(alpha), int(rng.integers(0, 40)))) for _ in range(n)]
        a, b = P.build(group, "min"), P.build(group, "max")   # (every update asserts that the graph is acyclic)
        assert a.byte == b.byte and a.pred == b.pred and a.st == b.st and a.en == b.en
        assert a.consensus() == b.consensus()


def test_quality_on_noisy_reads():
    """100 groups, depth 15, 3 % errors of which 70 % are indels, STR haplotypes of 16 .. 240 bases: the hidden haplotype
    comes back in at least 90 groups, and in strictly more groups than the best representative gives."""
    corpus = read_corpus(20261017, 100, 15, 0.03)
    n_poa = sum(P.poa(reads) == hap for hap, reads in corpus)
    n_rep = sum(reads[BR.best_representative(reads)[0]] == hap for hap, reads in corpus)
    print(f"poa {n_poa}/100, best_rep {n_rep}/100")
    assert n_poa >= 90
    assert n_poa > n_rep


def test_clean_reads_are_recovered():
    corpus = read_corpus(3, 100, 8, 0.002)
    assert sum(P.poa(reads) == hap for hap, reads in corpus) == 100
