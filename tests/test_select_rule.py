"""CPU: the read-selection rule.  frontend/select.py's readable statement and the library's host entry
strk_select_reads against tests/select_restatement.py on the corpus of tests/select_cases.py; rules == 0 against fetch_many's
cap; the input check's refusals; and that the corpus holds the shapes it is meant to hold."""
import ctypes as C
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest

from select_cases import CAP_LOCUS, NO_CAP, caps, corpus, expected
from select_restatement import select
from strkit_amd import _lib
from strkit_amd.frontend.native import NativeBam
from strkit_amd.frontend.select import select_items, select_reads, select_segments

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def bam(tmp_path_factory):
    return NativeBam(corpus().write(str(tmp_path_factory.mktemp("select") / "corpus.bam")))


def test_the_corpus_holds_the_shapes(bam):
    c = corpus()
    k = c.constants
    assert k["small_items"] >= 1024 and k["small_slots"] == 2 * k["small_items"] and k["threads"] % 64 == 0 and k["compare_step"] >= 1
    assert bam.n_records == len(c.names) and 2000 < len(c.names) < 6000
    assert [int(x) for x in bam.flag] == c.flags
    cls, step = k["small_items"], k["compare_step"]
    for n in (0, 1, 2, 63, 64, 65, 255, 256, 257, cls - 1, cls, cls + 1):
        assert len(c.loci[f"size_{n}"]) == n
    for key, idx in c.loci.items():
        assert list(idx) == sorted(idx), key                      # items in file order
    assert len({c.names[i] for i in c.loci["large_many_names"]}) > k["small_slots"] and len(c.loci["large_many_names"]) > cls
    assert len({c.names[i] for i in c.loci["one_name"]}) == 1 and len(c.loci["one_name"]) > 64
    # every name exactly twice, the two more than 256 items apart
    names = [c.names[i] for i in c.loci["twice_far"]]
    where = {}
    for p, n in enumerate(names):
        where.setdefault(n, []).append(p)
    assert all(len(v) == 2 and v[1] - v[0] > 256 for v in where.values())
    # repeated names inside the sized loci, near (adjacent) and far (more than 64 apart), and a name shared by two loci
    for key in ("size_257", f"size_{cls}", f"size_{cls + 1}"):
        at = {}
        for p, n in enumerate(c.names[i] for i in c.loci[key]):
            at.setdefault(n, []).append(p)
        gaps = [v[1] - v[0] for v in at.values() if len(v) > 1]
        assert 1 in gaps and max(gaps) > 64, key
    assert set(c.names[i] for i in c.loci["size_64"]) <= set(c.names[i] for i in c.loci["size_257"])
    # name shapes
    shapes = {c.names[i] for i in c.loci["shapes"]}
    lens = {len(s) for s in shapes}
    assert {0, 1, 254, step - 1, step, step + 1, 2 * step} <= lens
    assert set(range(1, 256)) <= {b for s in shapes for b in s}
    assert any(a != b and len(a) == len(b) and a[:-1] == b[:-1] for a in shapes for b in shapes if len(a) > 1)     # all but the last byte
    assert any(a != b and len(a) == len(b) and a[1:] == b[1:] for a in shapes for b in shapes if len(a) > 1)       # all but the first
    assert any(a != b and b.startswith(a) and a for a in shapes for b in shapes)                                     # a proper prefix
    # record offsets at all four residues mod 4
    assert set((bam.rec_off % 4).tolist()) == {0, 1, 2, 3}
    # flags
    f = lambda key: [c.flags[i] for i in c.loci[key]]  # noqa: E731
    assert f("supp_only") == [0x800] and f("primary_supp") == [0, 0x800] and f("supp_primary")[0] == 0x800 and not f("supp_primary")[1] & 0x900
    assert f("primary_sec") == [0, 0x100] and f("sec_supp") == [0x100, 0x800] and f("sec_primary") == [0x100, 0] and 0x900 in f("both_bits")


def test_restatement_on_the_flag_cases():
    c = corpus()
    for rules in range(8):
        r, s, n = select(c.items("supp_only"), rules, 250)
        assert s == [2] and r == [1 if rules & 1 else 0] and n == (0 if rules & 1 else 1)             # status 2: never chimeric
        r, s, n = select(c.items("supp_primary"), rules, 250)
        assert s == [3, 3]
        assert r == ([1, 0] if rules & 1 else ([0, 3] if rules & 4 else [0, 0]))      # a flag-skipped first occurrence shadows nothing
        r, s, n = select(c.items("primary_supp"), rules, 250)
        assert s == [3, 3] and r == [0, 1 if rules & 1 else (3 if rules & 4 else 0)]
        r, s, n = select(c.items("primary_sec"), rules, 250)
        assert s == [1, 1] and r == [0, 2 if rules & 2 else (3 if rules & 4 else 0)]
        r, s, n = select(c.items("both_bits"), rules, 250)
        assert r[0] == (1 if rules & 1 else (2 if rules & 2 else 0)) and s == [3, 3, 2]


def test_python_statement_equals_the_restatement():
    c = corpus()
    for key in c.loci:
        items = c.items(key)
        segs = [SimpleNamespace(name=n, flag=f, k=k) for k, (n, f) in enumerate(items)]
        for rules in range(8):
            for cap in (1, 7, NO_CAP) if key != CAP_LOCUS else caps(c, rules):
                reason, status, n = select(items, rules, cap)
                kept, st = select_segments(segs, rules, cap)
                assert [s.k for s in kept] == [k for k, r in enumerate(reason) if r == 0] and len(kept) == n, (key, rules, cap)
                assert st == [status[s.k] for s in kept]


def test_host_entry_equals_the_restatement(bam):
    c = corpus()
    loci = list(c.loci)
    item_off, rec_off = c.item_arrays(bam.rec_off, loci)
    for rules in range(8):
        for cap in caps(c, rules):
            reason, status, n_kept = select_items(bam, rec_off, item_off, rules, cap)
            e_reason, e_status, e_kept = expected(c, loci, rules, cap)
            assert np.array_equal(n_kept, e_kept), (rules, cap)
            assert np.array_equal(reason, e_reason) and np.array_equal(status, e_status), (rules, cap)


def test_rules_0_is_fetch_many_with_its_cap(bam):
    starts = np.array([0, 5, 1000, 2995, 20000, 10 * bam.n_records], np.int64)
    ends = np.array([700, 6, 9000, 3005, 20010, 10 * bam.n_records + 50], np.int64)
    for cap in (1, 3, 100, 250):
        rec, counts = bam.fetch_many("chr1", starts, ends, cap)
        all_rec, all_counts = bam.fetch_many("chr1", starts, ends, NO_CAP)
        assert all_counts.max() > 250
        got_rec, got_counts, _ = select_reads(bam, all_rec, all_counts, 0, cap)
        assert np.array_equal(got_rec, rec) and np.array_equal(got_counts, counts)


def _call(bam, item_off, rec_off, rules=4, max_reads=250, n_bytes=None):
    L = _lib.load()
    item_off, rec_off = np.asarray(item_off, np.int64), np.asarray(rec_off, np.int64)
    n = max(int(rec_off.size), 1)
    reason, status, kept = np.zeros(n, np.uint8), np.zeros(n, np.uint8), np.zeros(max(item_off.size - 1, 1), np.int32)
    rc = L.strk_select_reads(bam.data.ctypes.data, bam.data.size if n_bytes is None else n_bytes, item_off.size - 1, item_off.ctypes.data,
                             rec_off.ctypes.data, rules, max_reads, reason.ctypes.data, status.ctypes.data, kept.ctypes.data)
    return rc, L.strk_last_error().decode()


def test_the_input_check_refuses(bam):
    off = bam.rec_off[:6].copy()
    assert _call(bam, [0, 3, 6], off)[0] == 0
    rc, msg = _call(bam, [0, 4, 3], off)
    assert rc == _lib.STRK_E_INVALID and "item_off" in msg and "locus 1" in msg
    rc, msg = _call(bam, [1, 3, 6], off)
    assert rc == _lib.STRK_E_INVALID and "item_off" in msg
    rc, msg = _call(bam, [0, 3, 6], off, max_reads=0)
    assert rc == _lib.STRK_E_INVALID and "max_reads" in msg
    for rules in (-1, 8):
        rc, msg = _call(bam, [0, 3, 6], off, rules=rules)
        assert rc == _lib.STRK_E_INVALID and "rules" in msg
    for bad, what in ((int(off[4]) + 5, "malformed"), (bam.data.size, "outside"), (bam.data.size - 8, "outside"), (-1, "outside"),
                      (1 << 62, "outside")):
        x = off.copy()
        x[4] = bad
        rc, msg = _call(bam, [0, 3, 6], x)
        assert rc == _lib.STRK_E_INVALID and "item 4" in msg and what in msg, (bad, msg)
    # a stream cut inside the last record of the call: refused, and nothing behind the cut is read
    rc, msg = _call(bam, [0, 3, 6], off, n_bytes=int(off[5]) + 40)
    assert rc == _lib.STRK_E_INVALID and "item 5" in msg
    assert _call(bam, [0], np.zeros(0, np.int64))[0] == 0            # no locus: valid


def test_two_malformed_records_name_the_first(bam):
    """9 000 items in loci of 90, drawn with repetition from the first records: two threads take them 4 096 at a time where
    there are two cores.  Items 5 000 and 7, in different chunks, point into the middle of a record (five bytes in, as above):
    the call names item 7."""
    n = 9000
    off = bam.rec_off[np.random.default_rng(30).integers(0, 64, n)].copy()
    item_off = np.arange(0, n + 1, 90)
    off[[5000, 7]] += 5
    for _ in range(3):
        assert _call(bam, item_off, off) == (_lib.STRK_E_INVALID, "strk_select_reads: item 7: malformed BAM record")
    off[7] -= 5
    assert _call(bam, item_off, off) == (_lib.STRK_E_INVALID, "strk_select_reads: item 5000: malformed BAM record")
    off[5000] -= 5
    assert _call(bam, item_off, off)[0] == 0


def test_declared_bound_and_exported():
    text = open(os.path.join(ROOT, "include", "strkit_amd.h")).read()
    L = _lib.load()
    for name in ("strk_select_reads", "strk_dbam_select_reads", "strk_select_constants"):
        assert re.search(r"\b%s\(" % name, text) and name in _lib.EXPORTS and hasattr(L, name)
    out = (C.c_int32 * 4)()
    L.strk_select_constants(out)
    assert list(out) == list(corpus().constants.values())
