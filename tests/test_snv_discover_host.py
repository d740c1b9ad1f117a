"""CPU: strk_discover_snvs (the host twin of k_snv_pileup / k_snv_pick) gives the rule's cand_off / cand_pos on the whole corpus
of snv_discover_cases.py under both windows; the size query; every refusal of its checker; the symbol is exported."""
import numpy as np
import pytest

import snv_discover_cases as cases
from strkit_amd import _lib
from strkit_amd.frontend import NativeBam, write_bam
from strkit_amd.frontend import snv_discovery as sd


@pytest.fixture(scope="module")
def bam(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("snv_discover_host") / "corpus.bam")
    write_bam(path, [cases.CONTIG], cases.corpus()["records"])
    return NativeBam(path)


@pytest.mark.parametrize("window", cases.WINDOWS)
def test_the_host_function_gives_the_rule(bam, window):
    want_off, want_pos = cases.expected(window)
    off, pos = cases.library(bam, window)
    assert np.array_equal(off, want_off), [lc["name"] for lc, a, b in zip(cases.corpus()["loci"], np.diff(off), np.diff(want_off)) if a != b]
    assert np.array_equal(pos, want_pos)
    assert off.dtype == np.int32 and pos.dtype == np.int64 and int(np.diff(off).max()) == 1024


def _raw(bam, **over):
    """One call of the C function over the corpus with arguments replaced by name -> (return value, cand_off, cand_pos)."""
    c = cases.corpus()
    a = {"buf": bam.data, "n_bytes": int(bam.data.size), "n_items": int(c["item_locus"].size),
         "rec_off": np.ascontiguousarray(bam.rec_off[c["item_file_index"]], np.int64), "item_locus": c["item_locus"], "n_loci": c["n_loci"],
         "left": c["left"], "right": c["right"], "kept_off": c["kept_off"], "kept_item": c["kept_item"], "alt_cigar": None, "alt_off": None,
         "alt_start": None, "clip": 100, "take_in": 250, "window": 8192, "mbq": 20, "mar": 2, "cap": 1 << 16}
    a.update(over)
    n_loci = max(int(a["n_loci"]), 0)
    off = a.get("out_off", np.full(n_loci + 1, -7, np.int32))
    pos = a.get("out_pos", np.full(max(int(a["cap"]), 1), -7, np.int64))
    p = lambda x: None if x is None else _lib.ptr(x)  # noqa: E731
    rc = _lib.load().strk_discover_snvs(p(a["buf"]), a["n_bytes"], a["n_items"], p(a["rec_off"]), p(a["item_locus"]), a["n_loci"], p(a["left"]),
                                        p(a["right"]), p(a["kept_off"]), p(a["kept_item"]), p(a["alt_cigar"]), p(a["alt_off"]), p(a["alt_start"]),
                                        a["clip"], a["take_in"], a["window"], a["mbq"], a["mar"], p(off), p(pos), a["cap"])
    return int(rc), off, pos


def test_size_query(bam):
    want_off, want_pos = cases.expected(8192)
    c = cases.corpus()
    alt_cigar, alt_off, alt_start = __import__("strkit_amd.frontend.native", fromlist=["alt_arrays"]).alt_arrays(int(c["item_locus"].size), c["alt"])
    alt = {"alt_cigar": alt_cigar, "alt_off": alt_off, "alt_start": alt_start}
    total = int(want_off[-1])
    rc, off, pos = _raw(bam, cap=total - 1, **alt)
    assert rc == total and np.array_equal(off, want_off) and (pos == -7).all()         # told the size, the offsets filled, no position written
    rc, off, pos = _raw(bam, cap=total, **alt)
    assert rc == total and np.array_equal(pos[:total], want_pos)
    rc, off, pos = _raw(bam, cap=0, out_pos=None, **alt)
    assert rc == total and np.array_equal(off, want_off)
    # no locus, no item
    rc, off, _ = _raw(bam, n_loci=0, n_items=0, kept_off=np.zeros(1, np.int32))
    assert rc == 0 and off.tolist() == [0]
    rc, off, _ = _raw(bam, n_items=0, kept_off=np.zeros(cases.corpus()["n_loci"] + 1, np.int32))
    assert rc == 0 and not off.any()


def test_refusals(bam):
    c = cases.corpus()
    L = _lib.load()

    def refused(needle, **over):
        rc, _, _ = _raw(bam, **over)
        assert rc == _lib.STRK_E_INVALID and needle.encode() in L.strk_last_error(), (needle, rc, L.strk_last_error())

    refused("bad argument", cap=-1)
    refused("bad argument", out_off=None)
    refused("< 0", n_items=-1)
    refused("< 0", n_loci=-1)
    refused("< 0", n_bytes=-1)
    refused("NULL", left=None)
    refused("NULL", rec_off=None)
    refused("NULL", item_locus=None)
    refused("NULL", buf=None)
    refused("kept_off must be given", kept_off=None)
    refused("NULL", kept_item=None)
    refused("NULL", out_pos=None)              # (room for the candidates and no place to put them; with too little room it is a size query)
    refused(">= 0", clip=-1)
    refused(">= 0", take_in=-1)
    for w in (0, -5, sd.MAX_WINDOW + 1):
        refused("window must be in 1 .. 65536", window=w)
    for q in (-1, 256):
        refused("min_base_qual must be in 0 .. 255", mbq=q)
    refused("min_allele_reads", mar=0)
    left = c["left"].copy()
    left[7] = c["right"][7] + 1
    refused("locus 7: left_coord > right_coord", left=left)
    right = c["right"].copy()
    right[3] = 1 << 41
    refused("locus 3: coordinate", right=right)
    off = np.ascontiguousarray(bam.rec_off[c["item_file_index"]], np.int64)
    for bad in (-1, int(bam.data.size) - 3, 1 << 62):
        o = off.copy()
        o[5] = bad
        refused("item 5: rec_off outside the buffer", rec_off=o)
    loc = c["item_locus"].copy()
    loc[2] = c["n_loci"]
    refused("item 2: item_locus out of range", item_locus=loc)
    kept = c["kept_item"].copy()
    kept[0] = int(c["item_locus"].size)
    refused("out of range", kept_item=kept)
    kept = c["kept_item"].copy()
    kept[0] = int(c["item_locus"].size) - 1
    refused("belongs to locus", kept_item=kept)
    koff = c["kept_off"].copy()
    koff[0] = 1
    refused("start at 0", kept_off=koff)
    koff = c["kept_off"].copy()
    koff[4] = koff[3] - 1
    refused("decreasing", kept_off=koff)
    refused("both be given", alt_cigar=np.zeros(1, np.uint32))
    n = int(c["item_locus"].size)
    refused("alt_cigar_off[0]", alt_cigar=np.zeros(1, np.uint32), alt_off=np.ones(n + 1, np.int64))
    # an offset that is not a record start: the parser refuses the item
    o = off.copy()
    o[[9, 4]] += 2
    refused("item 4: malformed BAM record", rec_off=o)


def test_counter_width_refusal(bam):
    """The kernel's counts have 16 bits: a locus whose item list names one record 65 536 times is refused, 65 535 times counted."""
    c = cases.corpus()
    one = {"n_items": 1, "rec_off": np.ascontiguousarray(bam.rec_off[c["item_file_index"][:1]], np.int64), "item_locus": np.zeros(1, np.int32), "n_loci": 1,
           "left": c["left"][:1], "right": c["right"][:1]}
    rc, _, _ = _raw(bam, kept_off=np.array([0, sd.MAX_KEPT_READS + 1], np.int32), kept_item=np.zeros(sd.MAX_KEPT_READS + 1, np.int32), **one)
    assert rc == _lib.STRK_E_INVALID and b"locus 0: 65536 kept reads (at most 65535" in _lib.load().strk_last_error()
    rc, off, _ = _raw(bam, kept_off=np.array([0, sd.MAX_KEPT_READS], np.int32), kept_item=np.zeros(sd.MAX_KEPT_READS, np.int32), **one)
    assert rc == 0 and off.tolist() == [0, 0]          # (65 535 copies of one read agree everywhere)


def test_the_symbols_are_exported():
    L = _lib.load()
    for name in ("strk_discover_snvs", "strk_dbam_discover_snvs"):
        assert name in _lib.EXPORTS and getattr(L, name) is not None
    assert L.strk_discover_snvs.restype is __import__("ctypes").c_int64
