"""CPU: the library's host functions strk_phase_cells / strk_useful_snvs (the walks of strk_phase_inputs.h compiled for the host)
against the readable statement of the rule, frontend/phase_inputs.py, on the seeded corpus of phase_inputs_cases.py and on hand
vectors.  Nothing here needs a GPU; nothing is skipped."""
import struct

import numpy as np
import pytest

import phase_inputs_cases as cases
from strkit_amd import _lib
from strkit_amd.frontend import NativeBam, write_bam
from strkit_amd.frontend import phase_inputs as pi


@pytest.fixture(scope="module")
def bam(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("phase_inputs") / "corpus.bam")
    write_bam(path, [cases.CONTIG], cases.corpus()["records"])
    return NativeBam(path)


def _cells(bam, alt):
    c = cases.corpus()
    return pi.phase_cells(bam, c["item_file_index"], c["item_locus"], c["cand_off"], c["cand_pos"], alt=c["alt"] if alt else None)


def test_corpus_covers_what_it_should():
    c = cases.corpus()
    assert sum(r["name"].startswith("r") for r in c["items"]) >= 2000
    n_ops = {len(r["cigar"]) for r in c["items"]}
    assert {0, 1, 63, 64, 65, 129} <= n_ops
    n_cand = set(np.diff(c["cand_off"]).tolist())
    assert {0, 1, pi.MAX_CANDIDATES} <= n_cand
    assert any(r.get("long_cigar") for r in c["items"]) and any(r["qual"] is None for r in c["items"]) and c["alt"]
    e = cases.expected(False)
    assert (e["base"] == ord("_")).any() and (e["base"] == ord("-")).any() and (e["base"] == ord("A")).any()
    assert (e["hp"] != -1).sum() > 500 and (e["hp"] == -1).sum() > 500


def test_tags_of_every_integer_type_and_the_untagged_cases(bam):
    c = cases.corpus()
    got = _cells(bam, False)
    e = cases.expected(False)
    assert np.array_equal(got["hp"], e["hp"]) and np.array_equal(got["ps"], e["ps"])
    for i, r in enumerate(c["items"]):            # the rule itself against what the corpus was built to mean
        if r["name"] in c["want_tags"]:
            assert (int(e["hp"][i]), int(e["ps"][i])) == c["want_tags"][r["name"]], r["name"]


@pytest.mark.parametrize("alt", [False, True])
def test_cells_equal_the_rule(bam, alt):
    c = cases.corpus()
    got, e = _cells(bam, alt), cases.expected(alt)
    cell_item = np.repeat(np.arange(c["item_locus"].size), np.diff(c["cand_off"])[c["item_locus"]])
    bad = np.nonzero((got["base"] != e["base"]) | (got["qual"] != e["qual"]))[0]
    assert bad.size == 0, (c["items"][int(cell_item[bad[0]])]["name"], int(bad[0]), bytes(got["base"][bad[:8]]), bytes(e["base"][bad[:8]]))
    if alt:
        assert not np.array_equal(e["base"], cases.expected(False)["base"])


def _hand(cigar, pos, cand, seq=None, qual="q", clip_threshold=100, take_in=250):
    cig = np.array([(ln << 4) | "MIDNSHP=X".index(op) for ln, op in cigar], np.uint32)
    n_q = sum(ln for ln, op in cigar if op in "MIS=X")
    seq = seq or ("ACGT" * (n_q // 4 + 1))[:n_q]
    q = None if qual is None else (np.arange(n_q) % 50 + 1).astype(np.uint8)
    return pi.alignment_cells(cig, pos, seq, q, np.asarray(cand, np.int64), clip_threshold, take_in), seq, q


def test_the_rule_on_hand_vectors():
    # 5S 4M 2D 3M 1I 2M 3N 4M: reference 100.., read positions 5..
    (b, q), seq, qq = _hand([(5, "S"), (4, "M"), (2, "D"), (3, "M"), (1, "I"), (2, "M"), (3, "N"), (4, "M")], 100, range(98, 122))
    want = "--" + seq[5:9] + "__" + seq[9:12] + seq[13:15] + "---" + seq[15:19] + "----"
    assert bytes(b).decode() == want
    assert q[2] == qq[5] and q[6] == 0 and q[8] == qq[9] and q[11] == qq[13] and q[13] == 0 and q[16] == qq[15]
    # clip of 99 / 100: the take-in moves lo and hi by 250
    for clip, lo, hi in ((99, 1000, 1600), (100, 1250, 1350)):
        (b, _), seq, _ = _hand([(clip, "S"), (600, "M"), (clip, "S")], 1000, [lo - 1, lo, hi - 1, hi])
        assert bytes(b).decode() == "-" + seq[clip + lo - 1000] + seq[clip + hi - 1 - 1000] + "-"
    # the clip counts only as the first / last operation; without qualities every quality is 0
    (b, q), seq, _ = _hand([(5, "H"), (100, "S"), (600, "M")], 1000, [1000, 1599, 1600], qual=None)
    assert bytes(b).decode() == seq[100] + seq[699] + "-" and not q.any()
    # no aligned pair at all
    (b, _), _, _ = _hand([(10, "S")], 50, [49, 50, 51])
    assert bytes(b) == b"---"
    (b, _), _, _ = _hand([(4, "D")], 50, [49, 50, 51])
    assert bytes(b) == b"---"


def test_nearest_1024_candidates():
    pos = np.arange(0, 4000, 2, dtype=np.int64)                 # 2 000 positions, the flanked locus in the middle
    idx = pi.locus_candidates(pos, 10, 3990, 2000, 2100)
    assert idx.size == 1024 and (np.diff(idx) > 0).all()
    p = pos[idx]
    assert not ((p >= 2000) & (p < 2100)).any()
    # distances: 2000 - p on the left (2, 4, ...), p - 2099 on the right (1, 3, ...): 512 from either side
    assert (p < 2000).sum() == 512 and p.min() == 2000 - 2 * 512 and p.max() == 2100 + 2 * 511
    # a tie goes to the left: positions 1990 and 2109 are both 10 away
    idx = pi.locus_candidates(np.array([1990, 2050, 2109], np.int64), 0, 5000, 2000, 2100, limit=1)
    assert idx.tolist() == [0]
    assert pi.locus_candidates(np.array([5, 10, 20, 30], np.int64), 10, 30, 12, 15).tolist() == [1, 2]
    assert pi.locus_candidates(np.zeros(0, np.int64), 10, 30, 12, 15).size == 0
    pos = np.arange(1025, dtype=np.int64)
    assert pi.locus_candidates(pos, 0, 5000, 2000, 2100).tolist() == list(range(1, 1025))


# ---- hostile records ----------------------------------------------------------------------------------------------------
def _call_raw(buf: bytes, rec_off, cand=(105,)):
    L = _lib.load()
    data = np.frombuffer(buf, np.uint8).copy()               # exactly the bytes: nothing behind them belongs to the buffer
    n = len(rec_off)
    rec_off = np.asarray(rec_off, np.int64)
    loc = np.zeros(n, np.int32)
    cand_off = np.array([0, len(cand)], np.int32)
    cand = np.asarray(cand, np.int64)
    hp, ps = np.zeros(n, np.int32), np.zeros(n, np.int32)
    base, qual = np.zeros(n * cand.size + 1, np.uint8), np.zeros(n * cand.size + 1, np.uint8)
    rc = L.strk_phase_cells(_lib.ptr(data), data.size, n, _lib.ptr(rec_off), _lib.ptr(loc), 1, _lib.ptr(cand_off), _lib.ptr(cand), None, None,
                            None, 100, 250, _lib.ptr(hp), _lib.ptr(ps), _lib.ptr(base), _lib.ptr(qual), n * cand.size)
    return rc, L.strk_last_error().decode(), hp, ps, base[:n * cand.size]


HOSTILE = {
    "truncated chain (two bytes left over)": cases.int_tag(b"HP", "C", 1) + b"PS",
    "value past the end": cases.int_tag(b"HP", "C", 1) + b"PSi\1\0",
    "Z without its NUL": cases.int_tag(b"HP", "C", 1) + b"RGZgroup",
    "B count that overflows 32 bits": b"ZBBI" + struct.pack("<I", 0x40000001) + b"\0" * 4 + cases.int_tag(b"HP", "C", 1),
    "B count of 2^32 - 1": b"ZBBi" + struct.pack("<I", 0xFFFFFFFF),
    "B header cut off": b"ZBBi\1\0",
    "B of an unknown type": b"ZBBq" + struct.pack("<I", 0),
    "unknown type": b"XXq\0",
}


@pytest.mark.parametrize("what", sorted(HOSTILE))
def test_hostile_auxiliary_fields_are_refused_naming_the_item(what):
    good = cases.raw_record(100, [(10 << 4)], 10, cases.int_tag(b"HP", "C", 2) + cases.int_tag(b"PS", "s", 7))
    bad = cases.raw_record(100, [(10 << 4)], 10, HOSTILE[what])
    rc, msg, hp, ps, base = _call_raw(good + bad, [0, len(good)])
    assert rc == _lib.STRK_E_INVALID and "item 1" in msg, (rc, msg)
    rc, msg, hp, ps, base = _call_raw(good + good, [0, len(good)])
    assert rc == 0 and hp.tolist() == [2, 2] and ps.tolist() == [7, 7] and bytes(base) == b"AA"


def test_long_cigar_placeholders():
    real = [(6 << 4), (2 << 4) | 2, (4 << 4)]                     # 6M 2D 4M
    cg = b"CGBI" + struct.pack("<I", 3) + b"".join(struct.pack("<I", c) for c in real)
    place = [(10 << 4) | 4, (12 << 4) | 3]                         # 10S 12N
    ok = cases.raw_record(100, place, 10, cases.int_tag(b"HP", "C", 1) + cases.int_tag(b"PS", "C", 3) + cg)
    rc, msg, hp, ps, base = _call_raw(ok, [0], cand=(99, 100, 105, 106, 107, 108, 111, 112))
    assert rc == 0 and (hp[0], ps[0]) == (1, 3) and bytes(base) == b"-AA__AA-", (rc, msg, bytes(base))
    # the placeholder without its CG tag is a read that is all clip and skip: no cell
    rc, msg, hp, ps, base = _call_raw(cases.raw_record(100, place, 10, b""), [0], cand=(100, 105))
    assert rc == 0 and bytes(base) == b"--"
    # a CG array that claims more operations than the record holds
    lie = b"CGBI" + struct.pack("<I", 1000) + b"".join(struct.pack("<I", c) for c in real)
    rc, msg, *_ = _call_raw(cases.raw_record(100, place, 10, lie), [0])
    assert rc == _lib.STRK_E_INVALID and "item 0" in msg


def test_input_checks():
    L = _lib.load()
    good = cases.raw_record(100, [(10 << 4)], 10, b"")
    data = np.frombuffer(good, np.uint8).copy()
    hp, ps = np.zeros(1, np.int32), np.zeros(1, np.int32)
    base, qual = np.zeros(2000, np.uint8), np.zeros(2000, np.uint8)

    def call(rec_off=(0,), loc=(0,), cand_off=(0, 2), cand=(100, 105), n_loci=1, cap=2000, alt_off=None, alt=None):
        a = [np.asarray(rec_off, np.int64), np.asarray(loc, np.int32), np.asarray(cand_off, np.int32), np.asarray(cand, np.int64)]
        alt_off = None if alt_off is None else np.asarray(alt_off, np.int64)
        alt = None if alt is None else np.asarray(alt, np.uint32)
        rc = L.strk_phase_cells(_lib.ptr(data), data.size, len(rec_off), _lib.ptr(a[0]), _lib.ptr(a[1]), n_loci, _lib.ptr(a[2]), _lib.ptr(a[3]),
                                _lib.ptr(alt), _lib.ptr(alt_off), None, 100, 250, _lib.ptr(hp), _lib.ptr(ps), _lib.ptr(base), _lib.ptr(qual), cap)
        return rc, L.strk_last_error().decode()

    assert call()[0] == 0
    for kw, needle in (({"cand": (105, 100)}, "ascending"), ({"cand": (100, 100)}, "ascending"), ({"loc": (1,)}, "item_locus"),
                       ({"loc": (-1,)}, "item_locus"), ({"cand_off": (0, -1)}, "decreasing"), ({"cand_off": (1, 2)}, "start at 0"),
                       ({"rec_off": (-4,)}, "rec_off"), ({"rec_off": (len(good),)}, "rec_off"),
                       ({"cand_off": (0, 1025), "cand": tuple(range(1025))}, "at most 1024"),
                       ({"alt_off": (0, -1), "alt": (16,)}, "alt_cigar_off"), ({"alt_off": (1, 2), "alt": (16, 16)}, "alt_cigar_off")):
        rc, msg = call(**kw)
        assert rc == _lib.STRK_E_INVALID and needle in msg, (kw, rc, msg)
    rc, msg = call(cap=1)
    assert rc == _lib.STRK_E_NOMEM
    rc, msg = call(rec_off=(2,))                                   # not a record start: the parser refuses it
    assert rc == _lib.STRK_E_INVALID and "item 0" in msg


def test_two_malformed_records_name_the_first(bam):
    """2 100 items drawn with repetition from the corpus's first records, two threads at 1 024 items per thread where there
    are two cores: items 1 500 and 5 point two bytes into a record, and the call names item 5."""
    L = _lib.load()
    n = 2100
    off = bam.rec_off[np.random.default_rng(30).integers(0, 64, n)].copy()
    off[[1500, 5]] += 2
    loc, cand_off, cand = np.zeros(n, np.int32), np.array([0, 1], np.int32), np.array([1005], np.int64)
    hp, ps, base, qual = np.zeros(n, np.int32), np.zeros(n, np.int32), np.zeros(n, np.uint8), np.zeros(n, np.uint8)

    def call():
        rc = L.strk_phase_cells(_lib.ptr(bam.data), bam.data.size, n, _lib.ptr(off), _lib.ptr(loc), 1, _lib.ptr(cand_off), _lib.ptr(cand), None, None,
                                None, 100, 250, _lib.ptr(hp), _lib.ptr(ps), _lib.ptr(base), _lib.ptr(qual), n)
        return rc, L.strk_last_error().decode()

    for _ in range(3):
        assert call() == (_lib.STRK_E_INVALID, "strk_phase_cells: item 5: malformed BAM record or auxiliary fields")
    off[5] -= 2
    assert call() == (_lib.STRK_E_INVALID, "strk_phase_cells: item 1500: malformed BAM record or auxiliary fields")
    off[1500] -= 2
    assert call()[0] == 0


# ---- useful SNVs --------------------------------------------------------------------------------------------------------
def _useful(mats, kept, min_allele_reads=2):
    """mats: per locus the cells' bytes [n items, candidates]; kept: per locus the kept rows.  (library result, the rule's)"""
    n_loci = len(mats)
    item_locus = np.repeat(np.arange(n_loci), [m.shape[0] for m in mats]).astype(np.int32)
    cand_off = np.concatenate(([0], np.cumsum([m.shape[1] for m in mats]))).astype(np.int32)
    base = np.concatenate([m.ravel() for m in mats] + [np.zeros(0, np.uint8)]).astype(np.uint8)
    rng = np.random.default_rng(len(base))
    qual = rng.integers(0, 61, base.size).astype(np.uint8)
    first = np.concatenate(([0], np.cumsum([m.shape[0] for m in mats])))
    kept_off = np.concatenate(([0], np.cumsum([len(k) for k in kept]))).astype(np.int32)
    kept_item = np.concatenate([first[l] + np.asarray(k, np.int64) for l, k in enumerate(kept)] + [np.zeros(0, np.int64)]).astype(np.int32)
    got = pi.library_useful_snvs({"item_locus": item_locus, "cand_off": cand_off, "base": base, "qual": qual}, kept_off, kept_item, min_allele_reads)
    sel, bs, qs = [], [], []
    o = 0
    for l, m in enumerate(mats):
        q = qual[o:o + m.size].reshape(m.shape)
        o += m.size
        rows = np.asarray(kept[l], np.int64)
        sel.append(pi.useful_snvs(m[rows], min_allele_reads))
        bs.append(m[rows])
        qs.append(q[rows])
    want = pi.pack_cells(bs, qs, sel)
    return got, want, sel


def _same(got, want, sel):
    assert np.array_equal(got["snv_off"], want[0])
    assert np.array_equal(got["snv_cand"], np.concatenate(sel + [np.zeros(0, np.int32)]))
    assert np.array_equal(got["snv_base"], want[1]) and np.array_equal(got["snv_qual"], want[2])


def _column(n, counts: dict) -> np.ndarray:
    col = np.full(n, ord("-"), np.uint8)
    k = 0
    for ch, cnt in counts.items():
        col[k:k + cnt] = ord(ch)
        k += cnt
    assert k <= n
    return col


@pytest.mark.parametrize("n", [0, 1, 4, 5, 9, 10, 11, 29, 30, 31, 250])
@pytest.mark.parametrize("min_allele_reads", [1, 2, 8])
def test_useful_snvs_at_the_thresholds(n, min_allele_reads):
    a, t = pi.useful_thresholds(n, min_allele_reads)
    assert a == max(round(n / 5.0), min_allele_reads) and t == max(round(n * 0.55), 5)     # (Python's round: half to even)
    if n == 10:
        assert t == 6
    if n == 30:
        assert t == 16
    cols, want = [], []

    def add(counts, must=None):
        """A column with these byte counts (left out when it needs more than n reads); `must`: what it has to be by construction."""
        if sum(counts.values()) > n or any(v < 0 for v in counts.values()):
            return
        real = [v for ch, v in counts.items() if ch not in "-_"]
        useful = sum(v >= a for v in real) >= 2 and sum(real) >= t
        assert must is None or useful == must, (counts, a, t)
        cols.append(_column(n, counts))
        want.append(useful)

    rest = max(t - 2 * a, 0)
    add({"A": a, "C": a, "G": rest}, True)                            # exactly at both thresholds (G fills up the total)
    add({"A": a, "C": a, "_": rest}, rest == 0)                       # '_' does not count
    add({"A": a, "C": a - 1, "_": n - 2 * a + 1}, False)              # one below the allele threshold
    if rest:
        add({"A": a, "C": a, "G": rest - 1}, False)                   # one below the total threshold
    add({"A": a, "C": max(a, t - a - 1)})
    add({"A": n}, False)
    add({}, False)                                                    # all '-'
    add({"_": n}, False)
    add({"A": a, "T": a, "N": a})
    if not cols:
        cols, want = [np.zeros(0, np.uint8)], []
    m = np.stack(cols, axis=1) if n else np.zeros((0, len(cols)), np.uint8)
    got, exp, sel = _useful([m], [list(range(n))], min_allele_reads)
    _same(got, exp, sel)
    if n:
        assert sel[0].tolist() == [k for k, u in enumerate(want) if u], (a, t, want)
    else:
        assert got["snv_off"].tolist() == [0, 0]


@pytest.mark.parametrize("n_useful", [63, 64, 65, 300])
def test_the_first_64_useful_snvs_are_taken(n_useful):
    rng = np.random.default_rng(n_useful)
    n, nc = 10, min(n_useful * 2, 1024)
    m = np.full((n, nc), ord("-"), np.uint8)
    good = np.sort(rng.choice(nc, n_useful, replace=False))
    m[:5, good] = ord("A")
    m[5:, good] = ord("G")
    got, exp, sel = _useful([m, m[:, :3]], [list(range(n)), list(range(n))])
    _same(got, exp, sel)
    assert sel[0].tolist() == good[:64].tolist() and got["snv_off"][1] == min(n_useful, 64)


def test_useful_snvs_of_random_loci_and_of_the_corpus(bam):
    rng = np.random.default_rng(77)
    mats, kept = [], []
    for _ in range(1200):                                          # more loci than one thread takes
        n, nc = int(rng.integers(0, 40)), int(rng.integers(0, 30))
        mats.append(rng.choice(np.frombuffer(b"ACGT-_N=", np.uint8), (n, nc), p=[.3, .25, .1, .1, .15, .05, .03, .02]))
        kept.append(np.nonzero(rng.integers(0, 4, n) > 0)[0])
    got, exp, sel = _useful(mats, kept)
    _same(got, exp, sel)
    assert got["snv_off"][-1] > 100
    # the corpus: the library's cells through the library's choice against the rule's cells through the rule's choice
    c, e = cases.corpus(), cases.expected(True)
    kept_off, kept_item = cases.kept_reads()
    got = pi.library_useful_snvs(_cells(bam, True), kept_off, kept_item, 2)
    cell_off = np.concatenate(([0], np.cumsum(np.diff(c["cand_off"])[c["item_locus"]])))
    bs, qs, sel = [], [], []
    for l in range(c["n_loci"]):
        nc = int(c["cand_off"][l + 1] - c["cand_off"][l])
        rows = kept_item[kept_off[l]:kept_off[l + 1]]
        b = np.array([e["base"][cell_off[i]:cell_off[i] + nc] for i in rows], np.uint8).reshape(len(rows), nc)
        q = np.array([e["qual"][cell_off[i]:cell_off[i] + nc] for i in rows], np.uint8).reshape(len(rows), nc)
        bs.append(b)
        qs.append(q)
        sel.append(pi.useful_snvs(b, 2))
    _same(got, pi.pack_cells(bs, qs, sel), sel)


def test_useful_snvs_input_checks():
    L = _lib.load()
    item_locus = np.array([0, 0, 1], np.int32)
    cand_off = np.array([0, 2, 3], np.int32)
    base, qual = np.full(5, ord("A"), np.uint8), np.zeros(5, np.uint8)
    out = [np.zeros(3, np.int32), np.zeros(128, np.int32), np.zeros(64, np.uint8), np.zeros(64, np.uint8)]

    def call(kept_off=(0, 2, 3), kept_item=(0, 1, 2), mar=2):
        ko, ki = np.asarray(kept_off, np.int32), np.asarray(kept_item, np.int32)
        rc = L.strk_useful_snvs(3, _lib.ptr(item_locus), 2, _lib.ptr(cand_off), _lib.ptr(base), _lib.ptr(qual), _lib.ptr(ko), _lib.ptr(ki), mar,
                                *[_lib.ptr(o) for o in out], 64)
        return rc, L.strk_last_error().decode()

    assert call()[0] == 0
    for kw, needle in (({"kept_item": (0, 2, 2)}, "belongs to locus"), ({"kept_item": (0, 3, 2)}, "out of range"),
                       ({"kept_off": (0, 2, 1)}, "decreasing"), ({"kept_off": (1, 2, 3)}, "start at 0"), ({"mar": 0}, "min_allele_reads")):
        rc, msg = call(**kw)
        assert rc == _lib.STRK_E_INVALID and needle in msg, (kw, rc, msg)


def test_phase_set_remap_and_gates():
    remap = pi.PhaseSetRemap()
    assert remap(np.array([500, -1, 7, 500]), np.array([1, -1, 2, 2])).tolist() == [1, -1, 2, 1]
    assert remap(np.array([7, 9, -1]), np.array([1, 1, -1])).tolist() == [2, 3, -1] and len(remap) == 3
    ids = remap.snapshot()
    assert remap(np.array([11, 12]), np.array([1, 2])).tolist() == [4, 5]
    remap.restore(ids)                       # a block that is run again numbers its phase sets from where it began
    assert remap(np.array([12, 11]), np.array([1, 2])).tolist() == [4, 5] and len(remap) == 5
    assert pi.snv_step_allowed(2, 1, False) and not pi.snv_step_allowed(1, 0, False)
    assert not pi.snv_step_allowed(2, 2, False) and not pi.snv_step_allowed(2, 0, True)
