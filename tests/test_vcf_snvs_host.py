"""CPU, through the C ABI: strk_vcf_snvs (the host twin of the VCF kernels) and IndexedSnvVcf on the host cores against
read_snv_vcf on the corpus of vcf_cases.py; the capacity conventions, the resume across pieces, the error messages, and
open_snv_candidates' fall-back to the whole-file reader."""
import ctypes as C
import gzip
import re

import numpy as np
import pytest

import vcf_cases
from strkit_amd import _lib
from strkit_amd.frontend.snv_vcf import IndexedSnvVcf, SnvCandidates, open_snv_candidates, read_snv_vcf

CASES = vcf_cases.cases()
ACCEPTED = [c for c in CASES if not vcf_cases.refuses(c)]


def _buf(case):
    return np.frombuffer(case.text, np.uint8).copy()


def _err():
    return _lib.load().strk_last_error().decode()


@pytest.mark.parametrize("case", ACCEPTED, ids=lambda c: c.name)
def test_host_twin_equals_the_oracle_on_every_window(case):
    L = _lib.load()
    buf = _buf(case)
    for contig, beg, end in case.windows:
        k, pos, ids, ref, end_off, past, _ = vcf_cases.query(L, buf, buf.size, case.start, contig, beg, end)
        assert k >= 0, _err()
        assert (pos, ids, ref) == vcf_cases.expected(case, contig, beg, end), (case.name, contig, beg, end)
        assert end_off == buf.size


@pytest.mark.parametrize("case", [c for c in CASES if vcf_cases.refuses(c)], ids=lambda c: c.name)
def test_refusals_name_the_line(case):
    L = _lib.load()
    buf = _buf(case)
    k, *_ = vcf_cases.query(L, buf, buf.size, 0, "chr1", *vcf_cases.WHOLE)
    assert k == _lib.STRK_E_INVALID
    msg = _err()
    if case.unsorted:
        assert "not coordinate-sorted: the index cannot belong to this file" in msg
        assert f"byte {case.text.index(b'chr1' + bytes([9]) + b'20')}" in msg
    else:
        assert f"line at byte {case.bad_off}: POS is not 1 to 18 decimal digits" in msg


def test_resume_across_pieces_loses_and_repeats_nothing():
    """The text cut at every multiple of the case's block size (256-byte blocks: inside POS digits and IDs): a piece ends at a
    cut, the next begins at the first line the one before left incomplete."""
    L = _lib.load()
    n_cut_lines = 0
    for case in ACCEPTED:
        step = case.block_bytes if case.block_bytes < 0xFF00 else 300
        buf = _buf(case)
        for contig, beg, end in case.windows:
            got = ([], [], [])
            at, prev, seen = case.start, -1, 0
            cuts = list(range(step, buf.size, step)) + [buf.size]
            for cut in cuts:
                if cut <= at:
                    continue
                final = int(cut == buf.size)
                k, pos, ids, ref, end_off, past, _ = vcf_cases.query(L, buf, cut, at, contig, beg, end, final=final, prev=prev, seen=seen)
                assert k >= 0, _err()
                assert at <= end_off <= cut and (end_off == cut or not final)
                assert end_off == at or buf[end_off - 1] == 10 or end_off == buf.size
                n_cut_lines += end_off < cut
                for g, x in zip(got, (pos, ids, ref)):
                    g.extend(x)
                if pos:
                    prev, seen = pos[-1], 1
                at = end_off
            assert tuple(got) == vcf_cases.expected(case, contig, beg, end), (case.name, contig, beg, end)
    assert n_cut_lines > 100


def test_capacity_and_size_query_conventions():
    L = _lib.load()
    case = {c.name: c for c in CASES}["ids"]
    buf = _buf(case)
    want = vcf_cases.expected(case, "chr1", *vcf_cases.WHOLE)
    n, n_id = len(want[0]), sum(len(i) for i in want[1])
    # capacity 0: the count and the ID bytes alone
    k, pos, *_rest, id_bytes = vcf_cases.query(L, buf, buf.size, 0, "chr1", *vcf_cases.WHOLE, cap=0)
    assert (k, pos, id_bytes) == (n, None, n_id)
    k, pos, *_rest, id_bytes = vcf_cases.query(L, buf, buf.size, 0, "chr1", *vcf_cases.WHOLE, cap=n - 1)
    assert (k, pos, id_bytes) == (n, None, n_id)
    # ids == NULL: offsets without bytes
    k, pos, ids, ref, _e, _p, id_bytes = vcf_cases.query(L, buf, buf.size, 0, "chr1", *vcf_cases.WHOLE, cap=n, want_ids=False)
    assert (k, pos, ref, id_bytes) == (n, want[0], want[2], n_id)
    # exact capacities fit; one ID byte less does not
    k, pos, ids, ref, *_ = vcf_cases.query(L, buf, buf.size, 0, "chr1", *vcf_cases.WHOLE, cap=n, ids_cap=n_id)
    assert (pos, ids, ref) == want
    k, *_ = vcf_cases.query(L, buf, buf.size, 0, "chr1", *vcf_cases.WHOLE, cap=n, ids_cap=n_id - 1)
    assert k < 0 and "ID buffer too small" in _err()


def test_bad_arguments_are_refused_with_a_message():
    L = _lib.load()
    buf = _buf(CASES[0])
    for kw, text in ((dict(start=buf.size + 1), "outside the text"), (dict(start=-1), "outside the text"), (dict(beg=5, end=4), "bad window"),
                     (dict(beg=-1, end=4), "bad window"), (dict(contig=""), "no contig name"), (dict(prev=-2), "bad prev_pos")):
        a = dict(start=0, contig="chr1", beg=0, end=100, prev=-1)
        a.update(kw)
        k, *_ = vcf_cases.query(L, buf, buf.size, a["start"], a["contig"], a["beg"], a["end"], prev=a["prev"])
        assert k < 0 and text in _err(), (kw, _err())
    one = C.c_int64(0)
    p = C.c_int32(0)
    assert L.strk_vcf_snvs(buf.ctypes.data, buf.size, 0, b"chr1", 0, 10, 1, -1, 0, 4, None, None, None, None, 0, C.byref(one), C.byref(one), C.byref(p)) < 0
    assert "NULL output array" in _err()
    # a previous piece's last position: equal drops the record, greater refuses
    case = {c.name: c for c in CASES}["basic"]
    k, pos, *_ = vcf_cases.query(L, buf, buf.size, 0, "chr1", *vcf_cases.WHOLE, prev=99)
    assert pos == [199, 299]
    k, *_ = vcf_cases.query(L, buf, buf.size, 0, "chr1", *vcf_cases.WHOLE, prev=150)
    assert k < 0 and "not coordinate-sorted" in _err()
    assert case.text


def test_past_flag():
    L = _lib.load()
    by = {c.name: c for c in CASES}
    buf = _buf(by["contig_names"])
    q = lambda *a, **kw: vcf_cases.query(L, buf, buf.size, 0, *a, **kw)[5]      # noqa: E731
    assert q("chr1", 0, 15) == 1 and q("chr1", 0, 100) == 1          # a record at 19; then chr11 behind chr1
    assert q("chr1_x", 0, 100) == 0                                     # other contigs only in front
    assert q("chr1_x", 0, 100, seen=1) == 1                              # ... unless the piece before saw the contig
    assert q("chr9", 0, 100) == 0
    buf = _buf(by["lines_63"])
    assert vcf_cases.query(L, buf, buf.size, 0, "chr1", 0, 1 << 29)[5] == 0


@pytest.mark.parametrize("piece_bytes", [1, 700, 32 << 20])
def test_indexed_reader_on_the_host_equals_the_oracle(tmp_path, piece_bytes):
    for case in CASES:
        if not case.indexable or case.start:
            continue
        r = IndexedSnvVcf(vcf_cases.written(case, str(tmp_path)), front_end="host", piece_bytes=piece_bytes)
        for contig, beg, end in case.windows:
            if vcf_cases.refuses(case):
                with pytest.raises(_lib.StrkError, match="not coordinate-sorted|POS is not 1 to 18"):
                    r.window(contig, beg, end)
                continue
            w = r.window(contig, beg, end)
            assert w is not None and w.pos.dtype == np.int64
            assert (w.pos.tolist(), list(w.ids), list(w.ref)) == vcf_cases.expected(case, contig, beg, end), (case.name, contig, beg, end)
        assert r.window("chr9", 0, 100) is None and r.window("9", 0, 100) is None
        if "chr1" in r.references and not vcf_cases.refuses(case):       # with or without the prefix
            assert r.window("1", 0, 1 << 29).pos.tolist() == r.window("chr1", 0, 1 << 29).pos.tolist()


def test_open_snv_candidates_falls_back_without_an_index(tmp_path):
    case = CASES[0]
    plain = tmp_path / "a.vcf"
    plain.write_bytes(case.text)
    gzp = tmp_path / "b.vcf.gz"
    gzp.write_bytes(gzip.compress(case.text))
    for path in (plain, gzp):
        c = open_snv_candidates(str(path))
        assert isinstance(c, SnvCandidates)
        assert c.contig("chr1").pos.tolist() == read_snv_vcf(str(path)).contig("chr1").pos.tolist()
        assert c.window("1", 5, 6) is c.contig("chr1")
    # a .tbi next to a file that is not BGZF changes nothing; BGZF without a .tbi neither
    (tmp_path / "b.vcf.gz.tbi").write_bytes(b"whatever")
    assert isinstance(open_snv_candidates(str(gzp)), SnvCandidates)
    bg = vcf_cases.written(case, str(tmp_path / "x")) if (tmp_path / "x").mkdir() is None else None
    r = open_snv_candidates(bg)
    assert isinstance(r, IndexedSnvVcf) and r.front_end == "host" and r.references == ["chr1", "2"]
    import os
    os.remove(bg + ".tbi")
    assert isinstance(open_snv_candidates(bg), SnvCandidates)
    assert re.search("tabix", IndexedSnvVcf.__doc__)


def test_the_stand_alone_checker_builds_plain_and_passes(tmp_path):
    """tools/vcf_snvs_asan.cpp (a program of its own; tools/vcf_snvs_asan.sh builds it with -fsanitize=address,undefined), built
    plain here: the corpus and every truncation of its texts through parse_line and finish, exit 0."""
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = tmp_path / "vcf_snvs_check"
    subprocess.run(["g++", "-O2", "-std=c++17", "-o", str(exe), os.path.join(root, "tools", "vcf_snvs_asan.cpp")], check=True)
    vcf_cases.dump(str(tmp_path / "corpus"))
    r = subprocess.run([str(exe), str(tmp_path / "corpus")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and f"{len(CASES)} cases" in r.stdout and " 0 failed" in r.stdout, r.stdout + r.stderr
