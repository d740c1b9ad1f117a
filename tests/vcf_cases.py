"""Shared by tests/test_tabix.py, tests/test_vcf_snvs_host.py (CPU: strk_vcf_snvs, IndexedSnvVcf on the host cores),
tests/test_gpu_vcf_snvs.py (strk_dbam_vcf_snvs) and tools/vcf_snvs_asan.cpp (through dump()): one corpus of small VCF texts,
a few KB each, each with the windows to ask for.  What a query must give is ALWAYS frontend/snv_vcf.py::read_snv_vcf on the same
bytes, restricted to the contig and [beg, end) — never what the code under test makes of them.  Two kinds of refusal: a text
read_snv_vcf itself raises on (a malformed POS on a base-valid line; `bad_off` = the byte offset of that line), and a text whose
kept positions descend (`unsorted`: read_snv_vcf sorts, a region reader cannot).  A third, stated difference: POS
spellings Python's int() takes and the byte parser does not (19 digits, "+5"); check_coverage pins which cases those are.

A case: name, text, windows [(contig as the file spells it, beg, end)], block_bytes (the BGZF blocks it is written with), start
(the offset the C ABI calls begin at: a line start), indexable (False: positions a tabix index cannot hold, C ABI only)."""
from __future__ import annotations

import functools
import os
import tempfile
from dataclasses import dataclass, field

import numpy as np

WHOLE = (0, 1 << 29)
TILES = (256, 1024)            # tile sizes of the line passes the GPU tests run (1024 = the default)
LINES_PER_WAVE = 64


@dataclass
class Case:
    name: str
    text: bytes
    windows: list
    block_bytes: int = 0xFF00
    start: int = 0
    indexable: bool = True
    bad_off: int | None = None
    unsorted: bool = False
    tags: set = field(default_factory=set)


def rec(contig, pos, id_, ref, alt, rest="\t.\t.\t.", nl="\n") -> str:
    return f"{contig}\t{pos}\t{id_}\t{ref}\t{alt}{rest}{nl}"


HEAD = "##fileformat=VCFv4.2\n##contig=<ID=chr1>\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\n"
# every line kind of tests/test_snv_vcf.py's VCF, in coordinate order (a region reader needs that)
BASIC = (HEAD + rec("chr1", 100, "rs1", "c", "t") + rec("chr1", 200, ".", "G", "A,T") + rec("chr1", 250, "indel", "GA", "G")
         + rec("chr1", 260, "ins", "G", "GA") + rec("chr1", 270, "multi", "G", "A,TT") + rec("chr1", 280, "sym", "G", "<DEL>")
         + rec("chr1", 290, "star", "G", "*") + rec("chr1", 295, "noalt", "G", ".") + rec("chr1", 300, "rs3", "A", "G")
         + rec("chr1", 300, "dup", "A", "C") + rec("2", 50, "rs9", "T", "C") + "short line\n")


def _pad_to(text: str, at: int) -> str:
    """`text` plus one comment line that ends (its '\\n') exactly at byte at - 1, so that the next line starts at byte `at`."""
    need = at - len(text)
    assert need >= 2, (len(text), at)
    return text + "#" + "p" * (need - 2) + "\n"


def _snv_lines(n: int, first: int = 10, step: int = 7, contig: str = "chr1") -> str:
    return "".join(rec(contig, first + step * i, f"rs{i}", "ACGT"[i % 4], "ACGT"[(i + 1) % 4], rest="") for i in range(n))


TRIPLE = rec("chr1", 5000, "del", "AT", "A") + rec("chr1", 5000, "first", "A", "G") + rec("chr1", 5000, "second", "A", "C")


@functools.lru_cache(maxsize=None)
def cases() -> tuple:
    out = []

    def add(name, text, windows=None, tags=(), **kw):
        text = text.encode() if isinstance(text, str) else text
        out.append(Case(name, text, list(windows or [("chr1",) + WHOLE]), tags=set(tags), **kw))

    add("basic", BASIC, [("chr1",) + WHOLE, ("2",) + WHOLE, ("chr1", 99, 100), ("chr1", 100, 299), ("chr1", 100, 300), ("chr1", 199, 200),
                         ("chr1", 200, 299), ("chr1", 150, 150), ("chr1", 0, 99), ("chr1", 299, 300), ("chr1", 300, 400)],
        tags={"line_kinds", "edge_beg", "edge_end_minus_1", "edge_end", "edge_beg_minus_1", "empty_window", "one_per_position", "single_block_range"})
    add("crlf", HEAD.replace("\n", "\r\n") + rec("chr1", 10, "five", "A", "G", rest="", nl="\r\n") + rec("chr1", 20, "fiver", "C", "T", rest="", nl="\r\r\n")
        + rec("chr1", 30, "eight", "G", "A", nl="\r\n") + rec("chr1", 40, "short", "G", "", rest="", nl="\r\n"), tags={"crlf"})
    add("no_trailing_newline", HEAD + rec("chr1", 10, "a", "A", "G") + rec("chr1", 20, "last", "C", "T", nl=""), tags={"no_trailing_newline"})
    add("no_trailing_newline_cr", HEAD + rec("chr1", 10, "a", "A", "G") + rec("chr1", 20, "last", "C", "T", rest="", nl="\r"), tags={"no_trailing_newline"})
    add("empty_lines", "\n\n" + HEAD + "\n" + rec("chr1", 10, "a", "A", "G") + "\n\n" + rec("chr1", 20, "b", "C", "T") + "\n", tags={"empty_lines"})
    add("alt_ref_shapes", HEAD + rec("chr1", 10, "trail", "A", "A,") + rec("chr1", 20, "lead", "A", ",A") + rec("chr1", 30, "mid", "A", "C,,G")
        + rec("chr1", 40, "none", "A", "") + rec("chr1", 50, "refR", "R", "A") + rec("chr1", 60, "refN", "N", "A") + rec("chr1", 70, "lower", "n", "a,c,g")
        + rec("chr1", 80, "altR", "A", "R") + rec("chr1", 90, "noref", "", "A") + rec("chr1", 95, "three", "T", "A,C,G"), tags={"alt_ref_shapes"})
    add("mid_header", HEAD + rec("chr1", 10, "a", "A", "G") + "#chr1\t15\thidden\tA\tG\n##more\n" + rec("chr1", 20, "b", "C", "T") + "#\n", tags={"mid_header"})
    add("ids", HEAD + rec("chr1", 10, "rs1;rs2", "A", "G") + rec("chr1", 20, "i" * 300, "C", "T") + rec("chr1", 30, ".", "C", "T") + rec("chr1", 40, "..", "C", "T")
        + rec("chr1", 50, "", "C", "T"), tags={"ids"})
    add("long_fields", HEAD + rec("chr1", 10, "longref", "ACGTA" * 100, "A") + rec("chr1", 20, "a", "A", "G", rest="\t.\t.\t" + "I" * 20000)
        + rec("chr1", 30, "b", "C", "T"), tags={"long_fields", "line_longer_than_tile"})
    add("contig_names", HEAD + rec("chr1", 10, "a", "A", "G") + rec("chr1", 20, "b", "A", "G") + rec("chr11", 10, "c", "C", "T") + rec("chr11", 15, "d", "C", "T")
        + rec("chr1_x", 5, "e", "G", "T") + rec("chr1_x", 10, "f", "G", "T"),
        [("chr1",) + WHOLE, ("chr11",) + WHOLE, ("chr1_x",) + WHOLE, ("chr1", 0, 15)], tags={"contig_names"})
    add("pos_digits", HEAD + rec("chr1", 7, "a", "A", "G") + rec("chr1", 1234567890, "ten", "A", "G") + rec("chr1", "9" * 18, "eighteen", "C", "T")
        + rec("chr1", "0012", "padded_is_fewer", "AC", "T"),
        [("chr1", 0, 10 ** 18), ("chr1", 1234567889, 1234567890), ("chr1", 10 ** 18 - 2, 10 ** 18 - 1), ("chr1", 0, 100)], indexable=False, tags={"pos_digits"})
    for nm, bad in (("19_digits", "1" * 19), ("plus", "+5"), ("empty", "")):
        text = HEAD + rec("chr1", 3, "ok", "A", "G") + rec("chr1", bad, "bad", "A", "G") + rec("chr1", 9, "after", "A", "G")
        add("bad_pos_" + nm, text, bad_off=text.index(f"chr1\t{bad}\tbad"), tags={"bad_pos"})
        add("bad_pos_skipped_" + nm, HEAD + rec("chr1", 3, "ok", "A", "G") + rec("chr1", bad, "bad", "AT", "G") + rec("chr1", 9, "after", "A", "G"), tags={"bad_pos_skipped"})
    add("bad_pos_other_contig", HEAD + rec("chr1", 3, "ok", "A", "G") + rec("chr2", "x", "bad", "A", "G"),
        bad_off=(HEAD + rec("chr1", 3, "ok", "A", "G")).__len__(), tags={"bad_pos"})
    add("triple", HEAD + rec("chr1", 4000, "a", "A", "G") + TRIPLE + rec("chr1", 6000, "b", "A", "G"), tags={"one_per_position"})
    for at in (256, 1024):   # the triple's second line starts on a tile seam (and, with 256-byte blocks, on a piece seam)
        add(f"triple_seam_{at}", _pad_to(HEAD + rec("chr1", 4000, "a", "A", "G") + rec("chr1", 5000, "del", "AT", "A"), at) + TRIPLE[TRIPLE.index("\n") + 1:]
            + rec("chr1", 6000, "b", "A", "G"), block_bytes=256, tags={"triple_tile_seam", "triple_piece_seam"})
    add("triple_line_seam", "#h\n" + _snv_lines(62) + TRIPLE + rec("chr1", 6000, "b", "A", "G"), tags={"triple_line_seam"})
    for n in (63, 64, 65, 255, 256, 257):
        # (a one-line header in front: a record at virtual offset 0 is what no index can point at, 0 being "no entry")
        add(f"lines_{n}", "#h\n" + _snv_lines(n - 1), [("chr1",) + WHOLE, ("chr1", 10 + 7 * (n // 2), 10 + 7 * n)], tags={f"lines_{n}"})
    for at in (256, 1024):
        add(f"newline_last_of_tile_{at}", _pad_to(HEAD, at) + _snv_lines(5), tags={"newline_last_of_tile"})
        add(f"newline_first_of_tile_{at}", _pad_to(HEAD, at + 1) + _snv_lines(5), tags={"newline_first_of_tile"})
    add("line_longer_than_tile_256", HEAD + rec("chr1", 10, "a", "A", "G", rest="\t.\t.\t" + "J" * 700) + rec("chr1", 20, "b", "C", "T"), tags={"line_longer_than_tile"})
    t = HEAD + _snv_lines(40)
    add("start_offset", t, start=len(HEAD) + len(rec("chr1", 10, "rs0", "A", "C", rest="")), tags={"start_offset"})
    add("blocks_256", HEAD + "".join(rec("chr1", 1000003 + 11 * i, f"rs{100000 + 977 * i}", "ACGT"[i % 4], "ACGT"[(i + 2) % 4], rest="\t.\t.\tAF=0.5") for i in range(120)),
        [("chr1",) + WHOLE, ("chr1", 1000200, 1000700), ("chr1", 1000003, 1000004)], block_bytes=256, tags={"piece_cuts"})
    add("unsorted", HEAD + rec("chr1", 30, "a", "A", "G") + rec("chr1", 20, "b", "A", "G"), unsorted=True, tags={"unsorted"})
    add("index_fill", HEAD + rec("chr1", 100, "a", "A", "G") + rec("chr1", 40000, "b", "A", "G") + rec("chr1", 41000, "c", "A", "G"),
        [("chr1", 20000, 50000), ("chr1", 17000, 30000)], block_bytes=64, tags={"index_fill"})
    add("long_ref", HEAD + rec("chr1", 1001, "huge", "A" * 40000, "A") + rec("chr1", 1501, "a", "A", "G") + rec("chr1", 20001, "b", "A", "G")
        + rec("chr1", 35001, "c", "A", "G") + rec("chr1", 45001, "d", "A", "G") + rec("chr1", 70001, "e", "A", "G"),
        [("chr1", 33000, 46000), ("chr1",) + WHOLE, ("chr1", 45000, 45001)], block_bytes=512, tags={"long_ref"})
    return tuple(out)


_TMP = None


@functools.lru_cache(maxsize=None)
def _oracle(name: str):
    """read_snv_vcf on the case's bytes: {contig: (pos, ids, ref)}, or the exception it raised."""
    from strkit_amd.frontend.snv_vcf import read_snv_vcf
    global _TMP
    if _TMP is None:
        _TMP = tempfile.TemporaryDirectory(prefix="vcf_cases_")
    case = {c.name: c for c in cases()}[name]
    path = os.path.join(_TMP.name, name + ".vcf")
    with open(path, "wb") as fh:
        fh.write(case.text[case.start:])
    try:
        got = read_snv_vcf(path)
    except ValueError as e:
        return e
    return {k: (v.pos, list(v.ids), list(v.ref)) for k, v in got.by_contig.items()}


def refuses(case: Case) -> bool:
    return case.unsorted or case.bad_off is not None


def expected(case: Case, contig: str, beg: int, end: int):
    """(pos list, ids, ref) read_snv_vcf gives for the window; a contig the text does not have gives three empty lists."""
    o = _oracle(case.name)
    assert not isinstance(o, Exception), (case.name, o)
    if contig not in o:
        return [], [], []
    pos, ids, ref = o[contig]
    keep = np.flatnonzero((pos >= beg) & (pos < end))
    return pos[keep].tolist(), [ids[k] for k in keep], [ref[k] for k in keep]


def written(case: Case, directory: str) -> str:
    """The case as <directory>/<name>.vcf.gz (blocks of case.block_bytes) with its .tbi; returns the path."""
    from strkit_amd.frontend.synth_snvs import write_bgzf_vcf, write_tbi
    path = os.path.join(directory, case.name + ".vcf.gz")
    if not os.path.exists(path + ".tbi"):
        offs = write_bgzf_vcf(path, case.text, case.block_bytes)
        write_tbi(path + ".tbi", case.text, offs, case.block_bytes)
    return path


def query(L, target, n_bytes: int, start: int, contig: str, beg: int, end: int, final: int = 1, prev: int = -1, seen: int = 0, tile: int = 0,
          cap: int | None = None, ids_cap: int | None = None, want_ids: bool = True):
    """One call of the C ABI: `target` = a numpy byte buffer (strk_vcf_snvs) or a strk_dbam handle (strk_dbam_vcf_snvs).  Returns
    (return value, pos list, ids, ref, end_off, past, id_bytes); the lists are None when the arrays were not filled."""
    import ctypes as C
    cap = (n_bytes // 8 + 2) if cap is None else cap
    ids_cap = (n_bytes + 1) if ids_cap is None else ids_cap
    pos, ref, id_off, ids = np.full(cap, -7, np.int64), np.zeros(cap, np.uint8), np.full(cap + 1, -7, np.int64), np.zeros(ids_cap, np.uint8)
    id_bytes, end_off, past = C.c_int64(-1), C.c_int64(-1), C.c_int32(-1)
    tail = (cap, pos.ctypes.data, ref.ctypes.data, id_off.ctypes.data, ids.ctypes.data if want_ids else None, ids_cap, C.byref(id_bytes),
            C.byref(end_off), C.byref(past))
    if isinstance(target, np.ndarray):
        k = L.strk_vcf_snvs(target.ctypes.data, n_bytes, start, contig.encode(), beg, end, final, prev, seen, *tail)
    else:
        k = L.strk_dbam_vcf_snvs(target, start, contig.encode(), beg, end, final, prev, seen, tile, *tail)
    k = int(k)
    if k < 0 or k > cap:
        return k, None, None, None, end_off.value, past.value, id_bytes.value
    assert id_off[0] == 0 and id_off[k] == id_bytes.value and (np.diff(id_off[:k + 1]) >= 0).all()
    names = [ids[id_off[i]:id_off[i + 1]].tobytes().decode() for i in range(k)] if want_ids else None
    return k, pos[:k].tolist(), names, [chr(c) for c in ref[:k]], end_off.value, past.value, id_bytes.value


def _field_spans(text: bytes, col: int):
    """[a, b) of column `col` of every line with at least five fields that is no header."""
    u = 0
    for raw in text.split(b"\n"):
        f = raw.split(b"\t")
        if raw[:1] != b"#" and len(f) >= 5:
            a = u + sum(len(x) + 1 for x in f[:col])
            yield a, a + len(f[col])
        u += len(raw) + 1


def check_coverage() -> dict:
    """Asserts that the corpus holds what tests/README of the feature (the issue's list) asks for; returns what it counted."""
    cs = cases()
    tags = set().union(*(c.tags for c in cs))
    wanted = {"line_kinds", "crlf", "no_trailing_newline", "empty_lines", "alt_ref_shapes", "mid_header", "ids", "long_fields", "contig_names",
              "pos_digits", "bad_pos", "bad_pos_skipped", "one_per_position", "triple_tile_seam", "triple_piece_seam", "triple_line_seam",
              "edge_beg", "edge_end_minus_1", "edge_end", "edge_beg_minus_1", "empty_window", "newline_last_of_tile", "newline_first_of_tile",
              "line_longer_than_tile", "start_offset", "piece_cuts", "single_block_range", "unsorted", "index_fill", "long_ref"}
    wanted |= {f"lines_{n}" for n in (63, 64, 65, 255, 256, 257)}
    assert wanted <= tags, wanted - tags
    by = {c.name: c for c in cs}
    assert len(by) == len(cs)
    for c in cs:
        assert len(c.text) < 64 << 10 and (c.start == 0 or c.text[c.start - 1:c.start] == b"\n"), c.name
        o = _oracle(c.name)
        # the oracle refuses the malformed POS too, but for the spellings int() accepts (the stated difference)
        assert isinstance(o, Exception) == (c.bad_off is not None and c.name not in ("bad_pos_19_digits", "bad_pos_plus")), (c.name, o)
        if c.bad_off is not None:
            assert c.text[c.bad_off - 1:c.bad_off] == b"\n"
    # line counts are what their names say
    for n in (63, 64, 65, 255, 256, 257):
        assert by[f"lines_{n}"].text.count(b"\n") == n
    # tile seams: a '\n' at offset at - 1 / at, for both tile sizes
    for at in TILES:
        assert by[f"newline_last_of_tile_{at}"].text[at - 1:at] == b"\n" and by[f"newline_first_of_tile_{at}"].text[at:at + 1] == b"\n"
        t = by[f"triple_seam_{at}"].text
        assert t[at - 1:at] == b"\n" and t[at:].startswith(b"chr1\t5000\tfirst")
    t = by["triple_line_seam"].text.split(b"\n")
    assert t[LINES_PER_WAVE - 1].startswith(b"chr1\t5000\tdel") and t[LINES_PER_WAVE].startswith(b"chr1\t5000\tfirst")
    assert max(len(x) for x in by["line_longer_than_tile_256"].text.split(b"\n")) > 256
    assert max(len(x) for x in by["long_fields"].text.split(b"\n")) > 1024
    s = by["start_offset"].start
    assert s % 256 and s % by["start_offset"].block_bytes
    # 256-byte blocks: cuts inside POS digits and inside an ID
    t = by["blocks_256"].text
    cuts = range(256, len(t), 256)
    in_pos = sum(1 for a, b in _field_spans(t, 1) for c in cuts if a < c < b)
    in_id = sum(1 for a, b in _field_spans(t, 2) for c in cuts if a < c < b)
    assert in_pos >= 1 and in_id >= 1, (in_pos, in_id)
    # IDs: a ';' and 300 bytes
    ids = expected(by["ids"], "chr1", *WHOLE)[1]
    assert "rs1;rs2" in ids and any(len(i) == 300 for i in ids) and "" in ids
    # the triple: the SNV behind the indel stays, the second SNV goes
    assert expected(by["triple"], "chr1", 4999, 5000) == ([4999], ["first"], ["A"])
    return {"cases": len(cs), "windows": sum(len(c.windows) for c in cs), "cuts_in_pos": in_pos, "cuts_in_id": in_id}


def dump(directory: str) -> None:
    """The corpus as files for tools/vcf_snvs_asan.cpp: <name>.vcf and <name>.q, per window "contig beg end start" followed by
    the positions read_snv_vcf gives, or by "refuse"."""
    os.makedirs(directory, exist_ok=True)
    for c in cases():
        with open(os.path.join(directory, c.name + ".vcf"), "wb") as fh:
            fh.write(c.text)
        with open(os.path.join(directory, c.name + ".q"), "w") as fh:
            for contig, beg, end in c.windows:
                want = ["refuse"] if refuses(c) else [str(p) for p in expected(c, contig, beg, end)[0]]
                fh.write(" ".join([contig, str(beg), str(end), str(c.start)] + want) + "\n")
