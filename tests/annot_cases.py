"""Shared by tests/test_annotations.py (CPU: strk_gff_overlaps, IndexedAnnotations on the host cores), tests/test_gpu_annotations.py
(strk_dbam_gff_overlaps) and tools/gff_asan.cpp (through dump()): one corpus of small GFF3 / GTF texts, each with its loci.  What a
call must give is ALWAYS frontend/annotations.py's rule (parse_text + annotate) on the same bytes, never what the code under test
makes of them; the hand cases also carry their ids written out (`literal`), so that the rule itself is held to something.

A case: name, text, loci [(contig as the catalog spells it, start, end)], gtf, literal (the expected lists, or None), bad_off (the
byte offset of the line the call must refuse, or None), block_bytes (the BGZF blocks it is written with)."""
from __future__ import annotations

import ctypes as C
import functools
import os
from dataclasses import dataclass

import numpy as np

from strkit_amd import _lib
from strkit_amd.frontend import annotations as rule
from strkit_amd.frontend.loci import resolve_contig

TILES = (0, 256)               # tile sizes of the line passes the GPU tests run (0 = the default, 1024)


@dataclass
class Case:
    name: str
    text: bytes
    loci: list
    gtf: bool = False
    literal: list | None = None
    bad_off: int | None = None
    block_bytes: int = 0xFF00


def ln(contig, type_, start, end, attrs, nl="\n", extra="") -> str:
    return f"{contig}\tsrc\t{type_}\t{start}\t{end}\t.\t+\t.\t{attrs}{extra}{nl}"


def expected(case: Case) -> list:
    return rule.annotate(case.loci, rule.parse_text(case.text, case.gtf))


def file_contigs(case: Case) -> list:
    out = []
    for raw in case.text.split(b"\n"):
        raw = raw.rstrip(b"\r")
        if raw and raw[:1] != b"#":
            c = raw.split(b"\t")[0].decode("latin-1")
            if c not in out:
                out.append(c)
    return out


def _pad_to(text: str, at: int) -> str:
    """`text` plus one comment line whose '\\n' is byte at - 1, so that the next line starts at byte `at`."""
    need = at - len(text)
    assert need >= 2, (len(text), at)
    return text + "#" + "p" * (need - 2) + "\n"


@functools.lru_cache(maxsize=None)
def cases() -> tuple:
    out = []

    def add(name, text, loci, **kw):
        out.append(Case(name, text.encode("latin-1") if isinstance(text, str) else text, list(loci), **kw))

    H = "##gff-version 3\n"
    # ---- overlap edges: the locus is [100, 110)
    edges = (H + ln("chr1", "a", 91, 100, "ID=ends_at_s") + ln("chr1", "a", 91, 101, "ID=ends_at_s_plus_1") + ln("chr1", "a", 95, 120, "ID=around")
             + ln("chr1", "a", 101, 110, "ID=identical") + ln("chr1", "a", 103, 105, "ID=inside") + ln("chr1", "a", 105, 105, "ID=one_base")
             + ln("chr1", "a", 110, 120, "ID=begins_at_e_minus_1") + ln("chr1", "a", 111, 120, "ID=begins_at_e"))
    add("overlap_edges", edges, [("chr1", 100, 110), ("chr1", 104, 105), ("chr1", 0, 90), ("chr1", 120, 130)],
        literal=[["ends_at_s_plus_1", "around", "identical", "inside", "one_base", "begins_at_e_minus_1"], ["around", "identical", "inside", "one_base"], [], []])
    # ---- the join: loci with 0, 1, 63, 64, 65 and 200 hits; a contig-long feature first
    text = H + ln("chr1", "region", 1, 100000000, "ID=chr1:1..100000000")
    loci = []
    for b, (base, n) in enumerate(((1000, 0), (2000, 1), (3000, 63), (4000, 64), (5000, 65), (7000, 200))):
        for i in range(n):
            text += ln("chr1", "exon", base + 1 + i // 8, base + 40 + (i % 7), f"ID=f{b}.{i}")
        loci.append(("chr1", base + 20, base + 30))
    lit = [["chr1:1..100000000"] + [f"f{b}.{i}" for i in range(n)] for b, n in enumerate((0, 1, 63, 64, 65, 200))]
    add("hit_counts", text, loci + [("chr1", 0, 1), ("chr1", 99999999, 100000000), ("chr1", 100000000, 100000010)], literal=lit + [["chr1:1..100000000"], ["chr1:1..100000000"], []])
    # ---- length classes: lengths 2^k - 1, 2^k, 2^k + 1 that end just behind / at the start of a locus at s = 1 << 21
    S = 1 << 21
    rows = []
    for k in (1, 2, 5, 6, 10, 16, 20):
        for length in ((1 << k) - 1, 1 << k, (1 << k) + 1):
            for over in (0, 1):                    # f_end = S (touches) or S + 1 (overlaps by one base)
                f_end = S + over
                rows.append((f_end - length, f_end, f"len{length}_{'hit' if over else 'touch'}"))
    rows.sort(key=lambda r: r[0])
    text = H + "".join(ln("chr1", "gene", b + 1, e, f"ID={i}") for b, e, i in rows)
    add("length_classes", text, [("chr1", S, S + 5), ("chr1", S - 1, S)],
        literal=[[i for _, _, i in rows if i.endswith("hit")], [i for _, _, i in rows if i != "len1_hit"]])   # (len1_hit is [S, S + 1): it begins at the second locus's end)
    # ---- several features with one f_beg (file order), loci that share features, loci before the first and after the last
    text = H + "".join(ln("chr1", "t", 500, 500 + w, f"ID=same{j}") for j, w in enumerate((300, 5, 90, 5, 1000, 40))) + ln("chr1", "t", 900, 950, "ID=late")
    add("same_start_shared", text, [("chr1", 0, 499), ("chr1", 499, 503), ("chr1", 502, 560), ("chr1", 600, 905), ("chr1", 1500, 1600)],
        literal=[[], [f"same{j}" for j in range(6)], [f"same{j}" for j in range(6)], ["same0", "same4", "late"], []])
    # ---- text seams: lines across the 256-byte step and the 1 024-byte tile; 63 / 64 / 65 / 129 lines
    for n_lines in (63, 64, 65, 129):
        text = "".join(ln("chr1", "exon", 10 * i + 1, 10 * i + 12, f"ID=e{i};Note=" + "x" * (i % 37)) for i in range(n_lines))
        add(f"lines_{n_lines}", text, [("chr1", 10 * (n_lines - 2), 10 * n_lines), ("chr1", 0, 5), ("chr1", 300, 331)])
    for at in (256, 1024):
        for shift in (-1, 0, 1):
            text = _pad_to(H, at - 20 + shift) + ln("chr1", "gene", 5, 50, "ID=straddles;Name=s") + ln("chr1", "gene", 7, 9, "ID=behind")
            add(f"seam_{at}_{shift + 1}", text, [("chr1", 0, 100)], literal=[["straddles", "behind"]])
    # ---- attribute columns longer than 64, 128 and 1 000 bytes, ID first, last, and across a 64-byte step
    for size in (64, 128, 1000):
        fill = ";".join(f"k{j}=v{j}" for j in range(size // 6 + 1))
        variants = [f"ID=first{size};{fill}", f"{fill};ID=last{size}"]
        for cut in (62, 63, 64, 65):            # the piece "ID=..." begins at byte `cut` of the column
            head = ("k=" + "y" * 200)[:cut - 1] + ";"
            variants.append(f"{head}ID=at{cut}_{size};{fill}")
        text = "".join(ln("chr1", "gene", 10 + j, 100, a) for j, a in enumerate(variants))
        add(f"attr_{size}", text, [("chr1", 50, 60)],
            literal=[[f"first{size}", f"last{size}"] + [f"at{cut}_{size}" for cut in (62, 63, 64, 65)]])
    # ---- CRLF, a last line without '\n', comment and blank lines between records, no ##FASTA, no header at all
    add("crlf", H.replace("\n", "\r\n") + ln("chr1", "gene", 5, 50, "ID=one", nl="\r\n") + ln("chr1", "gene", 6, 50, "ID=two", nl="\r\r\n") + "\r\n"
        + ln("chr1", "exon", 7, 50, "Parent=two", nl="\r\n"), [("chr1", 0, 100)], literal=[["one", "two", "exon:chr1-6-50"]])
    add("no_trailing_newline", ln("chr1", "gene", 5, 50, "ID=one") + ln("chr1", "gene", 6, 50, "ID=last;x=1", nl=""), [("chr1", 0, 100)], literal=[["one", "last"]])
    add("no_trailing_newline_cr", ln("chr1", "gene", 5, 50, "ID=one") + ln("chr1", "gene", 6, 50, "ID=last", nl="\r"), [("chr1", 0, 100)], literal=[["one", "last"]])
    add("comments_between", "\n\n" + H + "\n" + ln("chr1", "gene", 5, 50, "ID=one") + "# a comment\n\n###\n" + ln("chr1", "gene", 6, 50, "ID=two") + "\n",
        [("chr1", 0, 100)], literal=[["one", "two"]])
    # ---- ids
    ids = (H + ln("chr1", "gene", 10, 90, "ID=first;Name=n;ID=second") + ln("chr1", "gene", 11, 90, "geneID=g;Parent_ID=p;ID2=q;xID=r")
           + ln("chr1", "CDS", 12, 90, "Parent=t1;exon_id=E1") + ln("chr1", "CDS", 13, 90, "Parent=t1") + ln("chr1", "exon", 14, 90, "Parent=t1;exon_id=E1")
           + ln("chr1", "five_prime_UTR", 15, 90, ".") + ln("chr1", "gene", 16, 90, "Name=n;ID=trail;") + ln("chr1", "gene", 17, 90, "ID=;Name=empty")
           + ln("chr1", "gene", 18, 90, "Name=x; ID=spaced;  Alias=y") + ln("chr1", "gene", 19, 90, "ID=a%3Bb=c d") + ln("chr1", "gene", 20, 90, "ID")
           + ln("chr1", "3UTR", 21, 90, "exon_id=U1;ID=both") + ln("chr1", "stop_codon", 22, 90, "exon_id=one;exon_id=two") + ln("chr1", "gene", 23, 90, "ID =x;Name=y")
           + ln("chr1", "gene", 24, 90, "ID=ten", extra="\tcolumn ten"))
    add("ids_gff3", ids, [("chr1", 50, 60)],
        literal=[["second", "gene:chr1-10-90", "CDS:E1", "CDS:chr1-12-90", "exon:chr1-13-90", "five_prime_UTR:chr1-14-90", "trail", "", "spaced", "a%3Bb=c d", "",
                  "both", "stop_codon:two", "gene:chr1-22-90", "ten"]])
    gtf = (ln("1", "gene", 10, 90, 'gene_id "G1"; gene_name "a;b=c";') + ln("1", "CDS", 11, 90, 'gene_id "G1"; exon_number 007; exon_id "E;1";')
           + ln("1", "exon", 12, 90, 'gene_id "G1"; exon_id "E2";') + ln("1", "gene", 13, 90, 'gene_id "G1"; ID "quoted id"; note "x"')
           + ln("1", "gene", 14, 90, 'ID 007;') + ln("1", "gene", 15, 90, 'ID=5; gene_id "g"') + ln("1", "start_codon", 16, 90, 'exon_id   "padded"  ;')
           + ln("1", "gene", 17, 90, 'note "ID 9; inside"; gene_id "g"') + ln("1", "gene", 18, 90, 'ID "a"; ID "b"') + ln("1", "gene", 19, 90, 'ID "open; gene_id "g"')
           + ln("1", "gene", 20, 90, "ID") + ln("1", "gene", 21, 90, 'ID ""'))
    add("ids_gtf", gtf, [("chr1", 50, 60), ("1", 50, 60)], gtf=True,
        literal=[["gene:1-9-90", "CDS:E;1", "exon:1-11-90", "quoted id", "007", "gene:1-14-90", "start_codon:padded", "gene:1-16-90", "b", 'open; gene_id "g', "", ""]] * 2)
    # ---- contigs: chr1 beside chr10 and chr1_alt; the prefix on either side; a contig the file lacks; several contigs in one file
    text = (H + ln("chr1", "gene", 5, 50, "ID=on1") + ln("chr1", "gene", 40, 80, "ID=on1b") + ln("chr10", "gene", 5, 50, "ID=on10") + ln("chr1_alt", "gene", 5, 50, "ID=alt")
            + ln("2", "gene", 5, 50, "Name=two"))
    add("contigs", text, [("chr1", 0, 100), ("1", 0, 100), ("chr10", 0, 100), ("chr1_alt", 0, 100), ("chr2", 0, 100), ("2", 45, 60), ("chr7", 0, 100), ("chr1", 60, 61)],
        literal=[["on1", "on1b"], ["on1", "on1b"], ["on10"], ["alt"], ["gene:2-4-50"], ["gene:2-4-50"], [], ["on1b"]])
    # ---- a larger mixed text, a few thousand lines
    rng = np.random.default_rng(5)
    starts = np.sort(rng.integers(1, 400000, size=3000))
    text = H + ln("chr1", "region", 1, 500000, "ID=chr1:1..500000")
    for i, s in enumerate(starts.tolist()):
        length = int(2 ** rng.uniform(0, 14))
        kind = ("gene", "mRNA", "exon", "CDS")[i % 4]
        attrs = (f"ID=g{i};Name=N{i}", f"ID=r{i};Parent=g{i - 1}", f"Parent=r{i - 1}", f"Parent=r{i - 2};exon_id=E{i}")[i % 4] + (";Note=" + "n" * int(rng.integers(0, 150)))
        text += ln("chr1", kind, s, s + length, attrs)
    lo = np.sort(rng.integers(0, 400000, size=300))
    add("mixed_3000", text, [("chr1", int(s), int(s) + int(w)) for s, w in zip(lo, rng.integers(1, 400, size=300))], block_bytes=4096)
    # ---- errors: the call fails and names the line
    good = H + ln("chr1", "gene", 5, 50, "ID=ok")
    for name, bad in (("eight_fields", "chr1\tsrc\tgene\t60\t70\t.\t+\t.\n"), ("non_digit_start", ln("chr1", "gene", "6x", 70, "ID=b")),
                      ("end_before_start", ln("chr1", "gene", 60, 59, "ID=b")), ("start_zero", ln("chr1", "gene", 0, 59, "ID=b")),
                      ("descending", ln("chr1", "gene", 4, 59, "ID=b")), ("nineteen_digits", ln("chr1", "gene", 6, "1" * 19, "ID=b")),
                      ("bad_on_another_contig", ln("chr2", "gene", "+6", 70, "ID=b"))):
        add("error_" + name, good + bad + ln("chr1", "gene", 80, 90, "ID=after"), [("chr1", 0, 100)], bad_off=len(good))
    return tuple(out)


def check_literals() -> None:
    """The rule against the ids written out by hand."""
    n = 0
    for case in cases():
        if case.literal is not None:
            assert expected(case) == case.literal, case.name
            n += 1
    assert n >= 20, n


def written(case: Case, directory: str) -> str:
    """The case as a BGZF file with its .tbi under `directory` (written once)."""
    from strkit_amd.frontend.synth_annot import index_annotations
    path = os.path.join(directory, case.name + (".gtf.gz" if case.gtf else ".gff3.gz"))
    if not os.path.exists(path + ".tbi"):
        index_annotations(case.text, path, case.block_bytes)
    return path


def dump(directory: str) -> None:
    """What tools/gff_asan.cpp reads: <name>.txt (the text) and <name>.q: "gtf <0|1>", then "refuse <offset>" or one line per
    (contig, locus list): contig n s e ..., then per locus its ids' count and the ids, one per line, prefixed with '='."""
    os.makedirs(directory, exist_ok=True)
    for case in cases():
        with open(os.path.join(directory, case.name + ".txt"), "wb") as fh:
            fh.write(case.text)
        with open(os.path.join(directory, case.name + ".q"), "w", encoding="latin-1") as fh:
            fh.write(f"gtf {int(case.gtf)}\n")
            if case.bad_off is not None:
                fh.write(f"refuse {case.bad_off} {case.loci[0][0]}\n")
                continue
            want = expected(case)
            names = file_contigs(case)
            for contig in dict.fromkeys(l[0] for l in case.loci):
                name = resolve_contig(names, contig)
                if name is None:
                    continue
                idx = sorted((i for i, l in enumerate(case.loci) if l[0] == contig), key=lambda i: case.loci[i][1:])
                fh.write(f"query {name} {len(idx)}" + "".join(f" {case.loci[i][1]} {case.loci[i][2]}" for i in idx) + "\n")
                for i in idx:
                    fh.write(f"{len(want[i])}\n" + "".join(f"={x}\n" for x in want[i]))


def overlaps(L, src, n: int, start: int, contig: str, gtf: bool, starts, ends, final: int = 1, prev: int = -1, tile: int = 0):
    """One strk_gff_overlaps (src: a uint8 array) or strk_dbam_gff_overlaps (src: a strk_dbam handle) call, with the size query ->
    (return code or number of pairs, per-locus id lists, end_off, past, last f_beg)."""
    ls, le = np.ascontiguousarray(starts, np.int64), np.ascontiguousarray(ends, np.int64)
    caps = [0, 0, 0]
    for _ in range(2):
        pl, pf = np.empty(max(caps[0], 1), np.int32), np.empty(max(caps[0], 1), np.int32)
        fb, fe, fk, fo = (np.empty(max(caps[1], 1), np.int64), np.empty(max(caps[1], 1), np.int64), np.empty(max(caps[1], 1), np.int32),
                          np.empty(2 * caps[1] + 1, np.int64))
        text = np.empty(max(caps[2], 1), np.uint8)
        sizes, end_off, past = np.full(4, -7, np.int64), C.c_int64(0), C.c_int32(0)
        tail = (len(ls), ls.ctypes.data, le.ctypes.data, caps[0], pl.ctypes.data, pf.ctypes.data, caps[1], fb.ctypes.data, fe.ctypes.data, fk.ctypes.data,
                fo.ctypes.data, caps[2], text.ctypes.data, sizes.ctypes.data, C.byref(end_off), C.byref(past))
        if isinstance(src, np.ndarray):
            k = L.strk_gff_overlaps(src.ctypes.data, n, start, contig.encode(), int(gtf), final, prev, *tail)
        else:
            k = L.strk_dbam_gff_overlaps(src, start, contig.encode(), int(gtf), final, prev, tile, *tail)
        if k < 0:
            return int(k), None, 0, 0, -1
        if all(int(sizes[i]) <= caps[i] for i in range(3)):
            break
        caps = [int(sizes[i]) for i in range(3)]       # exactly what the size query asked for
    assert int(k) == int(sizes[0])
    raw = text[:int(sizes[2])].tobytes()
    ids = []
    for j in range(int(sizes[1])):
        t, v = raw[fo[2 * j]:fo[2 * j + 1]].decode("latin-1"), raw[fo[2 * j + 1]:fo[2 * j + 2]].decode("latin-1")
        ids.append(v if fk[j] == 0 else f"{t}:{v}" if fk[j] == 1 else f"{t}:{contig}-{int(fb[j])}-{int(fe[j])}")
    out = [[] for _ in range(len(ls))]
    assert np.all(np.diff(pl[:int(k)]) >= 0)           # locus order
    for l, j in zip(pl[:int(k)].tolist(), pf[:int(k)].tolist()):
        out[l].append(ids[j])
    return int(k), out, int(end_off.value), int(past.value), int(sizes[3])


def case_through_abi(L, case: Case, src, n: int, tile: int = 0):
    """The per-locus lists of a case, contig by contig, through the C ABI (loci sorted by start, as callers pass them)."""
    names = file_contigs(case)
    out = [[] for _ in case.loci]
    for contig in dict.fromkeys(l[0] for l in case.loci):
        name = resolve_contig(names, contig)
        if name is None:
            continue
        idx = sorted((i for i, l in enumerate(case.loci) if l[0] == contig), key=lambda i: case.loci[i][1:])
        k, got, end_off, _past, _last = overlaps(L, src, n, 0, name, case.gtf, [case.loci[i][1] for i in idx], [case.loci[i][2] for i in idx], tile=tile)
        assert k >= 0, L.strk_last_error()
        assert end_off == n
        for i, ids in zip(idx, got):
            out[i] = ids
    return out
