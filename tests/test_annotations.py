"""CPU: locus annotations.  strk_gff_overlaps against frontend/annotations.py's rule on the corpus of annot_cases.py
(and the rule against the ids written out by hand); IndexedAnnotations on the host cores against read_annotations + annotate on the
synth_annot files, whole and in small pieces; the opt-in tabix preset; the option type; the CLI; call_sample with the host front
end; write_vcf."""
import ctypes as C
import dataclasses
import gzip
import os
import subprocess

import numpy as np
import pytest

import annot_cases
from strkit_amd import _lib
from strkit_amd.frontend import options as O
from strkit_amd.frontend.annotations import AnnotationError, IndexedAnnotations, annotate, read_annotations
from strkit_amd.frontend.synth_annot import annotation_text, index_annotations, make_annotations
from strkit_amd.frontend.tabix import TabixIndex

CASES = annot_cases.cases()
GOOD = [c for c in CASES if c.bad_off is None]
BAD = [c for c in CASES if c.bad_off is not None]


def _err():
    return _lib.load().strk_last_error().decode()


def test_the_rule_gives_the_ids_written_out_by_hand():
    annot_cases.check_literals()
    assert len(BAD) >= 5 and any(c.gtf for c in GOOD)


@pytest.mark.parametrize("case", GOOD, ids=lambda c: c.name)
def test_host_entry_equals_the_rule(case):
    L = _lib.load()
    buf = np.frombuffer(case.text, np.uint8).copy()
    assert annot_cases.case_through_abi(L, case, buf, len(case.text)) == annot_cases.expected(case)


@pytest.mark.parametrize("case", BAD, ids=lambda c: c.name)
def test_refusals_name_the_line(case):
    L = _lib.load()
    buf = np.frombuffer(case.text, np.uint8).copy()
    k, *_ = annot_cases.overlaps(L, buf, len(case.text), 0, case.loci[0][0], case.gtf, [0], [100])
    assert k == _lib.STRK_E_INVALID and f"line at byte {case.bad_off}:" in _err(), _err()
    with pytest.raises(AnnotationError) as e:
        annot_cases.expected(case)
    assert e.value.offset == case.bad_off


def test_pieces_resume_and_check_order_across_them():
    """A text cut at every line start into two pieces: the second resumes at end_off with the first one's last f_beg; per locus the
    ids of both pieces, in that order, are the whole text's.  A descent across the cut is refused through prev_beg."""
    L = _lib.load()
    case = next(c for c in GOOD if c.name == "same_start_shared")
    buf = np.frombuffer(case.text, np.uint8).copy()
    n = len(case.text)
    idx = sorted(range(len(case.loci)), key=lambda i: case.loci[i][1:])
    ls, le = [case.loci[i][1] for i in idx], [case.loci[i][2] for i in idx]
    want = [annot_cases.expected(case)[i] for i in idx]
    for cut in [i + 1 for i, b in enumerate(case.text) if b == 10] + [n - 3, 40]:
        k1, a, end_off, _past, last = annot_cases.overlaps(L, buf, cut, 0, "chr1", False, ls, le, final=0)
        assert k1 >= 0 and end_off <= cut and (end_off == 0 or case.text[end_off - 1] == 10)
        k2, b, end2, _past, _ = annot_cases.overlaps(L, buf, n, end_off, "chr1", False, ls, le, final=1, prev=last)
        assert k2 >= 0 and end2 == n and [x + y for x, y in zip(a, b)] == want, cut
    k, *_ = annot_cases.overlaps(L, buf, n, 0, "chr1", False, ls, le, prev=5000)
    assert k == _lib.STRK_E_INVALID and "not coordinate-sorted" in _err() and "line at byte 16:" in _err()


def test_past_flag_and_bad_arguments():
    L = _lib.load()
    case = next(c for c in GOOD if c.name == "contigs")
    buf = np.frombuffer(case.text, np.uint8).copy()
    n = len(case.text)
    assert annot_cases.overlaps(L, buf, n, 0, "chr1", False, [0], [100])[3] == 1        # chr10 follows chr1
    assert annot_cases.overlaps(L, buf, n, 0, "2", False, [0], [100])[3] == 0           # nothing follows the last contig
    assert annot_cases.overlaps(L, buf, n, 0, "chr7", False, [0], [100])[3] == 0        # never seen
    assert annot_cases.overlaps(L, buf, n, 0, "chr7", False, [0], [100], prev=3)[3] == 1   # seen in an earlier piece
    for start in (n + 1, -1):
        k, *_ = annot_cases.overlaps(L, buf, n, start, "chr1", False, [0], [100])
        assert k == _lib.STRK_E_INVALID and "outside the text" in _err()
    k, *_ = annot_cases.overlaps(L, buf, n, 0, "", False, [0], [100])
    assert k == _lib.STRK_E_INVALID and "contig" in _err()
    out3 = (C.c_int32 * 3)()
    L.strk_gff_constants(out3)
    assert list(out3) == [64, 64, 64]


def test_the_stand_alone_checker_builds_plain_and_passes(tmp_path):
    """tools/gff_asan.cpp (a program of its own; tools/gff_asan.sh builds it with -fsanitize=address,undefined), built plain here."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = tmp_path / "gff_check"
    subprocess.run(["g++", "-O2", "-std=c++17", "-o", str(exe), os.path.join(root, "tools", "gff_asan.cpp")], check=True)
    annot_cases.dump(str(tmp_path / "corpus"))
    r = subprocess.run([str(exe), str(tmp_path / "corpus")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and f"{len(CASES)} cases" in r.stdout and " 0 failed" in r.stdout, r.stdout + r.stderr


# ---- the indexed reader on the host cores -----------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def synth(tmp_path_factory):
    rng = np.random.default_rng(3)
    loci = []
    for contig, n in (("chr1", 300), ("chr2", 100), ("chr3", 20)):
        s = np.sort(rng.integers(5000, 2_000_000, size=n))
        loci += [(contig, int(a), int(a) + int(w)) for a, w in zip(s, rng.integers(6, 300, size=n))]
    lengths = {"chr1": 2_200_000, "chr2": 2_100_000, "chrEmpty": 1000, "chr3": 2_300_000, "chrX_features": 50_000}
    paths = make_annotations(str(tmp_path_factory.mktemp("synth_annot")), loci, lengths, block_bytes=4096)
    # a contig without features, a contig neither file has, one locus over nearly a whole contig, named without its prefix
    return paths, loci + [("chrEmpty", 10, 20), ("chr9", 10, 20), ("3", 100, 2_000_000)]


@pytest.mark.parametrize("piece_bytes", [32 << 20, 6000, 1])
@pytest.mark.parametrize("kind", ["gff3", "gtf"])
def test_indexed_reader_on_the_host_equals_the_rule(synth, kind, piece_bytes):
    """6000: pieces of one 4 096-byte block, so that lines span two pieces and the hits of the contig-long locus come from all of them."""
    paths, loci = synth
    want = annotate(loci, read_annotations(paths[kind]))
    r = IndexedAnnotations(paths[kind], front_end="host", piece_bytes=piece_bytes)
    got = annotate(loci, r)
    assert got == want
    assert len(want[-1]) > 50 and want[-3] == want[-2] == [] and sum(map(len, want)) > 2 * len(loci)
    assert r.text_bytes > 0 and r.compressed_bytes > 0 and r.seconds > 0 and r.n_queries == 4 and r.kernel_ms == [0.0, 0.0]      # (chr1, chr2, chr3 and "3")
    if piece_bytes == 32 << 20:        # one walk per contig: the file's text once, plus at most the block two contigs share, per contig
        once = IndexedAnnotations(paths[kind])
        annotate(loci[:-1], once)
        assert once.n_queries == 3 and once.text_bytes <= len(gzip.decompress(open(paths[kind], "rb").read())) + 3 * 4096
    # loci in any order give the same lists in that order
    rev = list(reversed(loci))
    assert annotate(rev, IndexedAnnotations(paths[kind])) == list(reversed(want))


@pytest.mark.parametrize("case", [c for c in GOOD if not c.name.startswith("mixed")], ids=lambda c: c.name)
def test_indexed_reader_on_the_corpus(case, tmp_path):
    r = IndexedAnnotations(annot_cases.written(case, str(tmp_path)), piece_bytes=1 if case.name.startswith("hit") else 32 << 20)
    assert annotate(case.loci, r) == annot_cases.expected(case)


def test_a_file_without_index_or_bgzf_is_refused(tmp_path):
    text = annotation_text([("chr1", 100, 200)], {"chr1": 10000}, gene_share=0.0)
    plain = tmp_path / "genes.gff3"
    plain.write_bytes(text)
    assert read_annotations(str(plain)).contig_overlaps("1", [100], [200]) == [["chr1:1..10000"]]
    with pytest.raises(ValueError, match="BGZF-compressed with a tabix index"):
        IndexedAnnotations(str(plain))
    gz = index_annotations(text, str(tmp_path / "genes.gff3.gz"))
    os.remove(gz + ".tbi")
    with pytest.raises(ValueError, match="tabix index"):
        IndexedAnnotations(gz)
    with pytest.raises(ValueError, match="front_end"):
        IndexedAnnotations(gz, front_end="gpu")


def test_the_gff_preset_is_opt_in(synth):
    paths, _ = synth
    tbi = paths["gff3"] + ".tbi"
    with pytest.raises(ValueError, match="not the index of a VCF"):
        TabixIndex(tbi)
    with pytest.raises(ValueError, match="not the index of a VCF"):
        TabixIndex(tbi, paths["gff3"])
    idx = TabixIndex(tbi, paths["gff3"], preset="gff")
    assert idx.names == ["chr1", "chr2", "chr3", "chrX_features"] and idx.contig_range("chrEmpty") is None
    start, last = idx.contig_range("1")
    assert start == idx.block_range("chr1", 0, 1 << 29)[0] and last < os.path.getsize(paths["gff3"])
    with pytest.raises(ValueError, match="preset"):
        TabixIndex(tbi, preset="bed")


def test_a_vcf_index_is_not_a_gff_index(tmp_path):
    from strkit_amd.frontend.synth_snvs import index_snv_vcf, make_dbsnp_like
    make_dbsnp_like(str(tmp_path / "s.vcf"), 50)
    gz = index_snv_vcf(str(tmp_path / "s.vcf"))
    TabixIndex(gz + ".tbi")
    with pytest.raises(ValueError, match="not the index of a GFF3 / GTF"):
        TabixIndex(gz + ".tbi", preset="gff")


# ---- options, CLI ------------------------------------------------------------------------------------------------------------------
def test_options_widen_validate_and_report(synth, tmp_path):
    paths, _ = synth
    plain = O.with_keywords(None, flank_size=50)
    assert type(plain) is O.CallOptions and "annotation_file" not in O.report_parameters(plain, 1)
    opts = O.with_keywords(None, annotation_file=paths["gff3"], flank_size=50)
    assert type(opts) is O.AnnotationCallOptions and isinstance(opts, O.ReadSelectionCallOptions) and opts.flank_size == 50
    assert O.ANNOTATION_OPTION_NAMES == ("annotation_file",)
    assert [f.name for f in dataclasses.fields(O.AnnotationCallOptions)][-1] == "annotation_file"
    opts.validate()
    assert O.report_parameters(opts, 1)["annotation_file"] == paths["gff3"]
    assert list(O.report_parameters(opts, 1))[:-1] == list(O.report_parameters(plain, 1))
    wide = O.with_keywords(O.ReadSelectionCallOptions(unique_reads=True), annotation_file=paths["gtf"])
    assert type(wide) is O.AnnotationCallOptions and wide.unique_reads
    assert "annotation_file" not in O.report_parameters(O.AnnotationCallOptions(), 1)
    with pytest.raises(ValueError, match="does not exist"):
        O.with_keywords(None, annotation_file=str(tmp_path / "none.gff3.gz")).validate()
    lone = tmp_path / "lone.gff3.gz"
    lone.write_bytes(b"x")
    with pytest.raises(ValueError, match="no tabix index"):
        O.with_keywords(None, annotation_file=str(lone)).validate()


def test_cli_parser():
    from strkit_amd.__main__ import build_parser
    ap = build_parser()
    base = ["call", "r.bam", "--ref", "r.fa", "--loci", "l.bed"]
    assert ap.parse_args(base).annotation_file is None
    assert ap.parse_args(base + ["--gff", "g.gff3.gz"]).annotation_file == "g.gff3.gz"
    assert ap.parse_args(base + ["--annotation-file", "g.gtf.gz"]).annotation_file == "g.gtf.gz"


# ---- call_sample, write_vcf --------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def dataset(tmp_path_factory):
    from strkit_amd.frontend.synth_dataset import make_dataset
    d = tmp_path_factory.mktemp("annot_ds")
    ds = make_dataset(str(d / "ds"), n_loci=4, reads_per_locus=6, read_len=1500, seed=2)
    ds["annot"] = make_annotations(str(d / "annot"), ds["loci"], {"chr1": 40000, "chrOther_features": 500})
    return ds


def _strip(report: dict) -> dict:
    return {k: v for k, v in report.items() if k not in ("runtime", "stage_times")}


def test_cli_refuses_a_missing_file(dataset, capsys):
    from strkit_amd.__main__ import main
    p = dataset["paths"]
    with pytest.raises(SystemExit):
        main(["call", p["bam"], "--ref", p["ref"], "--loci", p["loci"], "--gff", p["loci"] + ".none.gz"])
    assert "tabix index" in capsys.readouterr().err


def test_call_sample_annotates_the_merged_rows(dataset, monkeypatch):
    """call_sample with a stubbed block loop (no device): every row, the one without reference data included, gets its list, from
    the catalog's coordinates and the file alone; stage_times gets annotate_s; without the option nothing is read."""
    from strkit_amd.frontend import call
    from strkit_amd.frontend.block import _locus_dict

    def fake_call_blocks(blocks, bam, ref, opts=None, ctx=None, ref_cache=None):
        rows = [_locus_dict(locus) for block in blocks for locus in block]
        return rows, 0, {"errors": []}

    class Reader:
        references = ["chr1"]

    monkeypatch.setattr(call, "call_blocks", fake_call_blocks)
    p = dataset["paths"]
    for kind in ("gff3", "gtf"):
        rep = call.call_sample(Reader(), Reader(), p["loci"], annotation_file=dataset["annot"][kind])
        want = annotate([("chr1", l["start"], l["end"]) for l in dataset["loci"]], read_annotations(dataset["annot"][kind]))
        assert [r["annotations"] for r in rep["results"]] == want and all(len(w) >= 2 for w in want)
        assert rep["stage_times"]["annotate_s"] > 0 and rep["parameters"]["annotation_file"] == dataset["annot"][kind]
    rep = call.call_sample(Reader(), Reader(), p["loci"])
    assert all(r["annotations"] == [] for r in rep["results"]) and "annotate_s" not in rep["stage_times"] and "annotation_file" not in rep["parameters"]


@pytest.mark.gpu        # (a real call counts its reads on the device, whatever the front end)
@pytest.mark.parametrize("kind", ["gff3", "gtf"])
def test_call_sample_fills_annotations_and_changes_nothing_else(dataset, kind, tmp_path):
    from strkit_amd.frontend import call_sample
    p = dataset["paths"]
    plain = call_sample(p["bam"], p["ref"], p["loci"], front_end="host")
    with_gff = call_sample(p["bam"], p["ref"], p["loci"], front_end="host", annotation_file=dataset["annot"][kind])
    want = annotate([(r["contig"], r["start"], r["end"]) for r in plain["results"]], read_annotations(dataset["annot"][kind]))
    assert [r["annotations"] for r in with_gff["results"]] == want and all(want)
    assert all(r["annotations"] == [] for r in plain["results"])
    assert "annotate_s" in with_gff["stage_times"] and "annotate_s" not in plain["stage_times"]
    assert with_gff["parameters"].pop("annotation_file") == dataset["annot"][kind]
    for r in with_gff["results"]:
        r["annotations"] = []
    assert _strip(with_gff) == _strip(plain)


def _report(annotation_file=None, annotations=()):
    row = {"locus_index": 1, "locus_id": "syn0", "contig": "chr1", "start": 100, "end": 112, "motif": "CAG", "annotations": list(annotations),
           "assign_method": None, "call": None, "call_95_cis": None, "call_99_cis": None, "ref_cn": 4, "ref_start_anchor": "ACGTA",
           "ref_seq": "CAGCAGCAGCAG", "peaks": None, "read_peaks_called": False, "reads": {}}
    bare = dict(row, locus_index=2, locus_id="syn1", start=300, end=312, annotations=[])
    return {"sample_id": "s", "parameters": {"flank_size": 70, **({"annotation_file": annotation_file} if annotation_file else {})},
            "contigs": ["chr1"], "results": [row, bare]}


def test_write_vcf_declares_and_writes_annot_only_with_the_option(tmp_path):
    from strkit_amd.frontend.output import write_vcf
    ids = ["gene1", "a b;c=d,e", "CDS:E1", "100%"]
    a, b, c = str(tmp_path / "a.vcf"), str(tmp_path / "b.vcf"), str(tmp_path / "c.vcf")
    assert write_vcf(_report("genes.gff3.gz", ids), a, date="20260101") == 2
    assert write_vcf(_report(None, ids), b, date="20260101") == 2       # annotations without the option (a hand-made report): nothing
    assert write_vcf(_report(None), c, date="20260101") == 2
    ta, tb, tc = (open(x).read() for x in (a, b, c))
    assert tb == tc and "ANNOT" not in tb
    head = '##INFO=<ID=ANNOT,Number=1,Type=String,Description="Locus annotations (e.g., genomic regions)">\n'
    assert head in ta and ta.index(head) > ta.index("##INFO=<ID=ANCH,")
    assert ta.replace(head, "").replace(";ANNOT=gene1,a%20b%3Bc%3Dd%2Ce,CDS:E1,100%25", "") == tb
    recs = [l for l in ta.splitlines() if not l.startswith("#")]
    assert ";ANCH=5;ANNOT=gene1," in recs[0].split("\t")[7] and "ANNOT" not in recs[1]
