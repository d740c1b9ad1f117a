"""GPU: strk_dbam_gff_overlaps (k_lines_count / k_lines_scan / k_lines_starts of strk_lines.h, k_gff_coords, k_gff_gather, k_gff_classes, k_gff_join,
k_gff_hits, k_gff_order, k_gff_ids, k_gff_text) on the corpus of annot_cases.py: identical to frontend/annotations.py's rule on every
case, with the default tile and with tile_bytes = 256; the refusals match the host's; the device IndexedAnnotations equals the host one
on the synth_annot files; one end-to-end `call --front-end device --gff` equals the host front end's report."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import annot_cases
from strkit_amd import _lib
from strkit_amd.frontend.annotations import IndexedAnnotations, annotate, read_annotations

pytestmark = pytest.mark.gpu

CASES = annot_cases.cases()


@pytest.fixture(scope="module")
def dbam():
    L = _lib.load()
    h = C.c_void_p()
    _lib.check(L.strk_dbam_open(0, C.byref(h)))
    yield h
    L.strk_dbam_close(h)


@pytest.fixture(scope="module")
def corpus_dir(tmp_path_factory):
    return str(tmp_path_factory.mktemp("annot_corpus"))


def _err():
    return _lib.load().strk_last_error().decode()


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_device_equals_the_rule(dbam, corpus_dir, case):
    L = _lib.load()
    n = L.strk_dbam_inflate_file(dbam, os.fsencode(annot_cases.written(case, corpus_dir)), 0, None)
    assert n == len(case.text), (_err(), n)
    buf = np.frombuffer(case.text, np.uint8).copy()
    for tile in annot_cases.TILES:
        if case.bad_off is not None:
            contig = case.loci[0][0]
            host = annot_cases.overlaps(L, buf, n, 0, contig, case.gtf, [0], [100])
            host_msg = _err()
            dev = annot_cases.overlaps(L, dbam, n, 0, contig, case.gtf, [0], [100], tile=tile)
            print(case.name, tile, "host", host[0], "device", dev[0], _err())
            assert host[0] == dev[0] == _lib.STRK_E_INVALID
            assert _err().replace("strk_dbam_gff_overlaps", "strk_gff_overlaps") == host_msg and f"line at byte {case.bad_off}:" in host_msg
            continue
        got = annot_cases.case_through_abi(L, case, dbam, n, tile=tile)
        want = annot_cases.expected(case)
        print(case.name, tile, sum(map(len, got)), "ids on the device,", sum(map(len, want)), "by the rule")
        assert got == want, (case.name, tile)


def test_arguments_are_checked_before_any_launch(dbam, corpus_dir):
    L = _lib.load()
    case = CASES[0]
    n = L.strk_dbam_inflate_file(dbam, os.fsencode(annot_cases.written(case, corpus_dir)), 0, None)
    for start in (n + 1, -1, 1 << 40):
        k, *_ = annot_cases.overlaps(L, dbam, n, start, "chr1", False, [0], [100])
        assert k == _lib.STRK_E_INVALID and "outside the text" in _err()
    k, *_ = annot_cases.overlaps(L, dbam, n, 0, "chr1", False, [0], [100], tile=100)
    assert k == _lib.STRK_E_INVALID and "tile_bytes" in _err()
    k, got, end_off, past, last = annot_cases.overlaps(L, dbam, n, n, "chr1", False, [0], [100], prev=7)   # nothing to read, nothing launched
    assert (k, got, end_off, past, last) == (0, [[]], n, 0, 7)
    k, got, *_ = annot_cases.overlaps(L, dbam, n, 0, "chr1", False, [], [])                                 # no loci: the text is still checked
    assert (k, got) == (0, [])
    out3 = (C.c_int32 * 3)()
    L.strk_gff_constants(out3)
    assert list(out3) == [64, 64, 64]


@pytest.fixture(scope="module")
def synth(tmp_path_factory):
    from strkit_amd.frontend.synth_annot import make_annotations
    rng = np.random.default_rng(3)
    loci = []
    for contig, n in (("chr1", 400), ("chr2", 150), ("chr3", 20)):
        s = np.sort(rng.integers(5000, 3_000_000, size=n))
        loci += [(contig, int(a), int(a) + int(w)) for a, w in zip(s, rng.integers(6, 300, size=n))]
    lengths = {"chr1": 3_200_000, "chr2": 3_100_000, "chrEmpty": 1000, "chr3": 3_300_000, "chrX_features": 50_000}
    paths = make_annotations(str(tmp_path_factory.mktemp("synth_annot")), loci, lengths, block_bytes=4096)
    return paths, loci + [("chrEmpty", 10, 20), ("chr9", 10, 20), ("3", 100, 3_000_000)]


@pytest.mark.parametrize("piece_bytes", [32 << 20, 6000])
@pytest.mark.parametrize("kind", ["gff3", "gtf"])
def test_indexed_reader_on_the_device_equals_the_host_one(synth, kind, piece_bytes):
    paths, loci = synth
    want = annotate(loci, read_annotations(paths[kind]))
    host = IndexedAnnotations(paths[kind], front_end="host", piece_bytes=piece_bytes)
    dev = IndexedAnnotations(paths[kind], front_end="device", piece_bytes=piece_bytes, tile_bytes=256 if piece_bytes < 1 << 20 else 0)
    try:
        got_h, got_d = annotate(loci, host), annotate(loci, dev)
        print(kind, piece_bytes, sum(map(len, got_d)), "ids,", dev.text_bytes, "text bytes, kernel ms", dev.kernel_ms)
        assert got_d == got_h == want
        assert sum(map(len, want)) > len(loci) and dev.kernel_s() > 0 and dev.text_bytes == host.text_bytes
    finally:
        dev.close()


def test_call_with_the_device_front_end_equals_the_host_front_end(tmp_path):
    from strkit_amd.__main__ import main
    from strkit_amd.frontend.synth_annot import make_annotations
    from strkit_amd.frontend.synth_dataset import make_dataset
    ds = make_dataset(str(tmp_path / "ds"), n_loci=4, reads_per_locus=6, read_len=1500, seed=2)
    gff = make_annotations(str(tmp_path / "annot"), ds["loci"], {"chr1": 40000})["gff3"]
    reports = {}
    for fe in ("host", "device"):
        out = str(tmp_path / f"{fe}.json")
        assert main(["call", ds["paths"]["bam"], "--ref", ds["paths"]["ref"], "--loci", ds["paths"]["loci"], "--json", out, "--vcf", str(tmp_path / f"{fe}.vcf"),
                     "--front-end", fe, "--gff", gff]) == 0
        with open(out) as fh:
            reports[fe] = json.load(fh)
        assert reports[fe]["stage_times"]["front_end"] == fe
    rows = {fe: [(r["locus_index"], r["annotations"]) for r in reports[fe]["results"]] for fe in reports}
    assert rows["device"] == rows["host"] and all(a for _, a in rows["host"])      # (every locus lies inside the region line)
    for key in ("parameters", "results", "contigs", "catalog"):
        assert reports["device"][key] == reports["host"][key], key
    with open(tmp_path / "host.vcf") as a, open(tmp_path / "device.vcf") as b:
        va, vb = [l for l in a if not l.startswith("##fileDate")], [l for l in b if not l.startswith("##fileDate")]
    assert va == vb and any(";ANNOT=" in l for l in va)
