"""CPU: the `mi` sub-command's parser, the readers of this project's JSON and VCF reports, the trio assembly and the report
writers, on the fixtures of tests/golden/mi (written by tests/golden/make_mi_golden.py, which says what every row is for).
The per-locus rule runs through strk_mi_trio_host (device="host"): nothing here needs a GPU."""
import gzip
import json
import os
import shutil

import numpy as np
import pytest

import mi_restatement as R
from strkit_amd import mi
from strkit_amd.__main__ import build_parser, main

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "mi")
CALLED = [("chr1", 1000, 1040, "CAG"), ("chr1", 2000, 2030, "AT"), ("chr1", 3000, 3024, "GGC"), ("chr2", 500, 548, "AAG"), ("chr2", 700, 730, "TG")]


def paths(ext):
    return [os.path.join(GOLDEN, f"{who}.{ext}") for who in ("child", "mother", "father")]


def test_parser_defaults_and_the_bare_test_flag():
    ap = build_parser()
    a = ap.parse_args(["mi", "c.json", "m.json", "f.json"])
    assert (a.cmd, a.child_calls, a.mother_calls, a.father_calls) == ("mi", "c.json", "m.json", "f.json")
    assert (a.caller, a.widen, a.contig, a.json, a.no_tsv, a.mismatch_out_mi, a.hist, a.bin_width) == ("strkit-json", 0.0, None, None, False, "pm1", False, 10)
    assert (a.test, a.sig_level, a.mt_corr, a.only_phased, a.seed) == ("none", 0.05, "none", False, None)
    assert ap.parse_args(["mi", "c", "m", "f", "--test"]).test == "x2"
    assert ap.parse_args(["mi", "c", "m", "f", "--test", "wmw-gt", "--mt-corr", "fdr_bh", "--caller", "strkit-vcf"]).test == "wmw-gt"
    with pytest.raises(SystemExit):
        ap.parse_args(["mi", "c", "m", "f", "--caller", "trgt"])
    with pytest.raises(SystemExit):
        main(["mi", "c", "m", "f", "--mt-corr", "fdr_tsbh"])
    c = ap.parse_args(["call", "x.bam", "--ref", "r.fa", "--loci", "l.bed"])      # call's parser is what it was
    assert (c.cmd, c.json, c.flank_size, c.max_reads, c.n_alleles, c.count_kmers, c.seed) == ("call", "-", 70, 250, 2, "none", None)


@pytest.mark.parametrize("ext", ["json", "vcf"])
def test_readers_and_assembly(ext):
    load = mi.load_trio_json if ext == "json" else mi.load_trio_vcf
    members = [load(p) for p in paths(ext)]
    child, mother, father = members
    assert child.contigs == {"chr1", "chr2", "chrX"} and len(child.loci) == 9 and len(father.loci) == 8
    assert ("chr1", 4000, 4020, "A") not in father.loci and mother.loci[("chr1", 5000, 5030, "TTA")] is None      # missing; failed call
    assert father.loci[("chr2", 100, 160, "CA")]["call"] == (31,)
    trio = mi.assemble_trio(*members)
    assert trio.keys == CALLED and trio.n_loci_skipped_ploidy == 1
    assert trio.n_loci_seen == 8 and sorted(trio.seen_lengths) == sorted([40, 30, 24, 20, 30, 60, 48, 30])      # without the sex contig
    assert trio.includes_seq == (ext == "vcf") and (trio.packed["seq_id"] is not None) == (ext == "vcf")
    assert trio.loci[0]["gt"] == [12, 15, 12, 13, 14, 15] and trio.loci[0]["ci95"][1] == (14, 16) and trio.loci[0]["ref_cn"] == 13
    assert sorted(trio.loci[0]["reads"][0]) == [11, 12, 12, 12, 12, 13]
    # the one-peak child of chr1:3000
    g0, g1 = trio.loci[2]["reads"][:2]
    assert sorted(g0 + g1) == [7, 7] + [8] * 8 + [9, 9] and len(g0) == len(g1) == 6
    if ext == "vcf":
        assert g0 == (7, 8, 8, 8, 8, 9) and g1 == (7, 8, 8, 8, 8, 9)      # interleaved: every other read of the sorted group
        assert trio.loci[0]["seqs"][0] == trio.loci[0]["seqs"][2] and trio.packed["seq_id"][0].tolist() == [0, 1, 0, 2, 3, 1]
    # two peaks assigned by SNVs stay as labelled, homozygous call or not
    assert sorted(trio.loci[4]["reads"][0]) == sorted(trio.loci[4]["reads"][1]) == [13, 14, 14, 14, 14, 15]
    assert mi.assemble_trio(*members, contigs=["chr2"]).keys == CALLED[3:]
    if ext == "vcf":
        assert mi.assemble_trio(*members, only_phased=True).keys == [("chr2", 500, 548, "AAG")]


def test_json_split_condition_and_seeded_shuffle():
    res = {"reads": {f"r{i}": {"cn": 5 + i, "p": i % 2} for i in range(8)}, "peaks": {"modal_n": 2}, "call": [6, 6], "assign_method": "dist"}
    res["reads"]["unassigned"] = {"cn": 99}

    def split(seed=1, **change):
        return mi.split_reads_json({**res, **change}, np.random.default_rng([seed, 0]))

    by_label = ((5, 7, 9, 11), (6, 8, 10, 12))
    a = split()
    assert sorted(a[0] + a[1]) == list(range(5, 13)) and len(a[0]) == 4 and a != by_label      # homozygous by distance: shuffled halves
    assert split(call=[6, 7]) == by_label and split(assign_method="snv") == by_label
    # the precedence as written: (n < 2 or len(set(call))) == 1 -- one peak splits whatever the call is
    b = split(peaks={"modal_n": 1}, call=[6, 7], reads={f"r{i}": {"cn": 5 + i, "p": 0} for i in range(8)})
    assert len(b) == 2 and len(b[0]) == 4 and sorted(b[0] + b[1]) == list(range(5, 13))
    no_method = {k: v for k, v in res.items() if k != "assign_method"}      # (a missing assign_method counts as "dist")
    assert mi.split_reads_json(no_method, np.random.default_rng([1, 0])) == a
    assert split(seed=1) == a and split(seed=2) != a
    t1 = mi.assemble_trio(*[mi.load_trio_json(p) for p in paths("json")])
    t2 = mi.assemble_trio(*[mi.load_trio_json(p) for p in paths("json")])
    t3 = mi.assemble_trio(*[mi.load_trio_json(p, seed=5) for p in paths("json")])
    assert t1.loci[2]["reads"] == t2.loci[2]["reads"] != t3.loci[2]["reads"]
    assert np.array_equal(t1.packed["cn"], t2.packed["cn"]) and mi.DEFAULT_SEED == 2718


def test_gzip_vcf_reads_the_same(tmp_path):
    gz = []
    for p in paths("vcf"):
        gz.append(str(tmp_path / (os.path.basename(p) + ".gz")))
        with open(p, "rb") as src, gzip.open(gz[-1], "wb") as dst:
            shutil.copyfileobj(src, dst)
    assert mi.assemble_trio(*[mi.load_trio_vcf(p) for p in gz]).loci == mi.assemble_trio(*[mi.load_trio_vcf(p) for p in paths("vcf")]).loci


@pytest.mark.parametrize("ext", ["json", "vcf"])
def test_result_report_and_tsv(ext, tmp_path):
    caller = "strkit-" + ext
    trio, out, res = mi.run_mi(*paths(ext), caller=caller, device="host")
    want = [R.respects_mi(l) for l in trio.loci]
    assert res["n_loci_trio_called"] == 5 and res["n_loci_total"] == 8 and res["n_loci_skipped_ploidy"] == 1
    for k in ("strict", "pm1", "ci_95"):
        assert res["mi"][k] == sum(w[k] for w in want) / 5
    assert res["mi"]["strict"] == 0.8 and res["mi"]["ci_99"] is None and (res["mi"]["seq"] is None) == (ext == "json")
    assert [trio.keys[i] for i in res["output_index"]] == [("chr1", 2000, 2030, "AT")]      # the de novo locus fails pm1
    assert [h["bin"] for h in res["hist"]] == [0, 10, 20, 30, 40, 50] and [h["bin_count"] for h in res["hist"]] == [0, 0, 1, 2, 2, 0]
    assert [h["bin_total"] for h in res["hist"]] == [0, 0, 2, 3, 2, 0] and res["hist"][3]["mi"] == 0.5 and res["hist"][0]["mi"] is None
    rows = mi.locus_tsv(trio, out, res).splitlines()
    assert rows == ["chr1\t2000\t2030\tAT\t10|15\t9,11|14,16\t\t10|11\t9,11|10,12\t\t12|13\t11,13|12,14\t\t15"]
    path = str(tmp_path / "mi.json")
    mi.write_report_json(trio, out, res, path)
    rep = json.load(open(path))
    assert list(rep) == ["mi", "mi_pm1", "mi_95", "mi_99", "mi_seq", "mi_sl", "mi_sl_pm1", "n_loci_trio_called", "n_loci_total",
                         "n_loci_skipped_ploidy", "test", "hist", "significant_loci"]
    assert rep["mi"]["val"] == 0.8 and rep["mi"]["est_std_err"] == pytest.approx((0.8 * 0.2 / 8) ** 0.5) and rep["mi_99"] is None
    assert rep["mi"]["est_95_ci"] == pytest.approx([0.8 - 1.96 * rep["mi"]["est_std_err"], 0.8 + 1.96 * rep["mi"]["est_std_err"]])
    assert rep["significant_loci"][0]["child_gt"] == [10, 15] and "p" not in rep["significant_loci"][0]
    # with a test: the loci rejected after the correction, sorted by adjusted p
    trio, out, res = mi.run_mi(*paths(ext), caller=caller, test="x2", mt_corr="fdr_bh", device="host")
    exp = [R.de_novo(l, "x2") for l in trio.loci]
    assert [float(p) for p in out["p"]] == pytest.approx([e["p"] for e in exp], rel=1e-9)
    rej, adj = R.multipletests([e["p"] for e in exp], 0.05, "fdr_bh")
    order = sorted((i for i in range(5) if rej[i]), key=lambda i: adj[i])
    assert res["output_index"] == order and trio.keys[order[0]] == ("chr1", 2000, 2030, "AT")
    cols = mi.locus_tsv(trio, out, res).splitlines()[0].split("\t")
    assert len(cols) == 17 and float(cols[14]) == out["p"][order[0]] and float(cols[15]) == pytest.approx(adj[order[0]]) and cols[16] == exp[order[0]]["mutation_from"]
    sig = mi.report_object(trio, out, res)["significant_loci"][0]
    assert sig["p"] == out["p"][order[0]] and sig["mutation_from"] == cols[16] and sig["p_adj"] == pytest.approx(adj[order[0]])


def test_command_line(tmp_path, capsys, monkeypatch):
    real = mi.mi_trio_batch
    monkeypatch.setattr(mi, "mi_trio_batch", lambda *a, **kw: real(*a, **{**kw, "device": "host"}))      # (no GPU in this test)
    out_json = str(tmp_path / "r.json")
    assert main(["mi", *paths("vcf"), "--caller", "strkit-vcf", "--test", "--hist", "--json", out_json]) == 0
    text = capsys.readouterr().out
    assert text.startswith("chr1\t2000\t2030\tAT\t") and "MI% (±1)" in text and "0-9\t10-19" in text
    assert json.load(open(out_json))["test"] == "x2"


def test_synthetic_trio_dataset(tmp_path):
    from strkit_amd.frontend import NativeBam
    from strkit_amd.frontend.synth_trio import MEMBERS, make_trio_dataset
    t = make_trio_dataset(str(tmp_path), n_loci=6, de_novo=(1, 4), reads_per_haplotype=3)
    assert len(t["loci"]) == 6 and [L["index"] for L in t["loci"] if L["de_novo"]] in ([1, 4], [4, 1])
    assert {L["contig"] for L in t["loci"]} == {"chr1", "chr2"}
    for L in t["loci"]:
        m, f = L["mother"][L["inherited"][0]], L["father"][L["inherited"][1]]
        want = [m, f]
        if L["de_novo"]:
            assert 1 <= L["de_novo"][1] <= 3
            want[L["de_novo"][0]] += L["de_novo"][1]
        assert L["child"] == tuple(want) and L["mother"][0] < L["mother"][1] and L["father"][0] < L["father"][1]
    bed = open(t["paths"]["loci"]).read().splitlines()
    assert len(bed) == 6 and bed[0].split("\t")[0] == "chr1" and "MOTIF=" + t["loci"][0]["motif"] in bed[0]
    for member in MEMBERS:
        bam = NativeBam(t["paths"][member])
        assert bam.rec_off.size == 6 * 2 * 3 and bam.name(0).startswith(member + "_l")
    again = make_trio_dataset(str(tmp_path / "again"), n_loci=6, de_novo=(1, 4), reads_per_haplotype=3)
    assert again["loci"] == t["loci"]
