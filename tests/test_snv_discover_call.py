"""`call --discover-snvs` on the data set of frontend/synth_phased.py (12 loci x 24 reads of 3 kb; every locus has heterozygous
flank sites, and homozygous decoys that a pileup must not select).

CPU: the rule and the host function select, per locus, exactly the truth's heterozygous positions; the option refusals; the
report's parameters.  The allele call itself runs on the GPU whichever reader feeds it, so the reports are compared in the `gpu`
part: the device front end, the native host reader and the readable block path give one report, and every row equals the row of
`--incorporate-snvs snvs.vcf` in call, peaks, assign_method, the SNVs' pos / ref / call / rcs and per read p and snvu; only the
SNVs' ids differ (the VCF's ID against <contig>_<1-based position>)."""
import json
import os

import numpy as np
import pytest

from strkit_amd.__main__ import build_parser, main
from strkit_amd.frontend import Fasta, NativeBam, call_sample, load_loci, read_bam
from strkit_amd.frontend import snv_discovery as sd
from strkit_amd.frontend.call import call_blocks
from strkit_amd.frontend.gather import SHARDING_REFUSALS
from strkit_amd.frontend.options import (SNV_DISCOVERY_OPTION_NAMES, AnnotationCallOptions, CallOptions, SnvDiscoveryCallOptions, phased, report_parameters,
                                         with_keywords)
from strkit_amd.frontend.output import write_vcf
from strkit_amd.frontend.synth_phased import make_phased_dataset

SEED = 4321


@pytest.fixture(scope="module")
def data(tmp_path_factory):
    return make_phased_dataset(str(tmp_path_factory.mktemp("discover_call")))


# ---- CPU ----------------------------------------------------------------------------------------------------------------------
def test_the_rule_selects_exactly_the_heterozygous_sites(data):
    bam = read_bam(data["paths"]["bam"])
    loci = [l for block in load_loci(data["paths"]["loci"]) for l in block]
    assert len(loci) == 12
    for locus, truth in zip(loci, data["loci"]):
        segs = bam.fetch(locus.contig, locus.left_flank_coord, locus.right_flank_coord)
        entries = [(s, False) for s in segs]
        assert len(segs) == 24                                   # a_thr = max(rint(24 / 5), 2) = 5
        got = sd.discover_candidates(entries, entries, locus.left_flank_coord, locus.right_flank_coord)
        assert got.tolist() == truth["het"] and not set(got.tolist()) & set(truth["decoys"]), locus.locus_id


def test_the_host_function_selects_exactly_the_heterozygous_sites(data):
    bam = NativeBam(data["paths"]["bam"])
    loci = [l for block in load_loci(data["paths"]["loci"]) for l in block]
    rec = [bam.fetch_indices(l.contig, l.left_flank_coord, l.right_flank_coord) for l in loci]
    n = np.array([r.size for r in rec])
    off, pos = sd.library_discover_snvs(bam, np.concatenate(rec), np.repeat(np.arange(12), n), [l.left_flank_coord for l in loci],
                                        [l.right_flank_coord for l in loci], np.concatenate(([0], np.cumsum(n))), np.arange(n.sum()))
    assert [pos[off[l]:off[l + 1]].tolist() for l in range(12)] == [t["het"] for t in data["loci"]]


def test_options():
    names = lambda t: [f.name for f in __import__("dataclasses").fields(t)]  # noqa: E731
    assert SNV_DISCOVERY_OPTION_NAMES == ("discover_snvs", "snv_discover_window")
    assert names(SnvDiscoveryCallOptions) == names(AnnotationCallOptions) + list(SNV_DISCOVERY_OPTION_NAMES)
    assert not set(names(AnnotationCallOptions)) & set(SNV_DISCOVERY_OPTION_NAMES)
    wide = with_keywords(CallOptions(flank_size=55), discover_snvs=True, call_alleles=True, seed=1)
    assert type(wide) is SnvDiscoveryCallOptions and wide.flank_size == 55 and wide.snv_discover_window == 8192 and phased(wide)
    wide.validate()
    assert type(with_keywords(None, snv_discover_window=100)) is SnvDiscoveryCallOptions and not phased(with_keywords(None, snv_discover_window=100))
    assert type(with_keywords(None, annotation_file=None)) is AnnotationCallOptions          # (the narrower types stay what they were)
    with pytest.raises(ValueError, match="requires call_alleles"):
        with_keywords(None, discover_snvs=True).validate()
    with pytest.raises(ValueError, match="two sources"):
        with_keywords(None, discover_snvs=True, call_alleles=True, seed=1, snv_vcf="x.vcf").validate()
    with pytest.raises(ValueError, match="snv_phase_sets=True requires snv_vcf"):
        with_keywords(None, discover_snvs=True, call_alleles=True, seed=1, snv_phase_sets=True).validate()
    for w in (0, 65537, 2.5, True):
        with pytest.raises(ValueError, match="snv_discover_window"):
            with_keywords(None, snv_discover_window=w).validate()
    with pytest.raises(ValueError, match="discover_snvs must be"):
        with_keywords(None, discover_snvs=1, call_alleles=True, seed=1).validate()
    # the report's parameters carry the two names only with the switch on
    plain = report_parameters(CallOptions(call_alleles=True, seed=1), 1)
    assert report_parameters(SnvDiscoveryCallOptions(call_alleles=True, seed=1, snv_discover_window=100), 1) == plain
    on = report_parameters(wide, 1)
    assert on["discover_snvs"] is True and on["snv_discover_window"] == 8192 and on["snv_min_base_qual"] == 20 and on["significant_clip_threshold"] == 100
    assert "snv_vcf" not in on and set(on) - set(plain) == {"discover_snvs", "snv_discover_window", "snv_min_base_qual", "significant_clip_threshold"}


def test_refusals_of_the_command_line_and_under_torch_distributed(data, monkeypatch, capsys):
    p = data["paths"]
    base = ["call", p["bam"], "--ref", p["ref"], "--loci", p["loci"], "--json", os.devnull]
    a = build_parser().parse_args(base + ["--call-alleles", "--discover-snvs", "--snv-discover-window", "700"])
    assert a.discover_snvs is True and a.snv_discover_window == 700
    for extra, words in ((["--discover-snvs"], "--discover-snvs needs --call-alleles"),
                         (["--call-alleles", "--discover-snvs", "--incorporate-snvs", p["snvs"]], "two sources of candidate SNVs"),
                         (["--call-alleles", "--discover-snvs", "--snv-phase-sets"], "--snv-phase-sets needs --incorporate-snvs"),
                         (["--call-alleles", "--discover-snvs", "--snv-discover-window", "0"], "--snv-discover-window must be in 1 .. 65536")):
        with pytest.raises(SystemExit):
            main(base + extra)
        assert words in capsys.readouterr().err
    # under torch.distributed: refused before a file is opened, in the same words by call_sample and by the command line
    from strkit_amd.frontend import call as call_mod
    monkeypatch.setattr(call_mod, "_distributed", lambda: True)
    with pytest.raises(NotImplementedError) as e:
        call_sample("/nonexistent.bam", "/nonexistent.fa", "/nonexistent.bed", call_alleles=True, seed=1, discover_snvs=True)
    assert str(e.value) == SHARDING_REFUSALS["discover_snvs"] and "discover_snvs=True under torch.distributed" in str(e.value)
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(SystemExit):
        main(["call", "/nonexistent.bam", "--ref", "/nonexistent.fa", "--loci", "/nonexistent.bed", "--json", os.devnull, "--call-alleles", "--discover-snvs"])
    assert SHARDING_REFUSALS["discover_snvs"] in capsys.readouterr().err


# ---- GPU ----------------------------------------------------------------------------------------------------------------------
def _call(t, **kw):
    return call_sample(t["paths"]["bam"], t["paths"]["ref"], t["paths"]["loci"], call_alleles=True, seed=SEED, **kw)


@pytest.fixture(scope="module")
def reports(gpu_ctx, data):
    return {"device": _call(data, discover_snvs=True, consensus=True, front_end="device"),
            "host": _call(data, discover_snvs=True, consensus=True, front_end="host"),
            "vcf": _call(data, snv_vcf=data["paths"]["snvs"], consensus=True, front_end="device")}


@pytest.mark.gpu
def test_discovered_snvs_give_the_rows_of_the_candidate_file(data, reports):
    dev, vcf = reports["device"], reports["vcf"]
    assert dev["stage_times"]["front_end"] == "device" and dev["parameters"]["discover_snvs"] is True and dev["parameters"]["snv_discover_window"] == 8192
    assert "snv_vcf" not in dev["parameters"] and "discover_snvs" not in vcf["parameters"] and "snv_discover_window" not in vcf["parameters"]
    assert dev["stage_times"]["snv_discover_s"] > 0 and dev["stage_times"]["snv_discover_device_s"] > 0 and "snv_candidates_s" not in dev["stage_times"]
    assert len(dev["results"]) == len(vcf["results"]) == 12
    for row, ref_row, truth in zip(dev["results"], vcf["results"], data["loci"]):
        for k in ("call", "peaks", "assign_method"):
            assert row[k] == ref_row[k], (row["locus_id"], k)
        assert row["assign_method"] in ("snv", "snv+dist"), row["locus_id"]      # (every locus of the data set has a site that all its reads cover)
        strip = lambda snvs: [{k: s[k] for k in ("pos", "ref", "call", "rcs")} for s in snvs]  # noqa: E731
        assert strip(row["snvs"]) == strip(ref_row["snvs"]) and row["snvs"], row["locus_id"]
        assert {s["pos"] for s in row["snvs"]} <= set(truth["het"])
        assert [s["id"] for s in row["snvs"]] == [f"{row['contig']}_{s['pos'] + 1}" for s in row["snvs"]]
        assert all(s["id"].startswith("het") for s in ref_row["snvs"])
        assert list(row["reads"]) == list(ref_row["reads"])
        for name, r in row["reads"].items():
            assert (r["p"], r["snvu"]) == (ref_row["reads"][name]["p"], ref_row["reads"][name]["snvu"]), (row["locus_id"], name)
        # nothing else differs either
        same = json.loads(json.dumps(row))
        for s, t in zip(same["snvs"], ref_row["snvs"]):
            s["id"] = t["id"]
        assert same == ref_row, row["locus_id"]


@pytest.mark.gpu
def test_the_three_paths_give_one_report(gpu_ctx, data, reports):
    dev, host = reports["device"], reports["host"]
    assert host["stage_times"]["front_end"] == "host" and host["stage_times"]["snv_discover_s"] > 0 and "snv_discover_device_s" not in host["stage_times"]
    assert dev["results"] == host["results"] and dev["parameters"] == host["parameters"]
    opts = SnvDiscoveryCallOptions(call_alleles=True, consensus=True, seed=SEED, discover_snvs=True)
    rows, _n, tm = call_blocks(load_loci(data["paths"]["loci"]), read_bam(data["paths"]["bam"]), Fasta(data["paths"]["ref"]), opts, gpu_ctx)
    assert rows == dev["results"] and tm["snv_discover_s"] > 0
    # a window that reaches none of a locus's sites leaves it to the copy numbers, as a candidate file without its sites would
    near = _call(data, discover_snvs=True, snv_discover_window=1, front_end="device")
    assert near["parameters"]["snv_discover_window"] == 1
    edge = [{l.left_flank_coord - 1, l.right_flank_coord} for block in load_loci(data["paths"]["loci"]) for l in block]
    assert all({s["pos"] for s in r.get("snvs", [])} <= e & set(t["het"]) for r, e, t in zip(near["results"], edge, data["loci"]))
    assert any("snvs" not in r for r in near["results"]) and all(r["call"] for r in near["results"])


@pytest.mark.gpu
def test_the_vcf_carries_ps_and_nsnv_as_with_a_candidate_file(data, reports, tmp_path):
    out = {}
    for k in ("device", "vcf"):
        path = str(tmp_path / f"{k}.vcf")
        assert write_vcf(reports[k], path, Fasta(data["paths"]["ref"])) == 12
        out[k] = open(path).read()
    assert "ID=NSNV" in out["device"] and ("ID=PS," in out["device"]) == ("ID=PS," in out["vcf"])
    body = lambda text: [ln for ln in text.split("\n") if ln and not ln.startswith("##")]  # noqa: E731
    assert body(out["device"]) == body(out["vcf"])           # (the SNVs' ids are not written without snv_phase_sets)
    for row, ln in zip(reports["device"]["results"], body(out["device"])[1:]):
        f = ln.split("\t")
        rec = dict(zip(f[8].split(":"), f[9].split(":")))
        assert rec["PM"] == row["assign_method"] and rec["NSNV"] == str(len(row["snvs"]))


@pytest.mark.gpu
def test_the_command_line(data, tmp_path, reports):
    out = str(tmp_path / "cli.json")
    p = data["paths"]
    assert main(["call", p["bam"], "--ref", p["ref"], "--loci", p["loci"], "--json", out, "--call-alleles", "--seed", str(SEED), "--discover-snvs",
                 "--front-end", "device"]) == 0
    rep = json.load(open(out))
    assert rep["parameters"]["discover_snvs"] is True
    for row, want in zip(rep["results"], reports["device"]["results"]):
        assert row["call"] == want["call"] and [s["pos"] for s in row["snvs"]] == [s["pos"] for s in want["snvs"]]
