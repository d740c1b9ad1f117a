"""CPU: the options, the command line, the report's parameters, the VCF fields and the declarations of methylation from
MM / ML tags (no device needed)."""
import dataclasses
import os
import re

import pytest

from strkit_amd import _lib
from strkit_amd.__main__ import build_parser
from strkit_amd.frontend import call as call_mod
from strkit_amd.frontend import methyl as me
from strkit_amd.frontend.options import (METHYL_OPTION_NAMES, CallOptions, MethylCallOptions, PhasedCallOptions, PoaCallOptions,
                                         report_parameters, with_keywords)
from strkit_amd.frontend.output import write_vcf

HEADER = os.path.join(os.path.dirname(__file__), "..", "include", "strkit_amd.h")
ARGS = ["call", "x.bam", "--ref", "r.fa", "--loci", "l.bed"]


def test_command_line():
    ap = build_parser()
    a = ap.parse_args(ARGS)
    assert a.use_methyl is False and a.methyl_threshold == 127
    assert ap.parse_args(ARGS + ["--use-methyl"]).use_methyl is True
    a = ap.parse_args(ARGS + ["-m", "--methyl-threshold", "200"])
    assert a.use_methyl is True and a.methyl_threshold == 200
    with pytest.raises(SystemExit):
        ap.parse_args(ARGS + ["--methyl-threshold", "high"])


def test_the_existing_option_types_keep_their_fields():
    names = lambda t: [f.name for f in dataclasses.fields(t)]  # noqa: E731
    for t in (CallOptions, PoaCallOptions, PhasedCallOptions):
        assert not set(names(t)) & set(METHYL_OPTION_NAMES)
    assert names(PoaCallOptions) == names(CallOptions) + ["consensus_method", "max_mdn_poa_length"]
    assert names(PhasedCallOptions) == names(PoaCallOptions) + ["use_hp", "snv_vcf", "snv_min_base_qual", "significant_clip_threshold", "phase_params"]
    assert names(MethylCallOptions) == names(PhasedCallOptions) + ["use_methyl", "methyl_threshold"]
    assert METHYL_OPTION_NAMES == ("use_methyl", "methyl_threshold")
    assert issubclass(MethylCallOptions, PhasedCallOptions)


def test_options_by_name_widen_the_options_type():
    assert type(with_keywords(None, flank_size=50)) is CallOptions
    assert type(with_keywords(None, use_hp=True, call_alleles=True)) is PhasedCallOptions
    base = CallOptions(flank_size=50, realign=True)
    wide = with_keywords(base, use_methyl=True)
    assert type(wide) is MethylCallOptions and wide.use_methyl and wide.methyl_threshold == 127
    assert all(getattr(wide, f.name) == getattr(base, f.name) for f in dataclasses.fields(CallOptions))
    poa = PoaCallOptions(consensus_method="poa", call_alleles=True, consensus=True, seed=2)
    wide = with_keywords(poa, methyl_threshold=100)
    assert type(wide) is MethylCallOptions and wide.consensus_method == "poa" and wide.methyl_threshold == 100 and not wide.use_methyl
    assert with_keywords(wide, use_hp=True).methyl_threshold == 100 and type(with_keywords(wide, use_hp=True)) is MethylCallOptions
    with pytest.raises(TypeError):
        with_keywords(base, use_methylation=True)


def test_validate():
    MethylCallOptions(use_methyl=True).validate()                      # the switch does not need call_alleles
    MethylCallOptions(use_methyl=True, methyl_threshold=0).validate()
    MethylCallOptions(use_methyl=True, methyl_threshold=255).validate()
    for bad in (-1, 256, 127.0, True, None, "127"):
        with pytest.raises(ValueError, match="methyl_threshold"):
            MethylCallOptions(use_methyl=True, methyl_threshold=bad).validate()
    with pytest.raises(ValueError):                                    # the checks of the types below still hold
        MethylCallOptions(use_methyl=True, use_hp=True).validate()


def test_report_parameters():
    plain = report_parameters(CallOptions(), 1)
    assert "use_methyl" not in plain and "methyl_threshold" not in plain
    assert report_parameters(MethylCallOptions(), 1) == plain          # the switch off: the parameters a plain run reports
    assert report_parameters(MethylCallOptions(methyl_threshold=9), 1) == plain
    on = report_parameters(MethylCallOptions(use_methyl=True), 1)
    assert on == {**plain, "use_methyl": True}
    assert report_parameters(MethylCallOptions(use_methyl=True, methyl_threshold=200), 1) == {**plain, "use_methyl": True, "methyl_threshold": 200}


def test_not_under_sharding(monkeypatch):
    monkeypatch.setattr(call_mod, "_distributed", lambda: True)
    with pytest.raises(NotImplementedError, match="use_methyl"):
        call_mod.call_sample("no_such.bam", "no_such.fa", "no_such.bed", use_methyl=True)


def test_declarations():
    text = open(HEADER).read()
    for i, name in enumerate(("OK", "NOT_SPANNING", "NO_TAGS", "CLIPPED", "MALFORMED", "NO_SITES")):
        assert re.search(r"#define\s+STRK_METHYL_%s\s+%d\b" % (name, i), text)
        assert getattr(_lib, "STRK_METHYL_" + name) == i and me.STATUS_NAMES[i] == name
    for name in ("strk_methyl", "strk_dbam_methyl", "strk_methyl_constants"):
        assert re.search(r"\b%s\(" % name, text) and name in _lib.EXPORTS
    assert "MethylCallOptions" in call_mod.__all__ and call_mod.MethylCallOptions is MethylCallOptions
    for name in ("parse_mm", "read_methylation", "methyl", "allele_means"):
        assert name in me.__all__ and callable(getattr(me, name))
    from strkit_amd.frontend.synth_methyl import make_methyl_dataset
    assert callable(make_methyl_dataset)


def _report(use_methyl: bool, am=None) -> dict:
    peaks = {"means": [10.0, 14.0], "weights": [0.5, 0.5], "stdevs": [0.1, 0.1], "modal_n": 2, "n_reads": [2, 2]}
    if am is not None:
        peaks["am"], peaks["amc"] = am
    reads = {f"r{i}": {"s": "+", "cn": 10 + 4 * (i % 2), "w": 0.25, "sc": 1.0, "sl": 30 + 12 * (i % 2), "p": i % 2} for i in range(4)}
    row = {"locus_index": 1, "locus_id": "me0", "contig": "chr1", "start": 100, "end": 130, "motif": "CGG", "annotations": [],
           "assign_method": "dist", "call": [10, 14], "call_95_cis": [[10, 10], [14, 14]], "call_99_cis": [[10, 10], [14, 14]], "ref_cn": 10,
           "ref_start_anchor": "ACGTA", "ref_seq": "CGG" * 10, "peaks": peaks, "read_peaks_called": True, "mean_model_align_score": 1.0,
           "reads": reads}
    uncalled = {**row, "locus_index": 2, "locus_id": "me1", "start": 400, "end": 430, "call": None, "peaks": None, "assign_method": None}
    return {"sample_id": "s", "parameters": {"n_alleles": 2, **({"use_methyl": True} if use_methyl else {})}, "results": [row, uncalled]}


def _vcf(report, tmp_path, name):
    path = str(tmp_path / name)
    assert write_vcf(report, path, date="20250101") == 2
    return open(path).read()


def test_vcf_fields(tmp_path):
    plain = _vcf(_report(False), tmp_path, "plain.vcf")
    assert "ID=AM," not in plain and "ID=AMC," not in plain and ":AM:" not in plain
    # the rows carry values but the run's parameters do not carry the switch: the bytes of a plain report
    assert _vcf(_report(False, ([0.25, 0.75], [2.5, 9.0])), tmp_path, "plain2.vcf") == plain
    on = _vcf(_report(True, ([0.25, 2 / 3], [2.5, 9.0])), tmp_path, "on.vcf")
    assert '##FORMAT=<ID=AM,Number=.,Type=Float,Description="Average methylation level (5-methyl CpG sites) for each allele">' in on
    assert '##FORMAT=<ID=AMC,Number=.,Type=Float,Description="Average number of 5-methyl CpG sites for each allele">' in on
    ids = re.findall(r"##FORMAT=<ID=(\w+),", on)
    assert ids == sorted(ids)
    rec = [ln.split("\t") for ln in on.splitlines() if not ln.startswith("#")]
    fields = dict(zip(rec[0][8].split(":"), rec[0][9].split(":")))
    assert fields["AM"] == "0.25,0.666667" and fields["AMC"] == "2.5,9"
    assert "AM" not in rec[1][8].split(":")                              # no call: no per-allele fields
    none = _vcf(_report(True), tmp_path, "none.vcf")                     # a called row without values: '.' per allele
    rec = [ln.split("\t") for ln in none.splitlines() if not ln.startswith("#")]
    fields = dict(zip(rec[0][8].split(":"), rec[0][9].split(":")))
    assert fields["AM"] == ".,." and fields["AMC"] == ".,."
    # nothing else of the file changes: two more header lines, two more fields in the called row
    assert len(on.splitlines()) == len(plain.splitlines()) + 2
    assert [ln for ln in on.splitlines() if "ID=AM" not in ln and "\tme0\t" not in ln] == [ln for ln in plain.splitlines() if "\tme0\t" not in ln]
