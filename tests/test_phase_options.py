"""CPU: the options of phasing from files (frontend/options.py: PhasedCallOptions): widening by with_keywords, validate,
report_parameters, the command line; the field list of CallOptions stays what it was."""
import dataclasses

import pytest

from strkit_amd.__main__ import build_parser, main
from strkit_amd.frontend.options import (CallOptions, PhasedCallOptions, PoaCallOptions, phased, report_parameters, with_keywords)
from strkit_amd.phasing import PhaseParams

CALL_OPTION_FIELDS = ["flank_size", "realign", "min_avg_phred", "max_reads", "respect_ref", "rc_params", "min_read_align_score", "tie_rule",
                      "end_flags", "narrowing", "call_alleles", "consensus", "seed", "n_alleles", "allele_params", "large_consensus_length",
                      "max_n_large_consensus_reads", "count_kmers"]


def test_the_fields_of_call_options_are_unchanged():
    assert [f.name for f in dataclasses.fields(CallOptions)] == CALL_OPTION_FIELDS
    assert [f.name for f in dataclasses.fields(PoaCallOptions)] == CALL_OPTION_FIELDS + ["consensus_method", "max_mdn_poa_length"]
    assert [f.name for f in dataclasses.fields(PhasedCallOptions)][-5:] == ["use_hp", "snv_vcf", "snv_min_base_qual", "significant_clip_threshold",
                                                                           "phase_params"]
    d = PhasedCallOptions()
    assert (d.use_hp, d.snv_vcf, d.snv_min_base_qual, d.significant_clip_threshold, d.phase_params) == (False, None, 20, 100, None)


def test_with_keywords_widens():
    assert type(with_keywords(None, flank_size=50)) is CallOptions
    o = with_keywords(CallOptions(flank_size=50, realign=True), use_hp=True)
    assert type(o) is PhasedCallOptions and o.use_hp and o.flank_size == 50 and o.realign and o.consensus_method == "best_rep"
    o = with_keywords(PoaCallOptions(consensus_method="poa"), snv_vcf="x.vcf", phase_params=PhaseParams(min_hp_read_coverage=4))
    assert type(o) is PhasedCallOptions and o.consensus_method == "poa" and o.snv_vcf == "x.vcf" and o.phase_params.min_hp_read_coverage == 4
    assert type(with_keywords(o, consensus_method="best_rep")) is PhasedCallOptions
    with pytest.raises(TypeError):
        with_keywords(None, use_hap=True)
    assert phased(o) and not phased(CallOptions()) and not phased(PhasedCallOptions()) and phased(PhasedCallOptions(use_hp=True))


def test_validate():
    for kw in ({"use_hp": True}, {"snv_vcf": "x.vcf"}):
        with pytest.raises(ValueError, match="call_alleles"):
            PhasedCallOptions(**kw).validate()
        PhasedCallOptions(call_alleles=True, seed=1, **kw).validate()
    PhasedCallOptions().validate()
    for kw in ({"snv_min_base_qual": -1}, {"snv_min_base_qual": 256}, {"significant_clip_threshold": -1}, {"snv_min_base_qual": True}):
        with pytest.raises(ValueError):
            PhasedCallOptions(**kw).validate()
    with pytest.raises(ValueError, match="consensus"):          # the checks of the types below still run
        PhasedCallOptions(consensus=True).validate()


def test_report_parameters_name_the_switches_that_are_on():
    base = report_parameters(CallOptions(call_alleles=True, seed=3), 1)
    assert report_parameters(PhasedCallOptions(call_alleles=True, seed=3), 1) == base
    hp = report_parameters(PhasedCallOptions(call_alleles=True, seed=3, use_hp=True), 1)
    assert hp == {**base, "use_hp": True, "significant_clip_threshold": 100}
    snv = report_parameters(PhasedCallOptions(call_alleles=True, seed=3, snv_vcf="d.vcf", snv_min_base_qual=10, significant_clip_threshold=50), 1)
    assert snv == {**base, "snv_vcf": "d.vcf", "snv_min_base_qual": 10, "significant_clip_threshold": 50}


def test_command_line():
    a = build_parser().parse_args(["call", "r.bam", "--ref", "r.fa", "--loci", "l.bed", "--call-alleles", "--use-hp", "-v", "d.vcf.gz",
                                   "--snv-min-base-qual", "15", "--significant-clip-threshold", "80"])
    assert a.use_hp and a.incorporate_snvs == "d.vcf.gz" and a.snv_min_base_qual == 15 and a.significant_clip_threshold == 80
    for flag in ("--incorporate-snvs", "--snv"):
        assert build_parser().parse_args(["call", "r.bam", "--ref", "r.fa", "--loci", "l.bed", flag, "x.vcf"]).incorporate_snvs == "x.vcf"
    with pytest.raises(SystemExit):                              # a switch without --call-alleles
        main(["call", "r.bam", "--ref", "r.fa", "--loci", "l.bed", "--use-hp"])
