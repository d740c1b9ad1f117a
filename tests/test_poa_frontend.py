"""CPU: the options, the command line and the declarations of the partial-order-alignment consensus (no device needed)."""
import dataclasses
import os
import re

import pytest

from strkit_amd import _lib
from strkit_amd import consensus as CS
from strkit_amd.__main__ import build_parser
from strkit_amd.frontend.options import CallOptions, PoaCallOptions, report_parameters, with_keywords

HEADER = os.path.join(os.path.dirname(__file__), "..", "include", "strkit_amd.h")


def test_options_are_validated_and_reported_only_off_their_defaults():
    base = CallOptions(call_alleles=True, consensus=True, seed=1)
    base.validate()
    assert base.consensus_method == "best_rep" and base.max_mdn_poa_length == 5000
    params = report_parameters(base, 1)
    assert "consensus_method" not in params and "max_mdn_poa_length" not in params
    poa = PoaCallOptions(call_alleles=True, consensus=True, seed=1, consensus_method="poa", max_mdn_poa_length=300)
    poa.validate()
    params = report_parameters(poa, 1)
    assert params["consensus_method"] == "poa" and params["max_mdn_poa_length"] == 300
    for bad in (dict(consensus_method="spoa"), dict(consensus_method=None), dict(max_mdn_poa_length=-1),
                dict(max_mdn_poa_length=2.5), dict(max_mdn_poa_length=True)):
        with pytest.raises(ValueError):
            PoaCallOptions(call_alleles=True, consensus=True, seed=1, **bad).validate()


def test_options_by_name_widen_the_options_type_and_leave_its_fields_alone():
    names = [f.name for f in dataclasses.fields(CallOptions)]
    assert "consensus_method" not in names and "max_mdn_poa_length" not in names
    assert with_keywords(None) == CallOptions() and type(with_keywords(None, flank_size=50)) is CallOptions
    base = CallOptions(call_alleles=True, consensus=True, seed=3, flank_size=50)
    wide = with_keywords(base, consensus_method="poa")
    assert type(wide) is PoaCallOptions and wide.consensus_method == "poa" and wide.max_mdn_poa_length == 5000
    assert all(getattr(wide, n) == getattr(base, n) for n in names)
    assert with_keywords(wide, max_mdn_poa_length=800, realign=True) == dataclasses.replace(wide, max_mdn_poa_length=800, realign=True)
    assert with_keywords(wide, realign=True).consensus_method == "poa"
    with pytest.raises(TypeError):
        with_keywords(base, consensus_methods="poa")


def test_command_line():
    ap = build_parser()
    a = ap.parse_args(["call", "x.bam", "--ref", "r.fa", "--loci", "l.bed"])
    assert a.consensus_method == "best_rep" and a.max_mdn_poa_length == 5000
    a = ap.parse_args(["call", "x.bam", "--ref", "r.fa", "--loci", "l.bed", "--call-alleles", "--consensus",
                       "--consensus-method", "poa", "--max-mdn-poa-length", "800"])
    assert a.consensus_method == "poa" and a.max_mdn_poa_length == 800
    with pytest.raises(SystemExit):
        ap.parse_args(["call", "x.bam", "--ref", "r.fa", "--loci", "l.bed", "--consensus-method", "spoa"])


def test_declarations():
    text = open(HEADER).read()
    assert re.search(r"#define\s+STRK_CONS_POA\s+3\b", text)
    for name in ("strk_consensus", "strk_consensus_dseqs", "strk_consensus_ws"):
        assert re.search(r"\b%s\(" % name, text) and name in _lib.EXPORTS
    assert (CS.NONE, CS.SINGLE, CS.BEST_REP, CS.POA) == (0, 1, 2, 3)
    assert CS.METHOD_NAMES == ("none", "single", "best_rep", "poa")
    with pytest.raises(ValueError):
        CS.consensus_seq(["A"], method="spoa")
