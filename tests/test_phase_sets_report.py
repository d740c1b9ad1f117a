"""CPU: what phase sets across loci (frontend/phase_sets.py) do to rows, the VCF and the options: the fix-up of a
row that carries every per-peak field, SNV records in write_vcf, today's bytes without the parameter, the options type."""
import copy
import dataclasses

import numpy as np
import pytest

from strkit_amd.frontend.options import (PHASE_SET_OPTION_NAMES, CallOptions, PhaseSetCallOptions, PloidyCallOptions, report_parameters,
                                         with_keywords)
from strkit_amd.frontend.output import write_vcf
from strkit_amd.frontend.phase_sets import PEAK_LISTS, SNV_CACHE_MISMATCH, PhaseSets, demote, flip_row, resolve_block
from strkit_amd.phasing import ASSIGN_NONE, ASSIGN_SNV, SNV_CALLED, SNV_SAME_BASE


def _full_row(idx=1, ps=2):
    return {"locus_index": idx, "locus_id": f"l{idx}", "contig": "chr1", "start": 100 * idx, "end": 100 * idx + 12, "motif": "CAG",
            "assign_method": "snv", "call": [4, 7], "call_95_cis": [[4, 4], [6, 8]], "call_99_cis": [[3, 5], [6, 9]], "ps": ps,
            "peaks": {"means": [4.0, 7.1], "weights": [0.5, 0.5], "stdevs": [0.1, 0.4], "modal_n": 2, "n_reads": [2, 1],
                      "kmers": [{"CAG": 8}, {"CAG": 7}], "seqs": [["CAG" * 4, "single"], ["CAG" * 7, "best_rep"]],
                      "start_anchor_seqs": [["ACGTA", "single"], ["ACGTT", "single"]], "am": [0.25, 0.75], "amc": [1.0, 3.0]},
            "snvs": [{"id": "v1", "ref": "A", "pos": 50, "call": ["A", "C"], "rcs": [2, 1]},
                     {"id": "v2", "ref": "T", "pos": 60, "call": ["G", "T"], "rcs": [2, 1]}],
            "reads": {"r0": {"cn": 4, "p": 0, "ps": ps, "snvu": ["A", "G"]}, "r1": {"cn": 4, "p": 0, "ps": ps, "snvu": ["A", "G"]},
                      "r2": {"cn": 7, "p": 1, "ps": ps, "snvu": ["C", "T"]}, "r3": {"cn": 5, "hp": 1, "ps": 9}}}


def test_the_fix_up_turns_over_every_per_peak_field_of_a_row():
    row = _full_row()
    before = copy.deepcopy(row)
    s = PhaseSets()
    s.syn = {2: (1, True)}
    s.finish_contig([row])
    assert row["ps"] == 1
    assert row["call"] == [7, 4] and row["call_95_cis"] == [[6, 8], [4, 4]] and row["call_99_cis"] == [[6, 9], [3, 5]]
    assert set(PEAK_LISTS) == set(before["peaks"]) - {"modal_n"}
    for k in PEAK_LISTS:
        assert row["peaks"][k] == before["peaks"][k][::-1], k
    assert row["peaks"]["modal_n"] == 2
    assert [(v["call"], v["rcs"]) for v in row["snvs"]] == [(["C", "A"], [1, 2]), (["T", "G"], [1, 2])]
    assert [r.get("p") for r in row["reads"].values()] == [1, 1, 0, None]
    # the reads' phase sets follow (the reference leaves the old number on them); renumbering: reads first, then the row
    assert [r["ps"] for r in row["reads"].values()] == [1, 1, 1, 2]
    assert all(r.get("snvu") == b.get("snvu") for r, b in zip(row["reads"].values(), before["reads"].values()))
    # a synonym that does not turn the set over changes the number alone
    row = _full_row()
    s = PhaseSets()
    s.syn = {2: (1, False)}
    s.finish_contig([row])
    want = _full_row(ps=1)
    want["reads"]["r3"]["ps"] = 2
    assert row == want
    row = {"locus_index": 1, "call": [3, 4], "ps": 1, "reads": {}}
    flip_row(row)
    assert row["call"] == [4, 3]


class _Locus:
    def __init__(self, t_idx, contig="chr1"):
        self.t_idx, self.contig = t_idx, contig


class _Phase:
    snv_off = np.array([0, 2, 3, 4], np.int32)


def _block_arrays():
    """Three loci with 2, 1 and 1 SNVs and 3, 2 and 2 reads: locus 0 creates a set, locus 1 holds v1 the other way round and is
    turned over, locus 2 holds v1 with another pair of bases and is demoted."""
    return {"method": np.array([ASSIGN_SNV] * 3, np.int32), "status": np.zeros(3, np.int32), "modal_n": np.full(3, 2, np.int32),
            "call": np.array([[3, 5], [4, 9], [6, 7]], np.int32), "ci95": np.array([[[3, 3], [5, 5]], [[4, 4], [8, 9]], [[6, 6], [7, 7]]], np.int32),
            "ci99": np.array([[[3, 3], [5, 5]], [[3, 4], [8, 10]], [[6, 6], [7, 7]]], np.int32),
            "means": np.array([[3.0, 5.0], [4.0, 9.0], [6.0, 7.0]]), "weights": np.array([[0.5, 0.5], [0.4, 0.6], [0.5, 0.5]]),
            "stdevs": np.array([[0.1, 0.1], [0.2, 0.3], [0.1, 0.1]]), "peak_n_reads": np.array([[2, 1], [1, 1], [1, 1]], np.int32),
            "read_off": np.array([0, 3, 5, 7], np.int64), "read_peak": np.array([0, 0, 1, 0, 1, 0, 1], np.int32),
            "snv_status": np.array([SNV_CALLED, SNV_SAME_BASE, SNV_CALLED, SNV_CALLED], np.int32),
            "snv_call": np.frombuffer(b"ACGGCAAT", np.uint8).reshape(4, 2).copy(), "snv_rcs": np.array([[2, 1], [0, 0], [1, 1], [1, 1]], np.int32)}


def test_resolve_block_flips_the_arrays_filters_and_names_the_demoted_loci():
    al = _block_arrays()
    s = PhaseSets()
    ids = {0: "v1", 1: "v0", 2: "v1", 3: "v1"}
    rest = resolve_block(s, [_Locus(1), _Locus(2), _Locus(3)], al, _Phase, lambda l, i: ids[i])
    assert rest.tolist() == [2] and al["snv_ps"].tolist() == [1, 1, -1]
    assert al["snv_status"].tolist() == [SNV_CALLED, SNV_SAME_BASE, SNV_CALLED, SNV_CACHE_MISMATCH]
    assert SNV_CACHE_MISMATCH not in range(-1, 5)
    assert al["call"].tolist() == [[3, 5], [9, 4], [6, 7]] and al["ci99"][1].tolist() == [[8, 10], [3, 4]] and al["ci95"][1].tolist() == [[8, 9], [4, 4]]
    assert al["means"][1].tolist() == [9.0, 4.0] and al["weights"][1].tolist() == [0.6, 0.4] and al["stdevs"][1].tolist() == [0.3, 0.2]
    assert al["read_peak"].tolist() == [0, 0, 1, 1, 0, 0, 1]
    assert al["snv_call"].tobytes() == b"ACGGACAT" and al["snv_rcs"].tolist() == [[2, 1], [0, 0], [1, 1], [1, 1]]
    assert s.cache == {"v1": ("A", "C", 1)}
    # the plain call of the demoted locus takes the place of its phased call
    sub = {"status": np.zeros(1, np.int32), "modal_n": np.ones(1, np.int32), "call": np.array([[6, 6]], np.int32),
           "ci95": np.array([[[6, 7], [6, 7]]], np.int32), "ci99": np.array([[[5, 7], [5, 7]]], np.int32), "means": np.array([[6.5, 6.5]]),
           "weights": np.array([[1.0, 1.0]]), "stdevs": np.array([[0.5, 0.5]]), "peak_n_reads": np.array([[2, 0]], np.int32),
           "read_peak": np.zeros(2, np.int32)}
    demote(al, rest, sub, np.array([5, 6]))
    assert al["method"].tolist() == [ASSIGN_SNV, ASSIGN_SNV, ASSIGN_NONE] and al["call"][2].tolist() == [6, 6] and al["modal_n"].tolist() == [2, 2, 1]
    assert al["read_peak"].tolist() == [0, 0, 1, 1, 0, 0, 0] and al["call"][:2].tolist() == [[3, 5], [9, 4]]


# ---- the VCF ---------------------------------------------------------------------------------------------------------------
def _vcf_row(idx, start, ps, snvs, call=(4, 6), seqs=True):
    row = {"locus_index": idx, "locus_id": f"str{idx}", "contig": "chr1", "start": start, "end": start + 12, "motif": "CAG", "ref_cn": 4,
           "ref_start_anchor": "ACGTA", "ref_seq": "CAG" * 4, "assign_method": "snv", "call": list(call), "call_95_cis": [[4, 4], [6, 6]],
           "call_99_cis": [[4, 4], [6, 6]], "read_peaks_called": True, "mean_model_align_score": 2.0,
           "peaks": {"means": [4.0, 6.0], "weights": [0.5, 0.5], "stdevs": [0.1, 0.1], "modal_n": 2, "n_reads": [1, 1]},
           "snvs": snvs, "reads": {"a": {"s": "+", "cn": call[0], "w": 1.0, "sc": 2.0, "sl": 3 * call[0], "p": 0},
                                   "b": {"s": "-", "cn": call[1], "w": 1.0, "sc": 2.0, "sl": 3 * call[1], "p": 1}}}
    if seqs:
        row["peaks"]["seqs"] = [["CAG" * call[0], "single"], ["CAG" * call[1], "single"]]
        row["peaks"]["start_anchor_seqs"] = [["ACGTA", "single"], ["ACGTA", "single"]]
    if ps is not None:
        row["ps"] = ps
    return row


def _snv(i, pos, ref, call, rcs=(5, 7)):
    return {"id": i, "ref": ref, "pos": pos, "call": list(call), "rcs": list(rcs)}


def _report(rows, **params):
    return {"sample_id": "s", "parameters": {"call_alleles": True, **params}, "catalog": {"num_loci": len(rows)}, "results": rows}


def _body(path):
    return [ln.split("\t") for ln in open(path).read().split("\n") if ln and not ln.startswith("#")]


def _rows():
    return [_vcf_row(1, 1000, 1, [_snv("v_a", 900, "A", "AC"), _snv("v_b", 1100, "G", "TG", (3, 4))]),
            _vcf_row(2, 1200, 1, [_snv("v_b", 1100, "G", "TG"), _snv("v_tie", 1199, "C", "CT"), _snv("v_hom", 1300, "A", "AA")]),
            _vcf_row(3, 2000, None, [_snv("v_c", 1900, "T", "GA")])]


def test_write_vcf_writes_phased_str_records_and_snv_records(tmp_path):
    path = str(tmp_path / "on.vcf")
    n = write_vcf(_report(_rows(), snv_phase_sets=True), path, date="20240101")
    body = _body(path)
    assert n == len(body) == 7
    # (an STR record with allele sequences keeps one base of its anchor: POS = start; v_tie lies at the POS of str2 and comes after it)
    assert [(f[1], f[2]) for f in body] == [("901", "v_a"), ("1000", "str1"), ("1101", "v_b"), ("1200", "str2"), ("1200", "v_tie"), ("1901", "v_c"),
                                            ("2000", "str3")]
    by = {f[2]: (f, dict(zip(f[8].split(":"), f[9].split(":")))) for f in body}
    for i in ("str1", "str2"):
        assert by[i][1]["PS"] == "1" and by[i][1]["GT"] == "0|1" and by[i][0][7].startswith("VT=str;")
    assert "PS" not in by["str3"][1] and by["str3"][1]["GT"] == "0/1"
    f, rec = by["v_a"]
    assert f[:8] == ["chr1", "901", "v_a", "A", "C", ".", ".", "VT=snv"] and f[8] == "GT:DP:AD:PS" and f[9] == "0|1:12:5,7:1"
    f, rec = by["v_b"]                      # written once, by the first row that holds it; AD in call order
    assert f[3:5] == ["G", "T"] and f[9] == "1|0:7:3,4:1"
    f, rec = by["v_c"]                      # two alternatives, sorted; the row has no set
    assert f[3:5] == ["T", "A,G"] and f[8] == "GT:DP:AD" and f[9] == "2/1:12:5,7"
    assert "v_hom" not in by                # no alternative: left out
    text = open(path).read()
    assert '##FORMAT=<ID=PS,Number=1,Type=Integer,Description="Phase set">' in text


def test_an_snv_at_the_position_of_an_str_record_comes_after_it(tmp_path):
    """... also where the row has no allele sequences and its record keeps the whole anchor (POS = start - 4)."""
    rows = [_vcf_row(1, 1000, 1, [_snv("v_same", 995, "A", "AC")], seqs=False)]
    path = str(tmp_path / "tie.vcf")
    write_vcf(_report(rows, snv_phase_sets=True), path, date="20240101")
    assert [(f[1], f[2]) for f in _body(path)] == [("996", "str1"), ("996", "v_same")]


def test_an_id_is_written_once_per_contig(tmp_path):
    rows = _rows()[:2]
    other = _vcf_row(4, 1000, 2, [_snv("v_a", 900, "A", "AC")])
    other["contig"] = "chr2"
    path = str(tmp_path / "two.vcf")
    write_vcf(_report(rows + [other], snv_phase_sets=True), path, date="20240101")
    assert [(f[0], f[2]) for f in _body(path) if f[7] == "VT=snv"] == [("chr1", "v_a"), ("chr1", "v_b"), ("chr1", "v_tie"), ("chr2", "v_a")]


def test_a_report_without_the_parameter_gives_the_bytes_it_always_gave(tmp_path):
    rows = _rows()
    for r in rows:
        r.pop("ps", None)
    a, b = str(tmp_path / "a.vcf"), str(tmp_path / "b.vcf")
    assert write_vcf(_report(rows, snv_vcf="x.vcf"), a, date="20240101") == 3
    text = open(a).read()
    assert "VT=snv" not in text and "ID=PS," not in text and "|" not in text
    body = _body(a)
    assert [f[2] for f in body] == ["str1", "str2", "str3"] and all(f[8].startswith("GT:DP:PM:NSNV:MMAS:DPS:AD:MC:MCCI:ANCL:CONS:MCRL:SLR") for f in body)
    # the switch alone changes nothing of the STR records
    write_vcf(_report(rows, snv_vcf="x.vcf", snv_phase_sets=True), b, date="20240101")
    assert [ln for ln in open(b).read().split("\n") if "VT=snv" not in ln] == text.split("\n")


# ---- options ---------------------------------------------------------------------------------------------------------------
def test_options_validation_widening_and_report_key():
    assert [f.name for f in dataclasses.fields(PhaseSetCallOptions)][-1] == "snv_phase_sets" and PHASE_SET_OPTION_NAMES == ("snv_phase_sets",)
    assert len(dataclasses.fields(PhaseSetCallOptions)) == len(dataclasses.fields(PloidyCallOptions)) + 1
    assert PhaseSetCallOptions().snv_phase_sets is False
    o = with_keywords(CallOptions(call_alleles=True, seed=3), snv_phase_sets=True, snv_vcf="x.vcf")
    assert type(o) is PhaseSetCallOptions and o.snv_phase_sets and o.snv_vcf == "x.vcf" and o.seed == 3
    o.validate()
    assert type(with_keywords(PloidyCallOptions(ploidy="XY"), snv_phase_sets=False)) is PhaseSetCallOptions
    assert type(with_keywords(None, snv_vcf="x.vcf")).__name__ == "PhasedCallOptions"           # the other names widen as they did
    assert type(with_keywords(o, ploidy="XX")) is PhaseSetCallOptions
    with pytest.raises(ValueError, match="snv_vcf"):
        PhaseSetCallOptions(call_alleles=True, seed=1, snv_phase_sets=True).validate()
    with pytest.raises(ValueError, match="snv_vcf"):
        PhaseSetCallOptions(call_alleles=True, seed=1, snv_phase_sets=True, use_hp=True).validate()
    with pytest.raises(TypeError):
        with_keywords(None, snv_phase_set=True)
    assert report_parameters(o, 1)["snv_phase_sets"] is True and list(report_parameters(o, 1))[-1] == "snv_phase_sets"
    off = PhaseSetCallOptions(call_alleles=True, seed=3, snv_vcf="x.vcf")
    assert "snv_phase_sets" not in report_parameters(off, 1)
    assert report_parameters(off, 1) == report_parameters(with_keywords(CallOptions(call_alleles=True, seed=3), snv_vcf="x.vcf"), 1)


def test_the_command_line_switch():
    from strkit_amd.__main__ import build_parser
    a = build_parser().parse_args(["call", "reads.bam", "--ref", "ref.fa", "--loci", "loci.bed", "--call-alleles", "--incorporate-snvs", "x.vcf",
                                   "--snv-phase-sets"])
    assert a.snv_phase_sets is True
    a = build_parser().parse_args(["call", "reads.bam", "--ref", "ref.fa", "--loci", "loci.bed"])
    assert a.snv_phase_sets is False
