"""CPU: the options, the command line and the report parameters of read selection (frontend/options.py: ReadSelectionCallOptions;
DESIGN.md §17), and the synthetic data of frontend/synth_chimeric.py.  The report comparisons need the device for counting
(`_lib` has no CPU path): they are in tests/test_gpu_select_call.py."""
import dataclasses

import pytest

from strkit_amd.__main__ import build_parser
from strkit_amd.frontend.call import ReadSelectionCallOptions as FromCall
from strkit_amd.frontend.options import (READ_SELECTION_OPTION_NAMES, CallOptions, PhaseSetCallOptions, ReadSelectionCallOptions,
                                         report_parameters, with_keywords)
from strkit_amd.frontend.select import rules_of


def test_the_type_and_its_fields():
    names = lambda t: [f.name for f in dataclasses.fields(t)]  # noqa: E731
    assert FromCall is ReadSelectionCallOptions and issubclass(ReadSelectionCallOptions, PhaseSetCallOptions)
    assert names(ReadSelectionCallOptions) == names(PhaseSetCallOptions) + list(READ_SELECTION_OPTION_NAMES)
    assert READ_SELECTION_OPTION_NAMES == ("skip_supplementary", "skip_secondary", "unique_reads")
    o = ReadSelectionCallOptions()
    assert (o.skip_supplementary, o.skip_secondary, o.unique_reads) == (False, False, False) and rules_of(o) == 0
    assert rules_of(CallOptions()) == 0


def test_widening_and_validate():
    base = CallOptions(flank_size=50, max_reads=40)
    for k, name in enumerate(READ_SELECTION_OPTION_NAMES):
        wide = with_keywords(base, **{name: True})
        assert type(wide) is ReadSelectionCallOptions and rules_of(wide) == 1 << k
        assert all(getattr(wide, f.name) == getattr(base, f.name) for f in dataclasses.fields(CallOptions))
        wide.validate()
    assert type(with_keywords(base, flank_size=60)) is CallOptions                    # nothing of this type asked: no widening
    both = with_keywords(with_keywords(None, use_methyl=True), unique_reads=True, skip_secondary=True)
    assert type(both) is ReadSelectionCallOptions and both.use_methyl and rules_of(both) == 6
    assert type(with_keywords(both, consensus_method="poa")) is ReadSelectionCallOptions
    with pytest.raises(ValueError, match="unique_reads"):
        with_keywords(None, unique_reads=1).validate()
    with pytest.raises(TypeError):
        with_keywords(None, unique_read=True)


def test_report_parameters_only_when_on():
    plain = report_parameters(CallOptions(), 1)
    assert report_parameters(ReadSelectionCallOptions(), 1) == plain and not set(READ_SELECTION_OPTION_NAMES) & set(plain)
    on = report_parameters(with_keywords(None, skip_supplementary=True, unique_reads=True), 1)
    assert {k: v for k, v in on.items() if k not in plain} == {"skip_supplementary": True, "unique_reads": True}
    assert list(on)[:len(plain)] == list(plain)


def test_command_line_flags():
    ap = build_parser()
    base = ["call", "x.bam", "--ref", "r.fa", "--loci", "l.bed"]
    a = ap.parse_args(base)
    assert (a.skip_supplementary, a.skip_secondary, a.unique_reads) == (False, False, False)
    a = ap.parse_args(base + ["--skip-supplementary", "--skip-sec", "--unique-reads"])
    assert (a.skip_supplementary, a.skip_secondary, a.unique_reads) == (True, True, True)
    a = ap.parse_args(base + ["--skip-supp", "--skip-secondary"])
    assert (a.skip_supplementary, a.skip_secondary, a.unique_reads) == (True, True, False)
    text = ap._subparsers._group_actions[0].choices["call"].format_help()
    for flag in ("--skip-supplementary", "--skip-supp", "--skip-secondary", "--skip-sec", "--unique-reads"):
        assert flag in text


def test_synthetic_data(tmp_path):
    from strkit_amd.frontend import read_bam
    from strkit_amd.frontend.synth_chimeric import make_chimeric_dataset
    ds = make_chimeric_dataset(str(tmp_path), n_loci=12, reads_per_locus=12)
    clean, extra = read_bam(ds["paths"]["bam_clean"]), read_bam(ds["paths"]["bam"])
    x = ds["extras"]
    assert len(clean.segments) == 145 and len(extra.segments) == 146 + len(x["supplementary"]) + len(x["secondary"]) + len(x["duplicates"])
    # the long read: its primary spans loci 4 and 5 with their flanks, its supplementary record overlaps locus 5 only
    sp = x["spanning"]
    assert sp == {"name": "span4_5", "loci": (4, 5), "chimeric_at": 5}
    prim, supp = [s for s in extra.segments if s.name == sp["name"]]
    assert not prim.flag & 0x900 and supp.flag & 0x800 and [s.name for s in clean.segments].count(sp["name"]) == 1
    for li in sp["loci"]:
        assert prim.start < ds["loci"][li]["start"] - 70 and prim.end > ds["loci"][li]["end"] + 70
    assert supp.start > ds["loci"][4]["end"] + 70 and supp.start < ds["loci"][5]["start"] - 70 and supp.end > ds["loci"][5]["end"] + 70
    assert sorted(x["supplementary"].values()) == ["after"] * 4 + ["before"] * 4
    assert [s.start for s in extra.segments] == sorted(s.start for s in extra.segments)
    for name, where in x["supplementary"].items():
        recs = [s for s in extra.segments if s.name == name]
        assert len(recs) == 2 and sum(bool(s.flag & 0x800) for s in recs) == 1
        assert bool(recs[0].flag & 0x800) == (where == "before")
        supp = next(s for s in recs if s.flag & 0x800)
        assert 5 in (supp.cigar & 15).tolist()                                        # hard-clipped
        li = int(name[1:].split("_")[0])
        assert supp.start < ds["loci"][li]["start"] - 70 and supp.end > ds["loci"][li]["end"] + 70      # spans the locus and its flanks
    assert all(s.flag & 0x100 for s in extra.segments if s.name in x["secondary"]) and len(x["secondary"]) == 3
    for name in x["duplicates"]:
        a, b = [s for s in extra.segments if s.name == name]
        assert (a.flag, a.start, a.query_sequence, a.cigar.tolist()) == (b.flag, b.start, b.query_sequence, b.cigar.tolist())
    # the primaries are the clean file's records, in its order
    prim = [s for s in extra.segments if not s.flag & 0x900]
    firsts = {}
    for s in prim:
        firsts.setdefault(s.name, s)
    assert [(s.name, s.start, s.query_sequence) for s in clean.segments] == [(s.name, s.start, s.query_sequence) for s in
                                                                            sorted(firsts.values(), key=lambda s: s.start)]


def test_gathered_records_carry_the_chimeric_mark():
    """_encode_rows -> _decode_rows (what the ranks of a torch.distributed run exchange): `chimeric_in_region` comes back on the
    reads that had it and on no other, next to the flags that were there before."""
    from helpers import FakeRef, fake_rows, gloo_blocks
    from strkit_amd.frontend.gather import _decode_rows, _encode_rows
    blocks, ref = gloo_blocks(), FakeRef()
    rows, _n, tm = fake_rows(blocks, ref)
    recs = [x for r in rows for x in (r.get("reads") or {}).values()]
    assert len(recs) > 8 and not any("chimeric_in_region" in x for x in recs)
    plain = _encode_rows(rows, tm["errors"])
    for x in recs[::3]:
        x["chimeric_in_region"] = True
    assert any(x.get("realn") and "chimeric_in_region" in x for x in recs) or any(x["sc"] is None and "chimeric_in_region" in x for x in recs) \
        or any(x["s"] == "-" and "chimeric_in_region" in x for x in recs)
    loci_t, reads_t, names_t = _encode_rows(rows, tm["errors"])
    assert (reads_t[:, 3] & 8 != 0).sum() == len(recs[::3]) and ((reads_t[:, 3] & 7) == (plain[1][:, 3] & 7)).all() and not (plain[1][:, 3] & 8).any()
    got, _errors = _decode_rows({l.t_idx: l for blk in blocks for l in blk}, ref, False, loci_t, reads_t, names_t)
    assert got == sorted(rows, key=lambda r: r["locus_index"])
    back = [x for r in got for x in (r.get("reads") or {}).values()]
    assert sum("chimeric_in_region" in x for x in back) == len(recs[::3]) and all(x.get("chimeric_in_region", True) is True for x in back)
