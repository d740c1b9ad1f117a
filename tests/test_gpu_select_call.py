"""GPU: `call` with the read-selection switches on the synthetic data of frontend/synth_chimeric.py (12 loci x 12 reads and the
extra records: supplementary records behind and in front of their primaries, secondary records, exact duplicates).  The python,
host native and device block paths give identical reports; with all three switches the file with the extras gives the clean
file's report but for `chimeric_in_region`; a read kept at two loci of one block is marked only where its supplementary record
lies, in all three paths; a supplementary record in front of its primary stands in for the read when it is
not skipped; with the switches off nothing changes; unique_reads makes the allele call see the reads of the row."""
import json

import pytest

from strkit_amd.frontend import call_sample, read_bam
from strkit_amd.frontend.extract import get_read_coords_from_cigar, get_sequence_data_for_locus
from strkit_amd.frontend.synth_chimeric import make_chimeric_dataset
from strkit_amd.repeat_count_params import default_read_rc_params
from strkit_amd.repeats import get_repeat_count

pytestmark = pytest.mark.gpu
SEED = 11


@pytest.fixture(scope="module")
def data(tmp_path_factory):
    return make_chimeric_dataset(str(tmp_path_factory.mktemp("select_call")), n_loci=12, reads_per_locus=12)


@pytest.fixture(scope="module")
def reports(data, gpu_ctx):
    p = data["paths"]
    run = lambda bam, **kw: call_sample(bam, p["ref"], p["loci"], **kw)  # noqa: E731
    two = dict(unique_reads=True, skip_secondary=True)
    return {"device": run(p["bam"], **two), "host": run(p["bam"], front_end="host", **two), "python": run(read_bam(p["bam"]), **two),
            "all": run(p["bam"], skip_supplementary=True, **two), "clean": run(p["bam_clean"]),
            "off": run(p["bam"], unique_reads=False, skip_secondary=False, skip_supplementary=False), "plain": run(p["bam"]),
            "capped": run(p["bam"], max_reads=5)}


def test_the_data_has_the_extras(data):
    x = data["extras"]
    assert sorted(x["supplementary"].values()) == ["after"] * 4 + ["before"] * 4 and len(x["secondary"]) == 3 and len(x["duplicates"]) == 3
    segs = read_bam(data["paths"]["bam"]).segments
    assert len(segs) == 12 * 12 + 8 + 3 + 3 + 2
    for name, where in x["supplementary"].items():
        pos = [(s.start, k, s.flag & 0x800) for k, s in enumerate(segs) if s.name == name]
        assert len(pos) == 2 and (sorted(pos)[0][2] != 0) == (where == "before")


def test_the_three_paths_give_identical_reports(reports):
    dev, host, py = reports["device"], reports["host"], reports["python"]
    assert dev["errors"] == host["errors"] == py["errors"] == []
    assert dev["stage_times"]["front_end"] == "device" and host["stage_times"]["front_end"] == "host"
    assert dev["parameters"]["unique_reads"] is True and dev["parameters"]["skip_secondary"] is True and "skip_supplementary" not in dev["parameters"]
    assert "select_s" in dev["stage_times"] and "select_s" in host["stage_times"] and "select_s" in py["stage_times"]
    assert json.dumps(dev["results"]) == json.dumps(host["results"])
    assert dev["results"] == py["results"]
    assert sum("chimeric_in_region" in r for row in dev["results"] for r in row["reads"].values()) == 8 + 1


def test_a_read_at_two_loci_is_two_questions(data, reports):
    """The long read's primary is kept at loci 4 and 5, which one block holds; its supplementary record overlaps locus 5 only.
    The python path hands the SAME segment object to both loci: the mark belongs to the locus, not to the object."""
    sp = data["extras"]["spanning"]
    for key in ("device", "host", "python", "all"):
        rows = reports[key]["results"]
        here = [row for row in rows if sp["name"] in row["reads"]]
        assert len(here) == 2, key
        for row in here:
            li = next(int(n[1:].split("_")[0]) for n in row["reads"] if n.startswith("l"))
            assert li in sp["loci"]
            assert ("chimeric_in_region" in row["reads"][sp["name"]]) == (li == sp["chimeric_at"]), (key, li)


def test_with_all_switches_the_extras_change_nothing_but_the_chimeric_mark(data, reports):
    got, clean = reports["all"], reports["clean"]
    marked = set()
    assert len(got["results"]) == len(clean["results"]) == 12
    for a, b in zip(got["results"], clean["results"]):
        assert list(a) == list(b) and list(a["reads"]) == list(b["reads"])
        for name, r in a["reads"].items():
            if "chimeric_in_region" in r:
                assert r["chimeric_in_region"] is True
                marked.add(name)
        strip = {**a, "reads": {n: {k: v for k, v in r.items() if k != "chimeric_in_region"} for n, r in a["reads"].items()}}
        assert strip == b
    assert marked == set(data["extras"]["supplementary"]) | {data["extras"]["spanning"]["name"]}
    assert {k: v for k, v in got.items() if k not in ("parameters", "runtime", "stage_times", "results")} == \
        {k: v for k, v in clean.items() if k not in ("parameters", "runtime", "stage_times", "results")}


def test_a_supplementary_record_in_front_stands_in_for_its_read(data, reports):
    segs = read_bam(data["paths"]["bam"]).segments
    rows = {row["locus_index"]: row for row in reports["device"]["results"]}
    clean = {row["locus_index"]: row for row in reports["clean"]["results"]}
    n = 0
    for name, where in data["extras"]["supplementary"].items():
        row = next(r for r in rows.values() if name in r["reads"])
        seg = next(s for s in segs if s.name == name and bool(s.flag & 0x800) == (where == "before"))    # the first record of the name
        coords = get_read_coords_from_cigar(row["start"] - 70, row["start_adj"], row["end_adj"], row["end"] + 70, seg)
        sd = get_sequence_data_for_locus(seg, coords, 70, 13)
        motif = row["motif"]
        (cn, _), _, _ = get_repeat_count(round(len(sd.tr_seq) / len(motif)), sd.tr_seq_wc, sd.flank_left_seq_wc[-70:],
                                         sd.flank_right_seq_wc[:70], motif, default_read_rc_params())
        assert row["reads"][name]["cn"] == cn and row["reads"][name]["chimeric_in_region"] is True
        before = clean[row["locus_index"]]["reads"][name]["cn"]
        assert cn == (before + 2 if where == "before" else before)       # (the record in front carries a tract two copies longer)
        n += where == "before"
    assert n == 4


def test_with_the_switches_off_nothing_changes(reports):
    off, plain = reports["off"], reports["plain"]
    assert json.dumps(off["results"]) == json.dumps(plain["results"]) and off["parameters"] == plain["parameters"]
    assert "select_s" not in off["stage_times"] and "select_s" not in plain["stage_times"]
    assert not any("chimeric_in_region" in r for row in plain["results"] for r in row["reads"].values())
    # the plain cap is rules == 0 (tests/test_select_rule.py: test_rules_0_is_fetch_many_with_its_cap); a capped run keeps five
    for capped, row in zip(reports["capped"]["results"], plain["results"]):
        first = list(row["reads"])[:5]
        assert 3 <= len(capped["reads"]) <= 5 and list(capped["reads"]) == first[:len(capped["reads"])]     # (records of the first five may share a name)

def test_unique_reads_makes_the_allele_call_see_the_reads_of_the_row(data):
    """On the parent commit (and here without unique_reads) the two numbers differ on this file: a duplicated record collapses
    to one entry of the row's `reads`, keyed by name, while both records go to the allele call."""
    p = data["paths"]
    run = lambda **kw: call_sample(p["bam"], p["ref"], p["loci"], call_alleles=True, seed=SEED, **kw)  # noqa: E731
    with_, without = run(unique_reads=True), run()
    seen = lambda row: sum(row["peaks"]["n_reads"])  # noqa: E731
    n_differ = 0
    for a, b in zip(with_["results"], without["results"]):
        assert a["peaks"] and b["peaks"]
        assert seen(a) == len(a["reads"])
        n_differ += seen(b) != len(b["reads"])
        if any(name in b["reads"] for name in data["extras"]["duplicates"]):
            assert seen(b) > len(b["reads"])
    assert n_differ >= len(data["extras"]["duplicates"]) == 3
