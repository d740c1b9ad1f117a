"""GPU: `call` with use_methyl on the synthetic data of frontend/synth_methyl.py: every tagged kept read's mc and m equal the
truth the writer recorded, untagged reads carry null, the two haplotypes' am differ in the direction written, the control motif
has neither am nor amc; the device reader, the host reader and the readable path give equal rows; without the switch the rows
and the VCF are those of a plain run; the VCF with the switch on declares and carries AM / AMC."""
import json

import pytest

from strkit_amd.frontend import Fasta, call_sample, read_bam
from strkit_amd.frontend import methyl as me
from strkit_amd.frontend.output import write_vcf
from strkit_amd.frontend.synth_methyl import LEVELS, make_methyl_dataset

pytestmark = pytest.mark.gpu
SEED = 5


@pytest.fixture(scope="module")
def data(tmp_path_factory):
    return make_methyl_dataset(str(tmp_path_factory.mktemp("methyl_call")), n_loci=12, reads_per_locus=24, read_len=3000)


@pytest.fixture(scope="module")
def reports(data, gpu_ctx):
    p = data["paths"]
    run = lambda bam, **kw: call_sample(bam, p["ref"], p["loci"], call_alleles=True, seed=SEED, **kw)  # noqa: E731
    return {"device": run(p["bam"], use_methyl=True), "host": run(p["bam"], use_methyl=True, front_end="host"),
            "python": run(read_bam(p["bam"]), use_methyl=True), "plain": run(p["bam"]), "off": run(p["bam"], use_methyl=False)}


def test_reads_carry_the_truth_the_writer_recorded(data, reports):
    rep = reports["device"]
    assert rep["errors"] == [] and rep["parameters"]["use_methyl"] is True and "methyl_threshold" not in rep["parameters"]
    assert rep["stage_times"]["front_end"] == "device"
    n_tagged = n_untagged = n_value = 0
    for row in rep["results"]:
        assert len(row["reads"]) >= 20
        for name, r in row["reads"].items():
            t = data["reads"][name]
            assert "m" in r and "mc" in r
            if not t["tagged"]:
                assert r["m"] is None and r["mc"] is None
                n_untagged += 1
                continue
            n_tagged += 1
            if t["known"]:
                assert r["mc"] == t["mc"] and r["m"] == t["mc"] / t["known"], (name, r, t)
                n_value += 1
            else:
                assert r["m"] is None and r["mc"] is None, (name, r, t)
    assert n_tagged > 150 and n_untagged > 15 and n_value > 100
    print("call --use-methyl: %d tagged reads equal the writer's truth (%d with a value), %d untagged are null" % (n_tagged, n_value, n_untagged))


def test_alleles_differ_in_the_direction_written_and_the_control_has_none(data, reports):
    n_called = 0
    for row, truth in zip(reports["device"]["results"], data["loci"]):
        peaks = row["peaks"]
        assert row["call"] == list(truth["alleles"]) and peaks
        if truth["control"]:
            assert "am" not in peaks and "amc" not in peaks
            continue
        am, amc = peaks["am"], peaks["amc"]
        assert len(am) == len(amc) == 2 and am[0] < am[1] and amc[0] < amc[1]       # haplotype 0: fewer copies, lower level
        assert abs(am[0] - LEVELS[0]) < 0.2 and abs(am[1] - LEVELS[1]) < 0.2
        # allele_means against the rule on the row's own records: exact for amc's integer sums, 1e-12 relative for am
        for p in (0, 1):
            vals = [(r["m"], r["mc"]) for r in row["reads"].values() if r.get("p") == p and r["m"] is not None]
            assert amc[p] == sum(v[1] for v in vals) / len(vals)
            from fractions import Fraction
            exact = sum(Fraction(v[0]) for v in vals) / len(vals)
            assert abs(Fraction(am[p]) - exact) <= Fraction(1, 10**12) * exact
        n_called += 1
    assert n_called == 8
    recs = list(reports["device"]["results"][0]["reads"].values())
    assert me.allele_means([r["p"] for r in recs], [r["m"] for r in recs], [r["mc"] for r in recs], 2) == \
        (reports["device"]["results"][0]["peaks"]["am"], reports["device"]["results"][0]["peaks"]["amc"])


def test_the_three_paths_give_equal_rows(reports):
    assert reports["host"]["stage_times"]["front_end"] == "host"
    assert reports["device"]["results"] == reports["host"]["results"]
    assert reports["device"]["results"] == reports["python"]["results"]
    print("device reader == host reader == readable path: %d rows" % len(reports["device"]["results"]))


def test_without_the_switch_nothing_changes(data, reports, tmp_path):
    assert reports["off"]["results"] == reports["plain"]["results"] and reports["off"]["parameters"] == reports["plain"]["parameters"]
    assert json.dumps(reports["off"]["results"]) == json.dumps(reports["plain"]["results"])
    assert not any("m" in r or "mc" in r for row in reports["plain"]["results"] for r in row["reads"].values())
    assert not any("am" in (row["peaks"] or {}) for row in reports["plain"]["results"])
    # the switch adds fields and changes none
    for a, b in zip(reports["device"]["results"], reports["plain"]["results"]):
        strip = {**a, "peaks": {k: v for k, v in a["peaks"].items() if k not in ("am", "amc")},
                 "reads": {n: {k: v for k, v in r.items() if k not in ("m", "mc")} for n, r in a["reads"].items()}}
        assert strip == b
    ref = Fasta(data["paths"]["ref"])
    texts = {}
    for k in ("off", "plain", "device"):
        path = str(tmp_path / (k + ".vcf"))
        write_vcf(reports[k], path, ref, date="20250101")
        texts[k] = open(path).read()
    assert texts["off"] == texts["plain"] and "AM" not in texts["plain"].split("#CHROM")[0]
    on = texts["device"]
    assert "##FORMAT=<ID=AM,Number=.,Type=Float," in on and "##FORMAT=<ID=AMC,Number=.,Type=Float," in on
    recs = [ln.split("\t") for ln in on.splitlines() if not ln.startswith("#")]
    assert len(recs) == 12
    by_id = {row["locus_id"]: row for row in reports["device"]["results"]}
    for rec in recs:
        f = dict(zip(rec[8].split(":"), rec[9].split(":")))
        peaks = by_id[rec[2]]["peaks"]
        if "am" in peaks:
            assert f["AM"] == ",".join(f"{x:.6g}" for x in peaks["am"]) and f["AMC"] == ",".join(f"{x:.6g}" for x in peaks["amc"])
        else:
            assert f["AM"] == ".,." and f["AMC"] == ".,."


def test_another_threshold_is_reported_and_used(data, gpu_ctx):
    p = data["paths"]
    rep = call_sample(p["bam"], p["ref"], p["loci"], use_methyl=True, methyl_threshold=255)
    assert rep["parameters"]["methyl_threshold"] == 255 and "call_alleles" not in rep["parameters"]
    vals = [r["mc"] for row in rep["results"] for r in row["reads"].values() if r["mc"] is not None]
    assert vals and not any(vals)                                    # nothing is above 255
    assert all(row["peaks"] is None for row in rep["results"])       # per-read values stand alone: no calls, no am


def test_realigned_reads_get_their_values_through_the_substitute_alignment(gpu_ctx, tmp_path):
    """Soft-clipped reads come back with `realign`; their methylation is read through the substitute alignment (the native path
    hands it to the library per kept item, the readable path cuts the tract from the new pairs)."""
    t = make_methyl_dataset(str(tmp_path), n_loci=6, reads_per_locus=12, read_len=3000, soft_clipped=3, untagged=0.0, seed=3)
    p = t["paths"]
    run = lambda bam, **kw: call_sample(bam, p["ref"], p["loci"], realign=True, use_methyl=True, **kw)  # noqa: E731
    dev, host, py = run(p["bam"]), run(p["bam"], front_end="host"), run(read_bam(p["bam"]))
    assert dev["errors"] == [] and dev["results"] == host["results"] and dev["results"] == py["results"]
    n_realn = n_value = n_truth = 0
    for row, truth in zip(dev["results"], t["loci"]):
        for name, r in row["reads"].items():
            if not r.get("realn"):
                if t["reads"][name]["known"]:
                    assert (r["mc"], r["m"]) == (t["reads"][name]["mc"], t["reads"][name]["m"])
                continue
            n_realn += 1
            if truth["control"]:
                assert r["m"] is None and r["mc"] is None
                continue
            assert r["m"] is not None and 0.0 <= r["m"] <= 1.0 and r["mc"] >= 0
            n_value += 1
            n_truth += (r["mc"], r["m"]) == (t["reads"][name]["mc"], t["reads"][name]["m"])
    assert n_realn >= 12 and n_value >= 8
    print("realigned reads: %d, with a value %d, equal to the writer's truth %d" % (n_realn, n_value, n_truth))
