"""GPU: phasing from files end to end: `call` with a candidate-SNV VCF or with haplotags on the data set of
frontend/synth_phased.py, 12 loci x 24 reads of 3 kb whose two haplotypes have EQUAL copy numbers, so that only the phasing
separates them; the device reader, NativeBam and the readable block path; the VCF."""
import pytest

from strkit_amd.frontend import Fasta, call_sample, load_loci, read_bam
from strkit_amd.frontend.call import call_blocks
from strkit_amd.frontend import phase_block
from strkit_amd.frontend.options import PhasedCallOptions
from strkit_amd.frontend.output import write_vcf
from strkit_amd.frontend.synth_phased import make_phased_dataset

pytestmark = pytest.mark.gpu

SEED = 4321


@pytest.fixture(scope="module")
def data(tmp_path_factory):
    return make_phased_dataset(str(tmp_path_factory.mktemp("phased")), n_loci=12, reads_per_locus=24, read_len=3000, equal_cn=True)


def _call(t, **kw):
    return call_sample(t["paths"]["bam"], t["paths"]["ref"], t["paths"]["loci"], call_alleles=True, seed=SEED, **kw)


def _labels_equal_truth(row, t, swap_allowed):
    got = [r["p"] for r in row["reads"].values()]
    want = [t["read_hap"][name] for name in row["reads"]]
    return got == want or (swap_allowed and got == [1 - h for h in want])


@pytest.fixture(scope="module")
def snv_rows(gpu_ctx, data):
    return _call(data, snv_vcf=data["paths"]["snvs"], front_end="device")


@pytest.fixture(scope="module")
def hp_rows(gpu_ctx, data):
    return _call(data, use_hp=True, consensus=True, front_end="device")


def test_snvs_separate_two_haplotypes_of_equal_copy_number(data, snv_rows):
    rep = snv_rows
    assert rep["parameters"]["snv_vcf"] == data["paths"]["snvs"] and rep["stage_times"]["front_end"] == "device"
    assert len(rep["results"]) == 12
    for row, truth in zip(rep["results"], data["loci"]):
        # every locus of the data set has at least one heterozygous site that all 24 reads cover: none is unphaseable by construction
        assert len(truth["het"]) >= 1 and len(row["reads"]) == 24, row["locus_id"]
        assert row["call"] == list(truth["alleles"]), row["locus_id"]
        assert row["assign_method"] in ("snv", "snv+dist"), (row["locus_id"], row["assign_method"])
        assert _labels_equal_truth(row, data, swap_allowed=True), row["locus_id"]
        assert row["peaks"]["n_reads"] == [12, 12]
        assert row["snvs"] and {s["pos"] for s in row["snvs"]} <= set(truth["het"]), (row["locus_id"], row["snvs"], truth)
        assert all(s["id"].startswith("het") and len(s["call"]) == 2 and s["call"][0] != s["call"][1] and s["rcs"] == [12, 12] for s in row["snvs"])
        assert "ps" not in row
        for name, r in row["reads"].items():     # the read's own bases at the called SNVs are the called base of its peak
            assert r["snvu"] == [s["call"][r["p"]] for s in row["snvs"]], (row["locus_id"], name)


def test_haplotags_give_hp_calls_and_renumbered_phase_sets(data, hp_rows, tmp_path):
    rep = hp_rows
    assert rep["parameters"]["use_hp"] is True
    for li, (row, truth) in enumerate(zip(rep["results"], data["loci"])):
        assert row["assign_method"] == "hp", row["locus_id"]
        assert row["ps"] == li // 4 + 1, (row["locus_id"], row["ps"])          # 50000, 50007, 50014 in order of first appearance
        assert _labels_equal_truth(row, data, swap_allowed=False), row["locus_id"]      # peaks in ascending HP order
        assert all(r["hp"] == data["read_hap"][name] + 1 and r["ps"] == row["ps"] for name, r in row["reads"].items())
        assert "snvs" not in row and all("snvu" not in r for r in row["reads"].values())
    path = str(tmp_path / "hp.vcf")
    assert write_vcf(rep, path, Fasta(data["paths"]["ref"])) == 12
    text = open(path).read()
    assert '##FORMAT=<ID=PS,Number=1,Type=Integer,Description="Phase set">' in text and "ID=NSNV" not in text
    body = [ln.split("\t") for ln in text.split("\n") if ln and not ln.startswith("#")]
    for li, f in enumerate(body):
        rec = dict(zip(f[8].split(":"), f[9].split(":")))
        assert rec["PM"] == "hp" and rec["PS"] == str(li // 4 + 1) and "|" in rec["GT"] and "/" not in rec["GT"], f[8:]


def test_snv_calls_in_the_vcf(data, tmp_path):
    rep = _call(data, snv_vcf=data["paths"]["snvs"], consensus=True, front_end="device")
    path = str(tmp_path / "snv.vcf")
    write_vcf(rep, path, Fasta(data["paths"]["ref"]))
    text = open(path).read()
    assert "ID=NSNV" in text and "ID=PS," not in text
    for row, ln in zip(rep["results"], [ln for ln in text.split("\n") if ln and not ln.startswith("#")]):
        f = ln.split("\t")
        rec = dict(zip(f[8].split(":"), f[9].split(":")))
        assert rec["PM"] == row["assign_method"] and rec["NSNV"] == str(len(row["snvs"])) and "/" in rec["GT"]


def test_without_a_switch_the_rows_are_those_of_a_plain_run(gpu_ctx, data):
    plain = _call(data, front_end="device")
    same = call_sample(data["paths"]["bam"], data["paths"]["ref"], data["paths"]["loci"], front_end="device",
                       opts=PhasedCallOptions(call_alleles=True, seed=SEED))
    assert same["results"] == plain["results"] and same["parameters"] == plain["parameters"]
    assert all(r["assign_method"] in ("dist", "single") for r in plain["results"])


@pytest.mark.parametrize("mode", ["snv", "hp", "both"])
def test_device_reader_native_reader_and_readable_path_give_equal_rows(gpu_ctx, data, snv_rows, mode):
    kw = {"snv": {"snv_vcf": data["paths"]["snvs"]}, "hp": {"use_hp": True},
          "both": {"use_hp": True, "snv_vcf": data["paths"]["snvs"]}}[mode]
    dev = snv_rows if mode == "snv" else _call(data, front_end="device", **kw)
    host = _call(data, front_end="host", **kw)
    assert dev["stage_times"]["front_end"] == "device" and host["stage_times"]["front_end"] == "host"
    assert dev["results"] == host["results"]
    opts = PhasedCallOptions(call_alleles=True, seed=SEED, **kw)
    rows, _n, _tm = call_blocks(load_loci(data["paths"]["loci"]), read_bam(data["paths"]["bam"]), Fasta(data["paths"]["ref"]), opts, gpu_ctx)
    assert rows == dev["results"]
    if mode == "both":          # haplotags come first (call_locus.py:1381-1495)
        assert all(r["assign_method"] == "hp" for r in rows)


def test_a_share_of_untagged_reads_and_unequal_copy_numbers(gpu_ctx, tmp_path):
    t = make_phased_dataset(str(tmp_path / "u"), n_loci=4, reads_per_locus=24, read_len=3000, seed=5, equal_cn=False, untagged=0.25)
    rep = _call(t, use_hp=True, front_end="device")
    for row, truth in zip(rep["results"], t["loci"]):
        assert row["call"] == list(truth["alleles"]) or row["call"] == list(truth["alleles"])[::-1]
        tagged = [name for name, r in row["reads"].items() if "hp" in r]
        assert 0 < len(tagged) < 24 and all(row["reads"][n]["hp"] == t["read_hap"][n] + 1 for n in tagged)


def test_loci_cut_into_pieces_of_cells_give_the_same_rows(gpu_ctx, data, snv_rows, monkeypatch):
    """The cell workspace bound: with room for one locus's cells per pair of calls the rows are those of the uncut run."""
    monkeypatch.setattr(phase_block, "MAX_CELLS", 24 * 8)
    for fe in ("device", "host"):
        assert _call(data, snv_vcf=data["paths"]["snvs"], use_hp=True, front_end=fe)["results"] == \
            _call_uncut(data, fe, monkeypatch)["results"]


def _call_uncut(data, fe, monkeypatch):
    with monkeypatch.context() as m:
        m.setattr(phase_block, "MAX_CELLS", 1 << 28)
        return _call(data, snv_vcf=data["paths"]["snvs"], use_hp=True, front_end=fe)


@pytest.mark.parametrize("soft_clipped", [1, 3])
def test_realigned_reads_and_the_realign_gates(gpu_ctx, tmp_path, soft_clipped):
    """--realign: a realigned read's substitute alignment spans the flanked locus only, so its cells are '-' in every path; one
    realigned kept read leaves the SNV step on, two or more (many_realigns_threshold) switch it off."""
    t = make_phased_dataset(str(tmp_path / "r"), n_loci=4, reads_per_locus=24, read_len=3000, seed=9, equal_cn=True, tags=False,
                            soft_clipped=soft_clipped)
    kw = {"snv_vcf": t["paths"]["snvs"], "realign": True}
    dev, host = _call(t, front_end="device", **kw), _call(t, front_end="host", **kw)
    assert dev["results"] == host["results"]
    opts = PhasedCallOptions(call_alleles=True, seed=SEED, **kw)
    rows, _n, _tm = call_blocks(load_loci(t["paths"]["loci"]), read_bam(t["paths"]["bam"]), Fasta(t["paths"]["ref"]), opts, gpu_ctx)
    assert rows == dev["results"]
    for row in rows:
        n_re = sum(1 for r in row["reads"].values() if r.get("realn"))
        assert n_re == soft_clipped, (row["locus_id"], n_re)
        if soft_clipped >= 2:
            assert row["assign_method"] in ("dist", "single") and "snvs" not in row, (row["locus_id"], row["assign_method"])
        else:
            assert row["assign_method"] in ("snv", "snv+dist"), (row["locus_id"], row["assign_method"])
            for name, r in row["reads"].items():
                if r.get("realn"):
                    assert set(r["snvu"]) == {"-"}, (row["locus_id"], name, r["snvu"])
