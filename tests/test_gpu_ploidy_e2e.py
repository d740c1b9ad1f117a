"""GPU: ploidy configurations end to end: `call --ploidy` on the data set of frontend/synth_ploidy.py, contigs
chr1 / chrX / chrY / chrM with 3 loci each and 12 reads of 2 kb per haplotype; the device reader, NativeBam and the readable
block path; the VCF."""
import pytest

from strkit_amd.frontend import Fasta, call_sample, load_loci, read_bam
from strkit_amd.frontend.call import call_blocks
from strkit_amd.frontend.options import PloidyCallOptions
from strkit_amd.frontend.output import write_vcf
from strkit_amd.frontend.synth_ploidy import make_ploidy_dataset

pytestmark = pytest.mark.gpu

SEED = 1907


@pytest.fixture(scope="module")
def male(tmp_path_factory):
    return make_ploidy_dataset(str(tmp_path_factory.mktemp("ploidy_xy")))


@pytest.fixture(scope="module")
def tetraploid(tmp_path_factory):
    return make_ploidy_dataset(str(tmp_path_factory.mktemp("ploidy_4")), 4)


def _call(t, **kw):
    return call_sample(t["paths"]["bam"], t["paths"]["ref"], t["paths"]["loci"], call_alleles=True, seed=SEED, **kw)


@pytest.fixture(scope="module")
def xy_rows(gpu_ctx, male):
    return _call(male, ploidy="XY", consensus=True, front_end="device")


@pytest.fixture(scope="module")
def plain_rows(gpu_ctx, male):
    return _call(male, front_end="device")


@pytest.fixture(scope="module")
def tetra_rows(gpu_ctx, tetraploid):
    return _call(tetraploid, ploidy={"default": 4}, consensus=True, count_kmers="both", front_end="device")


def test_xy_calls_one_allele_on_the_sex_chromosomes_and_chrM(male, xy_rows, plain_rows, tmp_path):
    rep = xy_rows
    assert rep["parameters"]["ploidy"] == "XY" and rep["catalog"]["num_loci_ploidy_ignored"] == 0
    assert [r["contig"] for r in rep["results"]] == [t["contig"] for t in male["loci"]] and len(rep["results"]) == 12
    for row, truth in zip(rep["results"], male["loci"]):
        assert row["call"] == truth["alleles"], (row["locus_id"], row["call"], truth)
        assert len(row["call"]) == (2 if row["contig"] == "chr1" else 1)
        assert row["assign_method"] == ("dist" if row["contig"] == "chr1" else "single")
        assert row["peaks"]["n_reads"] == [12] * len(truth["alleles"]) and all("p" in r for r in row["reads"].values())
        assert len(row["peaks"]["seqs"]) == len(truth["alleles"])
    # the plain run calls two alleles everywhere; where both runs ask for two, the rows are equal (same index, same seed)
    for row, old in zip(rep["results"], plain_rows["results"]):
        assert len(old["call"]) == 2
        if row["contig"] == "chr1":
            assert {k: v for k, v in row.items() if k != "peaks"} == {k: v for k, v in old.items() if k != "peaks"}
    path = str(tmp_path / "xy.vcf")
    assert write_vcf(rep, path, Fasta(male["paths"]["ref"])) == 12
    body = [ln.split("\t") for ln in open(path).read().split("\n") if ln and not ln.startswith("#")]
    for f in body:
        rec = dict(zip(f[8].split(":"), f[9].split(":")))
        n = 2 if f[0] == "chr1" else 1
        assert len(rec["GT"].split("/")) == n and len(rec["MC"].split(",")) == n and len(rec["AD"].split(",")) == n, f


def test_xx_and_diploid_autosomes_leave_contigs_out(male, xy_rows):
    by_index = {r["locus_index"]: r for r in xy_rows["results"]}
    xx = _call(male, ploidy="XX", front_end="device")
    assert [r["contig"] for r in xx["results"]] == ["chr1"] * 3 + ["chrX"] * 3 + ["chrM"] * 3
    assert xx["catalog"] == {"num_loci": 9, "num_loci_unknown_contig": 0, "num_loci_ploidy_ignored": 3}
    assert all(len(r["call"]) == (1 if r["contig"] == "chrM" else 2) for r in xx["results"])
    auto = _call(male, ploidy="diploid_autosomes", front_end="device")
    assert [r["contig"] for r in auto["results"]] == ["chr1"] * 3 + ["chrM"] * 3 and auto["catalog"]["num_loci_ploidy_ignored"] == 6
    # a locus keeps its index, so its seed, so its call, whatever is left out around it
    for rep in (xx, auto):
        for r in rep["results"]:
            if r["contig"] in ("chr1", "chrM"):
                assert r["call"] == by_index[r["locus_index"]]["call"] and r["call_95_cis"] == by_index[r["locus_index"]]["call_95_cis"]


def test_four_alleles_on_a_four_haplotype_file(tetraploid, tetra_rows, tmp_path):
    rep = tetra_rows
    assert len(rep["results"]) == 12
    exact = 0
    for row, truth in zip(rep["results"], tetraploid["loci"]):
        assert len(row["call"]) == 4 and len(truth["alleles"]) == 4
        assert max(abs(a - b) for a, b in zip(row["call"], truth["alleles"])) <= 1, (row["locus_id"], row["call"], truth)
        exact += row["call"] == truth["alleles"]
        assert row["peaks"]["modal_n"] == 4 and row["peaks"]["n_reads"] == [] and len(row["peaks"]["means"]) == 4
        assert len(row["call_95_cis"]) == 4 and len(row["call_99_cis"]) == 4
        assert len(row["reads"]) == 48 and all("p" not in r for r in row["reads"].values())
        assert all("kmers" in r for r in row["reads"].values())            # per read: as ever
        assert not any(k in row["peaks"] for k in ("seqs", "start_anchor_seqs", "kmers", "am", "amc"))
    assert exact >= 0.9 * 12, exact
    path = str(tmp_path / "tetra.vcf")
    assert write_vcf(rep, path, Fasta(tetraploid["paths"]["ref"])) == 12
    for f in (ln.split("\t") for ln in open(path).read().split("\n") if ln and not ln.startswith("#")):
        rec = dict(zip(f[8].split(":"), f[9].split(":")))
        assert rec["GT"] == "./././." and len(rec["MC"].split(",")) == 4 and rec["AD"] == "." and len(rec["MCCI"].split(",")) == 4
        assert "," not in rec["MCRL"] and "," not in rec["SLR"]           # one group over all kept reads


@pytest.mark.parametrize("which", ["xy", "tetra"])
def test_device_reader_native_reader_and_readable_path_give_equal_rows(gpu_ctx, male, tetraploid, xy_rows, tetra_rows, which):
    t, dev, kw = {"xy": (male, xy_rows, dict(ploidy="XY", consensus=True)),
                  "tetra": (tetraploid, tetra_rows, dict(ploidy={"default": 4}, consensus=True, count_kmers="both"))}[which]
    host = _call(t, front_end="host", **kw)
    assert dev["stage_times"]["front_end"] == "device" and host["stage_times"]["front_end"] == "host"
    assert dev["results"] == host["results"] and dev["catalog"] == host["catalog"]
    opts = PloidyCallOptions(call_alleles=True, seed=SEED, **kw)
    rows, _n, _tm = call_blocks(load_loci(t["paths"]["loci"]), read_bam(t["paths"]["bam"]), Fasta(t["paths"]["ref"]), opts, gpu_ctx)
    assert rows == dev["results"]


def test_without_the_option_the_report_is_the_plain_one(gpu_ctx, male, plain_rows):
    same = call_sample(male["paths"]["bam"], male["paths"]["ref"], male["paths"]["loci"], front_end="device",
                       opts=PloidyCallOptions(call_alleles=True, seed=SEED))
    assert same["results"] == plain_rows["results"] and same["parameters"] == plain_rows["parameters"]
    assert same["catalog"] == plain_rows["catalog"] and "num_loci_ploidy_ignored" not in same["catalog"]


def test_a_phased_run_calls_loci_of_more_than_two_alleles_plainly(gpu_ctx, tetraploid, tetra_rows):
    rep = _call(tetraploid, ploidy={"default": 4, "overrides": {"chrX": 2}}, use_hp=True, front_end="device")
    for row, old in zip(rep["results"], tetra_rows["results"]):
        if row["contig"] == "chrX":
            assert len(row["call"]) == 2 and row["assign_method"] == "dist"
        else:   # never phased: the call of the run without the switch
            assert row["call"] == old["call"] and row["call_95_cis"] == old["call_95_cis"] and row["peaks"]["means"] == old["peaks"]["means"]
            assert row["assign_method"] == "dist" and all("p" not in r for r in row["reads"].values())
