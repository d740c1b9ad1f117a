"""GPU: `call` with candidate SNVs from a tabix-indexed file end to end, on the data sets of
frontend/synth_phased.py (12 loci x 24 reads) and frontend/synth_linked.py (15 loci on two contigs): the rows equal those of the
run on the plain file for the device reader, the host reader, the readable block path and blocks of one locus; only the windows
of the blocks are read; a run without an index is what it was.  Every run is made once per module."""
import os

import pytest

from strkit_amd.frontend import DeviceBam, Fasta, call_sample, load_loci, read_bam
from strkit_amd.frontend.call import call_blocks
from strkit_amd.frontend.options import PhaseSetCallOptions
from strkit_amd.frontend.synth_linked import make_linked_dataset
from strkit_amd.frontend.synth_phased import make_phased_dataset
from strkit_amd.frontend.synth_snvs import index_snv_vcf

pytestmark = pytest.mark.gpu

SEED = 4321
NEW_KEYS = ("snv_candidates_s", "snv_vcf_compressed_mb", "snv_vcf_device_s")


@pytest.fixture(scope="module")
def phased(tmp_path_factory):
    t = make_phased_dataset(str(tmp_path_factory.mktemp("phased")))
    t["paths"]["snvs_gz"] = index_snv_vcf(t["paths"]["snvs"], block_bytes=512)
    return t


@pytest.fixture(scope="module")
def linked(tmp_path_factory):
    t = make_linked_dataset(str(tmp_path_factory.mktemp("linked")))
    t["paths"]["snvs_gz"] = index_snv_vcf(t["paths"]["snvs"], block_bytes=512)
    return t


def _call(t, **kw):
    return call_sample(t["paths"]["bam"], t["paths"]["ref"], t["paths"]["loci"], call_alleles=True, seed=SEED, **kw)


@pytest.fixture(scope="module")
def phased_plain(gpu_ctx, phased):
    return _call(phased, snv_vcf=phased["paths"]["snvs"], front_end="device")


def test_phased_rows_equal_the_plain_file_run(gpu_ctx, phased, phased_plain):
    assert any(r.get("assign_method") in ("snv", "snv+dist") for r in phased_plain["results"])
    for fe in ("device", "host"):
        got = _call(phased, snv_vcf=phased["paths"]["snvs_gz"], front_end=fe)
        assert got["results"] == phased_plain["results"], fe
        tm = got["stage_times"]
        assert tm["front_end"] == fe and tm["snv_candidates_s"] > 0 and tm["snv_vcf_compressed_mb"] > 0
        assert ("snv_vcf_device_s" in tm) == (fe == "device")


def test_linked_rows_equal_the_plain_file_run_with_and_without_phase_sets(gpu_ctx, linked):
    for sets in (False, True):
        kw = {"snv_phase_sets": True} if sets else {}
        want = _call(linked, snv_vcf=linked["paths"]["snvs"], front_end="device", **kw)
        for fe in ("device", "host"):
            got = _call(linked, snv_vcf=linked["paths"]["snvs_gz"], front_end=fe, **kw)
            assert got["results"] == want["results"], (sets, fe)


def test_blocks_of_one_locus_and_the_readable_path_agree(gpu_ctx, linked):
    kw = dict(snv_phase_sets=True)
    want = _call(linked, snv_vcf=linked["paths"]["snvs"], front_end="device", **kw)["results"]
    opts = PhaseSetCallOptions(call_alleles=True, seed=SEED, snv_vcf=linked["paths"]["snvs_gz"], **kw)
    ref = Fasta(linked["paths"]["ref"])
    single = load_loci(linked["paths"]["loci"], max_block_size=1)
    assert all(len(b) == 1 for b in single)
    bam = DeviceBam(linked["paths"]["bam"])
    try:
        rows, _n, tm = call_blocks(single, bam, ref, opts, gpu_ctx)
    finally:
        bam.close()
    assert rows == want and "snv_vcf_device_s" in tm
    rows, _n, tm = call_blocks(load_loci(linked["paths"]["loci"]), read_bam(linked["paths"]["bam"]), ref, opts, gpu_ctx)
    assert rows == want and "snv_candidates_s" in tm and "snv_vcf_device_s" not in tm


def test_only_the_windows_of_the_blocks_are_read(gpu_ctx, phased, phased_plain, tmp_path):
    """A base-valid record whose POS is no number, behind records 1 to 5 Mb past every locus: the whole-file reader meets it and
    raises, the indexed reader never inflates its block."""
    text = open(phased["paths"]["snvs"]).read()
    last = max(int(ln.split("\t")[1]) for ln in text.split("\n") if ln and ln[0] != "#")
    far = "".join(f"chr1\t{last + 1_000_000 + 50_000 * i}\tfar{i}\tA\tG\t.\t.\t.\n" for i in range(81))
    assert f"\t{last + 5_000_000}\t" in far
    plain = tmp_path / "snvs_bad.vcf"
    plain.write_text(text + far + "chr1\tNaN\tbad\tA\tG\t.\t.\t.\n")
    gz = index_snv_vcf(str(plain), block_bytes=512)
    with pytest.raises(ValueError):
        _call(phased, snv_vcf=str(plain), front_end="device")
    for fe in ("device", "host"):
        got = _call(phased, snv_vcf=gz, front_end=fe)
        assert got["results"] == phased_plain["results"] and not got["errors"], fe
        assert 0 < got["stage_times"]["snv_vcf_compressed_mb"] < os.path.getsize(gz) / 1e6


def test_a_run_without_an_index_has_none_of_the_new_stage_times(phased_plain, phased, gpu_ctx, tmp_path):
    assert not any(k in phased_plain["stage_times"] for k in NEW_KEYS)
    # BGZF without a .tbi: the whole-file path
    import shutil
    alone = str(tmp_path / "alone.vcf.gz")
    shutil.copy(phased["paths"]["snvs_gz"], alone)
    got = _call(phased, snv_vcf=alone, front_end="device")
    assert got["results"] == phased_plain["results"] and not any(k in got["stage_times"] for k in NEW_KEYS)
