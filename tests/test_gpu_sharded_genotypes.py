"""GPU: `call` with genotypes under torch.distributed.  Two ranks over gloo, both on device 0, each calling its
share of at least four locus blocks: on every rank the report's results (as JSON text), errors, catalog, contigs and parameters,
and the VCF written from it, are those of one process with the same seed."""
import json
import os
import queue
import time

import pytest

from strkit_amd.frontend import Fasta, call_sample
from strkit_amd.frontend.output import write_vcf
from strkit_amd.frontend.synth_dataset import make_dataset
from strkit_amd.frontend.synth_phased import make_phased_dataset
from strkit_amd.frontend.synth_ploidy import make_ploidy_dataset
from strkit_amd.frontend.synth_snvs import index_snv_vcf

pytestmark = pytest.mark.gpu

SEED = 9157
DATE = "20261021"
PARTS = ("errors", "catalog", "contigs", "parameters")


def _summary(rep, paths, vcf_path):
    write_vcf(rep, vcf_path, Fasta(paths["ref"]), date=DATE)
    return {"results": json.dumps(rep["results"]), **{k: rep[k] for k in PARTS}, "stage": sorted(rep["stage_times"]),
            "front_end": rep["stage_times"]["front_end"], "vcf": open(vcf_path, "rb").read()}


def _rank_worker(rank, world, port, paths, kw, out_dir, q):
    os.environ["STRKIT_AMD_DEVICE"] = "0"            # both ranks share the one GPU of the test box
    import torch.distributed as dist
    dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{port}", rank=rank, world_size=world)
    rep = call_sample(paths["bam"], paths["ref"], paths["loci"], processes=4, **kw)
    q.put((rank, _summary(rep, paths, os.path.join(out_dir, f"rank{rank}.vcf"))))
    dist.barrier()
    dist.destroy_process_group()


def _two_ranks(paths, kw, out_dir, limit=240.0):
    """The summaries of both ranks, by rank.  Every wait is bounded; a rank that ends with anything but 0 fails the test at once
    (the other rank, which would wait for it in a collective, is ended)."""
    import socket

    import torch.multiprocessing as mp
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_rank_worker, args=(r, 2, port, paths, kw, str(out_dir), q)) for r in range(2)]
    for p in procs:
        p.start()
    got, deadline = {}, time.monotonic() + limit
    try:
        while len(got) < len(procs):
            try:
                rank, summary = q.get(timeout=0.5)
                got[rank] = summary
            except queue.Empty:
                bad = [(r, p.exitcode) for r, p in enumerate(procs) if p.exitcode not in (None, 0)]
                assert not bad, f"(rank, exit code) {bad}"
                assert time.monotonic() < deadline, "the ranks did not report in time"
        for r, p in enumerate(procs):
            p.join(timeout=60)
            assert p.exitcode == 0, (r, p.exitcode)
    finally:
        for p in procs:
            if p.is_alive():
                p.kill()
                p.join(timeout=30)
    return got


def _same_as_one_process(paths, kw, tmp_path, front_end, want_blocks=4):
    from strkit_amd.frontend import load_loci
    assert len(load_loci(paths["loci"], processes=4)) >= want_blocks
    kw = dict(kw, front_end=front_end)
    one = call_sample(paths["bam"], paths["ref"], paths["loci"], processes=4, **kw)
    want = _summary(one, paths, str(tmp_path / "one.vcf"))
    assert want["front_end"] == front_end
    got = _two_ranks(paths, kw, tmp_path)
    for rank in (0, 1):
        g = got[rank]
        assert g["results"] == want["results"], rank
        for k in PARTS:
            assert g[k] == want[k], (rank, k)
        assert g["vcf"] == want["vcf"], rank
        assert g["front_end"] == front_end and "gather_s" in g["stage"] and "alleles_s" in g["stage"]
    return one, got


@pytest.fixture(scope="module")
def phased(tmp_path_factory):
    t = make_phased_dataset(str(tmp_path_factory.mktemp("sharded_phased")))
    t["paths"]["snvs_gz"] = index_snv_vcf(t["paths"]["snvs"], block_bytes=512)
    return t


def test_haplotags(gpu_ctx, phased, tmp_path):
    one, got = _same_as_one_process(phased["paths"], dict(call_alleles=True, seed=SEED, use_hp=True, consensus=True), tmp_path, "device")
    rows = one["results"]
    assert sum(r["assign_method"] == "hp" for r in rows) >= 6 and len({r["ps"] for r in rows if "ps" in r}) >= 2
    assert "phase_inputs_s" in got[0]["stage"] and "phase_cells_s" in got[1]["stage"]


@pytest.mark.parametrize("indexed,front_end", [(False, "host"), (True, "device")])
def test_snv_candidates(gpu_ctx, phased, tmp_path, indexed, front_end):
    kw = dict(call_alleles=True, seed=SEED, snv_vcf=phased["paths"]["snvs_gz" if indexed else "snvs"], snv_min_base_qual=15,
              significant_clip_threshold=50, consensus=True)
    one, got = _same_as_one_process(phased["paths"], kw, tmp_path, front_end)
    rows = one["results"]
    assert sum(r["assign_method"] in ("snv", "snv+dist") for r in rows) >= 4 and all("snvu" in x for r in rows if "snvs" in r for x in r["reads"].values())
    assert ("snv_candidates_s" in got[0]["stage"]) == indexed


def test_ploidy_with_a_wide_and_an_ignored_contig(gpu_ctx, tmp_path):
    t = make_ploidy_dataset(str(tmp_path / "d"), {"chr1": 3, "chrX": 1, "chrY": 2, "chrM": 1})
    ploidy = {"default": 2, "overrides": {"chr1": 3, "(chr)?X": 1}, "ignore": ["chrM"]}
    one, _got = _same_as_one_process(t["paths"], dict(call_alleles=True, seed=SEED, ploidy=ploidy, consensus=True, count_kmers="both"),
                                     tmp_path, "device", want_blocks=4)
    assert one["catalog"]["num_loci_ploidy_ignored"] == 3 and one["contigs"] == ["chr1", "chrX", "chrY"]
    assert {len(r["call"]) for r in one["results"] if r["call"]} == {1, 2, 3}
    assert any(r["peaks"] and r["peaks"]["modal_n"] == 3 and not r["read_peaks_called"] for r in one["results"])


def test_poa_sequences_and_kmers(gpu_ctx, tmp_path):
    t = make_dataset(str(tmp_path / "d"), n_loci=12, reads_per_locus=14, read_len=2000, seed=5, sub=0.01, indel=0.015, low_qual=0.01)
    kw = dict(call_alleles=True, seed=SEED, consensus=True, consensus_method="poa", max_mdn_poa_length=4000, count_kmers="both", n_alleles=2)
    one, got = _same_as_one_process(t["paths"], kw, tmp_path, "host")
    methods = {m for r in one["results"] if r["call"] for _s, m in r["peaks"]["seqs"]}
    assert "poa" in methods and all("kmers" in x for r in one["results"] for x in r.get("reads", {}).values())
    assert any(r["peaks"] and "kmers" in r["peaks"] for r in one["results"])
    assert {"consensus_s", "kmers_s"} <= set(got[1]["stage"])


def test_one_seed_for_the_run_when_none_is_given(gpu_ctx, tmp_path):
    t = make_dataset(str(tmp_path / "d"), n_loci=8, reads_per_locus=12, read_len=2000, seed=3)
    kw = dict(call_alleles=True, n_alleles=1, front_end="device")
    got = _two_ranks(t["paths"], kw, tmp_path)
    seed = got[0]["parameters"]["seed"]
    assert isinstance(seed, int) and got[1]["parameters"]["seed"] == seed
    one = call_sample(t["paths"]["bam"], t["paths"]["ref"], t["paths"]["loci"], processes=4, seed=seed, **kw)
    want = _summary(one, t["paths"], str(tmp_path / "one.vcf"))
    for rank in (0, 1):
        assert got[rank]["results"] == want["results"] and got[rank]["vcf"] == want["vcf"] and got[rank]["parameters"] == want["parameters"]
