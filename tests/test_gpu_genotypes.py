"""GPU: genotypes from files — call_sample(call_alleles=True[, consensus=True]) on synthetic data sets with known truth."""
import numpy as np
import pytest

import alleles_restatement as AR
import consensus_restatement as CR
from strkit_amd.alleles import AlleleParams, call_alleles_batch, locus_seed
from strkit_amd.frontend import (Fasta, call_sample, get_read_coords_from_cigar, get_sequence_data_for_locus, load_loci,
                                 read_bam)
from strkit_amd.frontend.call import CallOptions, call_blocks
from strkit_amd.frontend.output import allele_calling_inputs, write_vcf
from strkit_amd.frontend.synth_dataset import make_dataset

pytestmark = pytest.mark.gpu

SEED = 1234
ROW_KEYS = ("assign_method", "call", "call_95_cis", "call_99_cis", "peaks", "read_peaks_called", "reads")


def _call(t, **kw):
    return call_sample(t["paths"]["bam"], t["paths"]["ref"], t["paths"]["loci"], call_alleles=True, seed=SEED, **kw)


def test_error_free_reads_give_the_true_genotype(gpu_ctx, tmp_path):
    t = make_dataset(str(tmp_path / "a"), n_loci=60, reads_per_locus=12, read_len=2500, seed=11)
    rep = _call(t, consensus=True)
    assert rep["parameters"]["call_alleles"] is True and rep["parameters"]["seed"] == SEED and rep["parameters"]["consensus"] is True
    left_out = 0
    n_hom = 0
    for row, truth in zip(rep["results"], t["loci"]):
        a1, a2 = truth["alleles"]
        cns, w = allele_calling_inputs(row)
        ours = AR.call_locus(cns, w, 2, locus_seed(SEED, row["locus_index"]))
        if sorted(ours["call"]) != sorted((a1, a2)):
            left_out += 1        # the restatement itself, on the row's own inputs, does not return the truth
            continue
        assert sorted(row["call"]) == sorted((a1, a2)), row["locus_id"]
        assert row["assign_method"] == "dist" and row["read_peaks_called"] is True
        assert row["mean_model_align_score"] == 2.0
        peaks = row["peaks"]
        n1 = sum(1 for c in truth["reads"].values() if c == a1)
        if a1 == a2:
            n_hom += 1
            assert peaks["modal_n"] == 1 and peaks["n_reads"] == [len(truth["reads"])]
            assert all(r["p"] == 0 for r in row["reads"].values())
        else:
            assert peaks["modal_n"] == 2
            by_call = dict(zip(row["call"], peaks["n_reads"]))
            assert by_call == {a1: n1, a2: len(truth["reads"]) - n1}
            for name, r in row["reads"].items():
                assert row["call"][r["p"]] == truth["reads"][name]
        assert len(peaks["seqs"]) == peaks["modal_n"] == len(peaks["start_anchor_seqs"])
        for k, (seq, method) in enumerate(peaks["seqs"]):
            assert seq == truth["motif"] * row["call"][k] and method == "single"
        for anchor, method in peaks["start_anchor_seqs"]:
            assert anchor == row["ref_start_anchor"] and method == "single"
    share = left_out / len(rep["results"])
    print(f"loci left out because the restatement does not return the truth: {left_out} of {len(rep['results'])} ({share:.1%})")
    assert share <= 0.05
    assert n_hom >= 3
    # fewer reads than min_reads: nothing is called, the rows are today's
    t2 = make_dataset(str(tmp_path / "b"), n_loci=8, reads_per_locus=3, read_len=2000, seed=3)
    plain = call_sample(t2["paths"]["bam"], t2["paths"]["ref"], t2["paths"]["loci"])
    assert _call(t2, consensus=True)["results"] == plain["results"]
    assert all(r["call"] is None and r["peaks"] is None and r["read_peaks_called"] is False for r in plain["results"])


def _noisy(tmp_path):
    return make_dataset(str(tmp_path / "n"), n_loci=30, reads_per_locus=14, read_len=2000, seed=5, sub=0.01, indel=0.015,
                        low_qual=0.01)


def test_noisy_rows_equal_the_library_and_the_restatement(gpu_ctx, tmp_path):
    t = _noisy(tmp_path)
    rep = _call(t, consensus=True, respect_ref=True)
    bam, (block,) = read_bam(t["paths"]["bam"]), load_loci(t["paths"]["loci"])
    n_called = n_best_rep = 0
    for locus, row in zip(block, rep["results"]):
        cns, w = allele_calling_inputs(row)
        out = call_alleles_batch([0, len(cns)], cns, w, [2], [locus_seed(SEED, row["locus_index"])], AlleleParams(), gpu_ctx)
        assert [r["p"] for r in row["reads"].values()] == out["read_peak"].tolist()
        if int(out["status"][0]) == 2:     # a peak without reads: the call is nullified, the reads keep their labels
            assert row["call"] is None and row["peaks"] is None and row["read_peaks_called"] is True
            continue
        assert int(out["status"][0]) == 0 and row["call"] is not None
        n_called += 1
        k = int(out["modal_n"][0])
        assert row["call"] == out["call"][0].tolist() and row["peaks"]["modal_n"] == k
        assert row["call_95_cis"] == out["ci95"][0].tolist() and row["call_99_cis"] == out["ci99"][0].tolist()
        assert row["peaks"]["n_reads"] == out["peak_n_reads"][0, :k].tolist()
        assert [r["p"] for r in row["reads"].values()] == out["read_peak"].tolist()
        for key in ("means", "weights", "stdevs"):
            assert np.allclose(row["peaks"][key], out[key][0, :k], rtol=0, atol=1e-12), key
        # the sequences: the restatement's pick over the raw tracts / anchors of the readable path
        raw = {}
        for s in bam.fetch(locus.contig, locus.left_flank_coord, locus.right_flank_coord):
            c = get_read_coords_from_cigar(locus.left_flank_coord, locus.left_coord, locus.right_coord, locus.right_flank_coord, s)
            if c.is_incomplete():
                continue
            sd = get_sequence_data_for_locus(s, c, 70)
            raw[s.name] = (sd.tr_seq, s.query_sequence[max(c.left_flank_start, c.left_flank_end - 5):c.left_flank_end])
        for p in range(k):
            names = [nm for nm, r in row["reads"].items() if r["p"] == p]
            for which, key in ((0, "seqs"), (1, "start_anchor_seqs")):
                group = [raw[nm][which] for nm in names]
                i, method, _ = CR.best_representative(group)
                assert row["peaks"][key][p] == [group[i], method], (row["locus_id"], key, p)
                n_best_rep += method == "best_rep"
                assert "X" not in row["peaks"][key][p][0]
    assert n_called >= 27 and n_best_rep >= 10


def test_device_host_and_readable_paths_agree(gpu_ctx, tmp_path):
    t = _noisy(tmp_path)
    dev = _call(t, consensus=True, front_end="device")
    host = _call(t, consensus=True, front_end="host")
    assert dev["stage_times"]["front_end"] == "device" and host["stage_times"]["front_end"] == "host"
    assert dev["results"] == host["results"]
    opts = CallOptions(call_alleles=True, consensus=True, seed=SEED)
    rows, _n, _tm = call_blocks(load_loci(t["paths"]["loci"]), read_bam(t["paths"]["bam"]), Fasta(t["paths"]["ref"]), opts, gpu_ctx)
    assert rows == dev["results"]
    assert sum(1 for r in rows if r["call"]) >= 27
    # realigned reads: both extractions cut the same positions
    t2 = make_dataset(str(tmp_path / "r"), n_loci=10, reads_per_locus=8, read_len=2500, seed=2, soft_clip_frac=0.7, expansion=40)
    a = _call(t2, consensus=True, realign=True, front_end="device")
    b = _call(t2, consensus=True, realign=True, front_end="host")
    assert a["results"] == b["results"] and any(r.get("realn") for row in a["results"] for r in row["reads"].values())


def test_calls_do_not_depend_on_the_blocks_and_follow_the_seed(gpu_ctx, tmp_path):
    t = _noisy(tmp_path)
    one = _call(t, consensus=True)
    assert _call(t, consensus=True)["results"] == one["results"]
    four = _call(t, consensus=True, processes=4)
    assert four["results"] == one["results"]
    other = call_sample(t["paths"]["bam"], t["paths"]["ref"], t["paths"]["loci"], call_alleles=True, seed=SEED + 1)
    assert [r["reads"].keys() for r in other["results"]] == [r["reads"].keys() for r in one["results"]]
    drawn = call_sample(t["paths"]["bam"], t["paths"]["ref"], t["paths"]["loci"], call_alleles=True)
    assert isinstance(drawn["parameters"]["seed"], int)


def test_off_by_default_and_consensus_needs_calls(gpu_ctx, tmp_path):
    t = make_dataset(str(tmp_path), n_loci=10, reads_per_locus=10, read_len=2000, seed=8, sub=0.005)
    plain = call_sample(t["paths"]["bam"], t["paths"]["ref"], t["paths"]["loci"])
    off = call_sample(t["paths"]["bam"], t["paths"]["ref"], t["paths"]["loci"], call_alleles=False)
    assert off["results"] == plain["results"] and off["parameters"] == plain["parameters"]
    assert "call_alleles" not in plain["parameters"] and "seed" not in plain["parameters"]
    with pytest.raises(ValueError):
        call_sample(t["paths"]["bam"], t["paths"]["ref"], t["paths"]["loci"], consensus=True)
    # calls without sequences
    rep = _call(t)
    assert all(r["call"] and "seqs" not in r["peaks"] for r in rep["results"])
    assert "consensus" not in rep["parameters"]


def test_vcf_of_the_error_free_data_set(gpu_ctx, tmp_path):
    t = make_dataset(str(tmp_path), n_loci=60, reads_per_locus=12, read_len=2500, seed=11)
    rep = _call(t, consensus=True)
    path = str(tmp_path / "o.vcf")
    assert write_vcf(rep, path, Fasta(t["paths"]["ref"])) == 60
    text = open(path).read().splitlines()
    assert any(l.startswith("##FORMAT=<ID=ANCL,") for l in text) and any(l.startswith("##FORMAT=<ID=CONS,") for l in text)
    recs = [l.split("\t") for l in text if not l.startswith("#")]
    by_id = {r["locus_id"]: (r, tr) for r, tr in zip(rep["results"], t["loci"])}
    n_het = n_homref = 0
    for f in recs:
        row, truth = by_id[f[2]]
        a1, a2 = truth["alleles"]
        if sorted(row["call"]) != sorted((a1, a2)):
            continue
        s = dict(zip(f[8].split(":"), f[9].split(":")))
        ref_allele, alts = f[3], ([] if f[4] == "." else f[4].split(","))
        info = dict(kv.split("=") for kv in f[7].split(";"))
        anchor = ref_allele[:int(info["ANCH"])]
        assert ref_allele == anchor + truth["motif"] * truth["ref_cn"] and int(info["ANCH"]) >= 1
        gt = [int(x) for x in s["GT"].split("/")]
        alleles = [ref_allele, *alts]
        assert [int(x) for x in s["MC"].split(",")] == row["call"]
        assert sum(int(x) for x in s["AD"].split(",")) == int(s["DPS"]) == len(row["reads"]) == int(s["DP"])
        if a1 != a2:
            n_het += 1
            assert gt[0] != gt[1]
            assert [alleles[g] for g in gt] == [anchor + truth["motif"] * c for c in row["call"]]
        else:
            assert gt[0] == gt[1]
        for a in (a1, a2):
            if a != truth["ref_cn"]:
                assert anchor + truth["motif"] * a in alts
        assert len(alts) == len({a for a in (a1, a2) if a != truth["ref_cn"]})
        if a1 == a2 == truth["ref_cn"]:
            n_homref += 1
            assert s["GT"] == "0/0" and f[4] == "." and s["CONS"] == "."
        else:
            assert set(s["CONS"].split(",")) == {"single"}
    assert n_het >= 30      # (the hand-made rows of tests/test_genotype_report.py hold a homozygous-reference locus whatever the draw)
    print(f"heterozygous {n_het}, homozygous reference {n_homref}")
