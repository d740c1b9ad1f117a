"""GPU: k-mer counts from files — call_sample(count_kmers=...) on synthetic data sets, against the CPU restatement
(tests/kmers_restatement.py) on the raw tracts of the readable path."""
from collections import Counter

import pytest

import kmers_restatement as R
from strkit_amd.frontend import (Fasta, call_sample, get_read_coords_from_cigar, get_sequence_data_for_locus, load_loci,
                                 read_bam)
from strkit_amd.frontend.call import CallOptions, call_blocks
from strkit_amd.frontend.synth_dataset import make_dataset

pytestmark = pytest.mark.gpu

SEED = 1234


def _call(t, **kw):
    return call_sample(t["paths"]["bam"], t["paths"]["ref"], t["paths"]["loci"], seed=SEED, **kw)


def _noisy(tmp_path):
    return make_dataset(str(tmp_path / "n"), n_loci=30, reads_per_locus=14, read_len=2000, seed=5, sub=0.01, indel=0.015,
                        low_qual=0.01)


def _strip(rows):
    """The rows without any k-mer field."""
    out = []
    for row in rows:
        row = dict(row)
        if row.get("peaks"):
            row["peaks"] = {k: v for k, v in row["peaks"].items() if k != "kmers"}
        if "reads" in row:
            row["reads"] = {nm: {k: v for k, v in r.items() if k != "kmers"} for nm, r in row["reads"].items()}
        out.append(row)
    return out


def _expect(tract: str, k: int) -> dict:
    return {w.decode("ascii"): c for w, c in R.count_dict([tract], k).items()}


def test_read_and_peak_counts_equal_the_restatement(gpu_ctx, tmp_path):
    t = _noisy(tmp_path)
    rep = _call(t, call_alleles=True, count_kmers="both", respect_ref=True)
    assert rep["parameters"]["count_kmers"] == "both"
    assert "kmers_s" in rep["stage_times"] and "kmers_device_s" in rep["stage_times"]
    bam, (block,) = read_bam(t["paths"]["bam"]), load_loci(t["paths"]["loci"])
    n_reads = n_peaks = n_interrupted = 0
    for locus, row in zip(block, rep["results"]):
        k = len(locus.motif)
        raw = {}
        for s in bam.fetch(locus.contig, locus.left_flank_coord, locus.right_flank_coord):
            c = get_read_coords_from_cigar(locus.left_flank_coord, locus.left_coord, locus.right_coord, locus.right_flank_coord, s)
            if c.is_incomplete():
                continue
            raw[s.name] = get_sequence_data_for_locus(s, c, 70).tr_seq
        for nm, r in row["reads"].items():      # every kept read, none left out
            assert "kmers" in r, (row["locus_id"], nm)
            assert list(r["kmers"].items()) == list(_expect(raw[nm], k).items()), (row["locus_id"], nm)
            assert sum(r["kmers"].values()) == max(len(raw[nm]) - k + 1, 0) and "X" not in "".join(r["kmers"])
            n_reads += 1
            n_interrupted += len(r["kmers"]) > k
        if row["call"] is None:                 # uncalled, or nullified: no peak counts
            assert row["peaks"] is None or "kmers" not in row["peaks"]
            continue
        assert len(row["peaks"]["kmers"]) == row["peaks"]["modal_n"]
        for p, got in enumerate(row["peaks"]["kmers"]):
            total = Counter()
            members = [r for r in row["reads"].values() if r["p"] == p]
            for r in members:
                total.update(r["kmers"])
            assert got == dict(total) and list(got) == sorted(got), (row["locus_id"], p)
            assert len(members) == row["peaks"]["n_reads"][p]
            n_peaks += 1
    assert n_reads >= 300 and n_peaks >= 27 and n_interrupted >= 20


def test_error_free_peaks_are_multiples_of_the_allele_sequence(gpu_ctx, tmp_path):
    t = make_dataset(str(tmp_path / "a"), n_loci=60, reads_per_locus=12, read_len=2500, seed=11)
    rep = _call(t, call_alleles=True, consensus=True, count_kmers="peak")
    n = 0
    for row, truth in zip(rep["results"], t["loci"]):
        assert all("kmers" not in r for r in row["reads"].values())      # `peak`: read records carry no counts
        if row["call"] is None:
            continue
        k = len(truth["motif"])
        for p, (seq, method) in enumerate(row["peaks"]["seqs"]):
            if method != "single":
                continue
            one = _expect(seq, k)
            assert row["peaks"]["kmers"][p] == {w: c * row["peaks"]["n_reads"][p] for w, c in one.items()}, (row["locus_id"], p)
            n += 1
    assert n >= 60


def test_device_host_and_readable_paths_agree(gpu_ctx, tmp_path):
    t = _noisy(tmp_path)
    dev = _call(t, call_alleles=True, consensus=True, count_kmers="both", front_end="device")
    host = _call(t, call_alleles=True, consensus=True, count_kmers="both", front_end="host")
    assert dev["stage_times"]["front_end"] == "device" and host["stage_times"]["front_end"] == "host"
    assert dev["results"] == host["results"]
    opts = CallOptions(call_alleles=True, consensus=True, seed=SEED, count_kmers="both")
    rows, _n, _tm = call_blocks(load_loci(t["paths"]["loci"]), read_bam(t["paths"]["bam"]), Fasta(t["paths"]["ref"]), opts, gpu_ctx)
    assert rows == dev["results"]
    assert sum(1 for r in rows if r["call"] and "kmers" in r["peaks"]) >= 27
    # realigned reads: the tracts are those of the substitute alignments
    t2 = make_dataset(str(tmp_path / "r"), n_loci=10, reads_per_locus=8, read_len=2500, seed=2, soft_clip_frac=0.7, expansion=40)
    a = _call(t2, call_alleles=True, count_kmers="both", realign=True, front_end="device")
    b = _call(t2, call_alleles=True, count_kmers="both", realign=True, front_end="host")
    assert a["results"] == b["results"] and any(r.get("realn") for row in a["results"] for r in row["reads"].values())


def test_modes_and_the_run_without_the_option(gpu_ctx, tmp_path):
    t = _noisy(tmp_path)
    plain = _call(t)
    assert "count_kmers" not in plain["parameters"] and "kmers_s" not in plain["stage_times"]
    assert _call(t, count_kmers="none")["results"] == plain["results"]
    # `read` needs no allele calls; the rest of the rows is today's
    for fe in ("device", "host"):
        rd = _call(t, count_kmers="read", front_end=fe)
        assert rd["parameters"]["count_kmers"] == "read" and "call_alleles" not in rd["parameters"]
        assert all("kmers" in r for row in rd["results"] for r in row["reads"].values())
        assert _strip(rd["results"]) == plain["results"]
    rows, _n, _tm = call_blocks(load_loci(t["paths"]["loci"]), read_bam(t["paths"]["bam"]), Fasta(t["paths"]["ref"]),
                                CallOptions(count_kmers="read"), gpu_ctx)
    assert rows == rd["results"]
    # with calls: the rows without the k-mer fields are the rows of a run without the option
    calls = _call(t, call_alleles=True, consensus=True)
    both = _call(t, call_alleles=True, consensus=True, count_kmers="both")
    peak = _call(t, call_alleles=True, consensus=True, count_kmers="peak")
    assert _strip(both["results"]) == calls["results"] == _strip(peak["results"])
    assert all("kmers" not in r for row in peak["results"] for r in row["reads"].values())
    assert [row["peaks"]["kmers"] for row in peak["results"] if row["call"]] == [row["peaks"]["kmers"] for row in both["results"] if row["call"]]
    assert [{nm: r["kmers"] for nm, r in row["reads"].items()} for row in both["results"]] == \
        [{nm: r["kmers"] for nm, r in row["reads"].items()} for row in rd["results"]]
    with pytest.raises(ValueError):
        _call(t, count_kmers="peak")


def test_counts_do_not_depend_on_the_blocks(gpu_ctx, tmp_path):
    t = _noisy(tmp_path)
    one = _call(t, call_alleles=True, count_kmers="both")
    four = _call(t, call_alleles=True, count_kmers="both", processes=4)
    assert four["results"] == one["results"]
    assert _call(t, call_alleles=True, count_kmers="both")["results"] == one["results"]
