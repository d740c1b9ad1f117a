"""The VCF writer on hand-made rows that carry calls, peaks and allele sequences (output/vcf.py:202-342), and the front end's
locus seed."""
import json
import os

import alleles_restatement as AR
from strkit_amd.alleles import locus_seed, locus_seeds
from strkit_amd.frontend.output import write_vcf

HERE = os.path.dirname(os.path.abspath(__file__))


def _row(idx=0, start=1000, ref_cn=4, motif="CAG", anchor="ACGTA", call=None, seqs=None, anchors=None, modal_n=None, n_reads=None,
         reads=None, **extra):
    row = {"locus_index": idx, "locus_id": f"locus{idx}", "contig": "chr1", "start": start, "end": start + ref_cn * len(motif),
           "motif": motif, "annotations": [], "assign_method": None, "call": None, "call_95_cis": None, "call_99_cis": None,
           "ref_cn": ref_cn, "start_adj": start, "end_adj": start + ref_cn * len(motif), "ref_start_anchor": anchor,
           "ref_seq": motif * ref_cn, "peaks": None, "read_peaks_called": False, "reads": reads or {}}
    if call is not None:
        modal_n = modal_n if modal_n is not None else len(set(call))
        row.update(assign_method="dist", call=list(call), call_95_cis=[[c, c] for c in call], call_99_cis=[[c - 1, c + 1] for c in call],
                   read_peaks_called=True, mean_model_align_score=1.5,
                   peaks={"means": [float(c) for c in call[:modal_n]], "weights": [1.0 / modal_n] * modal_n,
                          "stdevs": [0.1] * modal_n, "modal_n": modal_n, "n_reads": n_reads or [3] * modal_n})
        if seqs is not None:
            row["peaks"]["seqs"] = [[s, m] for s, m in seqs]
            row["peaks"]["start_anchor_seqs"] = [[a, "single"] for a in (anchors or [anchor] * len(seqs))]
    row.update(extra)
    return row


def _reads(per_peak):
    """per_peak: list of lists of (cn, sl)."""
    out = {}
    for p, lst in enumerate(per_peak):
        for k, (cn, sl) in enumerate(lst):
            out[f"r{p}_{k}"] = {"s": "+", "cn": cn, "w": 1.0, "sc": 1.5, "sl": sl, "p": p}
    return out


def _write(tmp_path, rows, **kw):
    path = str(tmp_path / "o.vcf")
    n = write_vcf({"results": rows, "sample_id": "s"}, path, date="20261016", **kw)
    lines = open(path).read().splitlines()
    recs = [l.split("\t") for l in lines if not l.startswith("#")]
    return n, [l for l in lines if l.startswith("#")], recs


def _sample(f):
    return dict(zip(f[8].split(":"), f[9].split(":")))


def test_alleles_genotype_and_anchor_cut(tmp_path):
    reads = _reads([[(4, 12), (4, 12), (3, 10)], [(6, 18), (6, 18)]])
    row = _row(call=[4, 6], seqs=[("CAG" * 4, "single"), ("CAG" * 6, "best_rep")], n_reads=[3, 2], reads=reads)
    n, header, (f,) = _write(tmp_path, [row])
    assert n == 1
    # all anchors are ACGTA: four bases are cut, one stays
    assert f[1] == str(1000 - 1 + 1) and f[3] == "A" + "CAG" * 4 and f[4] == "A" + "CAG" * 6
    assert "ANCH=1" in f[7].split(";")
    s = _sample(f)
    assert f[8] == "GT:DP:PM:MMAS:DPS:AD:MC:MCCI:ANCL:CONS:MCRL:SLR"
    assert s["GT"] == "0/1" and s["DP"] == "5" and s["PM"] == "dist" and s["MMAS"] == "1.5" and s["DPS"] == "5" and s["AD"] == "3,2"
    assert s["MC"] == "4,6" and s["MCCI"] == "4-4,6-6" and s["ANCL"] == "1,1" and s["CONS"] == "best_rep"
    assert s["MCRL"] == "3x1|4x2,6x2" and s["SLR"] == "10x1|12x2,18x2"
    assert any(h.startswith("##FORMAT=<ID=ANCL,Number=.,Type=Integer") for h in header)
    assert any(h.startswith("##FORMAT=<ID=CONS,Number=.,Type=String") for h in header)
    ids = [h.split("ID=")[1].split(",")[0] for h in header if h.startswith("##FORMAT")]
    assert ids == sorted(ids)


def test_anchor_prefix_is_cut_only_as_far_as_it_is_shared(tmp_path):
    # the second allele's anchor differs at its fourth base: three bases are shared and cut
    row = _row(call=[5, 7], seqs=[("CAG" * 5, "single"), ("CAG" * 7, "single")], anchors=["ACGTA", "ACGCA"])
    _, _, (f,) = _write(tmp_path, [row])
    assert f[1] == str(1000 - 2 + 1) and f[3] == "TA" + "CAG" * 4
    assert f[4].split(",") == sorted(["TA" + "CAG" * 5, "CA" + "CAG" * 7]) and "ANCH=2" in f[7].split(";")
    s = _sample(f)
    assert s["GT"] == "2/1" and s["ANCL"] == "2,2,2" and s["CONS"] == "single,single"
    # lower case in the report is folded, as the reference does
    row = _row(call=[4, 5], seqs=[("cag" * 4, "single"), ("cag" * 5, "single")], anchors=["acgta", "acgta"])
    _, _, (f,) = _write(tmp_path, [row])
    assert f[3] == "A" + "CAG" * 4 and f[4] == "A" + "CAG" * 5 and _sample(f)["GT"] == "0/1"


def test_upstream_deletion_allele(tmp_path):
    # one allele lost the tract and its anchor: nothing is shared, nothing is cut, the allele is written as *
    row = _row(call=[0, 4], seqs=[("", "single"), ("CAG" * 4, "single")], anchors=["", "ACGTA"])
    _, _, (f,) = _write(tmp_path, [row])
    assert f[3] == "ACGTA" + "CAG" * 4 and f[4] == "*" and f[1] == str(1000 - 5 + 1)
    s = _sample(f)
    assert s["GT"] == "1/0" and s["ANCL"] == "5,0" and "ANCH=5" in f[7].split(";")


def test_one_sequence_is_repeated_for_one_peak_of_a_diploid(tmp_path):
    reads = _reads([[(6, 18)] * 4])
    row = _row(call=[6, 6], modal_n=1, seqs=[("CAG" * 6, "single")], n_reads=[4], reads=reads)
    _, _, (f,) = _write(tmp_path, [row])
    s = _sample(f)
    assert s["GT"] == "1/1" and f[4] == "A" + "CAG" * 6 and s["AD"] == "4" and s["MCRL"] == "6x4" and s["SLR"] == "18x4"
    # homozygous reference
    row = _row(call=[4, 4], modal_n=1, seqs=[("CAG" * 4, "single")], n_reads=[4], reads=_reads([[(4, 12)] * 4]))
    _, _, (f,) = _write(tmp_path, [row])
    assert _sample(f)["GT"] == "0/0" and f[4] == "." and _sample(f)["CONS"] == "." and _sample(f)["ANCL"] == "1"
    # one allele per locus
    row = _row(call=[5], modal_n=1, seqs=[("CAG" * 5, "single")], n_reads=[4])
    _, _, (f,) = _write(tmp_path, [row], n_alleles=1)
    assert _sample(f)["GT"] == "1"
    _, _, (f,) = _write(tmp_path, [row], n_alleles={"chr1": 1})
    assert _sample(f)["GT"] == "1"


def test_a_missing_sequence_skips_the_record(tmp_path):
    good = _row(0, call=[4, 6], seqs=[("CAG" * 4, "single"), ("CAG" * 6, "single")])
    bad = _row(1, start=5000, call=[4, 6], seqs=[("CAG" * 4, "single"), (None, "none")])
    n, _, recs = _write(tmp_path, [good, bad])
    assert n == 1 and [f[2] for f in recs] == ["locus0"]
    bad = _row(1, start=5000, call=[4, 6], seqs=[("CAG" * 4, "single"), ("CAG" * 6, "single")])
    bad["peaks"]["start_anchor_seqs"][1][0] = None
    assert _write(tmp_path, [good, bad])[0] == 1


def test_calls_without_sequences_and_rows_without_peaks(tmp_path):
    reads = _reads([[(4, 12)] * 2, [(6, 18)] * 3])
    row = _row(call=[4, 6], n_reads=[2, 3], reads=reads)
    _, header, (f,) = _write(tmp_path, [row])
    assert f[8] == "GT:DP:PM:MMAS:DPS:AD:MC:MCCI:MCRL:SLR" and f[4] == "." and f[3] == "ACGTA" + "CAG" * 4
    s = _sample(f)
    assert s["GT"] == "./." and s["AD"] == "2,3" and s["DPS"] == "5" and s["MCCI"] == "4-4,6-6" and s["MMAS"] == "1.5"
    assert not any("ID=ANCL" in h or "ID=CONS" in h for h in header)
    # a call but no peaks record: exactly the fields of a report that never had them
    row2 = dict(row, peaks=None)
    _, _, (f,) = _write(tmp_path, [row2])
    assert f[8] == "GT:DP:PM:MC:MCRL:SLR" and _sample(f)["MCRL"] == "4x2,6x3"
    del row2["peaks"]
    _, _, (f2,) = _write(tmp_path, [row2])
    assert f2 == f


def test_a_report_without_calls_is_written_as_before(tmp_path):
    """The golden rows (no calls) give the golden VCF, header included; only the contig lines need the reference file."""
    gold = json.load(open(os.path.join(HERE, "golden", "report_rows.json")))
    path = str(tmp_path / "g.vcf")
    write_vcf({"results": gold["results"], "sample_id": "golden"}, path, date="20261004")
    ours = open(path).read().splitlines()
    theirs = [l for l in open(os.path.join(HERE, "golden", "report.vcf")).read().splitlines() if not l.startswith("##contig")]
    assert ours == theirs and not any("ANCL" in l or "CONS" in l for l in ours)


def test_locus_seed_is_the_restatements():
    import numpy as np
    idx = np.array([0, 1, 2, 77, 10 ** 6, 2 ** 31 - 1])
    for seed in (0, 1, 1234, 2 ** 63 + 11, 2 ** 64 - 1):
        exp = [AR.locus_seed(seed, int(i)) for i in idx]
        assert [locus_seed(seed, int(i)) for i in idx] == exp
        assert locus_seeds(seed, idx).tolist() == exp
