"""GPU: strk_mi_trio (k_mi_small, k_mi_large) on the corpus of mi_cases.py against the oracle of mi_restatement.py under the
tolerances of DESIGN.md §16, and bit for bit against the host twin strk_mi_trio_host; the two kernels against each other on
loci around the threshold between them; pieces that change nothing; the fixtures of tests/golden/mi from files to report on
the device; a synthetic trio of alignment files through `call` and `mi`."""
import os

import numpy as np
import pytest

import mi_cases as cases
from strkit_amd import mi

pytestmark = pytest.mark.gpu
OUT = ("respects", "p", "config", "mutation_from", "status")


def run(pk, test, device, **kw):
    return mi.mi_trio_batch(pk["gt"], pk["ci95"], pk["grp_off"], pk["cn"], pk["ci99"], pk["seq_id"], pk["seq_len"], test=test,
                            sig_level=cases.SIG, device=device, **kw)


@pytest.fixture(scope="module")
def packed():
    return mi.pack_loci(cases.all_loci()[0])


@pytest.mark.parametrize("test", ("none",) + cases.TESTS)
def test_device_equals_scipy(packed, gpu_ctx, test):
    if test != "none":
        share = cases.lenient_share(test)
        assert max(share.values()) <= cases.MAX_LENIENT_SHARE, share
    got = run(packed, test, "gpu", ctx=gpu_ctx)
    line = cases.compare(got, test)
    host = run(packed, test, "host")
    for k in OUT:      # bit for bit, so that a NaN meets a NaN
        if got[k].tobytes() != host[k].tobytes():
            rows = got[k].reshape(len(got[k]), -1).view(np.uint8) != host[k].reshape(len(host[k]), -1).view(np.uint8)
            bad = int(np.nonzero(rows.any(axis=1))[0][0])
            raise AssertionError((test, k, bad, cases.all_loci()[1][bad], got[k][bad], host[k][bad]))
    if test != "none":
        assert 0 < got["stats"]["n_fallback"] < len(cases.all_loci()[0])      # both kernels ran
    print(line + f"; device = host on every locus; {got['stats']['n_fallback']} loci on k_mi_large, kernels {got['stats']['kernel_ms']:.3f} ms")


def threshold_loci():
    """Trios of threshold - 1, threshold and threshold + 1 reads together, and a small and a large one; the child's second allele
    is the father's 17 copies with a de novo step of +3 (even loci) or -3 (odd loci: what wmw-gt looks for)."""
    rng = np.random.default_rng(256)
    t = mi.small_threshold()
    loci = []
    for k, total in enumerate((t - 1, t, t + 1, t - 1, t, t + 1, 12, 2 * t + 5)):
        sizes = rng.multinomial(total - 6, [1 / 6] * 6) + 1
        alleles = [9, 20 if k % 2 == 0 else 14, 9, 12, 15, 17]
        loci.append(cases.locus([cases._reads(rng, a, n) for a, n in zip(alleles, sizes)], gt=alleles))
        assert sum(len(g) for g in loci[-1]["reads"]) == total
    return loci


@pytest.mark.parametrize("test", cases.TESTS)
def test_both_kernels_agree_at_the_threshold(gpu_ctx, test):
    pk = mi.pack_loci(threshold_loci())
    t = mi.small_threshold()
    sizes = np.diff(pk["grp_off"][::6])
    assert sizes.tolist()[:6] == [t - 1, t, t + 1] * 2
    by_size = run(pk, test, "gpu", ctx=gpu_ctx)
    forced = run(pk, test, "gpu", ctx=gpu_ctx, _force_large=True)
    host = run(pk, test, "host")
    assert by_size["stats"]["n_fallback"] == int((sizes > t).sum()) == 3 and forced["stats"]["n_fallback"] == sizes.size
    for k in OUT:
        assert by_size[k].tobytes() == forced[k].tobytes() == host[k].tobytes(), (test, k, by_size[k], forced[k], host[k])
    assert (by_size["status"] == 0).all() and (by_size["p"] < cases.SIG).sum() >= 2 and (by_size["mutation_from"] > 1).sum() >= 2


def test_pieces_do_not_change_a_byte(packed, gpu_ctx):
    ref = run(packed, "wmw", "gpu", ctx=gpu_ctx)
    for kw in ({"piece_loci": 1}, {"piece_loci": 7}, {"ws_budget": 1 << 16}):
        got = run(packed, "wmw", "gpu", ctx=gpu_ctx, **kw)
        assert got["stats"]["n_sub_batches"] > ref["stats"]["n_sub_batches"]
        for k in OUT:
            assert got[k].tobytes() == ref[k].tobytes(), (kw, k)


GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "mi")


@pytest.mark.parametrize("ext", ["json", "vcf"])
def test_files_to_report_on_the_device(gpu_ctx, ext, capsys):
    """run_mi and the command line over the fixtures of tests/golden/mi with the rule on the device: the report of the host."""
    from strkit_amd.__main__ import main
    files = [os.path.join(GOLDEN, f"{who}.{ext}") for who in ("child", "mother", "father")]
    for test, corr in (("none", "none"), ("x2", "fdr_bh"), ("wmw", "none")):
        trio, dev, res = mi.run_mi(*files, caller="strkit-" + ext, test=test, mt_corr=corr)
        _, host, res_h = mi.run_mi(*files, caller="strkit-" + ext, test=test, mt_corr=corr, device="host")
        assert "stats" in dev and "stats" not in host
        for k in OUT:
            assert dev[k].tobytes() == host[k].tobytes(), (ext, test, k)
        assert mi.report_object(trio, dev, res) == mi.report_object(trio, host, res_h) and res["n_loci_trio_called"] == 5
        assert mi.locus_tsv(trio, dev, res) == mi.locus_tsv(trio, host, res_h)
    assert main(["mi", *files, "--caller", "strkit-" + ext, "--test", "--mt-corr", "fdr_bh"]) == 0
    text = capsys.readouterr().out
    assert text.startswith("chr1\t2000\t2030\tAT\t10|15\t") and text.splitlines()[0].split("\t")[-1] == "pat" and "MI% (±1)" in text


def test_trio_from_alignment_files_through_call_and_mi(gpu_ctx, tmp_path):
    """Three synthetic alignment files over one catalog -> `call --call-alleles` per member -> `mi --test x2`: the genotypes are
    the truth's, the loci with a de novo step fail strict inheritance and are the ones the test rejects, with the parent the
    changed allele came from."""
    from strkit_amd.frontend import call_sample
    from strkit_amd.frontend.call import write_json
    from strkit_amd.frontend.synth_trio import MEMBERS, make_trio_dataset
    t = make_trio_dataset(str(tmp_path), n_loci=8, de_novo=(2, 5), reads_per_haplotype=12, allele_gap=(8, 11), apart=True)
    files = []
    for member in MEMBERS:
        rep = call_sample(t["paths"][member], t["paths"]["ref"], t["paths"]["loci"], call_alleles=True, seed=11)
        files.append(str(tmp_path / (member + ".json")))
        write_json(rep, files[-1])
    trio, out, res = mi.run_mi(*files, test="x2")
    truth = {(L["contig"], L["start"], L["end"], L["motif"]): L for L in t["loci"]}
    assert set(trio.keys) == set(truth) and res["n_loci_trio_called"] == 8 and res["n_loci_skipped_ploidy"] == 0
    rejected = {trio.keys[i] for i in res["output_index"]}
    n_de_novo = 0
    for i, key in enumerate(trio.keys):
        L = truth[key]
        want = sorted(L["child"]) + sorted(L["mother"]) + sorted(L["father"])
        assert trio.loci[i]["gt"] == want, (key, trio.loci[i]["gt"], want)
        strict = bool(out["respects"][i, 0])
        if L["de_novo"] is None:
            assert strict and out["p"][i] > 0.05 and key not in rejected and out["mutation_from"][i] == 0, (key, out["p"][i])
        else:
            n_de_novo += 1
            assert not strict and out["p"][i] < 0.05 and key in rejected, (key, out["p"][i])
            assert mi.FROM_NAMES[int(out["mutation_from"][i])] == ("mat", "pat")[L["de_novo"][0]], (key, L, int(out["mutation_from"][i]))
    assert n_de_novo == 2 and res["mi"]["strict"] == 0.75
