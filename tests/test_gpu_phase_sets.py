"""GPU: phase sets across loci for SNV calls end to end (frontend/phase_sets.py): `call` with
snv_phase_sets on the data set of frontend/synth_linked.py, 15 loci x 24 reads of 2 - 4 kb on two contigs; the device reader, the
host reader and the readable block path, blocks of one locus, the VCF and `mi --only-phased`.  Every run is made once per module."""
import pytest

from strkit_amd import mi
from strkit_amd.frontend import Fasta, call_sample, load_loci, read_bam
from strkit_amd.frontend.call import call_blocks
from strkit_amd.frontend.options import PhaseSetCallOptions
from strkit_amd.frontend.output import write_vcf
from strkit_amd.frontend.synth_linked import make_linked_dataset

pytestmark = pytest.mark.gpu

SEED = 4321
LINKED = ("chain", "equal", "bridge")
TAIL = {"consensus": True, "count_kmers": "peak"}


@pytest.fixture(scope="module")
def data(tmp_path_factory):
    return make_linked_dataset(str(tmp_path_factory.mktemp("linked")))


@pytest.fixture(scope="module")
def tagged(tmp_path_factory):
    return make_linked_dataset(str(tmp_path_factory.mktemp("linked_tags")), tags="conflict")


def _call(t, **kw):
    return call_sample(t["paths"]["bam"], t["paths"]["ref"], t["paths"]["loci"], call_alleles=True, seed=SEED, **kw)


@pytest.fixture(scope="module")
def off(gpu_ctx, data):
    return _call(data, snv_vcf=data["paths"]["snvs"], front_end="device", **TAIL)


@pytest.fixture(scope="module")
def on(gpu_ctx, data):
    return _call(data, snv_vcf=data["paths"]["snvs"], snv_phase_sets=True, front_end="device", **TAIL)


@pytest.fixture(scope="module")
def plain(gpu_ctx, data):
    return _call(data, front_end="device", **TAIL)


def _orientation(row, t):
    """False: peak label = truth haplotype for every read of the row; True: the other way round for every read; else None."""
    got = [r["p"] for r in row["reads"].values()]
    want = [t["read_hap"][name] for name in row["reads"]]
    return False if got == want else True if got == [1 - h for h in want] else None


def _by_id(rep):
    return {r["locus_id"]: r for r in rep["results"]}


def test_precondition_without_the_switch(data, off):
    """The data set is made so that this holds whatever its seed is: every linked locus has a site that all its reads cover, and
    in the chain the haplotype with the smaller allele (peak 0 of a call ordered by mean) alternates."""
    assert "snv_phase_sets" not in off["parameters"] and "phase_sets_s" not in off["stage_times"]
    rows = _by_id(off)
    for truth in data["loci"]:
        row = rows[truth["id"]]
        assert "ps" not in row and all("ps" not in r for r in row["reads"].values())
        if truth["region"] in LINKED:
            assert row["assign_method"] in ("snv", "snv+dist"), (truth["id"], row["assign_method"])
            assert _orientation(row, data) is not None, truth["id"]
    chain = [_orientation(rows[f"chain{i}"], data) for i in range(5)]
    assert len(set(chain)) == 2, chain


def test_linked_rows_get_a_phase_set_and_agree_with_the_truth_up_to_one_swap_per_set(data, on, off):
    assert on["parameters"]["snv_phase_sets"] is True and on["stage_times"]["phase_sets_s"] >= 0
    rows, before = _by_id(on), _by_id(off)
    per_set: dict = {}
    flipped = 0
    for truth in data["loci"]:
        if truth["region"] not in LINKED:
            continue
        row = rows[truth["id"]]
        assert row["assign_method"] in ("snv", "snv+dist") and isinstance(row.get("ps"), int), truth["id"]
        assert all(r["ps"] == row["ps"] for r in row["reads"].values() if r.get("p") is not None), truth["id"]
        o = _orientation(row, data)
        assert o is not None, truth["id"]
        per_set.setdefault((row["contig"], row["ps"]), set()).add(o)
        for s in row["snvs"]:       # the SNV calls follow the peaks: haplotype 1 carries the ALT base at every site
            assert s["call"][1 if not o else 0] != s["ref"] and s["call"][0 if not o else 1] == s["ref"], (truth["id"], s)
        for name, r in row["reads"].items():
            assert r["snvu"] == [s["call"][r["p"]] for s in row["snvs"]], (truth["id"], name)
        if o != _orientation(before[truth["id"]], data):
            flipped += 1
            if truth["region"] == "chain":      # ordered by mean before, so turned over it descends
                assert row["call"][0] > row["call"][1], (truth["id"], row["call"])
                assert row["call"] == before[truth["id"]]["call"][::-1]
        else:
            assert row["call"] == before[truth["id"]]["call"]
    assert all(len(v) == 1 for v in per_set.values()), per_set
    assert flipped >= 1 and len(per_set) < sum(t["region"] in LINKED for t in data["loci"])
    assert any(row["call"][0] > row["call"][1] for row in (rows[f"chain{i}"] for i in range(5)))


def test_consensus_and_kmers_follow_the_flipped_peaks(data, on):
    for truth, row in zip(data["loci"], on["results"]):
        if truth["region"] not in LINKED:
            continue
        k = len(row["motif"])
        labels = [r["p"] for r in row["reads"].values()]
        for i in (0, 1):
            assert len(row["peaks"]["seqs"][i][0]) == row["call"][i] * k, (truth["id"], i)
            assert row["peaks"]["n_reads"][i] == labels.count(i), (truth["id"], i)
            assert sum(row["peaks"]["kmers"][i].values()) == labels.count(i) * (row["call"][i] * k - k + 1), (truth["id"], i)
            assert round(row["peaks"]["means"][i]) == row["call"][i], (truth["id"], i)
        o = _orientation(row, data)
        assert (row["call"][::-1] if o else row["call"]) == list(truth["alleles"]), truth["id"]


def test_the_bridge_locus_joins_the_sets_of_its_two_neighbours(on):
    rows = _by_id(on)
    a, b, c = (rows["bridge" + x] for x in "ABC")
    assert a["ps"] == b["ps"] == c["ps"]
    assert [s["id"] for s in a["snvs"]] == ["bridge_s1"] and [s["id"] for s in b["snvs"]] == ["bridge_s2"]
    assert [s["id"] for s in c["snvs"]] == ["bridge_s1", "bridge_s2"]


def test_the_conflict_locus_is_demoted_to_the_plain_call(on, plain):
    b, want = _by_id(on)["conflictB"], _by_id(plain)["conflictB"]
    assert want["assign_method"] in ("dist", "single")
    for key in ("call", "call_95_cis", "call_99_cis", "peaks", "assign_method", "reads"):
        assert b[key] == want[key], key
    assert "snvs" not in b and "ps" not in b and all("snvu" not in r and "ps" not in r for r in b["reads"].values())
    a = _by_id(on)["conflictA"]
    assert [s["id"] for s in a["snvs"]] == ["conflict_s"] and isinstance(a["ps"], int)


def test_tags_on_one_region_hp_and_snv_numbers_are_distinct_and_ascend(gpu_ctx, tagged):
    rep = _call(tagged, use_hp=True, snv_vcf=tagged["paths"]["snvs"], snv_phase_sets=True, front_end="device")
    order, hp_sets, snv_sets = [], set(), set()
    for row in rep["results"]:
        for r in row["reads"].values():
            if "ps" in r and r["ps"] not in order:
                order.append(r["ps"])
        assert row.get("ps") is not None, row["locus_id"]
        if row["ps"] not in order:
            order.append(row["ps"])
        assert (row["assign_method"] == "hp") == row["locus_id"].startswith("conflict"), (row["locus_id"], row["assign_method"])
        (hp_sets if row["assign_method"] == "hp" else snv_sets).add(row["ps"])
    assert order == list(range(1, len(order) + 1)), order
    assert len(hp_sets) == 1 and not hp_sets & snv_sets
    ids = _by_id(rep)
    assert ids["chain0"]["ps"] == 1 and ids["chain4"]["ps"] < ids["conflictA"]["ps"] < ids["bridgeA"]["ps"] < ids["equal0"]["ps"]


def test_device_host_and_readable_paths_and_blocks_of_one_locus_give_equal_rows(gpu_ctx, data, on):
    kw = dict(snv_vcf=data["paths"]["snvs"], snv_phase_sets=True, **TAIL)
    host = _call(data, front_end="host", **kw)
    assert on["stage_times"]["front_end"] == "device" and host["stage_times"]["front_end"] == "host"
    assert host["results"] == on["results"]
    opts = PhaseSetCallOptions(call_alleles=True, seed=SEED, **kw)
    bam, ref = read_bam(data["paths"]["bam"]), Fasta(data["paths"]["ref"])
    rows, _n, tm = call_blocks(load_loci(data["paths"]["loci"]), bam, ref, opts, gpu_ctx)
    assert rows == on["results"] and "phase_sets_s" in tm
    single = load_loci(data["paths"]["loci"], max_block_size=1)
    assert all(len(b) == 1 for b in single)
    rows, _n, _tm = call_blocks(single, bam, ref, opts, gpu_ctx)
    assert rows == on["results"]


def _vcf_records(path):
    return [ln.split("\t") for ln in open(path).read().split("\n") if ln and not ln.startswith("#")]


def test_the_vcf_has_phased_str_records_and_snv_records_of_one_orientation_per_set(data, on, off, tmp_path):
    path = str(tmp_path / "on.vcf")
    n = write_vcf(on, path, Fasta(data["paths"]["ref"]))
    body = _vcf_records(path)
    assert n == len(body)
    rows = _by_id(on)
    strs = [f for f in body if f[7].startswith("VT=str")]
    snvs = [f for f in body if f[7] == "VT=snv"]
    assert len(strs) == 15 and len(strs) + len(snvs) == len(body)
    for f in strs:
        rec, row = dict(zip(f[8].split(":"), f[9].split(":"))), rows[f[2]]
        if "ps" in row:
            assert rec["PS"] == str(row["ps"]) and "|" in rec["GT"] and "/" not in rec["GT"], f[2]
        else:
            assert "PS" not in rec and "/" in rec["GT"], f[2]
    want_ids = {(r["contig"], s["id"]) for r in on["results"] for s in r.get("snvs") or []}
    assert sorted((f[0], f[2]) for f in snvs) == sorted(want_ids)            # once per id
    for contig in ("chr1", "chr2"):
        pos = [int(f[1]) for f in body if f[0] == contig]
        assert pos == sorted(pos) and len(pos) > 5
    sides: dict = {}
    for f in snvs:
        rec = dict(zip(f[8].split(":"), f[9].split(":")))
        # (bridge_s2 is written by bridgeB, whose reads are its own 24 and the 24 of bridgeC that span it)
        assert f[8] == "GT:DP:AD:PS" and (rec["DP"], rec["AD"]) in (("24", "12,12"), ("48", "24,24")), f
        assert int(f[1]) - 1 == data["sites"][f[0]][f[2]] and rec["GT"] in ("0|1", "1|0")
        sides.setdefault((f[0], rec["PS"]), set()).add(rec["GT"])
    assert all(len(v) == 1 for v in sides.values()), sides
    # without the switch: no SNV record, no PS
    path = str(tmp_path / "off.vcf")
    write_vcf(off, path, Fasta(data["paths"]["ref"]))
    text = open(path).read()
    assert "VT=snv" not in text and "ID=PS," not in text


def test_mi_only_phased_keeps_the_snv_phased_loci(data, on, off, tmp_path):
    ref = Fasta(data["paths"]["ref"])
    paths = []
    for name in ("child", "mother", "father"):
        paths.append(str(tmp_path / f"{name}.vcf"))
        write_vcf(on, paths[-1], ref, sample_id=name)
    trio, _out, res = mi.run_mi(*paths, caller="strkit-vcf", only_phased=True)
    want = {(r["contig"], r["start"], r["end"], r["motif"]) for r in on["results"] if "ps" in r}
    assert res is not None and set(trio.keys) == want and len(want) == 14
    path = str(tmp_path / "off.vcf")
    write_vcf(off, path, ref)
    trio, _out, _res = mi.run_mi(path, path, path, caller="strkit-vcf", only_phased=True)
    assert not trio.keys
