"""CPU: the call fields of the rows that the ranks of a torch.distributed run exchange (frontend/gather.py): the codec
on hand-made rows that hold every state a row can be in, the run-wide numbering of the phase sets, two ranks over gloo, and what
`call_sample` still refuses there."""
import copy
import json
import random

import numpy as np
import pytest

from helpers import FakeRef, fake_rows, gloo_blocks
from strkit_amd.frontend import call as call_mod
from strkit_amd.frontend.call import CallOptions, _locus_dict, _locus_row, deal_locus_blocks
from strkit_amd.frontend.gather import _NAME_BYTES, _decode_rows, _decode_shares, _encode_calls, _encode_rows, renumber_phase_sets
from strkit_amd.frontend.phase_inputs import PhaseSetRemap

SET_A, SET_B, SET_C = 70007, 50000, 60000          # original PS values, met in this order
LONG_KMER = "CAGCAGCAGCATCAGCAGCAGCAGCAGCAGCAGCAGCAG"      # 39 bytes
LONG_SEQ = "ACGGT" * 1000                          # 5 000 bytes
N_KINDS = 12


def _reads(t_idx, n, sc_none=False, long_name=False):
    return {f"r{t_idx}_{k}" + ("n" * (_NAME_BYTES + 9) if long_name and k == 1 else ""):
            {"s": "+-"[k % 2], "cn": 10 + (k % 3), "w": 1.0 / n, "sc": None if sc_none or k == 1 else 0.75 + 0.03125 * k, "sl": 30 + k,
             **({"realn": True} if k == 2 else {}), **({"chimeric_in_region": True} if k == 3 else {})} for k in range(n)}


def _called(row, method, call, cis, modal_n, n_reads, score=0.875):
    """What genotype_row leaves on a called row, keys in its order."""
    k = min(modal_n, len(call))
    row.update({"assign_method": method, "call": call, "call_95_cis": cis, "call_99_cis": [[a - 1, b + 1] for a, b in cis],
                "peaks": {"means": [c + 0.25 for c in call[:k]], "weights": [1.0 / k] * k, "stdevs": [0.5, float("nan"), 0.125][:k] + [0.0] * (k - 3),
                          "modal_n": modal_n, "n_reads": n_reads}})
    row["mean_model_align_score"] = score


def _tag(reads, ps, skip=()):
    """HP / PS on the reads as phase_row writes them (the original PS value: _number turns them into numbers); `skip`: untagged."""
    for k, r in enumerate(reads.values()):
        if k not in skip:
            r["hp"], r["ps"] = 1 + k % 2, ps


def call_rows(mine, ref, kinds):
    """Rows of the shapes `call` builds with call_alleles, consensus, count_kmers, use_hp and snv_vcf (ps = ORIGINAL values),
    one state per locus by `kinds[t_idx]`: (rows, reads, stage times with the failed loci)."""
    rows, errors = [], []
    for blk in mine:
        for l in blk:
            kind = kinds[l.t_idx]
            if kind == 0:
                rows.append(_locus_dict(l))                                    # skipped: no reference data
                continue
            if kind == 1:
                errors.append({"locus_index": l.t_idx, "error": "boom"})       # failed
                continue
            rd = {"ref_cn": 7, "left_coord_adj": l.left_coord - 1, "right_coord_adj": l.right_coord, "ref_seq": ref.fetch(l.contig, l.left_coord - 1, l.right_coord),
                  "ref_left_flank_seq": ref.fetch(l.contig, l.left_coord - 6, l.left_coord - 1)}
            reads = _reads(l.t_idx, 2 if kind == 2 else 6, sc_none=kind == 4, long_name=kind == 7)
            row = _locus_row(l, rd, reads, CallOptions())
            recs = list(reads.values())
            if kind == 2:          # too few reads: no call field on the row; a tagged read and per-read k-mers all the same
                _tag(reads, SET_B, skip=(1,))
                recs[0]["kmers"], recs[1]["kmers"] = {"CAG": 4, "AGC": 3}, {}
            elif kind == 3:        # a call with an empty peak is nullified: its reads keep their labels
                for k, r in enumerate(recs):
                    r["p"] = k % 2
                row["read_peaks_called"] = True
                row["mean_model_align_score"] = 0.8125
            elif kind in (4, 5):   # three peaks of six alleles: no read is labelled; n_reads None (4) or empty (5), no score (4)
                _called(row, "dist", [9, 9, 10, 10, 12, 12], [[8, 10]] * 4 + [[11, 13]] * 2, 3, None if kind == 4 else [], None if kind == 4 else 0.5)
            elif kind == 6:        # one allele
                for r in recs:
                    r["p"] = 0
                _called(row, "single", [10], [[10, 11]], 1, [6])
                row["read_peaks_called"] = True
                row["peaks"]["seqs"], row["peaks"]["start_anchor_seqs"] = [["CAG" * 10, "single"]], [["ACGTA", "single"]]
            elif kind == 7:        # two alleles; every method; sequences of 0 and 5 000 bytes; k-mers per read and per peak
                for k, r in enumerate(recs):
                    r["p"] = -1 if k == 5 else k % 2
                    r["kmers"] = {} if k == 4 else {"GCA": 1 + k, "CAG": 9, LONG_KMER: 1, "AGC": 2}
                _called(row, "dist", [10, 11], [[10, 10], [11, 12]], 2, [3, 2])
                row["read_peaks_called"] = True
                row["peaks"]["seqs"], row["peaks"]["start_anchor_seqs"] = [["", "best_rep"], [LONG_SEQ, "poa"]], [[None, "none"], ["ACGT", "single"]]
                row["peaks"]["kmers"] = [{}, {LONG_KMER: 3, "CAG": 2}]
            elif kind in (8, 10, 11):      # called by haplotags; sets A, B, A again over the catalog; an untagged read between tagged
                for k, r in enumerate(recs):
                    r["p"] = k % 2
                _tag(reads, {8: SET_A, 10: SET_B, 11: SET_C}[kind], skip=(2,))
                if kind == 10:     # a read with HP and no PS, and one of another set
                    recs[3]["ps"], recs[4]["ps"] = -1, SET_A
                _called(row, "hp", [10, 12], [[10, 10], [12, 12]], 2, [3, 3])
                row["read_peaks_called"] = True
                row["ps"] = recs[0]["ps"]
            elif kind == 9:        # called by SNVs: an SNV with and one without an id of its own, a read without a base
                for k, r in enumerate(recs):
                    r["p"] = k % 2
                _tag(reads, SET_A, skip=(0, 5))
                for k, r in enumerate(recs):
                    r["snvu"] = ["-", "-"] if k == 3 else ["AG"[k % 2], "CT"[k % 2]]
                _called(row, "snv+dist" if l.t_idx % 2 else "snv", [10, 12], [[10, 10], [12, 12]], 2, [3, 3])
                row["read_peaks_called"] = True
                row["snvs"] = [{"id": "rs4242", "ref": "A", "pos": l.left_coord - 300, "call": ["A", "G"], "rcs": [3, 2]},
                               {"id": f"{l.contig}_{l.right_coord + 412}", "ref": "C", "pos": l.right_coord + 411, "call": ["C", "T"], "rcs": [2, 3]}]
            rows.append(row)
    return rows, sum(len(r.get("reads") or {}) for r in rows), {"count_s": 0.1, "errors": errors}


def _kinds(blocks, offset=0):
    return {l.t_idx: (j + offset) % N_KINDS for j, l in enumerate(l for blk in blocks for l in blk)}


def _number(rows):
    """What one process's PhaseSetRemap makes of the original values, rows and reads in the order given; returns
    {number: original value}."""
    remap = PhaseSetRemap()
    for row in rows:
        recs = list((row.get("reads") or {}).values())
        hp = np.array([r.get("hp", -1) for r in recs], np.int32)
        ps = np.array([r.get("ps", -1) for r in recs], np.int32)
        for r, n in zip(recs, remap(ps, hp).tolist()):
            if "ps" in r:
                r["ps"] = n
        if "ps" in row:
            row["ps"] = remap._ids[row["ps"]]
    return remap.originals()


def _want(blocks, ref, kinds):
    rows, n, tm = call_rows(blocks, ref, kinds)
    rows.sort(key=lambda r: r["locus_index"])
    _number(rows)
    return rows, n, tm


def _through_codec(blocks, ref, shares):
    """Each share (rows, errors) numbered and encoded on its own, then decoded together, with no process group."""
    row_t, call_t = [], []
    for rows, errors in shares:
        rows = copy.deepcopy(rows)
        ids = _number(rows)
        row_t.append(_encode_rows(rows, errors))
        call_t.append(_encode_calls(rows, ids))
    return _decode_shares({l.t_idx: l for blk in blocks for l in blk}, ref, False, row_t, call_t)


def test_every_state_survives_the_codec_shuffled_and_as_two_shares():
    blocks, ref = gloo_blocks(), FakeRef()
    kinds = _kinds(blocks)
    assert set(kinds.values()) == set(range(N_KINDS))
    want, _n, tm = _want(blocks, ref, kinds)
    rows, _n, _tm = call_rows(blocks, ref, kinds)
    shuffled = list(rows)
    random.Random(5).shuffle(shuffled)
    # (a shuffled share numbers its phase sets in ITS order: the numbers come out right only through the original values)
    got, errors = _through_codec(blocks, ref, [(shuffled, tm["errors"])])
    assert json.dumps(got) == json.dumps(want)
    assert [e["locus_index"] for e in errors] == sorted(e["locus_index"] for e in tm["errors"]) != []
    # two shares: one holds the long name and the 5 000-byte sequence, the other neither, so widths and heaps differ
    heavy = [r for r in rows if kinds[r["locus_index"]] == 7]
    light = [r for r in reversed(rows) if kinds[r["locus_index"]] != 7]
    a, b = _encode_rows(heavy, []), _encode_rows(light, [])
    assert a[2].shape[1] > b[2].shape[1] == _NAME_BYTES
    assert len(_encode_calls(heavy)["heap"]) > 5000 > len(_encode_calls(light)["heap"]) > 0
    got, _errors = _through_codec(blocks, ref, [(light, tm["errors"]), (heavy, [])])
    assert json.dumps(got) == json.dumps(want)
    states = json.dumps(want)
    for text in ('"peaks": null', '"n_reads": null', '"n_reads": []', '[null, "none"]', '"mean_model_align_score": null', '"kmers": {}',
                 '"read_peaks_called": true', '"snvu": ["-", "-"]', '["", "best_rep"]', '"poa"', '"single"', "chr1_", LONG_KMER):
        assert text in states, text


def test_rows_without_call_fields_come_back_as_before():
    blocks, ref = gloo_blocks(), FakeRef()
    rows, _n, tm = fake_rows(blocks, ref)
    by_index = {l.t_idx: l for blk in blocks for l in blk}
    tables = _encode_rows(rows, tm["errors"])
    calls = _encode_calls(rows)
    assert all(len(t) == 0 for t in calls.values())
    old = _decode_rows(by_index, ref, False, *tables)
    new = _decode_shares(by_index, ref, False, [tables], [calls])
    assert json.dumps(new) == json.dumps(old) and new[0] == sorted(rows, key=lambda r: r["locus_index"])
    assert _decode_shares(by_index, ref, False, [tables]) == old


def test_phase_sets_are_numbered_as_one_process_numbers_them():
    blocks, ref = gloo_blocks(), FakeRef()
    kinds = {l.t_idx: (8, 10, 8, 11, 2, 9, 10)[j % 7] for j, l in enumerate(l for blk in blocks for l in blk)}     # A B A C B A B ...
    want, _n, _tm = _want(blocks, ref, kinds)
    rows, _n, _tm = call_rows(blocks, ref, kinds)
    first, second = rows[1::2], rows[0::2]              # set A is met first by the share that comes SECOND
    assert kinds[second[0]["locus_index"]] == 8 and kinds[first[0]["locus_index"]] == 10
    for shares in ([(first, []), (second, [])], [(second, []), (first, [])]):
        got, _errors = _through_codec(blocks, ref, shares)
        assert json.dumps(got) == json.dumps(want)
    numbers = [r["ps"] for row in want for r in row["reads"].values() if "ps" in r]
    assert numbers[0] == 1 and max(numbers) == 4 and sorted(set(numbers)) == [1, 2, 3, 4]      # A, B, -1 (HP alone), C
    assert any("hp" in r and "hp" not in nxt for row in want for r, nxt in zip(row["reads"].values(), list(row["reads"].values())[1:]))
    # numbers a share made stand for nothing without its table: taken as values, they still come out in order of appearance
    plain = copy.deepcopy(want)
    renumber_phase_sets(plain)
    assert json.dumps(plain) == json.dumps(want)


def _gloo_worker(rank, world, port, q, n_blocks):
    import torch.distributed as dist
    from strkit_amd.frontend.call import call_blocks_sharded
    dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{port}", rank=rank, world_size=world)
    ref, blocks = FakeRef(), gloo_blocks()[:n_blocks]
    kinds = _kinds(gloo_blocks(), offset=8 if n_blocks == 1 else 0)

    def fake_call(mine):
        rows, n, tm = call_rows(mine, ref, kinds)
        return rows, n, {**tm, "ps_ids": _number(rows), "alleles_s": 0.25 * (rank + 1)}

    merged, n, tm = call_blocks_sharded(blocks, fake_call, ref)
    q.put((rank, json.dumps(merged), n, tm))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("n_blocks", [11, 1])
def test_two_ranks_end_with_the_rows_of_one_process(n_blocks):
    """world_size-2 gloo over the hand-made rows (11 blocks, and one block: the second rank then gathers empty tables)."""
    import socket

    import torch.multiprocessing as mp
    blocks, ref = gloo_blocks()[:n_blocks], FakeRef()
    kinds = _kinds(gloo_blocks(), offset=8 if n_blocks == 1 else 0)
    if n_blocks > 1:       # set A is called on both ranks, and the rank that meets it first in catalog order is not the only one
        owner = {l.t_idx: r for r, share in enumerate(deal_locus_blocks(blocks, 2)) for k in share for l in blocks[k]}
        with_a = [owner[t] for t in sorted(kinds) if kinds[t] in (8, 9)]
        assert len(set(with_a)) == 2
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_gloo_worker, args=(r, 2, port, q, n_blocks)) for r in range(2)]
    for p in procs:
        p.start()
    got = [q.get(timeout=60) for _ in procs]
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    want, want_n, want_tm = _want(blocks, ref, kinds)
    assert any("ps" in r for row in want for r in (row.get("reads") or {}).values())
    for rank, text, n, tm in got:
        assert text == json.dumps(want) and n == want_n, rank
        assert [e["locus_index"] for e in tm["errors"]] == [e["locus_index"] for e in want_tm["errors"]]
        assert tm["alleles_s"] == (0.5 if n_blocks > 1 else 0.25) and tm["gather_s"] > 0 and "ps_ids" not in tm
        assert "consensus_s" not in tm and "kmers_s" not in tm          # no rank reported them


def test_what_is_refused_under_sharding_and_what_no_longer_is(monkeypatch):
    monkeypatch.setattr(call_mod, "_distributed", lambda: True)
    with pytest.raises(NotImplementedError, match="snv_phase_sets"):
        call_mod.call_sample("no_such.bam", "no_such.fa", "no_such.bed", call_alleles=True, seed=1, snv_vcf="no_such.vcf", snv_phase_sets=True)
    for kw in (dict(call_alleles=True, seed=1), dict(call_alleles=True, seed=1, count_kmers="both"), dict(count_kmers="read"),
               dict(call_alleles=True, seed=1, consensus=True, consensus_method="poa", use_hp=True, ploidy="XY")):
        with pytest.raises(OSError):           # the missing file: nothing refuses the options
            call_mod.call_sample("no_such.bam", "no_such.fa", "no_such.bed", front_end="host", **kw)
