"""One process per GPU: dealing the locus blocks to the ranks of a torch.distributed job and collecting their rows as
fixed-size records.  torch is imported only inside the functions that need it: a plain run never imports it."""
from __future__ import annotations

import sys

import numpy as np

from .block import _locus_dict, _locus_row
from .fasta import Fasta
from .loci import Locus
from .options import VCF_ANCHOR_SIZE, CallOptions


def _distributed() -> bool:
    import os
    if int(os.environ.get("WORLD_SIZE", "1")) <= 1 and "torch" not in sys.modules:
        return False                      # a plain run never pays for importing torch
    try:
        import torch.distributed as dist
        return dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1
    except Exception:  # noqa: BLE001
        return False


def deal_locus_blocks(blocks: list[list[Locus]], world: int, contiguous: bool = False) -> list[list[int]]:
    """Deterministic dealing of locus blocks to `world` ranks (indices into `blocks`), balanced by an estimate of the DP
    work: sum over loci of (tract + flanks) squared.  contiguous = False: longest-processing-time scatter (the best balance; the
    counting path, where a rank holds every read anyway).  contiguous = True: every rank gets ONE run of consecutive blocks
    whose cost is as close to an equal share as a prefix split allows — the file path: a rank then reads, uploads and inflates
    only the byte range of the alignment file its own blocks lie in (the reference's workers take consecutive blocks of a
    contig off one queue, call_sample.py:103-138,414-420)."""
    cost = [sum((l.right_coord - l.left_coord + 2 * l.flank_size) ** 2 for l in blk) for blk in blocks]
    owner: list[list[int]] = [[] for _ in range(world)]
    if contiguous:
        total = float(sum(cost)) or 1.0
        acc = 0.0
        for k, c in enumerate(cost):
            # the rank whose share the block's midpoint falls into
            owner[min(world - 1, int((acc + c / 2.0) / total * world))].append(k)
            acc += c
        return owner
    load = [0] * world
    for k in sorted(range(len(blocks)), key=lambda i: (-cost[i], i)):
        r = load.index(min(load))
        owner[r].append(k)
        load[r] += cost[k]
    return [sorted(o) for o in owner]


_STAGE_KEYS = ("ref_side_s", "realign_s", "extract_s", "count_s", "count_device_s", "report_s", "load_s", "load_wait_s")
_NAME_BYTES = 64          # fixed width of the read-name field of a gathered per-read record (longer names: the field grows)


def _encode_rows(rows: list[dict], errors: list[dict]):
    """Per-locus rows -> fixed-size records: loci int64[n, 6] = (locus_index, status, ref_cn, start_adj, end_adj, n reads)
    with status 0 called / 1 skipped (no reference data) / 2 failed; reads int64[m, 6] = (locus_index, cn, sl, flags,
    sc as float64 bits, w as float64 bits) with flags bit 0 reverse strand, bit 1 realigned, bit 2 sc is None, bit 3 chimeric in the region;
    names uint8[m, W]."""
    n_reads = sum(len(r.get("reads") or {}) for r in rows)
    width = max([_NAME_BYTES] + [len(nm.encode()) for r in rows for nm in (r.get("reads") or {})])
    loci = np.zeros((len(rows) + len(errors), 6), np.int64)
    reads = np.zeros((n_reads, 6), np.int64)
    names = np.zeros((n_reads, width), np.uint8)
    k = 0
    for i, r in enumerate(rows):
        called = "ref_cn" in r
        rd = r.get("reads") or {}
        loci[i] = (r["locus_index"], 0 if called else 1, r.get("ref_cn", 0), r.get("start_adj", r["start"]), r.get("end_adj", r["end"]), len(rd))
        for nm, x in rd.items():
            b = nm.encode()
            names[k, :len(b)] = np.frombuffer(b, np.uint8)
            sc = x.get("sc")
            reads[k] = (r["locus_index"], x["cn"], x.get("sl", 0), (x["s"] == "-") | (2 if x.get("realn") else 0) | (4 if sc is None else 0) | (8 if x.get("chimeric_in_region") else 0),
                        np.float64(0.0 if sc is None else sc).view(np.int64), np.float64(x["w"]).view(np.int64))
            k += 1
    for i, e in enumerate(errors):
        loci[len(rows) + i] = (e["locus_index"], 2, 0, 0, 0, 0)
    return loci, reads, names


def _decode_rows(loci_by_index: dict, ref: Fasta, respect_ref: bool, loci_t: np.ndarray, reads_t: np.ndarray, names_t: np.ndarray):
    """The inverse of _encode_rows on the gathered tables: rows in catalog order and the failed loci.  The strings of a row
    (reference tract, anchor) are cut from the reference again: get_ref_repeat_count only ever MOVES flank bases into the
    tract (repeats.py:171-176), so the adjusted tract is reference[start_adj:end_adj]."""
    order = np.argsort(reads_t[:, 0], kind="stable") if len(reads_t) else np.zeros(0, np.int64)
    reads_t, names_t = reads_t[order], names_t[order]
    first = np.searchsorted(reads_t[:, 0], loci_t[:, 0], side="left") if len(reads_t) else np.zeros(len(loci_t), np.int64)
    rows, errors = [], []
    for (idx, status, ref_cn, s_adj, e_adj, n_reads), a in sorted(zip(loci_t.tolist(), first.tolist())):
        locus = loci_by_index[idx]
        if status == 2:
            errors.append({"locus_index": idx, "error": "failed on the rank that owned it (see that rank's log)"})
            continue
        if status == 1:
            rows.append(_locus_dict(locus))
            continue
        reads = {}
        for k in range(a, a + n_reads):
            _li, cn, sl, flags, sc_bits, w_bits = reads_t[k].tolist()
            nm = names_t[k].tobytes().rstrip(b"\0").decode()
            reads[nm] = {"s": "-" if flags & 1 else "+", "cn": cn, "w": float(np.int64(w_bits).view(np.float64)),
                         "sc": None if flags & 4 else float(np.int64(sc_bits).view(np.float64)), "sl": sl,
                         **({"realn": True} if flags & 2 else {}), **({"chimeric_in_region": True} if flags & 8 else {})}
        rd = {"ref_cn": ref_cn, "left_coord_adj": s_adj, "right_coord_adj": e_adj,
              "ref_seq": ref.fetch(locus.contig, s_adj, e_adj),
              "ref_left_flank_seq": ref.fetch(locus.contig, max(0, s_adj - VCF_ANCHOR_SIZE), s_adj)}
        rows.append(_locus_row(locus, rd, reads, CallOptions(respect_ref=respect_ref)))
    return rows, errors


def _gather_padded(t, dist, device):
    """all_gather of a 2-D table whose first dimension differs between ranks: counts first, then ONE all_gather_into_tensor
    of the tables padded to the largest (fixed-size records: strkit_amd/sharding.py)."""
    import torch
    world = dist.get_world_size()
    n = torch.tensor([t.shape[0], t.shape[1]], dtype=torch.int64, device=device)
    ns = torch.zeros(world * 2, dtype=torch.int64, device=device)
    dist.all_gather_into_tensor(ns, n)
    ns = ns.cpu().numpy().reshape(world, 2)
    rows, cols = int(ns[:, 0].max()), int(ns[:, 1].max())
    pad = torch.zeros((max(rows, 1), max(cols, 1)), dtype=t.dtype, device=device)
    pad[:t.shape[0], :t.shape[1]] = t.to(device)
    out = torch.zeros((world * pad.shape[0], pad.shape[1]), dtype=t.dtype, device=device)
    dist.all_gather_into_tensor(out, pad)
    out = out.cpu().numpy().reshape(world, pad.shape[0], pad.shape[1])
    return [out[w, :int(ns[w, 0])] for w in range(world)]


def call_blocks_sharded(blocks, call_fn, ref: Fasta | None = None, respect_ref: bool = False,
                        contiguous: bool = False) -> tuple[list[dict], int, dict]:
    """One process per GPU (`--processes N` of the reference <-> N ranks of a torch.distributed job): every rank calls
    its share of the locus blocks with `call_fn(blocks) -> (results, reads kept, stage times)` and all ranks get the
    merged results ordered by locus index, as the reference's ordered merge does (call_sample.py:195-197,420).
    The only communication is the collection of the results as FIXED-SIZE records — one per locus, one per read, the
    read names as a fixed-width byte field — with all_gather_into_tensor (RCCL over xGMI on the GPU box, gloo in the CPU
    tests); no pickled Python objects cross ranks."""
    import torch
    import torch.distributed as dist
    world, rank = dist.get_world_size(), dist.get_rank()
    device = torch.device("cuda", torch.cuda.current_device()) if dist.get_backend() == "nccl" else torch.device("cpu")
    mine = [blocks[k] for k in deal_locus_blocks(blocks, world, contiguous)[rank]]
    results, _n_depth, tm = call_fn(mine) if mine else ([], 0, {})
    g_loci, g_reads, g_names = (_gather_padded(torch.from_numpy(t), dist, device) for t in _encode_rows(results, tm.get("errors", [])))
    width = max(x.shape[1] for x in g_names)
    g_names = [np.pad(x, ((0, 0), (0, width - x.shape[1]))) for x in g_names]
    stage_t = torch.tensor([[float(tm.get(k, 0.0)) for k in _STAGE_KEYS]], dtype=torch.float64)
    g_stage = np.concatenate(_gather_padded(stage_t, dist, device))
    by_index = {l.t_idx: l for blk in blocks for l in blk}
    merged, errors = _decode_rows(by_index, ref, respect_ref, np.concatenate(g_loci), np.concatenate(g_reads), np.concatenate(g_names))
    # ranks run side by side: the slowest one counts
    stage = {"errors": errors, **{k: v for k, v in zip(_STAGE_KEYS, g_stage.max(axis=0).tolist()) if v > 0 or k in tm}}
    return merged, sum(len(r.get("reads") or {}) for r in merged), stage
