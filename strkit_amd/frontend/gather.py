"""One process per GPU: dealing the locus blocks to the ranks of a torch.distributed job and collecting their rows as
fixed-size records.  torch is imported only inside the functions that need it: a plain run never imports it."""
from __future__ import annotations

import gc
import struct
import sys
import time
from contextlib import contextmanager

import numpy as np

from .block import _locus_dict, _locus_row
from .fasta import Fasta
from .loci import Locus
from .options import VCF_ANCHOR_SIZE, CallOptions


@contextmanager
def _collector_paused():
    # The report is hundreds of thousands of small dicts that reference nothing but strings and numbers: the cyclic collector
    # finds nothing in them and costs a third of the time it takes to build them (it runs every 700 new containers, and its
    # older generations grow with the report).  It is paused while the blocks run, and left as it was found.
    was_on = gc.isenabled()
    gc.disable()
    try:
        yield
    finally:
        if was_on:
            gc.enable()


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


_STAGE_KEYS = ("ref_side_s", "realign_s", "extract_s", "count_s", "count_device_s", "report_s", "load_s", "load_wait_s",
               "alleles_s", "alleles_device_s", "consensus_s", "consensus_device_s", "consensus_fetch_s", "kmers_s", "kmers_device_s",
               "phase_inputs_s", "phase_cells_s", "useful_snvs_s", "snv_candidates_s", "names_s")
_NAME_BYTES = 64          # fixed width of the read-name field of a gathered per-read record (longer names: the field grows)

# what a run under torch.distributed still refuses, by option (call_sample raises them, the command line reports them)
SHARDING_REFUSALS = {
    "snv_phase_sets": "snv_phase_sets=True under torch.distributed: the phase sets of SNV calls are a serial chain over the loci of a "
                      "contig that runs before the allele sequences and k-mer counts read the peaks (phase_sets.resolve_block), so "
                      "a rank cannot make it for its own blocks alone; run one process",
    "discover_snvs": "discover_snvs=True under torch.distributed: the ranks do not discover candidate SNVs yet (the gathered rows would "
                     "carry them as a file's candidates are carried, which is untested); run one process",
    "use_methyl": "use_methyl=True under torch.distributed: the records that the ranks gather (call_blocks_sharded) have no "
                  "fields for methylation yet; run one process",
}


@_collector_paused()      # (records and rows by the hundred thousand, as in call_blocks)
def _encode_rows(rows: list[dict], errors: list[dict]):
    """Per-locus rows -> fixed-size records: loci int64[n, 6] = (locus_index, status, ref_cn, start_adj, end_adj, n reads)
    with status 0 called / 1 skipped (no reference data) / 2 failed; reads int64[m, 6] = (locus_index, cn, sl, flags,
    sc as float64 bits, w as float64 bits) with flags bit 0 reverse strand, bit 1 realigned, bit 2 sc is None, bit 3 chimeric in the region;
    names uint8[m, W]."""
    read_dicts = [r.get("reads") or {} for r in rows]
    names_b = [nm.encode() for rd in read_dicts for nm in rd]
    n_reads = len(names_b)
    width = max(_NAME_BYTES, max(map(len, names_b), default=0))
    # column by column over all reads at once: a Python loop per read with numpy scalars in it costs ten times this
    loci = np.zeros((len(rows) + len(errors), 6), np.int64)
    if rows:
        loci[:len(rows)] = [(r["locus_index"], 0 if "ref_cn" in r else 1, r.get("ref_cn", 0), r.get("start_adj", r["start"]), r.get("end_adj", r["end"]), len(rd))
                            for r, rd in zip(rows, read_dicts)]
    if errors:
        loci[len(rows):, 0] = [e["locus_index"] for e in errors]
        loci[len(rows):, 1] = 2
    xs = [x for rd in read_dicts for x in rd.values()]
    scs = [x.get("sc") for x in xs]
    reads = np.zeros((n_reads, 6), np.int64)
    reads[:, 0] = np.repeat(loci[:len(rows), 0], loci[:len(rows), 5])
    reads[:, 1] = [x["cn"] for x in xs]
    reads[:, 2] = [x.get("sl", 0) for x in xs]
    reads[:, 3] = [(x["s"] == "-") | (2 if x.get("realn") else 0) | (4 if sc is None else 0) | (8 if x.get("chimeric_in_region") else 0)
                   for x, sc in zip(xs, scs)]
    reads[:, 4] = np.array([0.0 if sc is None else sc for sc in scs], np.float64).view(np.int64)
    reads[:, 5] = np.array([x["w"] for x in xs], np.float64).view(np.int64)
    names = np.frombuffer(b"".join(nm.ljust(width, b"\0") for nm in names_b), np.uint8).reshape(n_reads, width).copy()
    return loci, reads, names


@_collector_paused()      # (records and rows by the hundred thousand, as in call_blocks)
def _decode_rows(loci_by_index: dict, ref: Fasta, respect_ref: bool, loci_t: np.ndarray, reads_t: np.ndarray, names_t: np.ndarray,
                 calls: dict | None = None):
    """The inverse of _encode_rows on the gathered tables: rows in catalog order and the failed loci.  The strings of a row
    (reference tract, anchor) are cut from the reference again: get_ref_repeat_count only ever MOVES flank bases into the
    tract (repeats.py:171-176), so the adjusted tract is reference[start_adj:end_adj].  `calls`: the merged call tables
    (_merge_call_tables over the shares of _encode_calls); the rows then get their call fields back."""
    order = np.argsort(reads_t[:, 0], kind="stable") if len(reads_t) else np.zeros(0, np.int64)
    reads_t, names_t = reads_t[order], names_t[order]
    first = np.searchsorted(reads_t[:, 0], loci_t[:, 0], side="left") if len(reads_t) else np.zeros(len(loci_t), np.int64)
    # (the tables as Python values, once: no numpy scalar per read)
    read_recs, scs, ws = reads_t.tolist(), _floats(reads_t[:, 4]), _floats(reads_t[:, 5])
    name_bytes, width = names_t.tobytes(), names_t.shape[1]
    put_calls = _CallDecoder(calls) if calls is not None and any(len(calls[k]) for k in ("calls", "reads_x")) else None
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
            _li, cn, sl, flags, _sc_bits, _w_bits = read_recs[k]
            reads[name_bytes[k * width:(k + 1) * width].rstrip(b"\0").decode()] = {
                "s": "-" if flags & 1 else "+", "cn": cn, "w": ws[k], "sc": None if flags & 4 else scs[k], "sl": sl,
                **({"realn": True} if flags & 2 else {}), **({"chimeric_in_region": True} if flags & 8 else {})}
        rd = {"ref_cn": ref_cn, "left_coord_adj": s_adj, "right_coord_adj": e_adj,
              "ref_seq": ref.fetch(locus.contig, s_adj, e_adj),
              "ref_left_flank_seq": ref.fetch(locus.contig, max(0, s_adj - VCF_ANCHOR_SIZE), s_adj)}
        rows.append(_locus_row(locus, rd, reads, CallOptions(respect_ref=respect_ref)))
        if put_calls is not None:
            put_calls(rows[-1], idx)
    return rows, errors


# ---- the call fields of the rows (genotype.genotype_row / kmers_row, phase_block.phase_row) ------------------------------------
# Beside the three tables of _encode_rows a share sends, where its rows have call fields at all:
#   calls   int64[c, 14]  one record per row that has a row-level call field
#   peaks   int64[p, 22]  child of calls by (locus_index, ordinal): one record per slot of call / means / n_reads / seqs / kmers
#   snvs    int64[s, 16]  child of calls by (locus_index, ordinal): the called SNVs of a row
#   reads_x int64[x, 9]   one record per read that has p, hp, ps, snvu or kmers, by (locus_index, ordinal of the read in its row)
#   kmers   int64[k, 4]   (locus_index, key, count): of a row first the pairs of its reads in read order, then of its peaks in
#                         peak order, each dict in insertion order; the owners hold the number of their pairs
#   heap    uint8[h, 1]   the bytes of every string; (offset, length) columns point into it (short strings are stored once)
#   ps_ids  int64[i, 2]   (the share's phase-set number, the original PS value): PhaseSetRemap's table, turned round
# A list keeps its own length and an optional value a flag bit of its own, so that an absent key, None and an empty list stay
# apart.  Floats are their 64-bit patterns.  Within a share the records of a row are in the order of the row's dicts and lists,
# and a stable sort by locus index keeps that order after the shares are put together.
_CALL_TABLES = {"calls": 14, "peaks": 22, "snvs": 16, "reads_x": 9, "kmers": 4, "heap": 1, "ps_ids": 2}
_OFFSET_COLUMNS = {"calls": (3,), "peaks": (11, 14, 16, 19), "snvs": (2, 4, 7), "reads_x": (6,), "kmers": (1,)}
# calls: 0 locus_index, 1 flags, 2 mean_model_align_score, 3-4 assign_method, 5 len(call), 6 len(peaks.means), 7 len(peaks.n_reads),
# 8 len(peaks.seqs), 9 len(peaks.start_anchor_seqs), 10 len(peaks.kmers), 11 peaks.modal_n, 12 ps, 13 len(snvs)
_C_SCORE_KEY, _C_SCORE, _C_READ_PEAKS, _C_PEAKS, _C_N_READS, _C_SEQS, _C_ANCHORS, _C_KMERS, _C_CALL, _C_CI95, _C_CI99, _C_PS, _C_SNVS, \
    _C_METHOD = (1 << b for b in range(14))
# peaks: 0 locus_index, 1 ordinal, 2 call, 3-4 call_95_cis, 5-6 call_99_cis, 7 mean, 8 weight, 9 stdev, 10 n_reads, 11-12 sequence,
# 13 sequence is None, 14-15 its method, 16-17 start anchor, 18 start anchor is None, 19-20 its method, 21 k-mer pairs
# snvs: 0 locus_index, 1 ordinal, 2-3 id, 4-5 ref, 6 pos, 7-8 call (one base per allele), 9 len(rcs), 10-15 rcs
_MAX_RCS = 6
# reads_x: 0 locus_index, 1 ordinal, 2 flags, 3 p, 4 hp, 5 ps, 6-7 snvu (one base per called SNV), 8 k-mer pairs
_X_P, _X_HP, _X_PS, _X_SNVU, _X_KMERS = (1 << b for b in range(5))
_READ_BASE_KEYS = 5       # s, cn, w, sc, sl: a read record with no more keys than these has no call field


class _Heap:
    """The strings of a share as one run of bytes; put() -> (offset, length).  A short string (method names, bases, k-mers) is
    stored once."""

    def __init__(self):
        self.parts: list[bytes] = []
        self.size = 0
        self.seen: dict[str, tuple[int, int]] = {}

    def put(self, s: str) -> tuple[int, int]:
        at = self.seen.get(s)
        if at is None:
            b = s.encode()
            at = (self.size, len(b))
            self.parts.append(b)
            self.size += len(b)
            if len(b) <= 64:
                self.seen[s] = at
        return at

    def table(self) -> np.ndarray:
        return np.frombuffer(b"".join(self.parts), np.uint8).reshape(-1, 1).copy()


def _bits(x: float) -> int:
    return struct.unpack("<q", struct.pack("<d", x))[0]


def _floats(column: np.ndarray) -> list:
    return np.ascontiguousarray(column).view(np.float64).tolist()


def _bases(values, what: str) -> str:
    if any(len(v) != 1 for v in values):
        raise ValueError(f"{what}: every entry is one base, got {values!r}")
    return "".join(values)


@_collector_paused()      # (records and rows by the hundred thousand, as in call_blocks)
def _encode_calls(rows: list[dict], ps_ids: dict | None = None) -> dict[str, np.ndarray]:
    """The call fields of per-locus rows -> the tables above (every one of them has 0 records for rows without call fields).
    `ps_ids`: {phase-set number in these rows: original PS value} (PhaseSetRemap.originals)."""
    heap = _Heap()
    put = heap.put
    calls, peaks, snvs, reads_x, kmers = [], [], [], [], []

    def put_kmers(idx, d):
        for key, n in d.items():
            kmers.append((idx, *put(key), n))
        return len(d)

    for r in rows:
        idx = r["locus_index"]
        rd = r.get("reads")
        # (rows without call fields, the whole of a run that does not genotype, pay one len() per read here and no more)
        for k, x in enumerate(rd.values()) if rd and max(map(len, rd.values())) > _READ_BASE_KEYS else ():
            if len(x) <= _READ_BASE_KEYS:
                continue
            fl = ((_X_P if "p" in x else 0) | (_X_HP if "hp" in x else 0) | (_X_PS if "ps" in x else 0)
                  | (_X_SNVU if "snvu" in x else 0) | (_X_KMERS if "kmers" in x else 0))
            if fl:
                reads_x.append((idx, k, fl, x.get("p", 0), x.get("hp", 0), x.get("ps", 0),
                                *(put(_bases(x["snvu"], "snvu")) if fl & _X_SNVU else (0, 0)), put_kmers(idx, x["kmers"]) if fl & _X_KMERS else 0))
        pk = r.get("peaks")
        call, ci95, ci99, method = r.get("call"), r.get("call_95_cis"), r.get("call_99_cis"), r.get("assign_method")
        fl = ((_C_SCORE_KEY if "mean_model_align_score" in r else 0) | (_C_READ_PEAKS if r.get("read_peaks_called") else 0)
              | (_C_PEAKS if pk is not None else 0) | (_C_CALL if call is not None else 0) | (_C_CI95 if ci95 is not None else 0)
              | (_C_CI99 if ci99 is not None else 0) | (_C_PS if "ps" in r else 0) | (_C_SNVS if "snvs" in r else 0)
              | (_C_METHOD if method is not None else 0))
        if not fl:
            continue
        score = r.get("mean_model_align_score")
        if score is not None:
            fl |= _C_SCORE
        pk = pk or {}
        means, weights, stdevs, n_reads = pk.get("means", []), pk.get("weights", []), pk.get("stdevs", []), pk.get("n_reads")
        seqs, anchors, pk_kmers = pk.get("seqs"), pk.get("start_anchor_seqs"), pk.get("kmers")
        fl |= ((_C_N_READS if n_reads is not None else 0) | (_C_SEQS if seqs is not None else 0) | (_C_ANCHORS if anchors is not None else 0)
               | (_C_KMERS if pk_kmers is not None else 0))
        call, ci95, ci99, n_reads, seqs, anchors, pk_kmers = (v or [] for v in (call, ci95, ci99, n_reads, seqs, anchors, pk_kmers))
        if any(len(ci) != len(call) for ci, flag in ((ci95, _C_CI95), (ci99, _C_CI99)) if fl & flag) or not len(means) == len(weights) == len(stdevs):
            raise ValueError(f"locus {idx}: a call and its intervals, and the means, weights and stdevs of the peaks, have one length each")
        row_snvs = r.get("snvs") or []
        calls.append((idx, fl, _bits(score) if score is not None else 0, *(put(method) if method is not None else (0, 0)), len(call), len(means),
                      len(n_reads), len(seqs), len(anchors), len(pk_kmers), pk.get("modal_n", 0), r.get("ps", 0), len(row_snvs)))
        for k in range(max(len(call), len(ci95), len(means), len(n_reads), len(seqs), len(anchors), len(pk_kmers))):
            rec = [idx, k] + [0] * 20
            if k < len(call):
                rec[2] = call[k]
            if k < len(ci95):
                rec[3:5] = ci95[k]
            if k < len(ci99):
                rec[5:7] = ci99[k]
            if k < len(means):
                rec[7:10] = _bits(means[k]), _bits(weights[k]), _bits(stdevs[k])
            if k < len(n_reads):
                rec[10] = n_reads[k]
            for at, pairs in ((11, seqs), (16, anchors)):
                if k < len(pairs):
                    seq, how = pairs[k]
                    rec[at:at + 5] = (*(put(seq) if seq is not None else (0, 0)), int(seq is None), *put(how))
            if k < len(pk_kmers):
                rec[21] = put_kmers(idx, pk_kmers[k])
            peaks.append(rec)
        for k, s in enumerate(row_snvs):
            if len(s["rcs"]) > _MAX_RCS:
                raise ValueError(f"locus {idx}: an SNV record holds at most {_MAX_RCS} read counts")
            snvs.append((idx, k, *put(s["id"]), *put(s["ref"]), s["pos"], *put(_bases(s["call"], "snvs.call")), len(s["rcs"]),
                         *s["rcs"], *([0] * (_MAX_RCS - len(s["rcs"])))))
    out = {"calls": calls, "peaks": peaks, "snvs": snvs, "reads_x": reads_x, "kmers": kmers, "ps_ids": sorted((ps_ids or {}).items())}
    out = {name: np.array(recs, np.int64).reshape(-1, _CALL_TABLES[name]) for name, recs in out.items()}
    out["heap"] = heap.table()
    return out


def _merge_call_tables(shares: list[dict]) -> dict[str, np.ndarray]:
    """The tables of _encode_calls of several shares as one set: the heaps back to back with every offset column moved by where
    its share's heap begins, the phase-set numbers of a share turned back into the original PS values they stand for (a share
    without a table keeps its numbers: they are then taken for original values), the records sorted by locus index (stable)."""
    out: dict[str, list] = {name: [] for name in _CALL_TABLES if name != "ps_ids"}
    base = 0
    for share in shares:
        sh = {name: np.array(share[name]) for name in out}     # (copies: the offsets and numbers are rewritten)
        ids = share.get("ps_ids")
        for name, cols in _OFFSET_COLUMNS.items():
            sh[name][:, cols] += base
        if ids is not None and len(ids):
            for name, col, flag_col, flag in (("reads_x", 5, 2, _X_PS), ("calls", 12, 1, _C_PS)):
                t = sh[name]
                has = (t[:, flag_col] & flag) != 0
                at = np.searchsorted(ids[:, 0], t[has, col])
                if (at >= len(ids)).any() or (ids[np.minimum(at, len(ids) - 1), 0] != t[has, col]).any():
                    raise ValueError("a gathered row holds a phase-set number that its share's table does not name")
                t[has, col] = ids[at, 1]
        base += len(sh["heap"])
        for name in out:
            out[name].append(sh[name])
    merged = {name: np.concatenate(parts) if parts else np.zeros((0, _CALL_TABLES[name]), np.uint8 if name == "heap" else np.int64)
              for name, parts in out.items()}
    for name in ("calls", "peaks", "snvs", "reads_x", "kmers"):
        merged[name] = merged[name][np.argsort(merged[name][:, 0], kind="stable")]
    return merged


class _CallDecoder:
    """The inverse of _encode_calls on merged tables: called with a row as _decode_rows built it and its locus index, it puts
    the call fields back, keys in the order genotype_row, phase_row and kmers_row add them.  Every table is sorted by locus
    index, so a locus finds its records by one searchsorted per table."""

    def __init__(self, t: dict):
        heap = t["heap"].tobytes()
        text = lambda off, ln: heap[off:off + ln].decode()  # noqa: E731
        self.text = text
        self.calls, self.peaks, self.snvs, self.reads_x = (t[k].tolist() for k in ("calls", "peaks", "snvs", "reads_x"))
        self.index = {k: t[k][:, 0] for k in ("calls", "peaks", "snvs", "reads_x", "kmers")}
        self.kmer_keys = [text(off, ln) for off, ln in t["kmers"][:, 1:3].tolist()]
        self.kmer_counts = t["kmers"][:, 3].tolist()
        self.score = _floats(t["calls"][:, 2])
        self.stats = [_floats(t["peaks"][:, c]) for c in (7, 8, 9)]
        self.k_at = 0

    def first(self, table: str, idx: int) -> int:
        return int(np.searchsorted(self.index[table], idx, side="left"))

    def take_kmers(self, n: int) -> dict:
        a = self.k_at
        self.k_at = a + n
        return dict(zip(self.kmer_keys[a:a + n], self.kmer_counts[a:a + n]))

    def __call__(self, row: dict, idx: int) -> None:
        text = self.text
        self.k_at = self.first("kmers", idx)
        x = self.first("reads_x", idx)
        if x < len(self.reads_x) and self.reads_x[x][0] == idx:
            recs = list(row["reads"].values())
            while x < len(self.reads_x) and self.reads_x[x][0] == idx:
                _i, k, fl, p, hp, ps, s_off, s_len, n_k = self.reads_x[x]
                r = recs[k]
                if fl & _X_P:
                    r["p"] = p
                if fl & _X_HP:
                    r["hp"] = hp
                if fl & _X_PS:
                    r["ps"] = ps
                if fl & _X_SNVU:
                    r["snvu"] = list(text(s_off, s_len))
                if fl & _X_KMERS:
                    r["kmers"] = self.take_kmers(n_k)
                x += 1
        c = self.first("calls", idx)
        if c == len(self.calls) or self.calls[c][0] != idx:
            return
        _i, fl, _score, m_off, m_len, n_call, n_means, n_n_reads, n_seqs, n_anchors, n_kmers, modal_n, ps, n_snvs = self.calls[c]
        a = self.first("peaks", idx)
        pk = self.peaks[a:a + max(n_call, n_means, n_n_reads, n_seqs, n_anchors, n_kmers)]
        if fl & _C_METHOD:
            row["assign_method"] = text(m_off, m_len)
        if fl & _C_CALL:
            row["call"] = [q[2] for q in pk[:n_call]]
        if fl & _C_CI95:
            row["call_95_cis"] = [[q[3], q[4]] for q in pk[:n_call]]
        if fl & _C_CI99:
            row["call_99_cis"] = [[q[5], q[6]] for q in pk[:n_call]]
        if fl & _C_PEAKS:
            means, weights, stdevs = (col[a:a + n_means] for col in self.stats)
            peaks = {"means": means, "weights": weights, "stdevs": stdevs, "modal_n": modal_n,
                     "n_reads": [q[10] for q in pk[:n_n_reads]] if fl & _C_N_READS else None}
            for name, flag, n, at in (("seqs", _C_SEQS, n_seqs, 11), ("start_anchor_seqs", _C_ANCHORS, n_anchors, 16)):
                if fl & flag:
                    peaks[name] = [[None if q[at + 2] else text(q[at], q[at + 1]), text(q[at + 3], q[at + 4])] for q in pk[:n]]
            if fl & _C_KMERS:
                peaks["kmers"] = [self.take_kmers(q[21]) for q in pk[:n_kmers]]
            row["peaks"] = peaks
        if fl & _C_READ_PEAKS:
            row["read_peaks_called"] = True
        if fl & _C_SCORE_KEY:
            row["mean_model_align_score"] = self.score[c] if fl & _C_SCORE else None
        if fl & _C_PS:
            row["ps"] = ps
        if fl & _C_SNVS:
            s0 = self.first("snvs", idx)
            row["snvs"] = [{"id": text(q[2], q[3]), "ref": text(q[4], q[5]), "pos": q[6], "call": list(text(q[7], q[8])),
                            "rcs": q[10:10 + q[9]]} for q in self.snvs[s0:s0 + n_snvs]]


def renumber_phase_sets(rows: list[dict]) -> None:
    """Rows in catalog order whose `ps` values are ORIGINAL PS values (-1: a read with HP and no PS) -> the run-wide numbers
    1, 2, ... in order of first appearance over the rows and, inside a row, over its reads: what one PhaseSetRemap gives a run
    of one process, which meets the kept reads in this order.  The row-level `ps` of an `hp` call is one of its reads' values
    and takes that value's number.  Exact, because the phased call reads `ps` only through equality and through which value a
    locus meets first in read order (strk_phase.h, k_phase_group): numbering the same sets differently, as a rank does that
    sees only its own blocks, gives the same calls."""
    ids: dict[int, int] = {}
    for row in rows:
        for r in (row.get("reads") or {}).values():
            if "ps" in r:
                r["ps"] = ids.setdefault(r["ps"], len(ids) + 1)
        if "ps" in row:
            row["ps"] = ids.setdefault(row["ps"], len(ids) + 1)


def _decode_shares(loci_by_index: dict, ref: Fasta, respect_ref: bool, row_shares: list[tuple], call_shares: list[dict] | None = None):
    """What every rank does with the gathered tables: per share the three tables of _encode_rows and, where some share has
    calls, the tables of _encode_calls -> (rows in catalog order, phase sets numbered run-wide, and the failed loci)."""
    width = max(names.shape[1] for _, _, names in row_shares)
    loci_t, reads_t, names_t = (np.concatenate(parts) for parts in zip(*((loci, reads, np.pad(names, ((0, 0), (0, width - names.shape[1]))))
                                                                         for loci, reads, names in row_shares)))
    calls = _merge_call_tables(call_shares) if call_shares is not None else None
    rows, errors = _decode_rows(loci_by_index, ref, respect_ref, loci_t, reads_t, names_t, calls)
    if calls is not None and ((calls["reads_x"][:, 2] & _X_PS).any() or (calls["calls"][:, 1] & _C_PS).any()):
        renumber_phase_sets(rows)
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


def shared_seed() -> int:
    """The run seed of a torch.distributed job: rank 0 draws it and broadcasts it as a one-element int64 tensor (on the device the
    backend uses, as call_blocks_sharded chooses it), so that every rank calls with it and reports it.  The seed of a locus is
    alleles.locus_seeds(run seed, t_idx): with one run seed a call does not depend on which rank owns its locus."""
    import torch
    import torch.distributed as dist
    device = torch.device("cuda", torch.cuda.current_device()) if dist.get_backend() == "nccl" else torch.device("cpu")
    seed = torch.tensor([int(np.random.default_rng().integers(0, 1 << 63)) if dist.get_rank() == 0 else 0], dtype=torch.int64, device=device)
    dist.broadcast(seed, src=0)
    return int(seed.cpu()[0])


def call_blocks_sharded(blocks, call_fn, ref: Fasta | None = None, respect_ref: bool = False,
                        contiguous: bool = False) -> tuple[list[dict], int, dict]:
    """One process per GPU (`--processes N` of the reference <-> N ranks of a torch.distributed job): every rank calls
    its share of the locus blocks with `call_fn(blocks) -> (results, reads kept, stage times)` and all ranks get the
    merged results ordered by locus index, as the reference's ordered merge does (call_sample.py:195-197,420).
    The only communication is the collection of the results as numeric tables with all_gather_into_tensor (RCCL over xGMI on
    the GPU box, gloo in the CPU tests): FIXED-SIZE records, one per locus and one per read, the read names as a fixed-width
    byte field, and, where the rows carry calls, the tables of _encode_calls (child records by locus index and ordinal, strings
    as bytes of one heap per rank); no pickled Python objects and no text rows cross ranks.  A rank without a block takes part
    with empty tables.  `stage times["ps_ids"]` of call_fn, {phase-set number in its rows: original PS value}, lets the merged
    rows be numbered as one process numbers them (renumber_phase_sets).  The stage times are the maximum over the ranks, but
    `gather_s`: what this rank spent here on encoding, the collectives and decoding."""
    import torch
    import torch.distributed as dist
    world, rank = dist.get_world_size(), dist.get_rank()
    device = torch.device("cuda", torch.cuda.current_device()) if dist.get_backend() == "nccl" else torch.device("cpu")
    mine = [blocks[k] for k in deal_locus_blocks(blocks, world, contiguous)[rank]]
    results, _n_depth, tm = call_fn(mine) if mine else ([], 0, {})
    t_gather = time.perf_counter()
    gather = lambda t: _gather_padded(torch.from_numpy(t), dist, device)  # noqa: E731
    g_loci, g_reads, g_names = (gather(t) for t in _encode_rows(results, tm.get("errors", [])))
    # the call tables: their sizes first, then only those that hold a record on some rank (a run without calls sends none)
    own = _encode_calls(results, tm.pop("ps_ids", None))
    sizes = np.stack(gather(np.array([[len(own[name]) for name in _CALL_TABLES]], np.int64)))[:, 0]
    shares = [{name: np.zeros((0, cols), own[name].dtype) for name, cols in _CALL_TABLES.items()} for _ in range(world)]
    for k, name in enumerate(_CALL_TABLES):
        if sizes[:, k].any():
            for share, table in zip(shares, gather(own[name])):
                share[name] = table
    stage_t = torch.tensor([[float(tm.get(k, 0.0)) for k in _STAGE_KEYS]], dtype=torch.float64)
    g_stage = np.concatenate(_gather_padded(stage_t, dist, device))
    by_index = {l.t_idx: l for blk in blocks for l in blk}
    merged, errors = _decode_shares(by_index, ref, respect_ref, list(zip(g_loci, g_reads, g_names)), shares if sizes.any() else None)
    # ranks run side by side: the slowest one counts
    stage = {"errors": errors, **{k: v for k, v in zip(_STAGE_KEYS, g_stage.max(axis=0).tolist()) if v > 0 or k in tm},
             "gather_s": time.perf_counter() - t_gather}
    return merged, sum(len(r.get("reads") or {}) for r in merged), stage
