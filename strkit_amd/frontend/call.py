"""`strkit call`-shaped driver over the device backend: alignment file + reference + catalog -> per-locus read copy
numbers, by the worker loop of strkit/call/call_sample.py:81-197 (blocks of loci, segments fetched once per block).  The
per-locus path is in block.py.  SNV phasing, haplotags and partial-order alignment are not part of this backend."""
from __future__ import annotations

import dataclasses
import itertools
import json
import sys
import time
from concurrent.futures import ThreadPoolExecutor
from contextlib import closing, contextmanager

import numpy as np

from .. import _lib
from .bam import BamFile
from .block import _call_block_native, _call_block_python, _locus_dict, _locus_row  # noqa: F401 (the last two: as before)
from .fasta import Fasta
from .gather import SHARDING_REFUSALS, _collector_paused, _distributed, call_blocks_sharded, deal_locus_blocks, shared_seed
from .loci import Locus, load_loci, resolve_contig
from .native import DeviceBam, IndexedBam, NativeBam
from .options import (DEFAULT_REF_MAX_ITERS, MAX_READS, AnnotationCallOptions, CallOptions, MethylCallOptions, PhasedCallOptions, PhaseSetCallOptions, PloidyCallOptions, PoaCallOptions, ReadSelectionCallOptions, SnvDiscoveryCallOptions,
                      allele_counts, phased, report_parameters, with_keywords)
from .phase_block import PhaseRun
from .reader import open_path
from .refside import get_loci_with_ref_data, get_locus_with_ref_data, ref_side_of_blocks

# (what moved to the other modules is still offered here under the names it had)
__all__ = ["AnnotationCallOptions", "CallOptions", "PoaCallOptions", "PhasedCallOptions", "MethylCallOptions", "PloidyCallOptions", "PhaseSetCallOptions", "ReadSelectionCallOptions", "SnvDiscoveryCallOptions", "call_sample", "call_locus", "call_blocks", "call_blocks_sharded", "deal_locus_blocks", "write_json", "get_locus_with_ref_data", "get_loci_with_ref_data", "MAX_READS"]


def ploidy_blocks(blocks, opts):
    """The blocks of a run without the loci that its ploidy configuration leaves out (a contig that is ignored, or has 0
    alleles: strkit/call/loci.py:224-230), and how many those are.  The loci that stay keep their t_idx, hence their seeds.
    Without a configuration: the blocks as they are."""
    if getattr(opts, "ploidy", None) is None:
        return blocks, 0
    config = allele_counts(opts)
    kept = [[locus for locus in block if config.called(locus.contig)] for block in blocks]
    return [b for b in kept if b], sum(len(b) for b in blocks) - sum(len(b) for b in kept)


def call_locus(locus: Locus, bam: BamFile, ref: Fasta, *, ctx: _lib.Context | None = None, opts: CallOptions | None = None,
               **option_keywords) -> dict:
    """The per-locus entry point (strkit/call/call_locus.py:974-995) over this backend: one locus, its LocusResult
    record up to the read records (a block of one through the same path as call_sample).  Options as for call_sample."""
    return call_blocks([[locus]], bam, ref, with_keywords(opts, **option_keywords), ctx)[0][0]


def call_sample(bam: BamFile | str, ref: Fasta | str, loci_file: str, *, sample_id: str | None = None,
                ctx: _lib.Context | None = None, processes: int = 1, front_end: str = "auto", span_bytes: int = 4 << 30,
                opts: CallOptions | None = None, **option_keywords) -> dict:
    """The report of one sample.  Options: the fields of `CallOptions` and of `PoaCallOptions` (described there), by name (an
    unknown one is a TypeError) and / or as `opts`; `seed=None` with `call_alleles` draws the run seed once and reports it.

    `front_end` (for a `bam` given as a path): "device" = the file is inflated, scanned and cut on the GPU (DeviceBam), whole or
    in spans of at most `span_bytes` compressed bytes; "host" = on the host cores (IndexedBam, or NativeBam without an index);
    "auto" = "device" where that is possible (reader.choose_reader has the rule, reader.BackgroundOpener the retry when device
    memory runs out).  Under torch.distributed every rank opens the file on its own GPU and calls its share of the blocks, genotypes
    included; `seed=None` is then drawn by rank 0 and broadcast, so that every rank calls with one seed and reports
    it: the seed of a locus is locus_seeds(run seed, t_idx), so a call does not depend on which rank owns its locus.
    `snv_phase_sets`, `discover_snvs` and `use_methyl` are refused there (NotImplementedError), before a file is opened."""
    opts = with_keywords(opts, **option_keywords)
    for name, why in SHARDING_REFUSALS.items():
        if getattr(opts, name, False) and _distributed():
            raise NotImplementedError(why)
    if opts.call_alleles and opts.seed is None:
        opts = dataclasses.replace(opts, seed=shared_seed() if _distributed() else int(np.random.default_rng().integers(0, 1 << 63)))
    opts.validate()
    t_open = time.perf_counter()
    own_reader = isinstance(bam, str)
    # a path: a host reader at once, or a device reader that opens in the background
    bam, opener = open_path(bam, front_end, span_bytes, ctx, _distributed()) if own_reader else (bam, None)
    t_open = time.perf_counter() - t_open       # (device reader: replaced below by the time its thread took)
    try:
        ref = Fasta(ref) if isinstance(ref, str) else ref
        t0 = time.perf_counter()
        # catalog, alignment file and reference may or may not carry the "chr" prefix (call_locus.py:758 normalize_contig):
        # a locus is called when its contig exists, under either spelling, in both files
        both = {c for c in (opener or bam).references if resolve_contig(ref.references, c) is not None}
        blocks = load_loci(loci_file, opts.flank_size, contigs=both, processes=processes)
        n_loaded = sum(len(b) for b in blocks)
        blocks, n_ploidy_ignored = ploidy_blocks(blocks, opts)
        tm_pre: dict = {}
        ref_cache = None
        if opener is not None and not _distributed():
            ref_cache = ref_side_of_blocks(blocks, ref, opts, ctx or _lib.default_context(), tm_pre)
    except BaseException:
        if opener is not None:
            opener.close_on_error()
        raise
    t_wait = 0.0
    if opener is not None:                       # the reader, or what kept it from opening
        bam, t_open, t_wait = opener.result()
    with open(loci_file) as fh:                  # the catalog's size (the lines parse_loci_bed yields), without parsing them again
        n_catalog = sum(1 for raw in fh if raw.strip() and not raw.lstrip().startswith("#"))
    if n_loaded < n_catalog:
        print(f"strkit_amd: {n_catalog - n_loaded} of {n_catalog} catalog loci lie on contigs that the alignment file or "
              f"the reference does not have; they are not called", file=sys.stderr)

    def run(bl):
        if not (_distributed() and getattr(opts, "use_hp", False)):
            return call_blocks(bl, bam, ref, opts, ctx, ref_cache=ref_cache)
        ps_ids: dict = {}       # this rank numbers the phase sets it meets; the gather needs the values the numbers stand for
        rows, n, tm_ = call_blocks(bl, bam, ref, opts, ctx, ref_cache=ref_cache, ps_ids=ps_ids)
        return rows, n, {**tm_, "ps_ids": ps_ids}

    try:
        if _distributed():          # launched under torch.distributed (one rank per GPU): shard the blocks
            # a reader that loads what its blocks need (spans of the file / blocks through the index) gets ONE run of
            # consecutive blocks: every rank then reads and inflates its own byte range of the file, not the whole of it
            ranged = (isinstance(bam, DeviceBam) and bam.streamed) or isinstance(bam, IndexedBam)
            results, n_depth, tm = call_blocks_sharded(blocks, run, ref, opts.respect_ref, contiguous=ranged)
        else:
            results, n_depth, tm = run(blocks)
    finally:
        fe_kernel_s = bam.kernel_s() if isinstance(bam, DeviceBam) else None
        if own_reader and isinstance(bam, DeviceBam):
            bam.close()             # gigabytes of device memory: not left to the garbage collector
    errors = tm.pop("errors", [])
    if getattr(opts, "annotation_file", None):      # on the merged rows: the annotations depend on the catalog and the file only
        from .annotations import annotate_rows
        on_device = isinstance(bam, DeviceBam)
        tm.update(annotate_rows(results, opts.annotation_file, "device" if on_device else "host", getattr(bam, "device", 0) if on_device else 0))
    tm["ref_side_s"] = tm.get("ref_side_s", 0.0) + tm_pre.get("ref_side_s", 0.0)
    tm["open_s"] = t_open
    if own_reader and isinstance(bam, DeviceBam):
        tm["open_wait_s"] = t_wait              # what this thread still waited for the reader after catalog + reference side
    tm["front_end"] = "device" if isinstance(bam, DeviceBam) else "host"
    if isinstance(bam, DeviceBam) and bam.streamed:      # this rank's own share of the file (compressed bytes read, uploaded, inflated)
        tm["front_end_compressed_mb"] = bam.open_stage_s.get("compressed_mb", 0.0)
        tm["front_end_spans"] = bam.open_stage_s.get("spans", 0)
    if fe_kernel_s is not None:
        tm["front_end_device_s"] = fe_kernel_s      # inflation + record scan + extraction kernels (HIP events)
        tm["open_stage_s"] = dict(getattr(bam, "open_stage_s", {}))
    # same top-level layout as the reference's report (strkit/call/output/json_report.py:37-60,127-154)
    return {"sample_id": sample_id,
            "caller": {"name": "strkit_amd", "version": _lib.load().strk_version().decode()},
            "parameters": report_parameters(opts, processes),
            "contigs": sorted({r["contig"] for r in results}),
            "catalog": {"num_loci": len(results), "num_loci_unknown_contig": n_catalog - n_loaded,
                        **({"num_loci_ploidy_ignored": n_ploidy_ignored} if getattr(opts, "ploidy", None) is not None else {})},
            "results": results,
            "errors": errors,
            "avg_read_depth": n_depth / max(1, sum(1 for r in results if "reads" in r)),
            "runtime": time.perf_counter() - t0, "stage_times": {k: (round(v, 4) if isinstance(v, float) else v) for k, v in tm.items()}}


@contextmanager
def _phase_run_closed(phase_run, tm):
    try:
        yield
    finally:
        if phase_run is not None:
            phase_run.close(tm)


def _one_contig_blocks(block):
    """A block as the loader builds it stays on one contig (loci.py:277-280); a hand-made one is split."""
    return [list(run) for _, run in itertools.groupby(block, key=lambda locus: locus.contig)]


def _span_feed(blocks, bam, tm):
    # a file larger than device memory: span by span through HBM (DeviceBam.plan / load_span)
    tm["load_s"] = 0.0
    for contig, beg, end, group in bam.plan([b for blk in blocks for b in _one_contig_blocks(blk)]):
        t0 = time.perf_counter()
        bam.load_span(contig, beg, end)
        tm["load_s"] += time.perf_counter() - t0
        for block in group:
            yield block, bam


class _PrefetchFeed:
    # Block-wise access through the index: the records of block k + 1 are inflated (all host cores, outside the GIL) while
    # block k is being called; memory holds three blocks' worth of the alignment file, never the file.  The first block is
    # requested at once: its records are being inflated while the caller computes the reference side.

    def __init__(self, blocks, bam, tm):
        self.blocks = [b for blk in blocks for b in _one_contig_blocks(blk)]
        self.bam, self.tm = bam, tm
        tm["load_s"] = tm["load_wait_s"] = 0.0
        self.pool = ThreadPoolExecutor(1)
        self.fut = self.pool.submit(self._load, 0) if self.blocks else None

    def _load(self, k):
        t0 = time.perf_counter()
        block = self.blocks[k]
        # (three buffers in rotation: the block being called, the one being loaded, and one of slack)
        reg = self.bam.region(block[0].contig, min(l.left_flank_coord for l in block), max(l.right_flank_coord for l in block) + 1,
                              slot=k % 3)
        return reg, time.perf_counter() - t0

    def __iter__(self):
        for k, block in enumerate(self.blocks):
            t0 = time.perf_counter()
            records, dt = self.fut.result()
            self.tm["load_wait_s"] += time.perf_counter() - t0
            self.tm["load_s"] += dt
            self.fut = self.pool.submit(self._load, k + 1) if k + 1 < len(self.blocks) else None
            yield block, records

    def close(self):
        self.pool.shutdown(wait=True)


def call_blocks(blocks, bam: BamFile, ref: Fasta, opts: CallOptions | None = None, ctx=None, ref_cache: dict | None = None,
                ps_ids: dict | None = None):
    """Worker loop over blocks of loci (strkit/call/call_sample.py:103-197): (results in locus order, reads kept,
    stage times).  An error of the library inside a block is handled the way the reference's worker handles any
    exception of call_locus (call_sample.py:159-166: logged, the locus is dropped, the run goes on): the block is
    re-run locus by locus so that only the locus that fails is lost; `stage times["errors"]` lists them.  `ps_ids` (a dict,
    with use_hp): filled with {phase-set number in the rows: original PS value, -1 for reads with HP and no PS}."""
    opts = opts or CallOptions()
    opts.validate()
    blocks, _ = ploidy_blocks(blocks, opts)
    # the candidate SNVs and the renumbering of the phase sets: one per run (an indexed SNV file is read where the alignments are)
    phase_run = PhaseRun(opts, device=getattr(bam, "device", 0) if isinstance(bam, DeviceBam) else None, ref=ref) if phased(opts) else None
    sets = phase_run.sets if phase_run is not None else None      # (snv_phase_sets: phase sets across loci, phase_sets.py)
    ctx = ctx or _lib.default_context()
    run_block = _call_block_native if isinstance(bam, (NativeBam, IndexedBam, DeviceBam)) else _call_block_python
    results: list[dict] = []
    n_depth = 0
    tm = {"ref_side_s": 0.0, "realign_s": 0.0, "extract_s": 0.0, "count_s": 0.0, "errors": []}

    def safe(block, records):
        nonlocal n_depth
        ids = None
        try:
            t_a = time.perf_counter()      # (a chunk of the reference side that failed is computed again here, block by block)
            ref_data = ([ref_cache[id(l)] for l in block] if all(id(l) in ref_cache for l in block)
                        else get_loci_with_ref_data(block, ref, opts.respect_ref, ctx))
            tm["ref_side_s"] += time.perf_counter() - t_a
            ids = phase_run.snapshot() if phase_run is not None else None
            # (without a switch of PhasedCallOptions the block paths are called as they always were)
            rows, n = run_block(block, records, opts, ctx, tm, ref_data, **({"phase_run": phase_run} if phase_run is not None else {}))
        except _lib.StrkError as e:
            if ids is not None:     # the phase sets a failed block has numbered are numbered again by its re-run, from where it began
                phase_run.restore(ids)
            if len(block) > 1:
                for locus in block:
                    safe([locus], records)
                return
            print(f"strkit_amd: {block[0].log_str()} - skipping locus: {e}", file=sys.stderr)
            tm["errors"].append({"locus_index": block[0].t_idx, "error": str(e)})
            return
        results.extend(rows)
        n_depth += n

    if isinstance(bam, IndexedBam):
        feed = _PrefetchFeed(blocks, bam, tm)
    elif isinstance(bam, DeviceBam) and bam.streamed:
        feed = _span_feed(blocks, bam, tm)
    elif sets is not None:          # (a hand-made block that mixes contigs is split, as the two feeds above split it)
        feed = ((b, bam) for block in blocks for b in _one_contig_blocks(block))
    else:
        feed = ((block, bam) for block in blocks)       # a reader that holds every record
    # a feed is a generator or has a close() of its own (the prefetcher's pool); the phase run gives its SNV reader back
    with closing(feed), _phase_run_closed(phase_run, tm):
        if ref_cache is None:       # reference side of ALL loci first (unless the caller has it already)
            ref_cache = ref_side_of_blocks(blocks, ref, opts, ctx, tm)
        with _collector_paused():
            # snv_phase_sets: all three feeds hand the blocks on in the order of `blocks`, the catalog's (PhaseSets.enter
            # refuses any other); when the contig changes, and at the end, the finished contig's rows get their fix-up
            contig, first_row = None, 0
            for block, records in feed:
                if sets is not None and block[0].contig != contig:
                    sets.finish_contig(results[first_row:])
                    contig, first_row = block[0].contig, len(results)
                safe(block, records)
            if sets is not None:
                sets.finish_contig(results[first_row:])
                tm["phase_sets_s"] = sets.seconds
            if ps_ids is not None and phase_run is not None:
                ps_ids.update(phase_run.remap.originals())
    results.sort(key=lambda r: r["locus_index"])
    return results, n_depth, tm


def write_json(report: dict, path: str) -> None:
    with open(path, "w") as fh:
        json.dump(report, fh, indent=1)
