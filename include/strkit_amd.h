/*
 * strkit_amd.h — C ABI of the MI355X (gfx950) repeat-count backend for STRkit's `strkit call`.
 *
 * This is the drop-in boundary for the per-read repeat-count hot path.  Reference call sites
 * (paths relative to the STRkit tree) each entry point replaces:
 *
 *   strk_repeat_count        strkit_rust_ext.get_repeat_count(start, tr, fl, fr, motif, max_iters,
 *                            local_search_range, step_size, use_shortcuts=False)
 *                            — strkit/call/repeats.py:58-68 (import at repeats.py:7)
 *   strk_count_loci[_device] the per-read loop of call_locus() that calls get_repeat_count once per
 *                            read with the running start-count feedback
 *                            — strkit/call/call_locus.py:1082,1125-1161; sharded over workers at
 *                            strkit/call/call_sample.py:103-138,414
 *   strk_submit_loci_device / strk_finish   the same loop, split so that successive blocks of loci
 *                            overlap on the device (the reference overlaps them across its worker
 *                            processes, strkit/call/call_sample.py:414)
 *   strk_ref_repeat_count    get_ref_repeat_count() incl. score_ref_boundaries(), once per locus
 *                            — strkit/call/repeats.py:23-43,73-192 (parasail sg_qe_scan_profile_sat);
 *                            strk_score_ref_table is its scoring primitive
 *   strk_ref_repeat_count_batch  the same for every locus of a block (call_locus.py:796-810 once per locus)
 *   strk_realign             the parasail sg_dx_trace_scan_16 call + CIGAR of realign_read()
 *                            — strkit/call/realign.py:56-72 (gate at realign.py:65, caller call_locus.py:867-901)
 *   strk_score_table         one parasail semi-global alignment score per candidate copy number
 *                            (the innermost operation; shape of strkit/call/repeats.py:33,40,124)
 *
 * Conventions: plain pointers and sizes, caller-owned buffers, no allocation crosses the ABI
 * except the opaque context.  Every function returns 0 on success or a negative STRK_E_* code;
 * strk_last_error() returns a thread-local message.  A context is bound to one HIP device and
 * must be used from one host thread at a time; it is created lazily inside a worker process
 * (fork-safe: nothing touches HIP before strk_init).
 *
 * Sequences are 1 byte per base, ASCII over ACGT + IUPAC codes + 'X' (low-quality wildcard),
 * case-insensitive (strkit/call/align_matrix.py:25-39).  Scoring is the reference's: match +2,
 * mismatch -7, gap 5 per base (align_matrix.py:15-17).
 */
#ifndef STRKIT_AMD_H
#define STRKIT_AMD_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define STRK_OK 0
#define STRK_E_INVALID (-22) /* bad argument (EINVAL) */
#define STRK_E_NOMEM (-12)   /* device or host allocation failed (ENOMEM); also: an input beyond what the scratch parts may grow
                                to (a window of more than 2^20 candidate rows, 32 GiB of generic-kernel rows) — strk_last_error()
                                says which.  Scratch that is merely too small for a call grows and the call runs again. */
#define STRK_E_DEVICE (-5)   /* HIP runtime / kernel failure (EIO) */
#define STRK_E_NODEV (-19)   /* no usable gfx950 device (ENODEV) */
#define STRK_E_EMPTY (-61)   /* nothing could be scored (Python's max() of an empty dict) */

/* end-gap flags; s1 = the read window fl+tr+fr, s2 = the candidate fl+motif*i+fr */
#define STRK_DB_BEG_FREE 1
#define STRK_DB_END_FREE 2
#define STRK_CAND_BEG_FREE 4
#define STRK_CAND_END_FREE 8
#define STRK_SG_ALL 15

#define STRK_TIE_FIRST 0 /* Python max(): first maximal element (repeats.py:135,154) */
#define STRK_TIE_LAST 1
#define STRK_NARROW_NONE 0       /* local_search_range fixed for the whole search (repeats.py:100-151) */
#define STRK_NARROW_DECREMENT 1  /* one less after every explored stack entry, never below 1 */
#define STRK_NARROW_HALVE 2      /* halved after every explored stack entry, never below 1 */
#define STRK_NARROW_AFTER_SEED 3 /* the three seed entries use it as given, every chased entry 1 */

typedef struct strk_ctx strk_ctx;

/* Search parameters = RepeatCountParams (strkit/call/repeat_count_params.py:9-14) + the two
 * semantic switches the un-vendored Rust crate leaves open (see DESIGN.md "parity unpinned"). */
typedef struct strk_params {
    int32_t max_iters;          /* rc_params.max_iters                (params.py:45  -> 50) */
    int32_t local_search_range; /* rc_params.initial_local_search_range (params.py:26 -> 3) */
    int32_t step_size;          /* rc_params.initial_step_size          (params.py:27 -> 1)
                                   The reference calls both INITIAL values that "can be narrowed within the
                                   get_repeat_count fn" (repeat_count_params.py:14); that function is in the un-vendored
                                   Rust crate, so here they stay fixed for the whole search, as in the in-tree sibling
                                   get_ref_repeat_count (repeats.py:100-151): a third unpinned choice next to tie_rule
                                   and end_flags; a different schedule would change
                                   search_replay() only, the score table is schedule-independent. */
    int32_t tie_rule;           /* STRK_TIE_FIRST */
    int32_t end_flags;          /* STRK_SG_ALL */
    int32_t feedback;           /* 1: start-count feedback across the reads of a locus
                                   (call_locus.py:1129-1136,1161); 0: start = est_cn as given */
    int32_t window;             /* half-width of the speculative score table per read; 0 = default */
    int32_t no_dedupe;          /* 0 (default): reads of a locus with identical bytes, split and estimate
                                   share one score table (the reference's lru_cache, repeats.py:47);
                                   1: score every read separately */
    int32_t no_band;            /* 0 (default): reads whose window is much wider than the band the search can
                                   reach are scored by the banded kernel first and re-scored exactly only when
                                   the exactness certificate fails; 1: exact kernels only */
    int32_t narrowing;          /* schedule by which local_search_range / step_size shrink inside one search
                                   (repeat_count_params.py:14: "can be narrowed within the get_repeat_count fn").
                                   STRK_NARROW_NONE (0): fixed for the whole search, as get_ref_repeat_count does
                                   (repeats.py:100-151) — the only schedule the tree states, and the default.  The Rust
                                   function's own schedule is not in the tree; STRK_NARROW_DECREMENT / _HALVE / _AFTER_SEED
                                   are the plausible forms (strk_search.h: LsrSchedule; step_size stays fixed in all of
                                   them), there so that reference vectors (tests/test_reference_vectors.py) or a report
                                   diff (tools/compare_strkit_json.py) can name the one that fits.  Other values:
                                   STRK_E_INVALID.  The scalar entry point strk_repeat_count always runs STRK_NARROW_NONE. */
} strk_params;

/* CSR-packed batch of loci.  Read r owns seqs[seq_off[r] .. seq_off[r+1]) laid out fl|tr|fr;
 * locus l owns reads read_off[l] .. read_off[l+1] (in caller order) and motif
 * motifs[motif_off[l] .. motif_off[l+1]).  est_cn[r] is the caller's integer start estimate
 * (get_est_copy_num(), call_locus.py:1129). */
typedef struct strk_batch {
    int32_t n_reads;
    int32_t n_loci;
    const uint8_t* seqs;
    const int64_t* seq_off; /* [n_reads + 1] */
    const int32_t* nfl;     /* [n_reads] */
    const int32_t* ntr;
    const int32_t* nfr;
    const int32_t* est_cn;
    const int32_t* read_off;  /* [n_loci + 1] */
    const uint8_t* motifs;
    const int32_t* motif_off; /* [n_loci + 1] */
} strk_batch;

/* Per-call statistics (all optional output).  The field comments describe strk_count_loci and its kin; the entry points that
 * are not about reads (strk_realign, strk_call_alleles, strk_best_representatives, strk_count_kmers) fill a few of the fields
 * with meanings of their own, named in each function's comment (strk_count_kmers: dp_cells = windows, n_fallback = groups
 * that spilled, n_miss_reads = groups on the general path, n_sub_batches = launches of the sort kernel). */
typedef struct strk_stats {
    int64_t dp_cells;      /* DP cell updates executed by the device kernels */
    int32_t n_fallback;    /* reads scored by the generic (non-systolic) kernel */
    int32_t n_miss_reads;  /* reads whose search left the speculative window (re-scored) */
    int32_t n_miss_rounds; /* extra launch rounds needed to resolve them */
    float kernel_ms;       /* HIP-event time of the device work of this call */
    float dp_kernel_ms;    /* ... of the exact DP kernel (k_dp_all) alone */
    int32_t n_dp_launches;
    int32_t n_dedup_reads; /* reads served by the score table of an identical earlier read */
    int32_t n_band_reads;  /* reads scored by the banded kernel ... */
    int32_t n_band_fallback; /* ... of which the certificate failed (re-scored by the exact kernels) */
    float band_kernel_ms;  /* HIP-event time of the banded kernel (k_dp_band) of this call */
    int32_t window_used;   /* half-width of the speculative candidate window this call ran with (params.window, or the
                              level the library's default has adapted to) */
    int64_t band_bytes;    /* algorithmic bytes (|window| + 16 per read) of the reads k_plan routed to k_dp_band / k_dp_band_wide */
    int64_t exact_bytes;   /* ... and to the exact kernels (k_dp_all / k_dp_long / generic) */
    float band_wide_kernel_ms; /* HIP-event time of k_dp_band_wide (band classes 2, 3: long windows) */
    float long_kernel_ms;      /* ... of k_dp_long (column-tiled exact kernel) */
    float generic_kernel_ms;   /* ... of k_dp_generic */
    float head_ms;             /* ... of what precedes the DP kernels (k_hash, k_plan) */
    float replay_ms;           /* ... of k_replay */
    int32_t n_long_reads;      /* reads scored by k_dp_long */
    int64_t wide_bytes;        /* algorithmic bytes of the reads routed to k_dp_band_wide (part of band_bytes) */
    int64_t long_bytes;        /* ... to k_dp_long (part of exact_bytes) */
    int64_t band_cells;        /* dp_cells by the kernel that executed them: k_dp_band (band classes of 8 and 16 lanes per read), */
    int64_t wide_cells;        /* ... k_dp_band_wide (32 and 64 lanes), */
    int64_t exact_cells;       /* ... k_dp_all / k_dp_ref, */
    int64_t long_cells;        /* ... k_dp_long; the remainder of dp_cells is the generic kernel's */
    int32_t window_bucket[5];  /* candidate-window half-width per motif-length bucket (1-2, 3-4, 5-6, 7-10, 11+ bases) this call
                                  ran with; 0: the call held no locus of that bucket */
    int32_t n_sub_batches;     /* strk_count_loci on host buffers: sub-batches the call was cut into (0: one piece) */
} strk_stats;
/* strk_count_loci on large HOST batches runs as a pipeline of sub-batches on two contexts (csrc/strk_host_pipe.inc): the *_ms
 * fields, *_bytes, *_cells and the n_* counts are then SUMS over the sub-batches — sub-batches overlap, so the sum of their
 * device times can exceed the call's wall time (it is not a throughput denominator); window_used / window_bucket are the last
 * sub-batch's.  Device-resident entry points (strk_count_loci_device, strk_submit_loci_device + strk_finish) report one call. */

int strk_init(int device, strk_ctx** out);
void strk_destroy(strk_ctx* ctx);
const char* strk_last_error(void);
const char* strk_version(void);
/* Consecutive reads whose band items the planning kernel lists in one order, by (band class, prefix rows), in a call of n_reads
 * reads (small calls use a smaller scope).  For tests and tools that place reads around a block edge. */
int32_t strk_plan_scope(int32_t n_reads);
/* The reads of one band class (0..7) in the order the planning kernel of ctx's last batched call listed them: up to `cap`
 * read indices into out_reads (host memory); returns the length of the list (>= 0) or an error.  For tests of the list
 * order; valid until the next call on ctx. */
int strk_band_list(strk_ctx* ctx, int32_t band_class, int32_t* out_reads, int32_t cap);
/* Test support for the exact scoring path.  strk_classify: the list the planning kernel gives an item of these lengths, candidate
 * window [lo, lo + n) and mode: 0..16 the fast classes, 17 the column-tiled kernel, 18 the generic kernel (the device's own
 * function, compiled for the host).  strk_score_constants: up to `cap` of {kTableMax, kFastFlankMax, kMotifMax, kRowSlack,
 * kNumClasses, kLongTile, kLongMaxTiles, kLongFlankMax, kStairMinG, the 17 class capacities, the 17 lanes-per-read values}.
 * strk_class_counts: the lengths of those 19 lists in ctx's last finished scoring call, from the counters that call downloaded
 * (an item the fast or the tiled kernel hands over to the generic one is counted in both lists); up to `cap` of them into out,
 * returns 19 (0 while a submitted call is pending; all lists empty before the first call) or an error. */
int32_t strk_classify(int32_t nfl, int32_t ntr, int32_t nfr, int32_t m, int32_t lo, int32_t n, int32_t force_generic, int32_t ref_mode);
void strk_score_constants(int32_t* out, int32_t cap);
int strk_class_counts(strk_ctx* ctx, int32_t* out, int32_t cap);
/* Test support for the band pass ("Band path: seam corpus"): what k_dp_band and k_dp_band_wide write, on HOST buffers.
 * Plans the batch as a counting call does (candidate window est_cn +- params->window, which must be > 0: the adaptive default is
 * not consulted) with the band on for every read (no probation, no dedupe) and the band placement tune[3] = {span_w, slack_m8,
 * max_m} (all zeros: the library's defaults), runs the planning kernel and the two band kernels and nothing behind them (no
 * replay pass, no exact kernel), and returns per read r the window (out_lo[r], out_n[r]), out_class[r] and, for a read a band
 * class scored, the band scores and their bounds in out_scores / out_ub[r * table_stride .. + out_n[r]).  out_class: 0..7 the band
 * class that scored the read; -1 the band geometry refuses it; -2 the band kernel handed it on for a symbol outside its six fixed
 * classes; the rows of both kinds are left as the caller filled them.  flags & 1: order the wide classes longest first (two more
 * kernels) as a counting call may.  Only params->window and params->end_flags are used.  The context's band probation, grid
 * history and the process's window level are neither read nor changed; the call does use the context's workspace, staging
 * buffer and class lists like any scoring call, so strk_band_list afterwards reports THIS call's lists (strk_class_counts keeps
 * the counters of the last finished scoring call).  Refuses a context with a submitted call pending. */
int strk_band_tables(strk_ctx* ctx, const strk_batch* batch, const strk_params* params, const int32_t* tune, int32_t flags,
                     int32_t* out_lo, int32_t* out_n, int32_t* out_class, int32_t table_stride, int32_t* out_scores,
                     int32_t* out_ub, strk_stats* stats);
/* Forget what the library has learnt about the current sample (the default candidate-window level per motif-length bucket,
 * process-wide): call it when a process moves on to ANOTHER sample (the reference runs one sample per process,
 * call_sample.py:265).  Per-context state (band probation, grid history) goes with strk_destroy. */
void strk_adaptive_reset(void);
/* free / total memory of a device in bytes (hipMemGetInfo): how the file front end decides whether an alignment file's
 * decompressed form stays resident or is streamed in spans. */
int strk_device_mem(int device, int64_t* free_bytes, int64_t* total_bytes);
/* Page-locks (hipHostRegister) / releases a host buffer the caller owns.  strk_count_loci copies the bases (batch.seqs) of a
 * batch to the device by DMA straight from the caller's array when that lies in registered (or hipHostMalloc'ed) memory — no
 * staging copy through the library's own pinned blocks, which is what bounds the pageable path (the reference's worker would
 * register the per-block array it reuses, call_sample.py:103-138).  Registering costs a few milliseconds per 100 MB: worth
 * it for buffers that are reused. */
int strk_host_register(void* ptr, int64_t bytes);
int strk_host_unregister(void* ptr);
/* 1 if [ptr, ptr + bytes) is page-locked host memory the library would read in place, 0 if not. */
int strk_host_is_pinned(const void* ptr, int64_t bytes);

/* Scalar drop-in for strkit_rust_ext.get_repeat_count (repeats.py:58-68).  Return contract
 * (repeats.py:55-56): ((out_cn, out_score), out_n_explored, out_cn - start_count). */
int strk_repeat_count(strk_ctx* ctx, int32_t start_count, const uint8_t* tr, int32_t tr_len,
                      const uint8_t* fl, int32_t fl_len, const uint8_t* fr, int32_t fr_len,
                      const uint8_t* motif, int32_t motif_len, int32_t max_iters,
                      int32_t local_search_range, int32_t step_size, int32_t* out_cn,
                      int32_t* out_score, int32_t* out_n_explored);

/* Batched per-locus path, HOST buffers in and out (all out_* are [n_reads] int32). */
int strk_count_loci(strk_ctx* ctx, const strk_batch* batch, const strk_params* params,
                    int32_t* out_cn, int32_t* out_score, int32_t* out_n_iters, int32_t* out_start,
                    strk_stats* stats);

/* Same, every pointer inside `batch` and every out_* pointer is DEVICE memory on ctx's device;
 * work is enqueued on `stream` (a hipStream_t, NULL = default stream) and the call returns after
 * the results are complete in out_* (it synchronises the stream once to check for window misses). */
int strk_count_loci_device(strk_ctx* ctx, const strk_batch* batch, const strk_params* params,
                           int32_t* out_cn, int32_t* out_score, int32_t* out_n_iters,
                           int32_t* out_start, void* stream, strk_stats* stats);

/* Pipelined form of strk_count_loci_device: strk_submit_loci_device enqueues the whole call on
 * `stream` and returns at once; strk_finish waits for it, resolves window misses and fills `stats`.
 * One call may be in flight per context (use one context per stream to overlap batches); every
 * pointer inside `batch` and every out_* pointer must stay valid until strk_finish returns. */
int strk_submit_loci_device(strk_ctx* ctx, const strk_batch* batch, const strk_params* params,
                            int32_t* out_cn, int32_t* out_score, int32_t* out_n_iters,
                            int32_t* out_start, void* stream);
int strk_finish(strk_ctx* ctx, strk_stats* stats);

/* Parity primitive: scores[table_off[r] + k] = semi-global score of (fl + motif*(lo[r]+k) + fr)
 * against (fl+tr+fr) for k < n[r].  HOST buffers.  table_off is [n_reads + 1]. */
int strk_score_table(strk_ctx* ctx, const strk_batch* batch, const int32_t* lo, const int32_t* n,
                     const int64_t* table_off, int32_t end_flags, int32_t force_generic,
                     int32_t* scores, strk_stats* stats);

/* Reference-side primitive (score_ref_boundaries, repeats.py:23-43): for k < n[r],
 * scores[table_off[r] + k] / end_query[...] = parasail sg_qe score and query end of the candidate
 * fl + motif*(lo[r]+k) (NO right flank) against the window fl+tr+fr whose end is free.  For the
 * reversed alignment pass the reversed window with the flanks swapped and the reversed motif.  HOST buffers. */
int strk_score_ref_table(strk_ctx* ctx, const strk_batch* batch, const int32_t* lo, const int32_t* n,
                         const int64_t* table_off, int32_t force_generic, int32_t* scores,
                         int32_t* end_query, strk_stats* stats);

/* Drop-in for get_ref_repeat_count (repeats.py:73-192), once per locus: boundary-extension search
 * + final count.  out9 = {cn, score, l_offset, r_offset, n_offset_scores, n_iters_final,
 * new fl_len, new tr_len, new fr_len} (the bases never change, only where the flank/tract
 * boundaries fall inside fl|tr|fr). */
int strk_ref_repeat_count(strk_ctx* ctx, int32_t start_count, const uint8_t* tr, int32_t tr_len,
                          const uint8_t* fl, int32_t fl_len, const uint8_t* fr, int32_t fr_len,
                          const uint8_t* motif, int32_t motif_len, int32_t ref_size,
                          int32_t vcf_anchor_size, int32_t max_iters, int32_t local_search_range,
                          int32_t step_size, int32_t respect_coords, int32_t* out9);

/* strk_ref_repeat_count for a block of loci in lock-step: every round of boundary-extension scoring is one device
 * call for all loci that still need scores, the final counts one call per distinct search schedule.  Locus i owns
 * seqs[seq_off[i] .. seq_off[i+1]) laid out fl|tr|fr and motifs[motif_off[i] .. motif_off[i+1]); max_iters /
 * local_search_range / step_size are per locus (get_reference_rc_params, repeat_count_params.py:17-42, depends on
 * the estimate).  out9 is [n_loci * 9], fields as strk_ref_repeat_count.  HOST buffers. */
int strk_ref_repeat_count_batch(strk_ctx* ctx, int32_t n_loci, const int32_t* start_count, const uint8_t* seqs,
                                const int64_t* seq_off, const int32_t* nfl, const int32_t* ntr, const int32_t* nfr,
                                const uint8_t* motifs, const int32_t* motif_off, const int32_t* ref_size,
                                int32_t vcf_anchor_size, const int32_t* max_iters, const int32_t* local_search_range,
                                const int32_t* step_size, int32_t respect_coords, int32_t* out9);

/* Batched drop-in for the parasail call of realign_read (strkit/call/realign.py:56-63,71):
 * sg_dx_trace_scan_16(s1 = reference window, s2 = wildcarded read, open, extend, dna_matrix) — s1 aligned end
 * to end, both ends of s2 free, a gap of length k costs open + (k-1)*extend (the reference passes 7 and 0).
 * Pair p owns s1[s1_off[p] .. s1_off[p+1]) and s2[s2_off[p] .. s2_off[p+1]); HOST buffers.
 * Outputs per pair: out_score = pr.score; out_end_ref = 0-based s2 position of the last aligned base
 * (pr.end_ref); the CIGAR of pr.cigar.seq in BAM encoding (len << 4 | op, ops "MIDNSHP=X": I consumes s1,
 * D consumes s2), written to cigar[cigar_off[p] ..] with out_n_cigar[p] runs; it starts at s2 position 0
 * (free leading s2 bases are one D run) and ends at out_end_ref.  2*|s1| + 4 runs always suffice.
 * gap_pref: which gap kind wins an exact score tie after the diagonal (0: I before D, the default; 1: D before I).
 * Accepted: 0 <= extend <= open <= 4096, 1 <= |s1| <= 2^20, 1 <= |s2| <= 2^24 and, per pair,
 * 2*open + (|s1| - 2)*extend < 2^24 (what the kernel's 28-bit scores hold: strk_realign.h at kRealignNeg).  Every accepted
 * pair is exact; anything else is STRK_E_INVALID before any launch, with the pair named in strk_last_error().  A CIGAR range
 * too small for its pair's runs is STRK_E_INVALID as well, found after the launch: nothing is written outside the pairs' ranges.
 * stats (optional): kernel_ms, dp_cells, exact_bytes = trace bytes written. */
int strk_realign(strk_ctx* ctx, int32_t n_pairs, const uint8_t* s1, const int64_t* s1_off, const uint8_t* s2,
                 const int64_t* s2_off, int32_t open, int32_t extend, int32_t gap_pref, int32_t* out_score,
                 int32_t* out_end_ref, int32_t* out_n_cigar, uint32_t* cigar, const int64_t* cigar_off,
                 strk_stats* stats);

/* What parasail's fixed 16-bit kernel (sg_dx_trace_scan_16, strkit/call/realign.py:56) would have done with these pairs:
 * strk_realign computes in 32 bits and never saturates, the reference's call can.  Per pair out_flags[p] =
 *   STRK_I16_SCORE_SATURATES (2)  the final score itself exceeds what the 16-bit kernel can hold (> 32767 - 2, the matrix
 *                                 maximum is kept as head-room): parasail would return a saturated result and
 *                                 realign_read would compare garbage with its threshold (realign.py:65);
 *   STRK_I16_CELL_MAY_SATURATE (1) the score fits, but an intermediate cell can reach the limit (2 * min(|s1|, |s2|) > 32765):
 *                                 whether the reference's result is affected cannot be told from the score alone;
 *   0                              no cell can reach the limit (every window of at most 16 382 bases).
 * Pure host arithmetic on the lengths and on strk_realign's scores; no context. */
#define STRK_I16_CELL_MAY_SATURATE 1
#define STRK_I16_SCORE_SATURATES 2
int strk_realign_i16_flags(int32_t n_pairs, const int64_t* s1_off, const int64_t* s2_off, const int32_t* scores,
                           int32_t* out_flags);

/* ---- allele calling ------------------------------------------------------------------------------------------------
 * Drop-in for call_alleles (strkit/call/allele.py:176-336) and the distance-based peak assignment of call_locus.py
 * (1536-1600): per locus, num_bootstrap weighted resamples of the read copy numbers, a k-means++-seeded spherical GMM
 * fit per resample (sklearn 1.7's EM), medians and percentiles across resamples, then every read's peak.  The random
 * stream is the library's own, seeded per locus by seed[l]; it does not reproduce numpy's Generator.
 * Defaults: min_reads 4, min_allele_reads 2, num_bootstrap 100, n_init 3, max_iter 100, filter_factor 3,
 * force_gm_filter 0, tol 1e-3, reg_covar 1e-6, expansion_ratio 5.0. */
typedef struct strk_allele_params {
    int32_t min_reads, min_allele_reads, num_bootstrap, n_init, max_iter, filter_factor, force_gm_filter, pad;
    double tol, reg_covar, expansion_ratio;
} strk_allele_params;

#define STRK_ALLELE_CALLED 0
#define STRK_ALLELE_TOO_FEW 1    /* fewer than min_reads reads: no call */
#define STRK_ALLELE_EMPTY_PEAK 2 /* a peak got no read (the reference nullifies such a call); every output is still set */

/* Locus l owns reads read_off[l] .. read_off[l+1] (copy number cn[r], weight w[r] > 0, at most 65 535 reads) and has
 * n_alleles[l] in {1, 2}.  All buffers are host buffers.  Per locus: out_status, out_modal_n; per allele a (2 slots per
 * locus, slot 1 unused when n_alleles is 1): out_call[2l+a], out_ci95[4l+2a .. +1] and out_ci99 (lo, hi), out_means,
 * out_weights, out_stdevs, out_peak_n_reads[2l+a]; per read: out_read_peak (-1 when no call).  Unused integer slots
 * are -1 (peak counts 0), unused doubles NaN.  num_bootstrap must be 2..1024, n_init 1..15 and reg_covar > 0; every
 * input is checked before the first launch.  stats (optional) receives kernel_ms. */
int strk_call_alleles(strk_ctx* ctx, int32_t n_loci, const int32_t* read_off /*[n_loci+1]*/, const int32_t* cn, const double* w,
                      const int32_t* n_alleles, const uint64_t* seed, const strk_allele_params* p,
                      int32_t* out_status, int32_t* out_modal_n, int32_t* out_call /*[2n]*/, int32_t* out_ci95 /*[4n]*/,
                      int32_t* out_ci99 /*[4n]*/, double* out_means, double* out_weights, double* out_stdevs /*[2n]*/,
                      int32_t* out_peak_n_reads /*[2n]*/, int32_t* out_read_peak /*[n_reads], -1 = none*/, strk_stats* stats);

/* ---- allele calling with one to six alleles per locus -------------------------------------------------------------------
 * strk_call_alleles for n_alleles[l] in 1 .. STRK_MAX_ALLELES (a ploidy configuration may give any count, strkit/ploidy.py):
 * a GMM of n_alleles components per resample whose useless components are removed round by round (allele.py:78-123) and
 * filled up again by a weighted draw (:276-288).  The whole rule: DESIGN.md §15.  For n_alleles <= 2 the results are those
 * of strk_call_alleles, byte for byte.  A locus with more than one distinct copy number and fewer reads than alleles is
 * STRK_ALLELE_TOO_FEW.  Reads get a peak only when at most two peaks are called (out_modal_n <= 2, on the first out_modal_n
 * rows); otherwise out_read_peak is -1, out_peak_n_reads 0 and the status STRK_ALLELE_CALLED.
 * Inputs and checks as strk_call_alleles.  The per-locus outputs have a fixed row stride of STRK_MAX_ALLELES:
 * out_call[6l+a], out_ci95[12l+2a .. +1] and out_ci99, out_means, out_weights, out_stdevs [6l+a]; out_peak_n_reads[2l+peak];
 * unused integer slots are -1, unused doubles NaN. */
#define STRK_MAX_ALLELES 6
int strk_call_alleles_n(strk_ctx* ctx, int32_t n_loci, const int32_t* read_off /*[n_loci+1]*/, const int32_t* cn, const double* w,
                        const int32_t* n_alleles, const uint64_t* seed, const strk_allele_params* p,
                        int32_t* out_status, int32_t* out_modal_n, int32_t* out_call /*[6n]*/, int32_t* out_ci95 /*[12n]*/,
                        int32_t* out_ci99 /*[12n]*/, double* out_means, double* out_weights, double* out_stdevs /*[6n]*/,
                        int32_t* out_peak_n_reads /*[2n]*/, int32_t* out_read_peak /*[n_reads], -1 = none*/, strk_stats* stats);

/* ---- phased allele calls: reads grouped by haplotags or by SNVs -------------------------------------------------------
 * Stands where the reference separates the reads of a locus before it calls alleles (call_locus.py:1381-1495):
 * call_alleles_with_haplotags (:222-288) for reads that carry HP / PS tags, else call_alleles_with_incorporated_snvs
 * (:457-714) for reads that carry useful SNVs, clustered by calculate_read_distance (:91-174) and average linkage cut at
 * two clusters, then call_and_filter_useful_snvs (snvs.py:63-171).  Every group is called as a single-allele locus by the
 * rule of strk_call_alleles (min_reads = min_allele_reads, weights renormalised inside the group, seed
 * mix64(seed[l] + 0x9E3779B97F4A7C15 * (g + 1)) for group g).  The whole rule: DESIGN.md §13.
 * Defaults (the reference's): min_hp_read_coverage 8, snv_quality_threshold 20, many_snvs_quantity 3, cn_weight_few 0.2,
 * cn_weight_many 0.1.  piece_loci and ws_budget (loci and workspace bytes of one piece of the call) are the library's
 * when 0; the result does not depend on them. */
typedef struct strk_phase_params {
    int32_t min_hp_read_coverage, snv_quality_threshold, many_snvs_quantity, piece_loci;
    double cn_weight_few, cn_weight_many;
    int64_t ws_budget;
} strk_phase_params;

#define STRK_ALLELE_NOT_PHASED 3 /* out_status of a locus with enough reads and STRK_ASSIGN_NONE: call it with strk_call_alleles */

#define STRK_ASSIGN_NONE 0       /* no phased call (the reference falls through to `dist` / `single`) */
#define STRK_ASSIGN_HP 1         /* `hp` */
#define STRK_ASSIGN_SNV 2        /* `snv`: SNVs alone */
#define STRK_ASSIGN_SNV_DIST 3   /* `snv+dist`: SNVs and the copy-number difference */

/* out_reason of a locus with STRK_ASSIGN_NONE (0 otherwise, and when the locus has fewer than min_reads reads) */
#define STRK_PHASE_NO_TAGS 1            /* no tags given, and no SNV step possible (one allele, or no SNV) */
#define STRK_PHASE_TAG_THRESHOLDS 2     /* tagged reads, distinct HP values or the top phase set miss their thresholds */
#define STRK_PHASE_FEW_SNV_READS 3      /* too few reads carry a real SNV base */
#define STRK_PHASE_GROUP_NOT_CALLED 4   /* a group has fewer than min_allele_reads reads */
#define STRK_PHASE_NO_SNV_CALLED 5      /* no SNV survived the SNV calls */

/* out_snv_status */
#define STRK_SNV_NOT_EVALUATED (-1)     /* the locus was not grouped by SNVs */
#define STRK_SNV_CALLED 0
#define STRK_SNV_ZERO_TOTAL 1           /* a peak has no cell that counts */
#define STRK_SNV_ONLY_OUT_OF_RANGE 2    /* '-' is a peak's only byte */
#define STRK_SNV_CROSS_TALK 3           /* the other peak carries a peak's byte too often */
#define STRK_SNV_SAME_BASE 4            /* both peaks call the same byte */

/* Inputs as strk_call_alleles, with at most 1 024 reads per locus, and optionally
 *   hp, ps [n_reads]       the reads' haplotag and (already remapped) phase set, -1 = untagged; both NULL or both given;
 *   snv_off [n_loci+1]     locus l has S_l = snv_off[l+1] - snv_off[l] useful SNVs (at most 64); its cells, one base byte and
 *   snv_base, snv_qual     one quality byte per read and SNV, read-major, start at the sum of reads x SNVs of the loci before
 *                          it; n_snv_cells bytes each.  Bases are raw ASCII, '-' out of range, '_' a gap.  All NULL together.
 * Outputs: those of strk_call_alleles in the same layout (a phased call has out_modal_n = the number of groups, weights
 * 1 / groups, out_peak_n_reads the group sizes; peaks in ascending HP order for STRK_ASSIGN_HP, by (mean, low end of the 95 %
 * interval) for the SNV methods; a read outside every group has peak -1), then per locus out_method, out_reason, out_ps (the
 * top phase set for STRK_ASSIGN_HP, else -1), and per SNV out_snv_status, out_snv_call[2s + peak] (bytes),
 * out_snv_rcs[2s + peak] (reads that carry the called byte).  The SNV outputs may be NULL when snv_off is.  A locus without a
 * phased call has the outputs of a locus with too few reads and out_status STRK_ALLELE_NOT_PHASED.  All buffers are host
 * buffers; every input is checked before the first launch.  stats (optional) receives kernel_ms. */
int strk_call_alleles_phased(strk_ctx* ctx, int32_t n_loci, const int32_t* read_off /*[n_loci+1]*/, const int32_t* cn, const double* w,
                             const int32_t* n_alleles, const uint64_t* seed, const strk_allele_params* p, const strk_phase_params* pp,
                             const int32_t* hp, const int32_t* ps, const int32_t* snv_off /*[n_loci+1]*/, const uint8_t* snv_base,
                             const uint8_t* snv_qual, int64_t n_snv_cells,
                             int32_t* out_status, int32_t* out_modal_n, int32_t* out_call /*[2n]*/, int32_t* out_ci95 /*[4n]*/,
                             int32_t* out_ci99 /*[4n]*/, double* out_means, double* out_weights, double* out_stdevs /*[2n]*/,
                             int32_t* out_peak_n_reads /*[2n]*/, int32_t* out_read_peak /*[n_reads]*/, int32_t* out_method,
                             int32_t* out_reason, int32_t* out_ps, int32_t* out_snv_status, uint8_t* out_snv_call /*[2 n_snvs]*/,
                             int32_t* out_snv_rcs /*[2 n_snvs]*/, strk_stats* stats);

/* ---- best representative of a group of sequences ------------------------------------------------------------------
 * Stands where the reference calls strkit_rust_ext.consensus_seq (call_locus.py:1602-1613) for the methods `single` and
 * `best_rep`; partial-order alignment is strk_consensus, below.  A group is an ordered list of byte strings.  No string: index -1,
 * STRK_CONS_NONE.  All strings byte-identical (a group of one included): index 0, STRK_CONS_SINGLE, distance sum 0.
 * Otherwise STRK_CONS_BEST_REP: the smallest i with minimal D(i) = sum over all j of the group of lev(s_i, s_j), lev the
 * unit-cost Levenshtein distance on raw bytes (case-sensitive; an empty string is legal).  Unpinned against STRkit, whose
 * consensus code is not in its tree. */
#define STRK_CONS_NONE 0
#define STRK_CONS_SINGLE 1
#define STRK_CONS_BEST_REP 2
/* Group g owns sequences group_off[g] .. group_off[g+1] (group_off[0] = 0, ascending, at most 250 per group); sequence i is
 * the seq_len[i] (0 .. 65 535) bytes at seqs + seq_start[i], which must lie inside n_seq_bytes; slices may overlap.
 * out_index is the index INSIDE the group.  All buffers are host buffers; every input is checked before the first launch.
 * stats (optional) receives kernel_ms. */
int strk_best_representatives(strk_ctx* ctx, int32_t n_groups, const int32_t* group_off /*[n_groups+1]*/, const uint8_t* seqs,
                              int64_t n_seq_bytes, const int64_t* seq_start, const int32_t* seq_len, int32_t* out_index,
                              int32_t* out_method, int64_t* out_dist_sum, strk_stats* stats);
/* The same with the bases already in memory of the context's device (what strk_dbam_extract leaves behind); everything
 * else on the host. */
int strk_best_representatives_dseqs(strk_ctx* ctx, int32_t n_groups, const int32_t* group_off, const void* d_seqs,
                                    int64_t n_seq_bytes, const int64_t* seq_start, const int32_t* seq_len, int32_t* out_index,
                                    int32_t* out_method, int64_t* out_dist_sum, strk_stats* stats);

/* ---- allele sequence of a group: partial-order alignment where the reads differ --------------------------------------
 * Stands where the reference calls strkit_rust_ext.consensus_seq with its default, POA (call_locus.py:1602-1613).  The
 * method of a group is chosen in this order: no string: STRK_CONS_NONE; all strings byte-identical: STRK_CONS_SINGLE,
 * string 0; the median length (element n / 2 of the ascending lengths) is greater than max_mdn_poa_length:
 * STRK_CONS_BEST_REP, the rule above; the group exceeds a device limit (a string longer than 4 096 bytes, or a graph of more
 * nodes than the node limit, 16 384): STRK_CONS_BEST_REP as well, counted in stats->n_fallback; otherwise STRK_CONS_POA: the
 * heaviest path through the partial-order graph of the group's distinct strings (global alignment with linear gaps, match
 * +5, mismatch -4, gap -8, ties by node number; DESIGN.md §12, the rule in full).  Raw bytes, case-sensitive, any byte value.
 * Unpinned against STRkit, whose POA is not in its tree.
 *
 * Groups and sequences as for strk_best_representatives, and max_mdn_poa_length >= 0.  out_index [n_groups] is the index
 * inside the group for SINGLE / BEST_REP and -1 for POA / NONE; out_method [n_groups]; the sequence of group g, whatever its
 * method, is the bytes out_seq_off[g] .. out_seq_off[g+1] of out_seqs.  Returns the number of bytes B of all sequences, or a
 * negative STRK_E_* code.  out_seq_off [n_groups + 1] is always written, out_seqs [cap] only if B <= cap: cap = 0 with NULL is
 * a size query.  All buffers are host buffers; every input is checked before the first launch.  stats (optional) receives
 * kernel_ms (device time of all kernels), dp_cells (graph nodes times string bytes, over all aligned strings),
 * n_fallback, n_dp_launches and n_sub_batches = the launches of the POA kernel. */
#define STRK_CONS_POA 3
int64_t strk_consensus(strk_ctx* ctx, int32_t n_groups, const int32_t* group_off /*[n_groups+1]*/, const uint8_t* seqs,
                       int64_t n_seq_bytes, const int64_t* seq_start, const int32_t* seq_len, int32_t max_mdn_poa_length,
                       int64_t cap, int32_t* out_index, int32_t* out_method, int64_t* out_seq_off /*[n_groups+1]*/,
                       uint8_t* out_seqs /*[cap]*/, strk_stats* stats);
/* The same with the bases already in memory of the context's device; everything else on the host. */
int64_t strk_consensus_dseqs(strk_ctx* ctx, int32_t n_groups, const int32_t* group_off, const void* d_seqs, int64_t n_seq_bytes,
                             const int64_t* seq_start, const int32_t* seq_len, int32_t max_mdn_poa_length, int64_t cap,
                             int32_t* out_index, int32_t* out_method, int64_t* out_seq_off, uint8_t* out_seqs,
                             strk_stats* stats);
/* The general form: exactly one of seqs (host) and d_seqs (device) is not NULL; node_limit is the node limit (1 .. 16 384;
 * <= 0: the default, 16 384), which is part of the rule; workspace_bytes bounds the device workspace of one launch of the
 * POA kernel (<= 0: the default, 4 GiB; a single group that needs more runs alone), which is not: the result does not depend
 * on it. */
int64_t strk_consensus_ws(strk_ctx* ctx, int32_t n_groups, const int32_t* group_off, const uint8_t* seqs, const void* d_seqs,
                          int64_t n_seq_bytes, const int64_t* seq_start, const int32_t* seq_len, int32_t max_mdn_poa_length,
                          int64_t cap, int32_t* out_index, int32_t* out_method, int64_t* out_seq_off, uint8_t* out_seqs,
                          int32_t node_limit, int64_t workspace_bytes, strk_stats* stats);

/* ---- distinct windows (k-mers) of a group of sequences, counted ----------------------------------------------------
 * Stands where the reference counts motif-sized k-mers per read (call_locus.py:1287) and per allele (:1526-1593, :1635).
 * A group is an ordered list of byte strings with one window length k >= 1.  Its windows are the s[i : i+k],
 * 0 <= i <= len(s) - k, of every string s (a string shorter than k has none).  The result holds one entry per distinct window:
 * the count over all strings (duplicates as often as they occur) and the place of the first occurrence (smallest string
 * index in the group, then smallest i).  Entries are in ascending unsigned lexicographic order of the window's bytes; raw
 * bytes, case-sensitive, exact for arbitrary byte values.  A group without windows has no entries; a group's counts add up
 * to its number of windows.  The result does not depend on launch geometry.  Unpinned against STRkit, whose counter is not
 * in its tree.
 *
 * Groups and sequences as for strk_best_representatives (at most 250 per group, lengths 0 .. 65 535, slices inside
 * n_seq_bytes, slices may overlap); k[g] >= 1 per group.  Returns the number of entries E of all groups, or a negative
 * STRK_E_* code.  out_entry_off [n_groups + 1] is always written; out_pos [cap] (byte offset into `seqs` of the window's first
 * occurrence) and out_count [cap] only if E <= cap: cap = 0 with NULL arrays is a size query (call again with larger
 * arrays, as for strk_bam_scan).  All buffers are host buffers; every input is checked before the first launch.  stats
 * (optional) receives kernel_ms, n_dp_launches, dp_cells = the windows, n_fallback = the groups whose distinct windows did
 * not fit the on-chip table, n_miss_reads = the groups whose windows do not pack into 64 bits, n_sub_batches = the launches
 * the workspace bound cut those groups into. */
int64_t strk_count_kmers(strk_ctx* ctx, int32_t n_groups, const int32_t* group_off /*[n_groups+1]*/, const uint8_t* seqs,
                         int64_t n_seq_bytes, const int64_t* seq_start, const int32_t* seq_len, const int32_t* k /*[n_groups]*/,
                         int64_t cap, int64_t* out_entry_off /*[n_groups+1]*/, int64_t* out_pos /*[cap]*/,
                         int32_t* out_count /*[cap]*/, strk_stats* stats);
/* The same with the bases already in memory of the context's device; everything else on the host. */
int64_t strk_count_kmers_dseqs(strk_ctx* ctx, int32_t n_groups, const int32_t* group_off, const void* d_seqs, int64_t n_seq_bytes,
                               const int64_t* seq_start, const int32_t* seq_len, const int32_t* k, int64_t cap,
                               int64_t* out_entry_off, int64_t* out_pos, int32_t* out_count, strk_stats* stats);
/* The general form: exactly one of seqs (host) and d_seqs (device) is not NULL, and workspace_bytes bounds the device
 * workspace of one launch over the groups that the on-chip table cannot take (<= 0: the default, 1 GiB; a single group that
 * needs more runs alone).  The result does not depend on it. */
int64_t strk_count_kmers_ws(strk_ctx* ctx, int32_t n_groups, const int32_t* group_off, const uint8_t* seqs, const void* d_seqs,
                            int64_t n_seq_bytes, const int64_t* seq_start, const int32_t* seq_len, const int32_t* k, int64_t cap,
                            int64_t* out_entry_off, int64_t* out_pos, int32_t* out_count, int64_t workspace_bytes,
                            strk_stats* stats);

/* ---- host-side front end (CPU only; no context, thread-safe) ---------------------------------------------------
 * What the reference's Rust extension does before the counter runs: walk the alignment records
 * (STRkitBAMReader / STRkitAlignedSegment, call sites strkit/call/call_sample.py:81-131) and cut each read into
 * (left flank, tract, right flank) for a locus (get_read_coords_from_matched_pairs + get_sequence_data_for_locus,
 * strkit/call/call_locus.py:875-877,1101-1146).  The rules are spelled out in strkit_amd/frontend/extract.py.
 *
 * strk_bam_scan: `buf` = the decompressed BAM stream, `first_rec` = byte offset of the first alignment record (after
 * header and reference list).  Writes, for up to `cap` records, the record's byte offset, refID, 0-based start, exclusive
 * reference end, flag, l_seq and the soft-clip lengths at its two ends; returns the number of records in the stream
 * (call again with larger arrays if it exceeds `cap`) or a negative STRK_E_* code. */
int64_t strk_bam_scan(const uint8_t* buf, int64_t n_bytes, int64_t first_rec, int64_t cap, int64_t* rec_off, int32_t* tid,
                      int32_t* pos, int32_t* end, int32_t* flag, int32_t* l_seq, int32_t* clip_l, int32_t* clip_r);

/* strk_bam_scan_piece: strk_bam_scan over a PIECE of the decompressed stream (block-wise access): a record cut off at the
 * end of the piece is not an error; *end_off = offset just past the last complete record (where the next piece resumes). */
int64_t strk_bam_scan_piece(const uint8_t* buf, int64_t n_bytes, int64_t first_rec, int64_t cap, int64_t* rec_off, int32_t* tid,
                            int32_t* pos, int32_t* end, int32_t* flag, int32_t* l_seq, int32_t* clip_l, int32_t* clip_r,
                            int64_t* end_off);

/* strk_bam_names: the read names of n records (without their terminating NUL), concatenated; out_off is [n + 1].
 * out == NULL: size query.  Returns the total length or a negative STRK_E_* code. */
int64_t strk_bam_names(const uint8_t* buf, int64_t n_bytes, int64_t n, const int64_t* rec_off, uint8_t* out, int64_t out_cap,
                       int64_t* out_off);

/* strk_bgzf_inflate: decompresses a whole BGZF stream (BAM, bgzipped FASTA) with n_threads host threads (0 = all
 * cores); blocks are independent deflate streams, every block's CRC is checked.  out == NULL: returns the decompressed
 * size.  Otherwise returns the number of bytes written, or a negative STRK_E_* code. */
int64_t strk_bgzf_inflate(const uint8_t* comp, int64_t n_comp, uint8_t* out, int64_t out_cap, int32_t n_threads);

/* strk_bgzf_inflate_range: block-wise access (what an index such as .bai points into): inflates the consecutive BGZF blocks
 * that start at compressed offset `coff` for as long as whole blocks fit into out_cap bytes; *next_coff = compressed offset
 * of the first block NOT inflated (n_comp at the end of the file).  Returns the bytes written or a negative STRK_E_* code.
 * A BAM virtual offset is (coff << 16 | offset inside the inflated block). */
int64_t strk_bgzf_inflate_range(const uint8_t* comp, int64_t n_comp, int64_t coff, uint8_t* out, int64_t out_cap,
                                int64_t* next_coff, int32_t n_threads);

/* strk_extract_reads: item i = (record at rec_off[i], locus boundaries coords[4i..4i+3] = left_flank_coord, left_coord,
 * right_coord, right_flank_coord).  An item with alt_cigar_off[i+1] > alt_cigar_off[i] uses that CIGAR (BAM encoding)
 * starting at alt_start[i] instead of the record's own alignment (a realigned read); alt_* may be NULL.
 * status[i]: 0 = extracted, 1 = the read does not span both flanks (skipped), 2 = mean base quality of the tract below
 * min_avg_phred (skipped).  Extracted items append fl|tr|fr (flanks cut to flank_size, bases with PHRED <=
 * wildcard_threshold replaced by 'X') to seqs; seq_off is [n_items + 1]; nfl/ntr/nfr the three lengths.
 * seqs == NULL is a size query: status, the lengths and seq_off are filled (seq_off[n_items] = bytes needed), no bases are
 * written.  A record that holds the long-CIGAR placeholder (<l_seq>S<ref_len>N) is read through its CG:B,I tag.  Items are
 * processed by all host cores when there are more than a few hundred. */
int strk_extract_reads(const uint8_t* buf, int64_t n_bytes, int32_t n_items, const int64_t* rec_off, const int64_t* coords,
                       const uint32_t* alt_cigar, const int64_t* alt_cigar_off, const int64_t* alt_start, int32_t flank_size,
                       int32_t min_avg_phred, int32_t wildcard_threshold, int32_t* status, int32_t* nfl, int32_t* ntr,
                       int32_t* nfr, uint8_t* seqs, int64_t seq_cap, int64_t* seq_off);

/* ---- alignment file on the device (strk_dbam): BGZF inflation, record scan and read extraction as HIP kernels ----------
 * Replaces, for a whole file or a stretch of it, the host functions above (what strkit_rust_ext's STRkitBAMReader and
 * STRkitAlignedSegment do in the reference, call sites strkit/call/call_sample.py:103-121, call_locus.py:837-958): the
 * decompressed stream lives in HBM only.  One object = one device buffer set; not thread-safe. */
typedef struct strk_dbam strk_dbam;
int strk_dbam_open(int device, strk_dbam** out);
void strk_dbam_close(strk_dbam* d);
/* A closed reader leaves its two largest device buffers (the decompressed stream, the compressed bytes) to the next reader of
 * the process instead of freeing them (allocating gigabytes right after freeing them can take longer than inflating the file);
 * this frees them. */
void strk_dbam_release_cache(void);
/* Inflates the consecutive BGZF blocks of `comp` (HOST memory) from byte `coff` on, as many as decompress into at most
 * max_out bytes, into the object's device buffer (one GPU lane per block, CRC checked); *next_coff = offset of the first block
 * not taken.  Returns the decompressed bytes or a negative STRK_E_* code. */
int64_t strk_dbam_inflate(strk_dbam* d, const uint8_t* comp, int64_t n_comp, int64_t coff, int64_t max_out, int64_t* next_coff);
/* The same for a whole file read by the library: `threads` readers (0: default) pread pieces of it into a ring of pinned
 * buffers, each piece is copied to the device as it comes in, the block headers are walked meanwhile and all blocks are
 * inflated by one launch at the end.  *n_comp (may be NULL) = size of the file.  Returns the decompressed bytes or a negative
 * STRK_E_* code. */
int64_t strk_dbam_inflate_file(strk_dbam* d, const char* path, int threads, int64_t* n_comp);
/* The same for the BGZF blocks in the file's bytes [coff_lo, coff_hi): both must be block boundaries (what the .bai's virtual
 * offsets >> 16 are); coff_hi < 0 or past the end = up to the end of the file.  A file whose decompressed form does not fit in
 * device memory is walked span by span with it (frontend.DeviceBam, streamed mode). */
int64_t strk_dbam_inflate_file_range(strk_dbam* d, const char* path, int64_t coff_lo, int64_t coff_hi, int threads, int64_t* n_comp);
/* bytes [off, off + n) of the decompressed stream -> host (headers, a single record for realignment, tests) */
int strk_dbam_download(strk_dbam* d, int64_t off, int64_t n, uint8_t* out);
/* the first n bytes of the bases of the last strk_dbam_extract -> host (tests) */
int strk_dbam_download_seqs(strk_dbam* d, int64_t n, uint8_t* out);
/* HIP-event time (ms) of all kernels the object has launched so far (inflation, scan, extraction) */
double strk_dbam_kernel_ms(strk_dbam* d);
/* wall-clock stages (ms) of the last strk_dbam_inflate_file: buffers (device + pinned ring), read + upload, inflation */
void strk_dbam_file_ms(strk_dbam* d, double* out3);
/* device address and size of the decompressed stream (valid until the next strk_dbam_inflate / strk_dbam_close) */
void* strk_dbam_data(strk_dbam* d, int64_t* n_bytes);
/* BAM virtual offsets (block offset << 16 | offset in the block) -> offsets in the decompressed stream (-1: not in it) */
int strk_dbam_voffsets(strk_dbam* d, const uint64_t* voff, int64_t n, int64_t* out);
/* strk_bam_scan on the device.  `starts`: ascending, distinct offsets of record starts (the first record and what the .bai
 * linear index points at); one GPU lane walks the record chain from each to the next.  Returns the number of records; the
 * host arrays (capacity cap) are filled, in stream order, when it fits. */
int64_t strk_dbam_scan(strk_dbam* d, const int64_t* starts, int64_t n_starts, int64_t cap, int64_t* rec_off, int32_t* tid,
                       int32_t* pos, int32_t* end, int32_t* flag, int32_t* l_seq, int32_t* clip_l, int32_t* clip_r, int32_t* l_name);
/* strk_extract_reads on the device (same arguments, alt_* may be NULL): the bases stay in HBM (*d_seqs, valid until the next
 * call on the object), status / lengths / seq_off and the name length of every item come back.  A rec_off that leaves no room for
 * a record's fixed 36 bytes inside the stream is refused before any launch (STRK_E_INVALID, "item k: ..."). */
int strk_dbam_extract(strk_dbam* d, int32_t n_items, const int64_t* rec_off, const int64_t* coords, const uint32_t* alt_cigar,
                      const int64_t* alt_cigar_off, const int64_t* alt_start, int32_t flank_size, int32_t min_avg_phred,
                      int32_t wildcard_threshold, int32_t* status, int32_t* nfl, int32_t* ntr, int32_t* nfr, int64_t* seq_off,
                      int32_t* name_len, void** d_seqs);
/* read names of n records into out[0 .. out_off[n]); out_off = running sum of the name lengths (input): ascending from 0, every
 * slice rec_off[i] + 36 .. + out_off[i+1] - out_off[i] inside the stream, or the call is refused (STRK_E_INVALID, "item k: ...") */
int strk_dbam_names(strk_dbam* d, int64_t n, const int64_t* rec_off, const int64_t* out_off, uint8_t* out);
/* strk_count_loci with the bases already on the device (d_seqs; batch->seqs is ignored), everything else on the host */
int strk_count_loci_dseqs(strk_ctx* ctx, const strk_batch* batch, const void* d_seqs, const strk_params* params, int32_t* out_cn,
                          int32_t* out_score, int32_t* out_n_iters, int32_t* out_start, strk_stats* stats);
/* test aid: the two statements of the CIGAR -> locus boundaries walk on one alignment (bit 0: run index, bit 1: one pass) */
int strk_read_coords_both(const uint32_t* cigar, int32_t n_cigar, int64_t start, const int64_t* coords, int64_t* out_runs,
                          int64_t* out_linear);
/* strk_bgzf_inflate's contract, served by the DEVICE inflater's code compiled for the host, one thread (test aid) */
int64_t strk_bgzf_inflate_sw(const uint8_t* comp, int64_t n_comp, uint8_t* out, int64_t out_cap);

/* ---- inputs of strk_call_alleles_phased read from an alignment file (the rule: DESIGN.md §13, frontend/phase_inputs.py) --
 * Stands where the reference reads STRkitAlignedSegment.hp / .ps and calls process_read_snvs_for_locus_and_calculate_useful_snvs
 * (strkit_rust_ext, not in its tree; call sites strkit/call/call_locus.py:1147-1260).
 *
 * strk_phase_cells: item i = (record at rec_off[i], locus item_locus[i]); locus l has the candidate SNV positions
 * cand_pos[cand_off[l] .. cand_off[l+1]) (0-based, ascending, distinct, at most 1 024).  alt_* as in strk_extract_reads: an item
 * with a substitute CIGAR is walked along that one.  Per item: out_hp / out_ps = its HP and PS tags (types c C s S i I, values
 * that fit an int32; -1 / -1 unless both are present), and one cell per candidate of its locus, items back to back in item
 * order (cell_cap >= their number): out_base = the read's base under the alignment as ASCII, '_' inside a deletion, '-'
 * outside [lo, hi) and inside a reference skip, out_qual = its quality (0 without qualities and for '-' / '_').
 * lo = first aligned reference base + (take_in if the left soft clip >= clip_threshold), hi likewise from the right.
 * A malformed record, or an auxiliary chain that runs past its record, is STRK_E_INVALID naming the item. */
int strk_phase_cells(const uint8_t* buf, int64_t n_bytes, int32_t n_items, const int64_t* rec_off, const int32_t* item_locus,
                     int32_t n_loci, const int32_t* cand_off /*[n_loci+1]*/, const int64_t* cand_pos, const uint32_t* alt_cigar,
                     const int64_t* alt_cigar_off, const int64_t* alt_start, int32_t clip_threshold, int32_t take_in, int32_t* out_hp,
                     int32_t* out_ps, uint8_t* out_base, uint8_t* out_qual, int64_t cell_cap);
/* strk_useful_snvs: over the cells of a strk_phase_cells call with the same n_items, item_locus, n_loci and cand_off.  Locus l
 * keeps the reads kept_item[kept_off[l] .. kept_off[l+1]) (items of that locus, in read order), n of them.  A candidate is
 * useful iff at least two distinct bytes other than '-' and '_' each occur >= max(rint(n / 5.0), min_allele_reads) times among
 * its cells of the kept reads and those bytes number >= max(rint(n * 0.55), 5) in all (float64, round half to even); the first
 * 64 in ascending position are taken.  out_snv_off [n_loci+1]; out_snv_cand (room for 64 * n_loci) = per useful SNV its index
 * among the locus's candidates; out_base / out_qual = the kept reads' cells of the useful SNVs, read-major per locus, loci
 * back to back: what strk_call_alleles_phased takes as snv_base / snv_qual.  Returns the number of packed cells; when it
 * exceeds cap no cell is written (a size query), everything else is. */
int64_t strk_useful_snvs(int32_t n_items, const int32_t* item_locus, int32_t n_loci, const int32_t* cand_off, const uint8_t* cells_base,
                         const uint8_t* cells_qual, const int32_t* kept_off /*[n_loci+1]*/, const int32_t* kept_item,
                         int32_t min_allele_reads, int32_t* out_snv_off, int32_t* out_snv_cand, uint8_t* out_base, uint8_t* out_qual,
                         int64_t cap);
/* The same two over the file resident on the device.  strk_dbam_phase_cells (kernel k_dbam_phase_cells: one wave per item) leaves
 * the cells in HBM, owned by the object until its next call (at most 512 MB of them: STRK_E_NOMEM beyond, call it for fewer loci);
 * the tags come back.  piece_items > 0 cuts the LAUNCHES into that many items each (every item's cells have their place in the one
 * workspace, so the result does not depend on it and the workspace is not made smaller by it): a caller whose cells would exceed
 * the workspace splits its loci over several pairs of calls, as frontend/phase_block.py does.
 * strk_dbam_useful_snvs (k_snv_useful: one workgroup per locus, then k_snv_gather) works on those cells.
 * strk_dbam_download_cells copies them to the host (tests; n_cells must be their number). */
int strk_dbam_phase_cells(strk_dbam* d, int32_t n_items, const int64_t* rec_off, const int32_t* item_locus, int32_t n_loci,
                          const int32_t* cand_off, const int64_t* cand_pos, const uint32_t* alt_cigar, const int64_t* alt_cigar_off,
                          const int64_t* alt_start, int32_t clip_threshold, int32_t take_in, int32_t piece_items, int32_t* out_hp,
                          int32_t* out_ps);
int strk_dbam_download_cells(strk_dbam* d, int64_t n_cells, uint8_t* out_base, uint8_t* out_qual);
int64_t strk_dbam_useful_snvs(strk_dbam* d, int32_t n_loci, const int32_t* kept_off, const int32_t* kept_item, int32_t min_allele_reads,
                              int32_t* out_snv_off, int32_t* out_snv_cand, uint8_t* out_base, uint8_t* out_qual, int64_t cap);

/* ---- candidate SNVs from a pileup of the reads (the rule: DESIGN.md §21, frontend/snv_discovery.py) ---------------------------
 * The reference takes its candidate SNVs from a VCF and has no such step: the rule is this project's own.
 *
 * strk_discover_snvs: items, alt_* and clip_threshold / take_in as in strk_phase_cells; locus l has the flanked locus
 * [left_coord[l], right_coord[l]) and keeps the reads kept_item[kept_off[l] .. kept_off[l+1]) (items of that locus), n of them
 * (at most 65 535; a locus that is to have no candidates is given no kept read).  The window of a locus is the positions p >= 0
 * with left_coord - window <= p < left_coord or right_coord <= p < right_coord + window (1 <= window <= 65 536,
 * |coordinates| <= 2^40).  At p a kept read counts for the base it would have as a cell of strk_phase_cells there, iff that
 * base is one of A C G T and the read has no qualities or its quality there is >= min_base_qual (0 .. 255).  p is a candidate
 * iff at least two of the four counts are >= max(rint(n / 5.0), min_allele_reads) (float64, round half to even).
 * out_cand_off [n_loci+1], out_cand_pos = the candidates of every locus, ascending, loci back to back; a locus with more than
 * 1 024 keeps the 1 024 nearest to its flanked locus (distance left_coord - p on the left, p - (right_coord - 1) on the right,
 * of two at one distance the left one first).  Returns the number of candidates; when it exceeds cap no position is written
 * (a size query), the offsets are.  A malformed record (any item's, kept or not) is STRK_E_INVALID naming the item.  Runs on
 * the host's cores.
 * strk_dbam_discover_snvs: the same over the file resident on the device (kernels k_snv_span: one wave per item; k_snv_pileup:
 * one workgroup per locus and tile of 4 096 positions, the counts in LDS; k_snv_pick: one workgroup per locus).  Its workspace is
 * 512 bytes per tile, n_loci x 2 x ceil(window / 4 096) tiles, at most 512 MB (STRK_E_NOMEM beyond: call it for fewer loci).
 * piece_items > 0 cuts the launches into that many items (spans) and tiles (pileup) each; the result does not depend on it. */
int64_t strk_discover_snvs(const uint8_t* buf, int64_t n_bytes, int32_t n_items, const int64_t* rec_off, const int32_t* item_locus,
                           int32_t n_loci, const int64_t* left_coord, const int64_t* right_coord, const int32_t* kept_off /*[n_loci+1]*/,
                           const int32_t* kept_item, const uint32_t* alt_cigar, const int64_t* alt_cigar_off, const int64_t* alt_start,
                           int32_t clip_threshold, int32_t take_in, int32_t window, int32_t min_base_qual, int32_t min_allele_reads,
                           int32_t* out_cand_off, int64_t* out_cand_pos, int64_t cap);
int64_t strk_dbam_discover_snvs(strk_dbam* d, int32_t n_items, const int64_t* rec_off, const int32_t* item_locus, int32_t n_loci,
                                const int64_t* left_coord, const int64_t* right_coord, const int32_t* kept_off, const int32_t* kept_item,
                                const uint32_t* alt_cigar, const int64_t* alt_cigar_off, const int64_t* alt_start, int32_t clip_threshold,
                                int32_t take_in, int32_t window, int32_t min_base_qual, int32_t min_allele_reads, int32_t piece_items,
                                int32_t* out_cand_off, int64_t* out_cand_pos, int64_t cap);

/* ---- 5-methyl CpG calls of a read inside a locus's tract, from its MM / ML tags (the rule: DESIGN.md §14, frontend/methyl.py) --
 * Stands where the reference calls STRkitAlignedSegment.get_methylation_prop(locus, 127, 0.0) (strkit_rust_ext, not in its tree;
 * call site strkit/call/call_locus.py:1301-1305): the rule is this project's own, built from the SAM tags specification.
 *
 * strk_methyl: item i = (record at rec_off[i], locus boundaries coords[4i..4i+3]) and alt_* exactly as strk_extract_reads takes
 * them.  The tract [q_l, q_r) is the bases that function returns as `tr`.  A site is a stored C inside the tract with a stored G
 * behind it; the first C+m entry of MM (first occurrence of MM:Z / ML:B,C; Mm / Ml where a record has neither) says which of
 * the read's Cs (as sequenced: the stored Gs from the end, for a reverse read) carry a call and ML its probability.
 * out_status[i]: STRK_METHYL_OK; _NOT_SPANNING (extraction would refuse the item for a reason other than base quality);
 * _NO_TAGS (no MM, or no C+m entry in it); _CLIPPED (an H in the record's CIGAR, or an MN that differs from l_seq); _MALFORMED
 * (MM not of the grammar, ML not B,C or not of the length MM asks for, a skip past the last target); _NO_SITES (no known site).
 * out_sites = the sites, out_known = those the tags speak about (a site without a call is known with probability 0 unless the
 * entry's mode is '?'), out_mc = the known ones with probability > threshold (0 .. 255).  All zero unless OK or NO_SITES.
 * m = out_mc / out_known is the caller's.  A malformed record, or an auxiliary chain that runs past its record, is STRK_E_INVALID
 * naming the item (the last such item). */
#define STRK_METHYL_OK 0
#define STRK_METHYL_NOT_SPANNING 1
#define STRK_METHYL_NO_TAGS 2
#define STRK_METHYL_CLIPPED 3
#define STRK_METHYL_MALFORMED 4
#define STRK_METHYL_NO_SITES 5
int strk_methyl(const uint8_t* buf, int64_t n_bytes, int32_t n_items, const int64_t* rec_off, const int64_t* coords,
                const uint32_t* alt_cigar, const int64_t* alt_cigar_off, const int64_t* alt_start, int32_t threshold,
                int32_t* out_status, int32_t* out_sites, int32_t* out_known, int32_t* out_mc);
/* The same over the file resident on the device (kernel k_dbam_methyl: one wave per item); piece_items > 0 cuts the launches into
 * that many items each, which changes no output. */
int strk_dbam_methyl(strk_dbam* d, int32_t n_items, const int64_t* rec_off, const int64_t* coords, const uint32_t* alt_cigar,
                     const int64_t* alt_cigar_off, const int64_t* alt_start, int32_t threshold, int32_t piece_items,
                     int32_t* out_status, int32_t* out_sites, int32_t* out_known, int32_t* out_mc);
/* the size constants of k_dbam_methyl as built: bases per lane and pass, bases per pass, MM bytes per pass, ordinals per window */
void strk_methyl_constants(int32_t* out4);

/* ---- Candidate SNVs out of VCF text ----------------------------------------------------------------------------
 * Stands where the reference asks its tabix-indexed SNV catalog for the candidates of one block of loci
 * (STRkitVCFReader.get_candidate_snvs of strkit_rust_ext, not in its tree; call site strkit/call/call_sample.py:124).  The rule
 * is frontend/snv_vcf.py::read_snv_vcf's, restated for a byte parser:
 *   lines end at '\n' (trailing '\r's are stripped; a lone '\r' ends nothing); lines that begin with '#' or have fewer than
 *   five tab-separated fields are skipped; a record counts when, after ASCII upper-casing, REF is one byte of ACGTN and ALT,
 *   split at ',', is non-empty with every piece one byte of ACGTN.  Only on such a line POS is read: 1 to 18 decimal digits,
 *   otherwise the call fails with STRK_E_INVALID and names the line's byte offset.  A record is reported when its CHROM field
 *   equals `contig` byte for byte and beg <= POS - 1 < end; of several such records at one position the first in the text
 *   stays; a reported position below the one before it (or below prev_pos) fails: not coordinate-sorted.
 * The text is buf[start, n_bytes), `start` a line start.  final != 0: the text ends its file, so that a last line without
 * '\n' is complete; otherwise it is left for the next piece: *end_off = the offset just past the last complete line.
 * prev_pos = the last position the previous piece reported (-1: none), contig_seen != 0: a record of the contig was seen before.
 * Outputs in text order: pos (0-based), ref (upper case), id_off [n + 1] into ids (the ID column; empty where it is ".").
 * *id_bytes = the ID bytes of all records; ids == NULL: none are written (size query).  *past = 1 when a record of the contig at
 * or beyond `end`, or one of another contig after one of this contig, was seen.  Returns the number of records n; the arrays
 * (capacity cap) are filled when n <= cap.  STRK_E_NOMEM when ids is given and ids_cap < *id_bytes. */
int64_t strk_vcf_snvs(const uint8_t* buf, int64_t n_bytes, int64_t start, const char* contig, int64_t beg, int64_t end, int32_t final,
                      int64_t prev_pos, int32_t contig_seen, int64_t cap, int64_t* pos, uint8_t* ref, int64_t* id_off, uint8_t* ids,
                      int64_t ids_cap, int64_t* id_bytes, int64_t* end_off, int32_t* past);
/* The same over the stream of a strk_dbam object (a BGZF-compressed VCF inflated by strk_dbam_inflate*), `start` an offset into
 * it, checked against the stream's size before any launch.  Kernels: k_lines_count, k_lines_scan, k_lines_starts (the lines),
 * k_vcf_parse (one lane per line), k_vcf_compact (the kept lines and their ID bytes); one record per position and sortedness are
 * applied on the host to what comes back.  tile_bytes: the text bytes one wave walks in the line passes, a multiple of 256
 * (0: the default); no output depends on it. */
int64_t strk_dbam_vcf_snvs(strk_dbam* d, int64_t start, const char* contig, int64_t beg, int64_t end, int32_t final, int64_t prev_pos,
                           int32_t contig_seen, int32_t tile_bytes, int64_t cap, int64_t* pos, uint8_t* ref, int64_t* id_off,
                           uint8_t* ids, int64_t ids_cap, int64_t* id_bytes, int64_t* end_off, int32_t* past);
/* the size constants of the kernels as built: default tile bytes, bytes per step, lines per wave */
void strk_vcf_constants(int32_t* out3);
/* The lines of the text in the stream of a strk_dbam object, from `start` on: what strk_dbam_vcf_snvs and
 * strk_dbam_gff_overlaps begin with (k_lines_count, k_lines_scan, k_lines_starts).  A line start is `start` itself and the offset just past every '\n' in
 * [start, the stream's size): *n_starts of them (the '\n's + 1), of which starts[0 .. min(cap, *n_starts)) are written.  Returns
 * the number of lines a reader takes: one per '\n', and the bytes behind the last '\n' when final != 0 and there are any;
 * *end_off = where the first line not taken begins (the stream's size when all were).  tile_bytes as in strk_dbam_vcf_snvs.
 * STRK_E_INVALID, before any launch, for a tile_bytes that is no multiple of 256 and a start outside the stream; start == the
 * stream's size: 0 lines, *end_off = start, *n_starts = 1, nothing launched. */
int64_t strk_dbam_text_lines(strk_dbam* d, int64_t start, int32_t final, int32_t tile_bytes, int64_t cap, int64_t* starts,
                             int64_t* end_off, int64_t* n_starts);

/* ---- Locus annotations out of GFF3 / GTF text -----------------------------------------------------------------
 * Stands where the reference asks its tabix-indexed annotation file for the features of every locus (strkit/call/loci.py:158-166,
 * 209-214, 250-253, through pysam's asGFF3 / asGTF, which are not in its tree).  The rule is frontend/annotations.py's:
 *   lines end at '\n' (trailing '\r's are stripped); empty lines and lines that begin with '#' are skipped; every other line
 *   must have nine tab-separated fields, start (field 4) and end (field 5) of 1 to 18 decimal digits with 1 <= start <= end,
 *   otherwise the call fails with STRK_E_INVALID and names the line's byte offset.  A feature is a line whose field 1 equals
 *   `contig` byte for byte; f_beg = start - 1, f_end = end; its f_beg must not lie below the one before it (or below prev_beg;
 *   -1: none): STRK_E_INVALID, not coordinate-sorted.  Feature and locus [s, e) overlap iff f_beg < e and f_end > s.
 *   The id of a feature comes from field 9: gtf == 0: split at ';', leading spaces dropped, key = the bytes before the first '=',
 *   value = the rest; gtf != 0: split at every ';' outside double quotes, spaces around a piece dropped, key = the bytes before
 *   the first space, value = the rest without the spaces around it and without one pair of double quotes.  The last piece of a
 *   key wins, a key matches as a whole.  kind 0: the value of `ID`; kind 1: no `ID`, field 3 is one of 5UTR, 3UTR, CDS,
 *   start_codon, stop_codon and there is an `exon_id`: its value; kind 2: neither (the caller writes type:contig-f_beg-f_end).
 * The text is buf[start, n_bytes), `start` a line start; final, *end_off as in strk_vcf_snvs.  l_start / l_end: the n_loci loci
 * of the contig (callers pass them sorted by start; the pairs come in the order given).  Outputs: the (locus, feature) pairs in
 * locus order and, per locus, file order (pair_feat indexes the hit features); per distinct hit feature, in file order, f_beg,
 * f_end, f_kind and f_text_off [2 n + 1]: feature k's type bytes are text[f_text_off[2k] .. f_text_off[2k + 1]), its id bytes
 * (none for kind 2) text[f_text_off[2k + 1] .. f_text_off[2k + 2]).  sizes[0..2] = pairs, hit features, text bytes, always;
 * sizes[3] = the f_beg of the contig's last feature in the text (prev_beg when it has none).  The arrays are filled when all three
 * sizes fit their capacities.  *past = 1 when a feature of another contig follows one of this contig (or prev_beg >= 0).
 * Returns the number of pairs. */
int64_t strk_gff_overlaps(const uint8_t* buf, int64_t n_bytes, int64_t start, const char* contig, int32_t gtf, int32_t final, int64_t prev_beg,
                          int32_t n_loci, const int64_t* l_start, const int64_t* l_end, int64_t pair_cap, int32_t* pair_locus, int32_t* pair_feat,
                          int64_t feat_cap, int64_t* f_beg, int64_t* f_end, int32_t* f_kind, int64_t* f_text_off, int64_t text_cap, uint8_t* text,
                          int64_t* sizes, int64_t* end_off, int32_t* past);
/* The same over the stream of a strk_dbam object, `start` an offset into it, checked before any launch.  Kernels: k_lines_count,
 * k_lines_scan, k_lines_starts (the lines), k_gff_coords (one lane per line), k_gff_gather, k_gff_classes (features partitioned by
 * length class), k_gff_join (one wave per locus: two binary searches per class, then ballots over the candidates; count and fill
 * pass), k_gff_hits, k_gff_order, k_gff_ids (one wave per hit feature), k_gff_text (compaction).  tile_bytes as in
 * strk_dbam_vcf_snvs. */
int64_t strk_dbam_gff_overlaps(strk_dbam* d, int64_t start, const char* contig, int32_t gtf, int32_t final, int64_t prev_beg, int32_t tile_bytes,
                               int32_t n_loci, const int64_t* l_start, const int64_t* l_end, int64_t pair_cap, int32_t* pair_locus, int32_t* pair_feat,
                               int64_t feat_cap, int64_t* f_beg, int64_t* f_end, int32_t* f_kind, int64_t* f_text_off, int64_t text_cap, uint8_t* text,
                               int64_t* sizes, int64_t* end_off, int32_t* past);
/* the size constants of the kernels as built: length classes, attribute bytes per step of k_gff_ids, lines per wave */
void strk_gff_constants(int32_t* out3);

/* ---- Which of the records fetched for a locus are used: one record per read name, skip flags, the cap -----------
 * Stands where the reference builds a locus's segments (block_segments.get_segments_for_locus of strkit_rust_ext, not in its
 * tree; call sites strkit/call/call_locus.py:1044-1057,1277-1285; --skip-supplementary / --skip-secondary; chimeric_in_region,
 * types.py:35-37): the rule is this project's own statement (frontend/select.py is the readable one).
 *
 * Locus l owns items item_off[l] .. item_off[l + 1] (item_off ascends from 0), item i is the record at rec_off[i] of the stream:
 * the overlapping mapped records in coordinate order, equal positions in file order.  A read name is the l_read_name - 1 bytes
 * behind the fixed part of the record (none when l_read_name is 0); names are equal when lengths and all bytes are.
 * rules (0 .. 7): 1 = skip supplementary, 2 = skip secondary, 4 = one record per name.  Per locus:
 *   1. status of a name = OR over all items of that name at the locus of (flag & 0x800 ? 2 : 1), whatever becomes of them;
 *   2. an item is flag-skipped with reason 1 when rules & 1 and flag & 0x800, else with reason 2 when rules & 2 and flag & 0x100;
 *   3. with rules & 4 an item that is not flag-skipped is a duplicate (reason 3) when an earlier item of its name at the locus is
 *      not flag-skipped (a flag-skipped first occurrence shadows nothing);
 *   4. of the items without a reason the first max_reads (>= 1) are kept (reason 0), the others get reason 4.
 * out_reason / out_status: per item (status = its name's); out_n_kept: per locus.  A kept read is chimeric in the region when
 * its status is 3.  rules == 0 is the plain cap.  The same read at two loci is two questions.
 * STRK_E_INVALID before any work: item_off not ascending from 0, max_reads < 1, rules outside 0 .. 7, a rec_off outside the
 * stream; a record the parser refuses is STRK_E_INVALID with the item named, and is never read past. */
#define STRK_SELECT_SKIP_SUPPLEMENTARY 1
#define STRK_SELECT_SKIP_SECONDARY 2
#define STRK_SELECT_UNIQUE 4
#define STRK_SELECT_KEPT 0
#define STRK_SELECT_SUPPLEMENTARY 1
#define STRK_SELECT_SECONDARY 2
#define STRK_SELECT_DUPLICATE 3
#define STRK_SELECT_OVER_CAP 4
int strk_select_reads(const uint8_t* buf, int64_t n_bytes, int32_t n_loci, const int64_t* item_off, const int64_t* rec_off,
                      int32_t rules, int32_t max_reads, uint8_t* out_reason, uint8_t* out_status, int32_t* out_n_kept);
/* The same over the file resident on the device (kernels k_select_small: one workgroup per locus, the name table in LDS, and
 * k_select_large for loci beyond its class: the table in the object's workspace). */
int strk_dbam_select_reads(strk_dbam* d, int32_t n_loci, const int64_t* item_off, const int64_t* rec_off, int32_t rules,
                           int32_t max_reads, uint8_t* out_reason, uint8_t* out_status, int32_t* out_n_kept);
/* the size constants of the kernels as built: items of a locus k_select_small takes, its table's slots, threads per workgroup,
 * bytes per step of the name compare */
void strk_select_constants(int32_t* out4);

/* ---- Mendelian inheritance and the de novo test of a child / mother / father trio ------------------------------
 * Stands where `strkit mi` builds one MILocusData per trio locus (strkit/mi/result.py:100-175): respects_mi (:352-389,
 * decimal=False) and de_novo_test (:391-501), with scipy.stats.chi2_contingency(correction=False) and
 * scipy.stats.mannwhitneyu(use_continuity=False, method="auto") as its statistics.
 *
 * Locus l owns six groups of reads in the order child 0, child 1, mother 0, mother 1, father 0, father 1: group g is
 * cn[grp_off[6l + g] .. grp_off[6l + g + 1]) (copy numbers >= 0, at most 65 535 per group, grp_off[6 n_loci] <= n_cn).
 * gt[6l ..] = the six called copy numbers, ci95 / ci99 [12l ..] = their intervals (lo, hi), ci99 NULL: none (that kind is -1).
 * seq_id / seq_len [6l ..] = the caller's small integer ids (equal ids = equal strings) and lengths of the six allele sequences;
 * both NULL, or a negative id in a locus, = no sequences (the three sequence kinds are -1).
 * out_respects[7l ..] = strict, pm1, ci_95, ci_99, seq, sl, sl_pm1 as 1, 0 or -1 (None).
 * With params->test != STRK_MI_TEST_NONE: out_status = STRK_MI_TESTED, _OVERLAP (the child's reads are one value and so are a
 * configuration's parents' under a WMW test, :416), _EMPTY_PARENT (:419) or _EMPTY_CHILD (this project's own: the reference
 * fails there); out_p = the largest of the four configurations' p-values (first largest; NaN unless tested), out_config = its
 * configuration 0..3 = (mother's allele, father's allele) in (0,0) (0,1) (1,0) (1,1), -1 unless tested; out_mutation_from =
 * STRK_MI_FROM_*.  With test == STRK_MI_TEST_NONE grp_off and cn may be NULL and only out_respects is written.
 * Every input is checked before any work: STRK_E_INVALID names the entry point and the locus.
 * strk_mi_trio: kernels k_mi_small (one wave per locus, loci of at most 256 reads) and k_mi_large (one workgroup per locus); the
 * call goes through in pieces of at most piece_loci loci (0: the default) whose workspace fits ws_budget bytes (0: the default);
 * the result does not depend on either.  stats: kernel_ms, n_dp_launches, n_fallback = loci on k_mi_large, n_sub_batches = pieces.
 * strk_mi_trio_host: the same rule on the host's cores, no device; piece_loci = the loci a thread takes at a time; it runs on
 * at most OMP_NUM_THREADS threads where that is set, at most 16 where it is not. */
#define STRK_MI_TEST_NONE 0
#define STRK_MI_TEST_X2 1
#define STRK_MI_TEST_WMW 2
#define STRK_MI_TEST_WMW_GT 3
#define STRK_MI_TESTED 0
#define STRK_MI_OVERLAP 1
#define STRK_MI_EMPTY_PARENT 2
#define STRK_MI_EMPTY_CHILD 3
#define STRK_MI_FROM_NONE 0
#define STRK_MI_FROM_UNKNOWN 1 /* "?" */
#define STRK_MI_FROM_MAT 2
#define STRK_MI_FROM_PAT 3
#define STRK_MI_FROM_BOTH 4
typedef struct strk_mi_params {
    int32_t test;        /* STRK_MI_TEST_* */
    int32_t piece_loci;  /* 0: the default */
    double sig_level;    /* in (0, 1) */
    double widen;        /* >= 0: the parents' intervals grow by this share of each bound */
    int64_t ws_budget;   /* workspace bytes of one piece; 0: the default */
    int32_t force_large; /* must be 0 outside tests; non-zero: every locus goes to k_mi_large (same results, slower) */
    int32_t pad;
} strk_mi_params;
int strk_mi_trio(strk_ctx* ctx, int32_t n_loci, const int64_t* grp_off /*[6n+1]*/, const int32_t* cn, int64_t n_cn,
                 const int32_t* gt /*[6n]*/, const int32_t* ci95 /*[12n]*/, const int32_t* ci99 /*[12n] or NULL*/,
                 const int32_t* seq_id /*[6n] or NULL*/, const int32_t* seq_len /*[6n] or NULL*/, const strk_mi_params* params,
                 int8_t* out_respects /*[7n]*/, double* out_p /*[n]*/, int32_t* out_config, int32_t* out_mutation_from,
                 int32_t* out_status, strk_stats* stats);
int strk_mi_trio_host(int32_t n_loci, const int64_t* grp_off, const int32_t* cn, int64_t n_cn, const int32_t* gt, const int32_t* ci95,
                      const int32_t* ci99, const int32_t* seq_id, const int32_t* seq_len, const strk_mi_params* params,
                      int8_t* out_respects, double* out_p, int32_t* out_config, int32_t* out_mutation_from, int32_t* out_status);
/* the size constants of the kernels as built: reads of k_mi_small's largest locus, loci per workgroup, reads per group */
void strk_mi_constants(int32_t* out3);

#ifdef __cplusplus
}
#endif
#endif /* STRKIT_AMD_H */
