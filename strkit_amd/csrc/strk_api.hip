// strk_api.hip — host side of libstrkit_amd.so (C ABI declared in include/strkit_amd.h).
// The batched counting path is here.  It stands on two host-only headers:
//   strk_host.h     the calling thread's error message (fail, HIP_TRY), the owning types (DevBuf, PinnedBuf, Stream, Event) and
//                   Staging: what a call sends up and takes back (its layout and copy plan: strk_stage_plan.h, no HIP in it)
//   strk_policy.h   the adaptive policies as plain state machines: default window, band gate, grid history (no HIP in it)
//   strk_groups.h   groups of byte strings as three calls take them: the view, its one check, the piece cutter (no HIP in it)
//   strk_threads.h  the CPUs of the process, the two thread fans, the first malformed item, the piece loop (no HIP in it)
//   strk_alleles_check.h, strk_phase_check.h   the input of the three allele calls and its checks (no HIP in them)
//   strk_realign_plan.h   strk_realign's input check, chunks and workspace layout (no HIP in it)
// and the other parts live in include fragments spliced into this file:
//   strk_host_miss.inc       window-miss rounds                       strk_host_pipe.inc       the pinned-slot host pipeline
//   strk_host_ref.inc        reference side                           strk_host_realign.inc    realignment
//   strk_host_alleles.inc    allele calling, 2 or 6 slots per locus   strk_host_consensus.inc  best representatives
//   strk_host_kmers.inc      distinct windows (k-mer counts)                 strk_host_phase.inc      phased allele calls
//   strk_host_files.inc      the CPU-only file front end (its parser: strk_frontend.h)
//   strk_dbam.inc            (at the end) the alignment file on the device: BGZF inflater, record scan, read extraction
//   strk_phase_inputs.inc    (after it) tags, SNV cells and useful SNVs for the phased call: host twins and device entry points (walks and kernels: strk_phase_inputs.h)
//
// One context = one HIP device.  A batched call enqueues, on the caller's stream:
//   memset(counters) -> k_hash -> k_plan -> k_dp_band -> k_dp_band_wide -> k_dp_all -> k_dp_long -> k_dp_generic -> k_replay
//   -> counters D2H
// (strk_submit_loci_device) and is completed by strk_finish, which synchronises once.  Only when a read's search left its speculative candidate window (rare;
// strk_stats.n_miss_reads) does the host run extra rounds: re-score the wanted window on the
// device, replay that locus on the host with the same search_replay() the device uses.
#include "strk_host.h"
#include "strk_policy.h"
#include "strk_groups.h"
#include "strk_threads.h"
#include "strk_phase_check.h"
#include "strk_phase_inputs.h"
#include "strk_snv_discover.h"
#include "strk_methyl.h"
#include "strk_vcf.h"
#include "strk_gff.h"
#include "strk_select.h"
#include "strk_mi_check.h"
#include "strk_mi.h"

#include <algorithm>
#include <array>
#include <atomic>
#include <cassert>
#include <chrono>
#include <cmath>
#include <condition_variable>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <mutex>
#include <thread>
#include <vector>
#include <fcntl.h>
#include <sys/stat.h>
#include <unistd.h>

#include "strk_kernels.h"
#include "strk_realign.h"
#include "strk_frontend.h"
#include "strk_inflate.h"
#include "strk_alleles.h"
#include "strk_phase.h"
#include "strk_consensus.h"
#include "strk_kmers.h"
#include "strk_poa.h"

namespace {

struct HostPipe;   // strk_host_pipe.inc: the pinned-slot pipeline behind strk_count_loci

// batched calls submitted and not yet finished, over all contexts of this process: a call that will share the
// device with others takes half the CU slots, so that the tail of one call and the head of the next co-run
std::atomic<int> g_calls_in_flight{0};

// default candidate window of this process, per motif-length bucket (strk_policy.h)
strk_policy::WindowPolicy g_window;
static_assert(strk_policy::kWinBuckets == strk::kWinBuckets, "strk_policy.h <-> strk_kernels.h");
static_assert(strk_groups::kInvalid == STRK_E_INVALID, "strk_groups.h <-> include/strkit_amd.h");
static_assert(strk_realign_plan::kNoMem == STRK_E_NOMEM, "strk_realign_plan.h <-> include/strkit_amd.h");

// The band pass most recently enqueued by any context of this process (its kEvBand event): in whole-grid mode the next call's
// band pass waits for it (enqueue_scoring), so that two calls in flight run half a period apart whatever their submit times.
std::mutex g_band_chain_mu;
hipEvent_t g_band_chain_ev = nullptr;
int g_band_chain_dev = -1;

using strk_threads::host_cpus;

// device layout of the `counters` buffer: int32[kCntTotal] | pad | u64 cells | u64 scratch_used
constexpr size_t kCellsOff = 64 * sizeof(int32_t);
constexpr size_t kCountersBytes = kCellsOff + 10 * sizeof(unsigned long long);   // cells, scratch_used, band / exact / wide-band / long-kernel bytes, cells per kernel (kCell*)
// slots of the 64-bit part that strk_kernels.h addresses by number (KArgs::scratch_used, KArgs::cells + 2 .. + 5)
constexpr int kU64ScratchUsed = 1, kU64BandBytes = 2, kU64ExactBytes = 3, kU64WideBytes = 4, kU64LongBytes = 5;
// behind them, zeroed with them but not copied back: k_plan's census of the wide band classes and k_sort_wide's cursors
constexpr size_t kWideHistOff = (kCountersBytes + 63) & ~(size_t)63;
constexpr size_t kCountersAllBytes = kWideHistOff + 2 * strk::kNumWideLists * 256 * sizeof(int32_t);

// The pinned host image of `counters` (its first kCountersBytes), as the copy at the end of a call left it.
struct HostCounters {
    PinnedBuf mem;
    int cnt(int k) const { return mem.as<const int32_t>()[k]; }
    unsigned long long u64(int k) const { return reinterpret_cast<const unsigned long long*>(mem.as<const char>() + kCellsOff)[k]; }
    unsigned long long cells() const { return u64(0); }                   // DP cells of all kernels
    unsigned long long cells_of(int k_cell) const { return u64(k_cell); }   // ... of one kernel (strk::kCellBand ...)
    unsigned long long scratch_used() const { return u64(kU64ScratchUsed); }
    unsigned long long band_bytes() const { return u64(kU64BandBytes); }
    unsigned long long exact_bytes() const { return u64(kU64ExactBytes); }
    unsigned long long wide_bytes() const { return u64(kU64WideBytes); }
    unsigned long long long_bytes() const { return u64(kU64LongBytes); }
    int band_reads() const {   // reads k_plan sent to the band kernels
        int n = 0;
        for (int k = 0; k < strk::kNumBandClasses; ++k) n += cnt(strk::kCntClass0 + strk::kBandClass0 + k);
        return n;
    }
};

}  // namespace

struct strk_ctx {
    int device = 0;
    int last_list_stride = 0;   // list_stride of the last call planned on this context (strk_band_list)
    // workspace
    DevBuf read_locus, win_lo, win_n, tab_off, table, ub, cls_list, band_recs, band_recs_w, long_list, counters, scratch, state_i32, state_f64, spec, rhash, rep, exact;
    DevBuf win_lo2, win_n2, tab_off2, table2, items;
    // staging for the host-buffer entry points: the arrays of a host batch (upload_batch; strk_repeat_count's fast path keeps
    // its one read's arrays there), the four result arrays of strk_count_loci
    DevBuf stage_in, stage_out;
    PinnedBuf sc_host, sc_out;      // the fast path's pinned host image (one copy up) and its pinned result (one copy down)
    // realignment (strk_realign): what a call sizes once (the bases, the queue counters), what it sizes per chunk
    DevBuf rl_call, rl_chunk;
    // The stream of every call for which the library chooses one (side_stream creates it on first use): the scalar, table,
    // reference-side and realign calls, strk_count_loci below the pipeline's threshold or with d_seqs, and the allele, group
    // and consensus calls below.  One serves them all: each of these calls synchronises before it returns and leaves no work
    // in flight, and a context serves one host thread at a time.  It is non-blocking, so nothing on it is ordered against the
    // NULL stream: whatever such a call copies, sets or launches goes on this stream and is waited for on it.
    Stream side;
    // The calls below hand their arrays to the device through a Staging (strk_host.h) on `side`: one staged buffer per call, one
    // per piece where a call has pieces (what goes up and what comes down share it), beside the workspaces that only kernels
    // touch.  `image` is the page-locked image of whichever of them is running; a piece's wait (timed_launch) gives it back.
    PinnedBuf image;
    // allele calling (strk_call_alleles, _n) and trio inheritance
    DevBuf al_stage, al_ws;
    DevBuf mi_stage, mi_ws;
    // phased allele calls (strk_call_alleles_phased) keep carved buffers and a copy per array, as measured in
    // profiles/r31_context_staging.txt: what goes up, what the kernels hand each other, the workspaces, what comes down
    DevBuf ph_in, ph_mid, ph_ws, ph_out;
    // best representatives (strk_best_representatives): the view and the results; the parked rows of long patterns
    DevBuf cs_stage, cs_bound;
    // distinct windows (strk_count_kmers): what the call holds, what a piece of k_kmers_sort holds, its runs, the entries
    DevBuf km_call, km_piece, km_ws, km_out;
    // allele sequences by partial-order alignment (strk_consensus): what the call holds, what a piece of k_poa holds (then the
    // gather's offsets and choices), the graphs, the pooled consensus bytes, the gathered bytes.  The call runs the
    // best-representative pass on some of its groups in mid-call, while the results of its own kernels lie in an image and wait
    // to be merged with that pass's: so what the call holds, results included, has an image of its own, and its pieces, the nested
    // pass and the gather take `image` in turn.
    PinnedBuf po_image;
    DevBuf po_call, po_piece, po_ws, po_pool, po_out;
    HostCounters h_counters;        // pinned: counters + cells + scratch_used
    // a chain of events along one call: start | after k_hash + k_plan | after k_dp_band | after k_dp_band_wide | after the
    // first k_replay pass | after k_dp_all / k_dp_ref | after k_dp_long | after k_dp_generic | end (after k_replay and the
    // counters' copy)
    Event ev[9];
    size_t scratch_ints = 0;        // = kLongWaves * long_slot_ints + generic_ints
    size_t long_slot_ints = 0, generic_ints = 0;   // (set where the constants are known: strk_create)
    strk_policy::BandGate band;       // whether, and for how many reads, the next call takes the band kernels
    strk_policy::GridHistory hist;    // queue lengths of the previous finished call: the grids of the sparsely used kernels
    bool p_window_auto = false;
    int p_window_b[strk::kWinBuckets] = {0, 0, 0, 0, 0};   // the pending call's window per motif-length bucket (0: params.window for all)
    // one submitted-but-not-finished batched call (strk_submit_loci_device .. strk_finish)
    bool pending = false;
    strk_batch p_batch;
    strk_params p_params;
    strk_params p_params_in;       // as the caller gave them (a call that is run again goes through check_params again)
    int scratch_reruns = 0;        // the submitted call is a re-run of one that asked for more scratch than there was (grow_scratch)
    strk::KArgs p_args;
    strk::ReplayArgs p_replay;
    hipStream_t p_stream = nullptr;
    HostPipe* pipe = nullptr;   // created by the first large strk_count_loci call of this context
};

namespace {

using namespace strk;

constexpr int kDefaultWindow = 8;
enum { kEvStart = 0, kEvHead, kEvBand, kEvWide, kEvPre, kEvExact, kEvLong, kEvGeneric, kEvEnd, kNumEvents };
constexpr int kBandProbationReads = 2048;
// defaults of BandTune (strk_search.h): the band is laid around the table's middle +- kBandSpanW candidate sizes for motifs of up
// to kBandSpanMaxMotif bases (the window buckets whose table is +-6 or +-8 sizes), around the whole table for longer ones.
// Off (64 covers every table): +-4 for motifs of up to 6 bases was measured again in round 15 with two calls in flight and lost
// 12-19 % of the headline to the reads it stops certifying (profiles/r15_band_order.txt); the knobs stay as tuning aids.
constexpr int kBandSpanW = 64, kBandSlackM8 = 0, kBandSpanMaxMotif = 6;
// Scratch pool (int32 units): kLongWaves slots of kLongSlotInts for k_dp_long (one per resident wave; a slot
// holds the backward row of all column tiles + two boundary columns: windows up to ~16 kb), then 16 Mi
// ints of H rows for the generic kernel.  448 MiB of the 288 GB, allocated once per context.
constexpr int kBandBlocksPerCU = std::max(1, std::min(8, (160 * 1024) / (4 * kBandWaveLds + kLdsSlack + 1024)));
constexpr int kLongBlocks = 512, kLongWaves = kLongBlocks * 4;   // 2 waves per SIMD
constexpr size_t kLongSlotInts = (size_t)48 << 10;
constexpr size_t kGenericPoolInts = (size_t)16 << 20;
// what the two parts may grow to when a call asks for more (grow_scratch): a slot for the longest window classify() sends to
// k_dp_long (64 column tiles + two boundary columns of 2^20 rows: 18 GB for the 2 048 slots), 32 GiB of generic-kernel rows
constexpr size_t kLongSlotMaxInts = (size_t)kLongTile * kLongMaxTiles + 2 * (((size_t)1 << 20) + 256);
constexpr unsigned long long kGenericPoolMaxInts = 8ull << 30;
int check_params(const strk_params* p, strk_params* out) {
    if (!p) return fail(STRK_E_INVALID, "params is NULL");
    *out = *p;
    if (out->window <= 0) out->window = kDefaultWindow;
    if (2 * out->window + 1 > kTableMax) out->window = (kTableMax - 1) / 2;
    if (out->local_search_range < 0 || out->step_size < 1)
        return fail(STRK_E_INVALID, "local_search_range must be >= 0 and step_size >= 1");
    if (out->tie_rule != STRK_TIE_FIRST && out->tie_rule != STRK_TIE_LAST) return fail(STRK_E_INVALID, "bad tie_rule");
    if (out->end_flags < 0 || out->end_flags > 15) return fail(STRK_E_INVALID, "bad end_flags");
    static_assert(STRK_NARROW_NONE == strk::kNarrowNone && STRK_NARROW_DECREMENT == strk::kNarrowDecrement &&
                  STRK_NARROW_HALVE == strk::kNarrowHalve && STRK_NARROW_AFTER_SEED == strk::kNarrowAfterSeed, "include/strkit_amd.h <-> strk_search.h");
    if (out->narrowing < 0 || out->narrowing >= strk::kNarrowModes)
        return fail(STRK_E_INVALID, "narrowing schedule %d is not one of STRK_NARROW_NONE / _DECREMENT / _HALVE / _AFTER_SEED", out->narrowing);
    return 0;
}

// Common workspace sizing for a batch with n_reads / n_loci and at most n_items DP items.
// band_tables: the call may run the band kernels, which write a bound beside every table entry (KArgs::ub: the table's size again).
int ensure_workspace(strk_ctx* c, int n_reads, int n_loci, size_t table_ints, size_t n_items, bool band_tables = false) {
    const size_t nr = (size_t)std::max(n_reads, 1), nl = (size_t)std::max(n_loci, 1);
    int rc;
    if ((rc = c->read_locus.ensure(nr * 4))) return rc;
    if ((rc = c->win_lo.ensure(nr * 4))) return rc;
    if ((rc = c->win_n.ensure(nr * 4))) return rc;
    if ((rc = c->tab_off.ensure(nr * 8))) return rc;
    if ((rc = c->table.ensure(std::max<size_t>(table_ints, 1) * 4))) return rc;
    if (band_tables && (rc = c->ub.ensure(std::max<size_t>(table_ints, 1) * 4))) return rc;
    if ((rc = c->cls_list.ensure((size_t)kNumLists * std::max<size_t>(n_items, 1) * 2 * 4))) return rc;
    if ((rc = c->band_recs.ensure((size_t)kNumBandClasses * std::max<size_t>(n_items, 1) * 3 * sizeof(int4)))) return rc;
    if ((rc = c->counters.ensure(kCountersAllBytes))) return rc;
    if ((rc = c->band_recs_w.ensure((size_t)kNumBandClasses * std::max<size_t>(n_items, 1) * 3 * sizeof(int4)))) return rc;
    if ((rc = c->state_i32.ensure(nl * 4 * 4))) return rc;
    if ((rc = c->state_f64.ensure(nl * 8))) return rc;
    if ((rc = c->spec.ensure(nr * 16))) return rc;
    if ((rc = c->rhash.ensure(nr * 8))) return rc;
    if ((rc = c->rep.ensure(nr * 4))) return rc;
    if ((rc = c->exact.ensure(nr))) return rc;
    if (!c->scratch.p) {
        if ((rc = c->scratch.ensure(((size_t)kLongWaves * c->long_slot_ints + c->generic_ints) * 4))) return rc;
        c->scratch_ints = (size_t)kLongWaves * c->long_slot_ints + c->generic_ints;
    }
    return 0;
}

KArgs make_args(strk_ctx* c, const strk_batch* b, int end_flags, int window, int table_stride, int list_stride,
                const strk_params* sp) {
    KArgs a;
    memset(&a, 0, sizeof a);
    a.seqs = b->seqs; a.seq_off = b->seq_off; a.nfl = b->nfl; a.ntr = b->ntr; a.nfr = b->nfr;
    a.est_cn = b->est_cn; a.read_off = b->read_off; a.motifs = b->motifs; a.motif_off = b->motif_off;
    a.n_reads = b->n_reads; a.n_loci = b->n_loci;
    a.read_locus = c->read_locus.as<int32_t>();
    a.win_lo = c->win_lo.as<int32_t>();
    a.win_n = c->win_n.as<int32_t>();
    a.tab_off = c->tab_off.as<int64_t>();
    a.table = c->table.as<int32_t>();
    a.ub = c->ub.as<int32_t>();   // (sized by the calls that can run the band kernels: ensure_workspace)
    a.cls_list = c->cls_list.as<int32_t>();
    a.band_recs = c->band_recs.as<int4>();
    a.band_recs_w = a.band_recs;   // (k_sort_wide's copy when that kernel is launched: enqueue_scoring)
    a.wide_hist = reinterpret_cast<int32_t*>(c->counters.as<char>() + kWideHistOff);
    a.counters = c->counters.as<int32_t>();
    a.cells = reinterpret_cast<unsigned long long*>(c->counters.as<char>() + kCellsOff);
    a.scratch_used = a.cells + 1;
    a.scratch = c->scratch.as<int32_t>();
    a.scratch_cap = (long long)c->scratch_ints;
    a.long_slot = (long long)c->long_slot_ints;
    a.long_waves = kLongWaves;
    a.list_stride = list_stride;
    c->last_list_stride = list_stride;
    a.band_tune = {kBandSpanW, kBandSlackM8, kBandSpanMaxMotif};
    a.end_flags = end_flags;
    a.window = window;
    for (int k = 0; k < kWinBuckets; ++k) a.window_b[k] = c->p_window_b[k] > 0 ? c->p_window_b[k] : window;
    a.table_stride = table_stride;
    if (sp) {  // speculative search for start == est_cn inside the DP kernel
        a.spec = static_cast<int4*>(c->spec.p);
        a.max_iters = sp->max_iters; a.lsr = sp->local_search_range; a.step = sp->step_size;
        a.tie_last = sp->tie_rule == STRK_TIE_LAST;
        a.narrow = sp->narrowing;
        a.rep = c->rep.as<int32_t>();
        a.rhash = sp->no_dedupe ? nullptr : c->rhash.as<unsigned long long>();
        a.exact = c->exact.as<uint8_t>();
        a.band_mode = (!sp->no_band && c->band.cooldown == 0) ? 1 : 0;
        a.band_limit = c->band.probation ? kBandProbationReads : INT32_MAX;
    }
    return a;
}

// plan (classification) + all DP kernels for the reads in `items` (NULL = all reads).
void enqueue_scoring(strk_ctx* c, const KArgs& a, int mode, const int32_t* d_items, int n_items, int force_generic,
                     hipStream_t st, bool time_dp, const ReplayArgs* pre_replay = nullptr) {
    // Longest-first order of the wide band classes (k_sort_wide) pays when their chunks are few against the ~2 000 resident waves —
    // the launch then lasts as long as its longest chunk and whatever was started late (BASELINE config 5 at one GPU's share:
    // 6 400 chunks, k_dp_band_wide 3.77 -> 3.38 ms).  Two small kernels (strk_kernels.h: k_sort_wide_hist, k_sort_wide); run when
    // the previous call had at most 8 192 wide chunks (a first call sorts).  With more — config 4's shard: 16 000 — the order
    // still shortens k_dp_band_wide (2.03 -> 1.80 ms with ONE call on the device, sort included), but with two calls in flight the
    // two extra launches between the band kernels moved the calls into the pattern in which their band passes co-run: the
    // default bench gave 92.8 M reads/s twice where the unsorted queue gives 103-111 (profiles/r04_sort_wide_always_experiment.txt).
    const bool hist = c->hist.usable(mode, a.band_mode);   // the previous call's queue lengths say something about this one's
    const bool sort_wide = a.band_mode && mode == 0 && !force_generic && (!hist || (c->hist.wide_chunks > 0 && c->hist.wide_chunks <= 8192));
    const int plan_scope = plan_scope_of(n_items);   // small calls: one read per thread over more blocks (strk_plan_order.h)
    hipLaunchKernelGGL(k_plan, dim3((n_items + plan_scope - 1) / plan_scope), dim3(kPlanThreads), 0, st, a, mode, d_items, n_items, force_generic,
                       plan_reads_per_thread(n_items));
    // A call that shares the device with other calls in flight takes fifteen sixteenths of the CU slots per kernel: the free
    // slots are what lets the LDS-holding tail kernels of one call (k_dp_band_wide, k_dp_all, k_dp_long) start while another
    // call's band pass is resident; k_hash / k_replay need no LDS, k_plan 4 KB, and all three fit NEXT to two band waves per SIMD
    // (2 x 168 of 512 VGPRs; strk_plan_order.h).  tools/grid_sweep2.sh, two calls in flight: 448 blocks 239 M reads/s, 480 -> 246 M, 496 -> 240 M, 512 -> 186 M
    // (round 2, three calls in flight and 219 VGPRs: 7/8 was the best).
    // ... which pays when ONE kernel carries the call (BASELINE config 2: k_dp_band 1.15 ms, the others 0.13 ms; configs 3 and 5
    // alike: k_dp_all / k_dp_band_wide alone).  Where k_dp_band AND k_dp_band_wide are both large — config 4's shard: 3.4 and 2.0
    // ms — two calls' big kernels take turns on fifteen sixteenths of the chip each (measured with two calls in flight: 7.1 ms
    // per call against 6.55 ms with whole grids; the other way round for configs 3 and 5: 8.9 against 7.7 ms, 3.5 against 2.65 ms):
    // such a context takes the whole grid (GridHistory::tail_heavy, from the previous call's cell counts).
    const bool overlap = g_calls_in_flight.load(std::memory_order_relaxed) > 1;
    const bool heavy = c->hist.valid && c->hist.tail_heavy;
    const int sixteenths = (overlap && !heavy) ? 15 : 16;
    // grids of the sparsely used kernels: what the previous call's queues predict for this batch (GridHistory)
    auto predicted_blocks = [&](int chunks, int full) { return c->hist.predicted_blocks(hist, chunks, a.n_reads, full); };
    if (time_dp) (void)hipEventRecord(c->ev[kEvHead], st);
    const bool band = a.band_mode && mode == 0 && !force_generic;
    // The band kernels leave their tables unsearched: the certificate search from the estimate, and the listing of the reads that
    // fail it, are step 1 of k_replay's first pass (strk_replay.h), which needs spec[] to store to.  A band call without that pass
    // would turn every band read into an event of the walk and break the fall-back counts: only submit_device turns the band on,
    // and it gives both.
    assert(!band || (pre_replay && a.spec));
    int band_blocks = 1;
    if (band && time_dp) {
        // Whole-grid mode (two large kernels per call): which way two calls in flight share the device is decided by their phase.
        // Half a period apart, one call's k_dp_band_wide and tails run inside the other's k_dp_band (config 4's shard: 5.8 ms per
        // call); in phase, the two band passes co-run at half speed, then the two wide passes, and the tails of both are left with
        // nothing to hide in (6.9 ms).  Both patterns sustain themselves; two submits in a row on an idle device start the second
        // one.  So a band pass waits for the band pass enqueued before it, whichever context that was: the calls fall half a
        // period apart by themselves.
        std::lock_guard<std::mutex> lk(g_band_chain_mu);
        if (sixteenths == 16 && overlap && g_band_chain_ev && g_band_chain_ev != c->ev[kEvBand].h && g_band_chain_dev == c->device)
            (void)hipStreamWaitEvent(st, g_band_chain_ev, 0);
    }
    if (band) {
        // banded first pass: band scores and their bounds per read; the first k_replay pass below searches them and appends the
        // reads that do not certify to the exact lists
        band_blocks = std::max(1, std::min(256 * kBandBlocksPerCU * sixteenths / 16, (a.list_stride + 3) / 4));
        hipLaunchKernelGGL(k_dp_band, dim3(band_blocks), dim3(256), 0, st, a);
    }
    if (time_dp) (void)hipEventRecord(c->ev[kEvBand], st);
    if (band && time_dp) {
        std::lock_guard<std::mutex> lk(g_band_chain_mu);
        g_band_chain_ev = c->ev[kEvBand].h;
        g_band_chain_dev = c->device;
    }
    if (band) {   // long windows
        KArgs aw = a;
        if (sort_wide) {
            hipLaunchKernelGGL(k_sort_wide_hist, dim3(kSortWideBlocks, kNumWideLists), dim3(256), 0, st, a);
            hipLaunchKernelGGL(k_sort_wide, dim3(kSortWideBlocks, kNumWideLists), dim3(256), 0, st, a, c->band_recs_w.as<int4>());
            aw.band_recs_w = c->band_recs_w.as<int4>();
        }
        const int wide_full = std::max(1, std::min(256 * kBandBlocksPerCU * sixteenths / 16, (a.list_stride + 3) / 4));
        hipLaunchKernelGGL(k_dp_band_wide, dim3(predicted_blocks(c->hist.wide_chunks, wide_full)), dim3(256), 0, st, aw);
    }
    if (time_dp) (void)hipEventRecord(c->ev[kEvWide], st);
    // first k_replay pass (strk_replay.h): the certificate search of the band tables, then each locus as far as certified tables
    // carry it, before the exact kernels
    if (band && pre_replay) hipLaunchKernelGGL(k_replay, dim3(a.n_loci), dim3(64), 0, st, a, *pre_replay);
    if (time_dp) (void)hipEventRecord(c->ev[kEvPre], st);
    if (!force_generic) {
        // persistent-style grid: every wave pulls chunks from the device-side queue until it is empty
        constexpr int kBlocksPerCU = std::max(1, std::min(8, (160 * 1024) / (4 * kWaveLdsBytes + kLdsSlack + 1024)));
        const int full = std::max(1, std::min(256 * kBlocksPerCU * sixteenths / 16, (a.list_stride + 3) / 4));
        const int blocks = a.ref_mode ? full : predicted_blocks(c->hist.exact_chunks, full);
        if (a.ref_mode) hipLaunchKernelGGL(k_dp_ref, dim3(blocks), dim3(256), 0, st, a);
        else hipLaunchKernelGGL(k_dp_all, dim3(blocks), dim3(256), 0, st, a);
    }
    if (time_dp) (void)hipEventRecord(c->ev[kEvExact], st);
    KArgs al = a;
    if (!force_generic && !a.ref_mode) {
        // longest first when there are more long items than resident waves (k_sort_long) — by the previous call's count, or
        // the item count the host knows (window-miss rounds, explicit tables); a call without them does not pay the launch
        const bool many_long = mode == 0 ? (!hist || c->hist.n_long > kLongWaves) : a.list_stride > kLongWaves;   // (no history: one block finds out)
        if (many_long && !c->long_list.ensure((size_t)std::max(1, a.list_stride) * 2 * 4)) {
            hipLaunchKernelGGL(k_sort_long, dim3(1), dim3(1024), 0, st, a, c->long_list.as<int32_t>());
            al.long_sorted = c->long_list.as<int32_t>();
        }
    }
    if (!force_generic && !a.ref_mode)   // (a window-miss round or an explicit table: never more blocks than items)
        hipLaunchKernelGGL(k_dp_long, dim3(mode == 0 ? predicted_blocks(c->hist.n_long, kLongBlocks) : std::max(1, std::min(kLongBlocks, a.list_stride))),
                           dim3(256), 0, st, al);
    if (time_dp) (void)hipEventRecord(c->ev[kEvLong], st);
    hipLaunchKernelGGL(k_dp_generic, dim3(1024), dim3(256), 0, st, a);   // one wave per (item, candidate): 4 096 waves
    if (time_dp) (void)hipEventRecord(c->ev[kEvGeneric], st);
}

// A call asked for more scratch than the context holds — rows of the generic kernel (its pool starts at 64 MiB), or a slot of
// k_dp_long for a window longer than ~20 000 candidate rows (a slot starts at 192 KiB): make that part as large as what was
// asked for (the device counted every request, served or not) and say that the call is to be run again.  Reads the generic
// kernel takes are rare (an empty flank, more than eight distinct symbols in a window, a motif longer than kMotifMax), and so
// are start counts dozens of times the tract's size, but a batch of a few hundred loci made of either must not fail for it.
bool grow_scratch(strk_ctx* c) {
    const int bits = c->h_counters.cnt(kCntError);
    if (!(bits & (kErrScratch | kErrLongSlot))) return false;
    size_t slot = c->long_slot_ints, gen = c->generic_ints;
    if (bits & kErrLongSlot) {
        const size_t need = (size_t)std::max(0, c->h_counters.cnt(kCntLongNeed));
        if (need <= slot || need > kLongSlotMaxInts) return false;
        slot = (need + need / 8 + 1023) & ~(size_t)1023;
    }
    if (bits & kErrScratch) {
        const unsigned long long used = c->h_counters.scratch_used();
        if (used <= gen || used > kGenericPoolMaxInts) return false;
        gen = (size_t)used + (1u << 16);
    }
    const size_t want = (size_t)kLongWaves * slot + gen;
    if (c->scratch.ensure(want * 4, false)) return false;
    c->long_slot_ints = slot;
    c->generic_ints = gen;
    c->scratch_ints = want;
    return true;
}

int check_error_bits(int bits) {
    if (bits & kErrBadInput) return fail(STRK_E_INVALID, "batch holds an empty motif or a negative length");
    if (bits & kErrScratch) return fail(STRK_E_NOMEM, "generic-kernel scratch exhausted (inputs too large for one call)");
    if (bits & kErrList) return fail(STRK_E_NOMEM, "a kernel's item list is full (more items than the call sized its lists for)");
    if (bits & kErrLongSlot) return fail(STRK_E_NOMEM, "a window is too long for the long-read kernel's scratch slot (|db| + 2 x candidate rows > %zu)", kLongSlotMaxInts);
    if (bits & kErrEmpty) return fail(STRK_E_EMPTY, "max() arg is an empty sequence: no candidate size could be scored for some read");
    return 0;
}

// Scores the windows `a` describes (enqueue_scoring in mode 1: explicit tables, window-miss rounds) and waits for the counters;
// a run that asked for more scratch than the context holds is repeated with the scratch grown (grow_scratch), up to three
// times, `a` (and `outer`, the arguments of the call a window-miss round belongs to) patched to it.  copy_bytes > 0: that much
// of `copy_src` comes back to `copy_dst` in the same stream-ordered batch as the counters.
int score_until_scratch_fits(strk_ctx* c, KArgs& a, const int32_t* d_items, int n_items, int force_generic, hipStream_t st,
                             bool timed, KArgs* outer = nullptr, void* copy_dst = nullptr, const void* copy_src = nullptr,
                             size_t copy_bytes = 0) {
    for (int attempt = 0;; ++attempt) {
        HIP_TRY(hipMemsetAsync(c->counters.p, 0, kCountersBytes, st));
        if (timed) HIP_TRY(hipEventRecord(c->ev[kEvStart], st));
        enqueue_scoring(c, a, 1, d_items, n_items, force_generic, st, timed);
        if (timed) HIP_TRY(hipEventRecord(c->ev[kEvEnd], st));
        HIP_TRY(hipMemcpyAsync(c->h_counters.mem.p, c->counters.p, kCountersBytes, hipMemcpyDeviceToHost, st));
        if (copy_bytes) HIP_TRY(hipMemcpyAsync(copy_dst, copy_src, copy_bytes, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        HIP_TRY(hipGetLastError());
        if (attempt >= 3 || !grow_scratch(c)) return 0;
        for (KArgs* k : {&a, outer}) {
            if (!k) continue;
            k->scratch = c->scratch.as<int32_t>();
            k->scratch_cap = (long long)c->scratch_ints;
            k->long_slot = (long long)c->long_slot_ints;
        }
    }
}

#include "strk_host_miss.inc"

// Enqueue one batched call on `st` and return without waiting.
int submit_device(strk_ctx* c, const strk_batch* b, const strk_params* params, int32_t* out_cn, int32_t* out_score,
                  int32_t* out_n, int32_t* out_start, hipStream_t st) {
    if (c->pending) return fail(STRK_E_INVALID, "context already holds a submitted call: strk_finish() it first");
    strk_params p;
    int rc;
    if ((rc = check_params(params, &p))) return rc;
    if (!b || b->n_reads < 0 || b->n_loci < 0) return fail(STRK_E_INVALID, "bad batch");
    // default window: 8 sizes either side of the estimate to begin with, then what the sample needs (g_window)
    c->p_window_auto = params->window <= 0;
    for (int k = 0; k < kWinBuckets; ++k) c->p_window_b[k] = 0;
    if (c->p_window_auto) {
        p.window = 0;
        for (int k = 0; k < kWinBuckets; ++k) {
            c->p_window_b[k] = g_window.window(k, p.local_search_range + p.step_size);
            p.window = std::max(p.window, c->p_window_b[k]);
        }
    }
    c->p_batch = *b;
    c->p_params = p;
    c->p_params_in = *params;
    c->p_stream = st;
    if (b->n_reads == 0 || b->n_loci == 0) {
        c->pending = true;
        g_calls_in_flight.fetch_add(1, std::memory_order_relaxed);
        return 0;
    }
    if (!out_cn || !out_score || !out_n || !out_start) return fail(STRK_E_INVALID, "output pointer is NULL");
    HIP_TRY(hipSetDevice(c->device));
    const int ts = std::min(kTableMax - 1, 2 * (p.window + 7) + 1);   // room for k_plan's per-read widening
    if ((rc = ensure_workspace(c, b->n_reads, b->n_loci, (size_t)b->n_reads * ts, (size_t)b->n_reads, !p.no_band))) return rc;
    KArgs a = make_args(c, b, p.end_flags, p.window, ts, b->n_reads, &p);
    ReplayArgs rp;
    rp.max_iters = p.max_iters; rp.lsr = p.local_search_range; rp.step = p.step_size;
    rp.tie_last = p.tie_rule == STRK_TIE_LAST; rp.feedback = p.feedback; rp.narrow = p.narrowing;
    rp.out_cn = out_cn; rp.out_score = out_score; rp.out_n = out_n; rp.out_start = out_start;
    rp.next_read = c->state_i32.as<int32_t>();
    rp.need_lo = rp.next_read + b->n_loci;
    rp.need_hi = rp.need_lo + b->n_loci;
    rp.stop = rp.need_hi + b->n_loci;
    rp.frac = c->state_f64.as<double>();
    rp.resume = 0;
    rp.pre_exact = 0;

    struct InFlight {   // counted before the launches (the grid size depends on it), un-counted on any early error return
        bool keep = false;
        InFlight() { g_calls_in_flight.fetch_add(1, std::memory_order_relaxed); }
        ~InFlight() { if (!keep) g_calls_in_flight.fetch_sub(1, std::memory_order_relaxed); }
    } in_flight;
    HIP_TRY(hipEventRecord(c->ev[kEvStart], st));
    HIP_TRY(hipMemsetAsync(c->counters.p, 0, kCountersAllBytes, st));
    if (a.rhash) hipLaunchKernelGGL(k_hash, dim3((b->n_reads + 31) / 32), dim3(256), 0, st, a);   // eight lanes per read
    ReplayArgs rp_pre = rp;
    rp_pre.pre_exact = 1;
    enqueue_scoring(c, a, 0, nullptr, b->n_reads, 0, st, true, a.band_mode ? &rp_pre : nullptr);
    rp.resume = a.band_mode ? 1 : 0;   // band calls: the second pass, behind the exact kernels (strk_replay.h)
    hipLaunchKernelGGL(k_replay, dim3(b->n_loci), dim3(64), 0, st, a, rp);
    HIP_TRY(hipMemcpyAsync(c->h_counters.mem.p, c->counters.p, kCountersBytes, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipEventRecord(c->ev[kEvEnd], st));
    HIP_TRY(hipGetLastError());
    c->p_args = a;
    c->p_replay = rp;
    c->pending = true;
    in_flight.keep = true;
    return 0;
}

// strk_stats of the call whose counters are in: event spans along the call, byte and cell counts, the windows it ran with
void fill_stats(strk_ctx* c, const HostCounters& n, strk_stats* stats) {
    auto span = [&](int from, int to) {
        float ms = 0.f;
        return hipEventElapsedTime(&ms, c->ev[from], c->ev[to]) == hipSuccess ? ms : 0.f;
    };
    stats->kernel_ms = span(kEvStart, kEvEnd);
    stats->head_ms = span(kEvStart, kEvHead);
    stats->band_kernel_ms = span(kEvHead, kEvBand);
    stats->band_wide_kernel_ms = span(kEvBand, kEvWide);
    stats->dp_kernel_ms = span(kEvPre, kEvExact);
    stats->long_kernel_ms = span(kEvExact, kEvLong);
    stats->generic_kernel_ms = span(kEvLong, kEvGeneric);
    stats->replay_ms = span(kEvGeneric, kEvEnd) + span(kEvWide, kEvPre);   // both k_replay passes
    stats->band_bytes = (int64_t)n.band_bytes();
    stats->exact_bytes = (int64_t)n.exact_bytes();
    stats->wide_bytes = (int64_t)n.wide_bytes();
    stats->long_bytes = (int64_t)n.long_bytes();
    stats->band_cells = (int64_t)n.cells_of(kCellBand);
    stats->wide_cells = (int64_t)n.cells_of(kCellWide);
    stats->exact_cells = (int64_t)n.cells_of(kCellExact);
    stats->long_cells = (int64_t)n.cells_of(kCellLong);
    stats->n_long_reads = n.cnt(kCntClass0 + kLongClass);
    stats->n_dp_launches = 2;
    stats->window_used = c->p_params.window;
    for (int k = 0; k < kWinBuckets; ++k)   // the window each motif-length bucket ran with (0: no locus of that bucket in the call)
        stats->window_bucket[k] = n.cnt(kCntLociB + k) > 0 ? (c->p_window_b[k] > 0 ? c->p_window_b[k] : c->p_params.window) : 0;
    if (c->p_window_auto) {   // the widest default window among the motif-length buckets that had loci in this call
        int w = 0;
        for (int k = 0; k < kWinBuckets; ++k) w = std::max(w, stats->window_bucket[k]);
        if (w > 0) stats->window_used = w;
    }
    stats->n_fallback = n.cnt(kCntClass0 + kGenericClass);
    stats->n_dedup_reads = n.cnt(kCntDup);
    stats->n_band_reads = n.band_reads();
    stats->n_band_fallback = n.cnt(kCntBandFallback);
    stats->dp_cells = (int64_t)n.cells();
}

// queue lengths of the finished call (wave chunks of k_dp_all and of k_dp_band_wide), for the grids of the next one
void update_grid_history(strk_ctx* c, const HostCounters& n) {
    int exact_chunks = 0, wide_chunks = 0;
    for (int k = 0; k < kNumClasses; ++k) {
        const int per = 64 / class_G(k);
        exact_chunks += (n.cnt(kCntClass0 + k) + per - 1) / per;
    }
    for (int k = 0; k < kNumBandClasses; ++k) {   // the classes of k_dp_band_wide
        if (!band_class_wide_kernel(k)) continue;
        const int per = 64 / band_class_G(k);
        wide_chunks += (n.cnt(kCntClass0 + kBandClass0 + k) + per - 1) / per;
    }
    const bool on_probation = c->p_args.band_mode && c->p_args.band_limit != INT32_MAX;
    c->hist.update(on_probation, c->p_args.band_mode, c->p_batch.n_reads, exact_chunks, wide_chunks, n.cnt(kCntClass0 + kLongClass),
                   n.cells_of(kCellBand), n.cells_of(kCellWide));
}

// Wait for the submitted call, check for errors and resolve window misses.
int finish_device(strk_ctx* c, strk_stats* stats) {
    if (stats) memset(stats, 0, sizeof *stats);
    if (!c->pending) return fail(STRK_E_INVALID, "nothing was submitted on this context");
    c->pending = false;
    g_calls_in_flight.fetch_sub(1, std::memory_order_relaxed);
    const strk_batch* b = &c->p_batch;
    if (b->n_reads == 0 || b->n_loci == 0) return 0;
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipEventSynchronize(c->ev[kEvEnd]));
    HIP_TRY(hipGetLastError());
    if (c->scratch_reruns < 3 && grow_scratch(c)) {   // the same call once more, with the scratch it asked for
        const strk_batch again = c->p_batch;
        const strk_params pin = c->p_params_in;
        const ReplayArgs rp = c->p_replay;
        ++c->scratch_reruns;
        int rc = submit_device(c, &again, &pin, rp.out_cn, rp.out_score, rp.out_n, rp.out_start, c->p_stream);
        if (!rc) rc = finish_device(c, stats);
        --c->scratch_reruns;
        return rc;
    }
    const HostCounters& n = c->h_counters;
    if (stats) fill_stats(c, n, stats);
    const int band_reads = n.band_reads(), band_fallbacks = n.cnt(kCntBandFallback);
    // (a call whose band certificates mostly failed reports those reads as misses too: not a window problem)
    const bool band_unhealthy = c->p_args.band_mode && strk_policy::BandGate::mostly_failed(band_reads, band_fallbacks);
    if (c->p_window_auto && !band_unhealthy)
        for (int k = 0; k < kWinBuckets; ++k) g_window.update(k, n.cnt(kCntLociB + k), n.cnt(kCntMissB + k));
    update_grid_history(c, n);
    c->band.update(band_reads, band_fallbacks);
    const int err = n.cnt(kCntError);
    int rc;
    if ((rc = check_error_bits(err & ~kErrEmpty))) return rc;
    if (n.cnt(kCntMiss) > 0) return resolve_misses(c, b, c->p_params, c->p_args, c->p_replay, c->p_stream, stats, err);
    return check_error_bits(err);
}

int count_device(strk_ctx* c, const strk_batch* b, const strk_params* params, int32_t* out_cn, int32_t* out_score,
                 int32_t* out_n, int32_t* out_start, hipStream_t st, strk_stats* stats) {
    if (stats) memset(stats, 0, sizeof *stats);
    const int rc = submit_device(c, b, params, out_cn, out_score, out_n, out_start, st);
    if (rc) return rc;
    return finish_device(c, stats);
}

// The offsets of loci [l0, l1) of a host batch: their reads in order, no motif empty.
int check_batch_loci(const strk_batch* b, size_t l0, size_t l1) {
    for (size_t l = l0; l < l1; ++l) {
        if (b->read_off[l + 1] < b->read_off[l]) return fail(STRK_E_INVALID, "read_off must be non-decreasing");
        if (b->motif_off[l + 1] <= b->motif_off[l]) return fail(STRK_E_INVALID, "locus %zu has an empty motif", l);
    }
    return 0;
}

// Loci [l0, l1) of a host batch and their reads are well-formed (every array of the batch is there; read_off[l0] is valid).
int check_batch_range(const strk_batch* b, size_t l0, size_t l1) {
    if (const int rc = check_batch_loci(b, l0, l1)) return rc;
    for (size_t r = (size_t)b->read_off[l0]; r < (size_t)b->read_off[l1]; ++r) {
        if (b->nfl[r] < 0 || b->ntr[r] < 0 || b->nfr[r] < 0) return fail(STRK_E_INVALID, "read %zu has a negative length", r);
        if (b->seq_off[r + 1] - b->seq_off[r] != (int64_t)b->nfl[r] + b->ntr[r] + b->nfr[r])
            return fail(STRK_E_INVALID, "read %zu: seq_off does not match nfl+ntr+nfr", r);
    }
    return 0;
}

// The stream of every call that is given none (strk_ctx::side).
int side_stream(strk_ctx* c, hipStream_t* st) {
    if (!c->side) HIP_TRY(hipStreamCreateWithFlags(&c->side.h, hipStreamNonBlocking));
    *st = c->side;
    return 0;
}

// uploads a host batch into the context's staging buffer on the context's side stream; returns a batch of device pointers and
// (unless the batch is empty) that stream
// `d_seqs` (optional): the bases are in device memory already (strk_dbam_extract); b->seqs is not read then
int upload_batch(strk_ctx* c, const strk_batch* b, strk_batch* d, hipStream_t* side, const uint8_t* d_seqs = nullptr) {
    if (!b || b->n_reads < 0 || b->n_loci < 0) return fail(STRK_E_INVALID, "bad batch");
    *d = *b;
    if (b->n_reads == 0 || b->n_loci == 0) return 0;
    if (!b->seq_off || !b->nfl || !b->ntr || !b->nfr || !b->read_off || !b->motifs || !b->motif_off)
        return fail(STRK_E_INVALID, "batch pointer is NULL");
    const size_t nr = (size_t)b->n_reads, nl = (size_t)b->n_loci;
    if (b->read_off[0] != 0 || b->read_off[nl] != b->n_reads) return fail(STRK_E_INVALID, "read_off must span [0, n_reads]");
    int rc;
    if ((rc = check_batch_range(b, 0, nl))) return rc;
    const size_t nbases = (size_t)b->seq_off[nr], nmot = (size_t)b->motif_off[nl];
    if (nbases && !b->seqs && !d_seqs) return fail(STRK_E_INVALID, "seqs is NULL");
    HIP_TRY(hipSetDevice(c->device));
    if ((rc = side_stream(c, side))) return rc;
    const hipStream_t st = *side;
    const struct { const void* src; size_t bytes; } part[9] = {
        {b->seqs, d_seqs ? 0 : nbases}, {b->seq_off, (nr + 1) * 8}, {b->nfl, nr * 4}, {b->ntr, nr * 4}, {b->nfr, nr * 4},
        {b->est_cn, nr * 4}, {b->read_off, (nl + 1) * 4}, {b->motifs, nmot}, {b->motif_off, (nl + 1) * 4}};
    Carve cv;
    size_t at[9];
    for (int k = 0; k < 9; ++k) at[k] = cv.take(part[k].bytes);
    if ((rc = c->stage_in.ensure(cv.bytes))) return rc;
    const DevBuf& s = c->stage_in;
    for (int k = 0; k < 9; ++k)
        if (part[k].src && part[k].bytes) HIP_TRY(hipMemcpyAsync(s.at<char>(at[k]), part[k].src, part[k].bytes, hipMemcpyHostToDevice, st));
    if (!b->est_cn) HIP_TRY(hipMemsetAsync(s.at<char>(at[5]), 0, nr * 4, st));
    d->seqs = d_seqs ? d_seqs : s.at<uint8_t>(at[0]);
    d->seq_off = s.at<int64_t>(at[1]); d->nfl = s.at<int32_t>(at[2]); d->ntr = s.at<int32_t>(at[3]); d->nfr = s.at<int32_t>(at[4]);
    d->est_cn = s.at<int32_t>(at[5]); d->read_off = s.at<int32_t>(at[6]); d->motifs = s.at<uint8_t>(at[7]);
    d->motif_off = s.at<int32_t>(at[8]);
    return 0;
}

// One timed launch sequence on `st`: the events of the context bracket it, `copies_down` (returns 0 or an error code) enqueues
// behind the closing event what the wait is to cover as well, the call waits for it: with one synchronise, or, given limit_s,
// by polling the stream for at most that many seconds.  A failed wait is reported as "<fn>: <what>: <error>" (fn may be NULL).
template <class F, class G = int (*)()>
int timed_launch(strk_ctx* c, hipStream_t st, strk_stats* stats, const char* fn, const char* what, int n_launches, F&& launch,
                 G&& copies_down = +[] { return 0; }, double limit_s = 0.0) {
    hipEvent_t ev0 = c->ev[0], ev1 = c->ev[kNumEvents - 1];
    HIP_TRY(hipEventRecord(ev0, st));
    launch();
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(ev1, st));
    if (const int rc = copies_down()) return rc;
    const char* sep = fn ? ": " : "";
    hipError_t q;
    if (limit_s > 0.0) {
        const auto t0 = std::chrono::steady_clock::now();
        while ((q = hipStreamQuery(st)) == hipErrorNotReady) {
            if (std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() > limit_s)
                return fail(STRK_E_DEVICE, "%s%s%s did not finish within %.0f s", fn ? fn : "", sep, what, limit_s);
            usleep(50);
        }
        (void)hipGetLastError();   // (a "not ready" of the polling is no error of the next call)
    } else {
        q = hipStreamSynchronize(st);
    }
    if (q != hipSuccess) return fail(STRK_E_DEVICE, "%s%s%s: %s", fn ? fn : "", sep, what, hipGetErrorString(q));
    float ms = 0.f;
    HIP_TRY(hipEventElapsedTime(&ms, ev0, ev1));
    if (stats) {
        stats->kernel_ms += ms;
        stats->n_dp_launches += n_launches;
    }
    return 0;
}

// bases that are on the device already must be on THIS context's device (no peer access is set up)
int check_dseqs(strk_ctx* c, const char* fn, const void* d_seqs) {
    (void)hipSetDevice(c->device);
    hipPointerAttribute_t attr;
    if (hipPointerGetAttributes(&attr, d_seqs) != hipSuccess || attr.type != hipMemoryTypeDevice || attr.device != c->device) {
        (void)hipGetLastError();
        return fail(STRK_E_INVALID, "%s: d_seqs is not device memory of device %d (the context's)", fn, c->device);
    }
    return 0;
}

// strk_params with the semantics of the scalar calls (strk_repeat_count, and the final counts of the reference side): the first
// maximum, every end free, no feedback, and the window those calls take for their search schedule
strk_params default_params(int32_t max_iters, int32_t lsr, int32_t step) {
    strk_params p;
    memset(&p, 0, sizeof p);
    p.max_iters = max_iters; p.local_search_range = lsr; p.step_size = step;
    p.tie_rule = STRK_TIE_FIRST; p.end_flags = STRK_SG_ALL; p.feedback = 0;
    p.window = std::min(15, std::max(kDefaultWindow, lsr + step + 1));
    return p;
}

// The offset arrays of a batch of one read of one locus, in one block (the head of the fast path's device image) ...
struct OneRead {
    int64_t seq_off[2];
    int32_t lens[4];   // nfl, ntr, nfr, est_cn
    int32_t read_off[2], motif_off[2];
};
// ... and the batch over such a block where it lies (`at`: host or device; only addresses are taken), its bases and its motif
strk_batch one_read_batch(const OneRead* at, const uint8_t* seqs, const uint8_t* motif) {
    return {1, 1, seqs, at->seq_off, at->lens, at->lens + 1, at->lens + 2, at->lens + 3, at->read_off, motif, at->motif_off};
}

#include "strk_host_pipe.inc"

// strk_repeat_count's fast path: ONE copy up (the read's arrays in one pinned image), k_scalar_plan + k_dp_all on one block,
// ONE copy down (the search result) — instead of the batched path's nine uploads, dozen launches and four downloads for a
// single read (about 0.1 ms).  Returns 0 with the result, 1 when the read has to go the general way (no fast class, more than
// eight symbol classes, a search that leaves the window, nothing scored), < 0 on an error.
constexpr size_t kScalarSeqMax = 1792, kScalarMotifMax = 256;
constexpr size_t kScOffMotif = sizeof(OneRead), kScOffSeq = kScOffMotif + kScalarMotifMax, kScBytes = kScOffSeq + kScalarSeqMax + 64;
static_assert(kScOffMotif == 48, "the fast path's image: 48 bytes of offsets, the motif, the bases");
int scalar_fast(strk_ctx* c, int32_t start, const uint8_t* tr, int32_t ntr, const uint8_t* fl, int32_t nfl, const uint8_t* fr, int32_t nfr,
                const uint8_t* motif, int32_t m, strk_params p, int32_t* cn, int32_t* score, int32_t* n_explored) {
    const size_t ndb = (size_t)nfl + ntr + nfr;
    if (c->pending || nfl < 1 || nfr < 1 || ndb + 1 > kScalarSeqMax || (size_t)m > kScalarMotifMax || p.local_search_range < 0 || p.step_size < 1)
        return 1;
    HIP_TRY(hipSetDevice(c->device));
    int rc;
    hipStream_t st;
    if ((rc = side_stream(c, &st))) return rc;
    if (!c->sc_host.p) HIP_TRY(c->sc_host.alloc(kScBytes));
    if (!c->sc_out.p) HIP_TRY(c->sc_out.alloc(64));
    if ((rc = c->stage_in.ensure(kScBytes))) return rc;
    const int ts = std::min(kTableMax - 1, 2 * (p.window + 7) + 1);
    if ((rc = ensure_workspace(c, 1, 1, (size_t)ts, 1))) return rc;
    uint8_t* h = c->sc_host.as<uint8_t>();
    const OneRead head{{0, (int64_t)ndb}, {nfl, ntr, nfr, start}, {0, 1}, {0, m}};
    memcpy(h, &head, sizeof head);
    memcpy(h + kScOffMotif, motif, (size_t)m);
    memcpy(h + kScOffSeq, fl, (size_t)nfl);
    if (ntr) memcpy(h + kScOffSeq + nfl, tr, (size_t)ntr);
    memcpy(h + kScOffSeq + nfl + ntr, fr, (size_t)nfr);
    const size_t up = kScOffSeq + ndb;
    HIP_TRY(hipMemcpyAsync(c->stage_in.p, h, up, hipMemcpyHostToDevice, st));
    const uint8_t* d = c->stage_in.as<uint8_t>();
    const strk_batch b = one_read_batch(c->stage_in.as<OneRead>(), d + kScOffSeq, d + kScOffMotif);
    p.no_dedupe = 1; p.no_band = 1;
    for (int k = 0; k < kWinBuckets; ++k) c->p_window_b[k] = 0;
    KArgs a = make_args(c, &b, p.end_flags, p.window, ts, 1, &p);
    hipLaunchKernelGGL(k_scalar_plan, dim3(1), dim3(64), 0, st, a, (int)(kCountersBytes / 4));
    hipLaunchKernelGGL(k_dp_all, dim3(1), dim3(256), 0, st, a);
    HIP_TRY(hipMemcpyAsync(c->sc_out.p, a.spec, sizeof(int4), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    HIP_TRY(hipGetLastError());
    const int4 r = *c->sc_out.as<int4>();
    if (r.w != 0) return 1;   // miss / nothing scored / not scored at all: the general path decides (and reports)
    *cn = r.x; *score = r.y; *n_explored = r.z;
    return 0;
}

// strk_score_table / strk_score_ref_table: explicit candidate windows per read, HOST buffers.
// ref_mode = 1 scores the reference-side candidate fl + motif*i (no right flank) and also returns
// the db position where the alignment ends (repeats.py:23-43).
int score_table_impl(strk_ctx* ctx, const strk_batch* batch, const int32_t* lo, const int32_t* n,
                     const int64_t* table_off, int32_t end_flags, int32_t force_generic, int32_t ref_mode,
                     int32_t* scores, int32_t* end_query, strk_stats* stats) {
    if (!ctx) return fail(STRK_E_INVALID, "ctx is NULL");
    if (ctx->pending) return fail(STRK_E_INVALID, "context holds a submitted call: strk_finish() it first");
    if (stats) memset(stats, 0, sizeof *stats);
    if (end_flags < 0 || end_flags > 15) return fail(STRK_E_INVALID, "bad end_flags");
    strk_batch d;
    int rc;
    hipStream_t st;
    if ((rc = upload_batch(ctx, batch, &d, &st))) return rc;
    if (batch->n_reads == 0 || batch->n_loci == 0) return 0;
    if (!lo || !n || !table_off || !scores) return fail(STRK_E_INVALID, "lo / n / table_off / scores is NULL");
    const size_t nr = (size_t)batch->n_reads;
    const int mul = ref_mode ? 2 : 1;
    size_t n_chunks = 0;
    for (size_t r = 0; r < nr; ++r) {
        if (lo[r] < 0 || n[r] < 0) return fail(STRK_E_INVALID, "read %zu: negative window", r);
        if (table_off[r + 1] - table_off[r] < n[r] || table_off[r] < 0) return fail(STRK_E_INVALID, "read %zu: table_off too small", r);
        n_chunks += ((size_t)n[r] + kTableMax - 1) / kTableMax;
    }
    const size_t tab = (size_t)table_off[nr];
    if ((rc = ensure_workspace(ctx, batch->n_reads, batch->n_loci, tab * mul, std::max<size_t>(n_chunks, 1)))) return rc;
    KArgs a = make_args(ctx, &d, end_flags, 0, 0, (int)std::max<size_t>(n_chunks, 1), nullptr);
    a.ref_mode = ref_mode;
    std::vector<int64_t> off_dev(table_off, table_off + nr);
    for (auto& o : off_dev) o *= mul;
    HIP_TRY(hipMemcpyAsync(a.win_lo, lo, nr * 4, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(a.win_n, n, nr * 4, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(a.tab_off, off_dev.data(), nr * 8, hipMemcpyHostToDevice, st));
    if ((rc = score_until_scratch_fits(ctx, a, nullptr, batch->n_reads, force_generic, st, true))) return rc;
    if ((rc = check_error_bits(ctx->h_counters.cnt(kCntError)))) return rc;
    if (tab) {
        std::vector<int32_t> pairs(ref_mode ? tab * 2 : 0);   // (score, end_query) per candidate
        HIP_TRY(hipMemcpyAsync(ref_mode ? pairs.data() : scores, a.table, tab * 4 * mul, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        for (size_t k = 0; k < pairs.size() / 2; ++k) {
            scores[k] = pairs[2 * k];
            end_query[k] = pairs[2 * k + 1];
        }
    }
    if (stats) {
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, ctx->ev[kEvStart], ctx->ev[kEvEnd]) == hipSuccess) stats->kernel_ms = ms;
        if (hipEventElapsedTime(&ms, ctx->ev[kEvPre], ctx->ev[kEvExact]) == hipSuccess) stats->dp_kernel_ms = ms;
        stats->n_dp_launches = 2;
        stats->n_fallback = ctx->h_counters.cnt(kCntClass0 + kGenericClass);
        stats->n_long_reads = ctx->h_counters.cnt(kCntClass0 + kLongClass);
        stats->dp_cells = (int64_t)ctx->h_counters.cells();
    }
    return 0;
}

// Lazily scored (fwd score, fwd end_query, rev score, rev end_query) per candidate size for one locus:
// two device "reads" — the window itself and its reversal with the flanks swapped
// (repeats.py:32-41: ext_l_seq = (tr_candidate + flank_right_seq)[::-1] against db_seq[::-1]).
#include "strk_host_ref.inc"

#include "strk_host_realign.inc"

// strk_groups::check with the refusal as this library reports one: "<function>: <what is wrong>"
int check_groups(const char* fn, const strk_groups::View& v, int max_group, int max_len, strk_groups::Totals* t) {
    strk_groups::Message m;
    const int rc = strk_groups::check(v, max_group, max_len, t, &m);
    return rc ? fail(rc, "%s: %s", fn, m.text) : 0;
}

#include "strk_host_alleles.inc"
#include "strk_host_phase.inc"
#include "strk_host_consensus.inc"
#include "strk_host_kmers.inc"
#include "strk_host_poa.inc"

}  // namespace

extern "C" {

const char* strk_last_error(void) { return g_err.c_str(); }
const char* strk_version(void) { return "strkit_amd 0.1.0 (gfx950)"; }
int32_t strk_plan_scope(int32_t n_reads) { return plan_scope_of(n_reads); }
int strk_band_list(strk_ctx* c, int32_t band_class, int32_t* out_reads, int32_t cap) {
    if (!c || band_class < 0 || band_class >= kNumBandClasses || cap < 0 || (cap > 0 && !out_reads)) return STRK_E_INVALID;
    if (c->last_list_stride <= 0 || !c->cls_list.p || !c->counters.p) return 0;
    if (hipSetDevice(c->device) != hipSuccess || hipDeviceSynchronize() != hipSuccess) return STRK_E_DEVICE;
    int32_t n = 0;
    if (hipMemcpy(&n, c->counters.as<int32_t>() + kCntClass0 + kBandClass0 + band_class, sizeof n, hipMemcpyDeviceToHost) != hipSuccess) return STRK_E_DEVICE;
    n = std::max(0, std::min(n, (int32_t)c->last_list_stride));
    const int32_t k = std::min(n, cap);
    if (k > 0) {   // (read, locus) pairs: every other int
        const int32_t* src = c->cls_list.as<int32_t>() + (size_t)(kBandClass0 + band_class) * c->last_list_stride * 2;
        if (hipMemcpy2D(out_reads, sizeof(int32_t), src, 2 * sizeof(int32_t), sizeof(int32_t), (size_t)k, hipMemcpyDeviceToHost) != hipSuccess) return STRK_E_DEVICE;
    }
    return n;
}

int32_t strk_classify(int32_t nfl, int32_t ntr, int32_t nfr, int32_t m, int32_t lo, int32_t n, int32_t force_generic, int32_t ref_mode) {
    return classify(nfl, ntr, nfr, m, lo, n, force_generic, ref_mode);
}
void strk_score_constants(int32_t* out, int32_t cap) {
    int32_t v[9 + 2 * kNumClasses] = {kTableMax, kFastFlankMax, kMotifMax, kRowSlack, kNumClasses, kLongTile, kLongMaxTiles, kLongFlankMax, kStairMinG};
    for (int k = 0; k < kNumClasses; ++k) { v[9 + k] = class_cap(k); v[9 + kNumClasses + k] = class_G(k); }
    for (int k = 0; k < cap && k < 9 + 2 * kNumClasses; ++k) out[k] = v[k];
}
int strk_class_counts(strk_ctx* c, int32_t* out, int32_t cap) {
    if (!c || cap < 0 || (cap > 0 && !out)) return STRK_E_INVALID;
    if (!c->h_counters.mem.p || c->pending) return 0;
    for (int k = 0; k < cap && k < kNumClasses + 2; ++k) out[k] = c->h_counters.cnt(kCntClass0 + k);
    return kNumClasses + 2;
}

// Test support for the band pass: k_plan in mode 0 with the band on for every read, then k_dp_band and k_dp_band_wide and
// nothing behind them, so that KArgs::table and KArgs::ub come back as the band kernels left them (in a counting call pass 1 of
// k_replay uses or replaces them on the device).  Launched here and not through enqueue_scoring, whose band pass needs the
// replay pass behind it; the context's BandGate, GridHistory and the process's WindowPolicy are neither read nor written.
int strk_band_tables(strk_ctx* ctx, const strk_batch* batch, const strk_params* params, const int32_t* tune, int32_t flags,
                     int32_t* out_lo, int32_t* out_n, int32_t* out_class, int32_t table_stride, int32_t* out_scores,
                     int32_t* out_ub, strk_stats* stats) {
    if (!ctx) return fail(STRK_E_INVALID, "ctx is NULL");
    if (ctx->pending) return fail(STRK_E_INVALID, "strk_band_tables: a submitted call is pending on this context");
    if (stats) memset(stats, 0, sizeof *stats);
    strk_params p;
    int rc;
    if ((rc = check_params(params, &p))) return rc;
    if (params->window <= 0) return fail(STRK_E_INVALID, "strk_band_tables: params->window must be given (> 0)");
    if (!tune || table_stride < 1 || table_stride > 2 * kTableMax + 1) return fail(STRK_E_INVALID, "strk_band_tables: tune is NULL or table_stride is not in [1, %d]", 2 * kTableMax + 1);
    if (batch && batch->n_reads > 0 && batch->n_loci > 0 && (!out_lo || !out_n || !out_class || !out_scores || !out_ub))
        return fail(STRK_E_INVALID, "strk_band_tables: output pointer is NULL");
    strk_batch d;
    hipStream_t st;
    if ((rc = upload_batch(ctx, batch, &d, &st))) return rc;
    if (batch->n_reads == 0 || batch->n_loci == 0) return 0;
    const size_t nr = (size_t)batch->n_reads, tab = nr * (size_t)table_stride;
    if ((rc = ensure_workspace(ctx, batch->n_reads, batch->n_loci, tab, nr, true))) return rc;
    for (int k = 0; k < kWinBuckets; ++k) ctx->p_window_b[k] = 0;   // params->window for every motif length
    KArgs a = make_args(ctx, &d, p.end_flags, params->window, table_stride, batch->n_reads, nullptr);
    a.spec = static_cast<int4*>(ctx->spec.p);
    a.rep = ctx->rep.as<int32_t>();
    a.rhash = nullptr;   // no dedupe: every read owns its row
    a.exact = ctx->exact.as<uint8_t>();
    a.band_mode = 1;
    a.band_limit = INT32_MAX;
    if (tune[0] || tune[1] || tune[2]) a.band_tune = {tune[0], tune[1], tune[2]};
    const int plan_scope = plan_scope_of(batch->n_reads);
    const int blocks = std::max(1, std::min(256 * kBandBlocksPerCU, (a.list_stride + 3) / 4));
    const size_t recs = (size_t)kNumBandClasses * nr * 2;
    std::vector<int32_t> h_cnt(kCntTotal), h_list(recs), h_tab(tab), h_ub(tab);
    std::vector<uint8_t> h_exact(nr);
    rc = timed_launch(ctx, st, stats, "strk_band_tables", "the band pass", (flags & 1) ? 5 : 3, [&] {
        (void)hipMemsetAsync(ctx->counters.p, 0, kCountersAllBytes, st);
        hipLaunchKernelGGL(k_plan, dim3((batch->n_reads + plan_scope - 1) / plan_scope), dim3(kPlanThreads), 0, st, a, 0, (const int32_t*)nullptr,
                           batch->n_reads, 0, plan_reads_per_thread(batch->n_reads));
        hipLaunchKernelGGL(k_dp_band, dim3(blocks), dim3(256), 0, st, a);
        KArgs aw = a;
        if (flags & 1) {   // longest first, as enqueue_scoring orders the wide classes of a call with few wide chunks
            hipLaunchKernelGGL(k_sort_wide_hist, dim3(kSortWideBlocks, kNumWideLists), dim3(256), 0, st, a);
            hipLaunchKernelGGL(k_sort_wide, dim3(kSortWideBlocks, kNumWideLists), dim3(256), 0, st, a, ctx->band_recs_w.as<int4>());
            aw.band_recs_w = ctx->band_recs_w.as<int4>();
        }
        hipLaunchKernelGGL(k_dp_band_wide, dim3(blocks), dim3(256), 0, st, aw);
    }, [&] {
        HIP_TRY(hipMemcpyAsync(h_cnt.data(), ctx->counters.p, h_cnt.size() * 4, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipMemcpyAsync(h_list.data(), ctx->cls_list.as<int32_t>() + (size_t)kBandClass0 * nr * 2, recs * 4, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipMemcpyAsync(h_exact.data(), ctx->exact.p, nr, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipMemcpyAsync(h_tab.data(), ctx->table.p, tab * 4, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipMemcpyAsync(h_ub.data(), ctx->ub.p, tab * 4, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipMemcpyAsync(out_lo, a.win_lo, nr * 4, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipMemcpyAsync(out_n, a.win_n, nr * 4, hipMemcpyDeviceToHost, st));
        return 0;
    });
    if (rc) return rc;
    if ((rc = check_error_bits(h_cnt[kCntError] & ~kErrEmpty))) return rc;
    for (size_t r = 0; r < nr; ++r) out_class[r] = -1;
    int n_band = 0;
    for (int c = 0; c < kNumBandClasses; ++c) {
        const int cnt = std::min(h_cnt[kCntClass0 + kBandClass0 + c], batch->n_reads);
        n_band += cnt;
        for (int k = 0; k < cnt; ++k) {
            const int32_t r = h_list[((size_t)c * nr + k) * 2];
            if (r < 0 || (size_t)r >= nr) return fail(STRK_E_DEVICE, "strk_band_tables: band list %d holds read %d", c, r);
            out_class[r] = h_exact[r] ? -2 : c;
        }
    }
    for (size_t r = 0; r < nr; ++r) {   // rows of the reads a band class scored; every other row stays as the caller left it
        if (out_class[r] < 0) continue;
        const size_t n = (size_t)std::max(0, std::min(out_n[r], table_stride));
        memcpy(out_scores + r * table_stride, h_tab.data() + r * table_stride, n * 4);
        memcpy(out_ub + r * table_stride, h_ub.data() + r * table_stride, n * 4);
    }
    if (stats) {
        stats->n_band_reads = n_band;
        stats->n_band_fallback = h_cnt[kCntBandFallback];
        stats->window_used = params->window;
    }
    return 0;
}

void strk_adaptive_reset(void) { g_window.reset(); }

int strk_host_register(void* ptr, int64_t bytes) {
    if (!ptr || bytes <= 0) return fail(STRK_E_INVALID, "strk_host_register: null pointer or no bytes");
    const hipError_t e = hipHostRegister(ptr, (size_t)bytes, hipHostRegisterDefault);
    if (e == hipErrorHostMemoryAlreadyRegistered) { (void)hipGetLastError(); return 0; }
    if (e != hipSuccess) { (void)hipGetLastError(); return fail(STRK_E_DEVICE, "hipHostRegister(%lld bytes): %s", (long long)bytes, hipGetErrorString(e)); }
    return 0;
}

int strk_host_is_pinned(const void* ptr, int64_t bytes) { return bytes > 0 && host_range_pinned(ptr, (size_t)bytes) ? 1 : 0; }

int strk_host_unregister(void* ptr) {
    if (!ptr) return fail(STRK_E_INVALID, "strk_host_unregister: null pointer");
    const hipError_t e = hipHostUnregister(ptr);
    if (e != hipSuccess) { (void)hipGetLastError(); return fail(STRK_E_DEVICE, "hipHostUnregister: %s", hipGetErrorString(e)); }
    return 0;
}

int strk_device_mem(int device, int64_t* free_bytes, int64_t* total_bytes) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) return fail(STRK_E_NODEV, "no HIP device visible");
    if (device < 0 || device >= n) return fail(STRK_E_NODEV, "device %d out of range (%d visible)", device, n);
    HIP_TRY(hipSetDevice(device));
    size_t f = 0, t = 0;
    HIP_TRY(hipMemGetInfo(&f, &t));
    if (free_bytes) *free_bytes = (int64_t)f;
    if (total_bytes) *total_bytes = (int64_t)t;
    return 0;
}

int strk_init(int device, strk_ctx** out) {
    if (!out) return fail(STRK_E_INVALID, "out is NULL");
    *out = nullptr;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) return fail(STRK_E_NODEV, "no HIP device visible");
    if (device < 0 || device >= n) return fail(STRK_E_NODEV, "device %d out of range (%d visible)", device, n);
    HIP_TRY(hipSetDevice(device));
    hipDeviceProp_t prop;
    HIP_TRY(hipGetDeviceProperties(&prop, device));
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return fail(STRK_E_NODEV, "device %d is %s; this library holds gfx950 code objects only", device, prop.gcnArchName);
    strk_ctx* c = new strk_ctx();
    c->device = device;
    c->long_slot_ints = kLongSlotInts;
    c->generic_ints = kGenericPoolInts;
    // testing aids: a context that starts with small scratch parts, so that a small input walks the grow-and-run-again path
    if (const char* e = getenv("STRKIT_AMD_GENERIC_POOL_INTS")) c->generic_ints = (size_t)std::max(1l, atol(e));
    if (const char* e = getenv("STRKIT_AMD_LONG_SLOT_INTS")) c->long_slot_ints = (size_t)std::max(1l, atol(e));
    strk::ScoreTables t;
    strk::build_score_tables(&t);
    hipError_t e = hipMemcpyToSymbol(HIP_SYMBOL(strk::c_mat), t.mat, sizeof t.mat);
    if (e == hipSuccess) e = hipMemcpyToSymbol(HIP_SYMBOL(strk::c_enc), t.enc, sizeof t.enc);
    if (e == hipSuccess) e = c->h_counters.mem.alloc(kCountersBytes);
    if (e == hipSuccess) memset(c->h_counters.mem.p, 0, kCountersBytes);   // (strk_class_counts before the first call: all lists empty)
    for (int i = 0; i < kNumEvents && e == hipSuccess; ++i) e = hipEventCreate(&c->ev[i].h);
    if (e != hipSuccess) {
        strk_destroy(c);
        return fail(STRK_E_DEVICE, "context setup: %s", hipGetErrorString(e));
    }
    *out = c;
    return 0;
}

void strk_destroy(strk_ctx* c) {
    if (!c) return;
    (void)hipSetDevice(c->device);
    delete c->pipe;   // the pipeline and its two sub-contexts first, then the context's own members
    c->pipe = nullptr;
    {   // no later call may wait for this context's band event
        std::lock_guard<std::mutex> lk(g_band_chain_mu);
        if (g_band_chain_ev == c->ev[kEvBand].h) g_band_chain_ev = nullptr;
    }
    delete c;
}

int strk_count_loci_device(strk_ctx* ctx, const strk_batch* batch, const strk_params* params, int32_t* out_cn,
                           int32_t* out_score, int32_t* out_n_iters, int32_t* out_start, void* stream,
                           strk_stats* stats) {
    if (!ctx) return fail(STRK_E_INVALID, "ctx is NULL");
    return count_device(ctx, batch, params, out_cn, out_score, out_n_iters, out_start, static_cast<hipStream_t>(stream), stats);
}

int strk_submit_loci_device(strk_ctx* ctx, const strk_batch* batch, const strk_params* params, int32_t* out_cn,
                            int32_t* out_score, int32_t* out_n_iters, int32_t* out_start, void* stream) {
    if (!ctx) return fail(STRK_E_INVALID, "ctx is NULL");
    return submit_device(ctx, batch, params, out_cn, out_score, out_n_iters, out_start, static_cast<hipStream_t>(stream));
}

int strk_finish(strk_ctx* ctx, strk_stats* stats) {
    if (!ctx) return fail(STRK_E_INVALID, "ctx is NULL");
    return finish_device(ctx, stats);
}

int strk_count_loci(strk_ctx* ctx, const strk_batch* batch, const strk_params* params, int32_t* out_cn,
                    int32_t* out_score, int32_t* out_n_iters, int32_t* out_start, strk_stats* stats) {
    return strk_count_loci_dseqs(ctx, batch, nullptr, params, out_cn, out_score, out_n_iters, out_start, stats);
}

int strk_count_loci_dseqs(strk_ctx* ctx, const strk_batch* batch, const void* d_seqs, const strk_params* params, int32_t* out_cn,
                          int32_t* out_score, int32_t* out_n_iters, int32_t* out_start, strk_stats* stats) {
    if (!ctx) return fail(STRK_E_INVALID, "ctx is NULL");
    if (stats) memset(stats, 0, sizeof *stats);
    strk_batch d;
    int rc;
    if (d_seqs) {
        if ((rc = check_dseqs(ctx, "strk_count_loci_dseqs", d_seqs))) return rc;
    } else {   // host bases: large batches go through the pinned four-slot pipeline (strk_host_pipe.inc)
        bool taken = false;
        rc = count_loci_pipelined(ctx, batch, params, out_cn, out_score, out_n_iters, out_start, stats, &taken);
        if (taken) return rc;
    }
    hipStream_t st;
    if ((rc = upload_batch(ctx, batch, &d, &st, static_cast<const uint8_t*>(d_seqs)))) return rc;
    if (batch->n_reads == 0 || batch->n_loci == 0) return 0;
    if (!batch->est_cn) return fail(STRK_E_INVALID, "est_cn is NULL");
    const size_t nb = (size_t)batch->n_reads * 4, stride = (nb + 255) & ~(size_t)255;   // the four result arrays, 256-aligned
    if ((rc = ctx->stage_out.ensure(4 * stride))) return rc;
    int32_t* dev[4];
    for (int k = 0; k < 4; ++k) dev[k] = ctx->stage_out.at<int32_t>(k * stride);
    rc = count_device(ctx, &d, params, dev[0], dev[1], dev[2], dev[3], st, stats);
    if (rc && rc != STRK_E_EMPTY) return rc;
    int32_t* const host[4] = {out_cn, out_score, out_n_iters, out_start};
    for (int k = 0; k < 4; ++k)
        if (host[k]) HIP_TRY(hipMemcpyAsync(host[k], dev[k], nb, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return rc;
}

int strk_repeat_count(strk_ctx* ctx, int32_t start_count, const uint8_t* tr, int32_t tr_len, const uint8_t* fl,
                      int32_t fl_len, const uint8_t* fr, int32_t fr_len, const uint8_t* motif, int32_t motif_len,
                      int32_t max_iters, int32_t local_search_range, int32_t step_size, int32_t* out_cn,
                      int32_t* out_score, int32_t* out_n_explored) {
    if (!ctx) return fail(STRK_E_INVALID, "ctx is NULL");
    if (tr_len < 0 || fl_len < 0 || fr_len < 0 || motif_len < 1) return fail(STRK_E_INVALID, "bad sequence length");
    if ((tr_len && !tr) || (fl_len && !fl) || (fr_len && !fr) || !motif) return fail(STRK_E_INVALID, "sequence pointer is NULL");
    const strk_params p = default_params(max_iters, local_search_range, step_size);
    int32_t cn = 0, sc = 0, n = 0, st = 0;
    auto done = [&] {
        if (out_cn) *out_cn = cn;
        if (out_score) *out_score = sc;
        if (out_n_explored) *out_n_explored = n;
        return 0;
    };
    const int rf = scalar_fast(ctx, start_count, tr, tr_len, fl, fl_len, fr, fr_len, motif, motif_len, p, &cn, &sc, &n);
    if (rf < 0) return rf;
    if (rf == 0) return done();
    std::vector<uint8_t> seq((size_t)fl_len + tr_len + fr_len);
    if (fl_len) memcpy(seq.data(), fl, (size_t)fl_len);
    if (tr_len) memcpy(seq.data() + fl_len, tr, (size_t)tr_len);
    if (fr_len) memcpy(seq.data() + fl_len + tr_len, fr, (size_t)fr_len);
    const OneRead head{{0, (int64_t)seq.size()}, {fl_len, tr_len, fr_len, start_count}, {0, 1}, {0, motif_len}};
    const strk_batch b = one_read_batch(&head, seq.data(), motif);
    const int rc = strk_count_loci(ctx, &b, &p, &cn, &sc, &n, &st, nullptr);
    return rc ? rc : done();
}

int strk_score_table(strk_ctx* ctx, const strk_batch* batch, const int32_t* lo, const int32_t* n,
                     const int64_t* table_off, int32_t end_flags, int32_t force_generic, int32_t* scores,
                     strk_stats* stats) {
    return score_table_impl(ctx, batch, lo, n, table_off, end_flags, force_generic, 0, scores, nullptr, stats);
}

int strk_score_ref_table(strk_ctx* ctx, const strk_batch* batch, const int32_t* lo, const int32_t* n,
                         const int64_t* table_off, int32_t force_generic, int32_t* scores, int32_t* end_query,
                         strk_stats* stats) {
    if (!end_query) return fail(STRK_E_INVALID, "end_query is NULL");
    return score_table_impl(ctx, batch, lo, n, table_off, STRK_DB_END_FREE, force_generic, 1, scores, end_query, stats);
}

int strk_ref_repeat_count(strk_ctx* ctx, int32_t start_count, const uint8_t* tr, int32_t tr_len, const uint8_t* fl,
                          int32_t fl_len, const uint8_t* fr, int32_t fr_len, const uint8_t* motif, int32_t motif_len,
                          int32_t ref_size, int32_t vcf_anchor_size, int32_t max_iters, int32_t local_search_range,
                          int32_t step_size, int32_t respect_coords, int32_t* out9) {
    if (!ctx) return fail(STRK_E_INVALID, "ctx is NULL");
    if (!out9) return fail(STRK_E_INVALID, "out9 is NULL");
    if (tr_len < 0 || fl_len < 0 || fr_len < 0 || motif_len < 1) return fail(STRK_E_INVALID, "bad sequence length");
    if ((tr_len && !tr) || (fl_len && !fl) || (fr_len && !fr) || !motif) return fail(STRK_E_INVALID, "sequence pointer is NULL");
    if (local_search_range < 0 || step_size < 1) return fail(STRK_E_INVALID, "local_search_range must be >= 0 and step_size >= 1");
    return ref_repeat_count_impl(ctx, start_count, tr, tr_len, fl, fl_len, fr, fr_len, motif, motif_len, ref_size,
                                 vcf_anchor_size, max_iters, local_search_range, step_size, respect_coords, out9);
}

int strk_realign(strk_ctx* ctx, int32_t n_pairs, const uint8_t* s1, const int64_t* s1_off, const uint8_t* s2,
                 const int64_t* s2_off, int32_t open, int32_t extend, int32_t gap_pref, int32_t* out_score,
                 int32_t* out_end_ref, int32_t* out_n_cigar, uint32_t* cigar, const int64_t* cigar_off, strk_stats* stats) {
    if (!ctx) return fail(STRK_E_INVALID, "ctx is NULL");
    if (ctx->pending) return fail(STRK_E_INVALID, "a submitted call is pending on this context");
    return realign_impl(ctx, n_pairs, s1, s1_off, s2, s2_off, open, extend, gap_pref, out_score, out_end_ref, out_n_cigar,
                        cigar, cigar_off, stats);
}

int strk_call_alleles(strk_ctx* ctx, int32_t n_loci, const int32_t* read_off, const int32_t* cn, const double* w,
                      const int32_t* n_alleles, const uint64_t* seed, const strk_allele_params* p, int32_t* out_status,
                      int32_t* out_modal_n, int32_t* out_call, int32_t* out_ci95, int32_t* out_ci99, double* out_means,
                      double* out_weights, double* out_stdevs, int32_t* out_peak_n_reads, int32_t* out_read_peak,
                      strk_stats* stats) {
    const char* fn = "strk_call_alleles";
    if (!ctx) return fail(STRK_E_INVALID, "%s: ctx is NULL", fn);
    if (ctx->pending) return fail(STRK_E_INVALID, "%s: a submitted call is pending on this context", fn);
    static_assert(STRK_ALLELE_CALLED == 0 && STRK_ALLELE_TOO_FEW == 1 && STRK_ALLELE_EMPTY_PEAK == 2, "include/strkit_amd.h <-> strk_alleles.h");
    const AlleleOut out{out_status, out_modal_n, out_call, out_ci95, out_ci99, out_means, out_weights, out_stdevs, out_peak_n_reads,
                        out_read_peak};
    return call_alleles_impl<2>(ctx, fn, {n_loci, read_off, cn, w, n_alleles, seed, p}, out, stats);
}

int strk_call_alleles_n(strk_ctx* ctx, int32_t n_loci, const int32_t* read_off, const int32_t* cn, const double* w,
                        const int32_t* n_alleles, const uint64_t* seed, const strk_allele_params* p, int32_t* out_status,
                        int32_t* out_modal_n, int32_t* out_call, int32_t* out_ci95, int32_t* out_ci99, double* out_means,
                        double* out_weights, double* out_stdevs, int32_t* out_peak_n_reads, int32_t* out_read_peak,
                        strk_stats* stats) {
    const char* fn = "strk_call_alleles_n";
    if (!ctx) return fail(STRK_E_INVALID, "%s: ctx is NULL", fn);
    if (ctx->pending) return fail(STRK_E_INVALID, "%s: a submitted call is pending on this context", fn);
    static_assert(STRK_MAX_ALLELES == kMaxAlleles, "include/strkit_amd.h <-> strk_alleles.h");
    const AlleleOut out{out_status, out_modal_n, out_call, out_ci95, out_ci99, out_means, out_weights, out_stdevs, out_peak_n_reads,
                        out_read_peak};
    return call_alleles_impl<kMaxAlleles>(ctx, fn, {n_loci, read_off, cn, w, n_alleles, seed, p}, out, stats);
}

int strk_call_alleles_phased(strk_ctx* ctx, int32_t n_loci, const int32_t* read_off, const int32_t* cn, const double* w,
                             const int32_t* n_alleles, const uint64_t* seed, const strk_allele_params* p, const strk_phase_params* pp,
                             const int32_t* hp, const int32_t* ps, const int32_t* snv_off, const uint8_t* snv_base,
                             const uint8_t* snv_qual, int64_t n_snv_cells, int32_t* out_status, int32_t* out_modal_n, int32_t* out_call,
                             int32_t* out_ci95, int32_t* out_ci99, double* out_means, double* out_weights, double* out_stdevs,
                             int32_t* out_peak_n_reads, int32_t* out_read_peak, int32_t* out_method, int32_t* out_reason,
                             int32_t* out_ps, int32_t* out_snv_status, uint8_t* out_snv_call, int32_t* out_snv_rcs, strk_stats* stats) {
    const char* fn = "strk_call_alleles_phased";
    if (!ctx) return fail(STRK_E_INVALID, "%s: ctx is NULL", fn);
    if (ctx->pending) return fail(STRK_E_INVALID, "%s: a submitted call is pending on this context", fn);
    static_assert(STRK_ALLELE_NOT_PHASED == kStatusNotPhased && STRK_ALLELE_TOO_FEW == kStatusTooFew, "include/strkit_amd.h <-> strk_phase.h");
    static_assert(STRK_ASSIGN_NONE == kAssignNone && STRK_ASSIGN_HP == kAssignHp && STRK_ASSIGN_SNV == kAssignSnv &&
                  STRK_ASSIGN_SNV_DIST == kAssignSnvDist, "include/strkit_amd.h <-> strk_phase.h");
    static_assert(STRK_PHASE_NO_TAGS == kReasonNoTags && STRK_PHASE_TAG_THRESHOLDS == kReasonTagThresholds &&
                  STRK_PHASE_FEW_SNV_READS == kReasonFewSnvReads && STRK_PHASE_GROUP_NOT_CALLED == kReasonGroupNotCalled &&
                  STRK_PHASE_NO_SNV_CALLED == kReasonNoSnvCalled, "include/strkit_amd.h <-> strk_phase.h");
    static_assert(STRK_SNV_NOT_EVALUATED == kSnvNotEvaluated && STRK_SNV_CALLED == kSnvCalled && STRK_SNV_ZERO_TOTAL == kSnvZeroTotal &&
                  STRK_SNV_ONLY_OUT_OF_RANGE == kSnvOnlyOutOfRange && STRK_SNV_CROSS_TALK == kSnvCrossTalk &&
                  STRK_SNV_SAME_BASE == kSnvSameBase, "include/strkit_amd.h <-> strk_phase.h");
    const strk_phase_check::Input in{{n_loci, read_off, cn, w, n_alleles, seed, p}, pp, hp, ps, snv_off, n_snv_cells, snv_base, snv_qual};
    const PhaseOut out{{out_status, out_modal_n, out_call, out_ci95, out_ci99, out_means, out_weights, out_stdevs, out_peak_n_reads,
                        out_read_peak}, out_method, out_reason, out_ps, out_snv_status, out_snv_call, out_snv_rcs};
    return call_alleles_phased_impl(ctx, fn, in, out, stats);
}

int strk_best_representatives(strk_ctx* ctx, int32_t n_groups, const int32_t* group_off, const uint8_t* seqs, int64_t n_seq_bytes,
                              const int64_t* seq_start, const int32_t* seq_len, int32_t* out_index, int32_t* out_method,
                              int64_t* out_dist_sum, strk_stats* stats) {
    const char* fn = "strk_best_representatives";
    if (!ctx) return fail(STRK_E_INVALID, "%s: ctx is NULL", fn);
    if (ctx->pending) return fail(STRK_E_INVALID, "%s: a submitted call is pending on this context", fn);
    static_assert(STRK_CONS_NONE == kConsNone && STRK_CONS_SINGLE == kConsSingle && STRK_CONS_BEST_REP == kConsBestRep,
                  "include/strkit_amd.h <-> strk_consensus.h");
    return best_rep_impl(ctx, fn, n_groups, group_off, seqs, nullptr, n_seq_bytes, seq_start, seq_len, out_index, out_method,
                         out_dist_sum, stats);
}

int strk_best_representatives_dseqs(strk_ctx* ctx, int32_t n_groups, const int32_t* group_off, const void* d_seqs,
                                    int64_t n_seq_bytes, const int64_t* seq_start, const int32_t* seq_len, int32_t* out_index,
                                    int32_t* out_method, int64_t* out_dist_sum, strk_stats* stats) {
    const char* fn = "strk_best_representatives_dseqs";
    if (!ctx) return fail(STRK_E_INVALID, "%s: ctx is NULL", fn);
    if (ctx->pending) return fail(STRK_E_INVALID, "%s: a submitted call is pending on this context", fn);
    if (!d_seqs) return fail(STRK_E_INVALID, "%s: d_seqs is NULL", fn);
    if (const int rc = check_dseqs(ctx, fn, d_seqs)) return rc;
    return best_rep_impl(ctx, fn, n_groups, group_off, nullptr, static_cast<const uint8_t*>(d_seqs), n_seq_bytes, seq_start, seq_len,
                         out_index, out_method, out_dist_sum, stats);
}

int64_t strk_count_kmers_ws(strk_ctx* ctx, int32_t n_groups, const int32_t* group_off, const uint8_t* seqs, const void* d_seqs,
                            int64_t n_seq_bytes, const int64_t* seq_start, const int32_t* seq_len, const int32_t* k, int64_t cap,
                            int64_t* out_entry_off, int64_t* out_pos, int32_t* out_count, int64_t workspace_bytes,
                            strk_stats* stats) {
    const char* fn = d_seqs ? "strk_count_kmers_dseqs" : "strk_count_kmers";
    if (!ctx) return fail(STRK_E_INVALID, "%s: ctx is NULL", fn);
    if (ctx->pending) return fail(STRK_E_INVALID, "%s: a submitted call is pending on this context", fn);
    if (seqs && d_seqs) return fail(STRK_E_INVALID, "strk_count_kmers_ws: both seqs and d_seqs are given");
    if (const int rc = d_seqs ? check_dseqs(ctx, fn, d_seqs) : 0) return rc;
    return count_kmers_impl(ctx, fn, n_groups, group_off, seqs, static_cast<const uint8_t*>(d_seqs), n_seq_bytes, seq_start,
                            seq_len, k, cap, out_entry_off, out_pos, out_count, workspace_bytes, stats);
}

int64_t strk_count_kmers(strk_ctx* ctx, int32_t n_groups, const int32_t* group_off, const uint8_t* seqs, int64_t n_seq_bytes,
                         const int64_t* seq_start, const int32_t* seq_len, const int32_t* k, int64_t cap,
                         int64_t* out_entry_off, int64_t* out_pos, int32_t* out_count, strk_stats* stats) {
    return strk_count_kmers_ws(ctx, n_groups, group_off, seqs, nullptr, n_seq_bytes, seq_start, seq_len, k, cap, out_entry_off,
                               out_pos, out_count, 0, stats);
}

int64_t strk_count_kmers_dseqs(strk_ctx* ctx, int32_t n_groups, const int32_t* group_off, const void* d_seqs, int64_t n_seq_bytes,
                               const int64_t* seq_start, const int32_t* seq_len, const int32_t* k, int64_t cap,
                               int64_t* out_entry_off, int64_t* out_pos, int32_t* out_count, strk_stats* stats) {
    if (!ctx) return fail(STRK_E_INVALID, "strk_count_kmers_dseqs: ctx is NULL");
    if (!d_seqs) return fail(STRK_E_INVALID, "strk_count_kmers_dseqs: d_seqs is NULL");
    return strk_count_kmers_ws(ctx, n_groups, group_off, nullptr, d_seqs, n_seq_bytes, seq_start, seq_len, k, cap, out_entry_off,
                               out_pos, out_count, 0, stats);
}

int64_t strk_consensus_ws(strk_ctx* ctx, int32_t n_groups, const int32_t* group_off, const uint8_t* seqs, const void* d_seqs,
                          int64_t n_seq_bytes, const int64_t* seq_start, const int32_t* seq_len, int32_t max_mdn_poa_length,
                          int64_t cap, int32_t* out_index, int32_t* out_method, int64_t* out_seq_off, uint8_t* out_seqs,
                          int32_t node_limit, int64_t workspace_bytes, strk_stats* stats) {
    const char* fn = d_seqs ? "strk_consensus_dseqs" : "strk_consensus";
    if (!ctx) return fail(STRK_E_INVALID, "%s: ctx is NULL", fn);
    if (ctx->pending) return fail(STRK_E_INVALID, "%s: a submitted call is pending on this context", fn);
    if (seqs && d_seqs) return fail(STRK_E_INVALID, "strk_consensus_ws: both seqs and d_seqs are given");
    static_assert(STRK_CONS_POA == kConsPoa, "include/strkit_amd.h <-> strk_poa.h");
    if (const int rc = d_seqs ? check_dseqs(ctx, fn, d_seqs) : 0) return rc;
    return consensus_impl(ctx, fn, n_groups, group_off, seqs, static_cast<const uint8_t*>(d_seqs), n_seq_bytes, seq_start, seq_len,
                          max_mdn_poa_length, cap, out_index, out_method, out_seq_off, out_seqs, node_limit, workspace_bytes, stats);
}

int64_t strk_consensus(strk_ctx* ctx, int32_t n_groups, const int32_t* group_off, const uint8_t* seqs, int64_t n_seq_bytes,
                       const int64_t* seq_start, const int32_t* seq_len, int32_t max_mdn_poa_length, int64_t cap,
                       int32_t* out_index, int32_t* out_method, int64_t* out_seq_off, uint8_t* out_seqs, strk_stats* stats) {
    return strk_consensus_ws(ctx, n_groups, group_off, seqs, nullptr, n_seq_bytes, seq_start, seq_len, max_mdn_poa_length, cap,
                             out_index, out_method, out_seq_off, out_seqs, 0, 0, stats);
}

int64_t strk_consensus_dseqs(strk_ctx* ctx, int32_t n_groups, const int32_t* group_off, const void* d_seqs, int64_t n_seq_bytes,
                             const int64_t* seq_start, const int32_t* seq_len, int32_t max_mdn_poa_length, int64_t cap,
                             int32_t* out_index, int32_t* out_method, int64_t* out_seq_off, uint8_t* out_seqs,
                             strk_stats* stats) {
    if (!ctx) return fail(STRK_E_INVALID, "strk_consensus_dseqs: ctx is NULL");
    if (!d_seqs) return fail(STRK_E_INVALID, "strk_consensus_dseqs: d_seqs is NULL");
    return strk_consensus_ws(ctx, n_groups, group_off, nullptr, d_seqs, n_seq_bytes, seq_start, seq_len, max_mdn_poa_length, cap,
                             out_index, out_method, out_seq_off, out_seqs, 0, 0, stats);
}

int strk_ref_repeat_count_batch(strk_ctx* ctx, int32_t n_loci, const int32_t* start_count, const uint8_t* seqs,
                                const int64_t* seq_off, const int32_t* nfl, const int32_t* ntr, const int32_t* nfr,
                                const uint8_t* motifs, const int32_t* motif_off, const int32_t* ref_size,
                                int32_t vcf_anchor_size, const int32_t* max_iters, const int32_t* local_search_range,
                                const int32_t* step_size, int32_t respect_coords, int32_t* out9) {
    if (!ctx) return fail(STRK_E_INVALID, "ctx is NULL");
    if (n_loci < 0) return fail(STRK_E_INVALID, "n_loci < 0");
    if (n_loci == 0) return 0;
    if (!start_count || !seqs || !seq_off || !nfl || !ntr || !nfr || !motifs || !motif_off || !ref_size || !max_iters ||
        !local_search_range || !step_size || !out9)
        return fail(STRK_E_INVALID, "NULL argument");
    std::vector<RefJob> jobs((size_t)n_loci);
    for (int32_t i = 0; i < n_loci; ++i) {
        const int32_t m = motif_off[i + 1] - motif_off[i];
        if (nfl[i] < 0 || ntr[i] < 0 || nfr[i] < 0 || m < 1 || seq_off[i + 1] - seq_off[i] != (int64_t)nfl[i] + ntr[i] + nfr[i])
            return fail(STRK_E_INVALID, "locus %d: bad sequence lengths", i);
        if (local_search_range[i] < 0 || step_size[i] < 1) return fail(STRK_E_INVALID, "locus %d: bad search schedule", i);
        const uint8_t* s0 = seqs + seq_off[i];
        ref_job_init(jobs[(size_t)i], start_count[i], s0 + nfl[i], ntr[i], s0, nfl[i], s0 + nfl[i] + ntr[i], nfr[i],
                     motifs + motif_off[i], m, ref_size[i], max_iters[i], local_search_range[i], step_size[i]);
    }
    return ref_repeat_count_batch_impl(ctx, jobs, vcf_anchor_size, respect_coords, out9);
}

int strk_realign_i16_flags(int32_t n_pairs, const int64_t* s1_off, const int64_t* s2_off, const int32_t* scores, int32_t* out_flags) {
    if (n_pairs < 0) return fail(STRK_E_INVALID, "n_pairs < 0");
    if (n_pairs == 0) return 0;
    if (!s1_off || !s2_off || !scores || !out_flags) return fail(STRK_E_INVALID, "NULL argument");
    constexpr int64_t kLimit = 32767 - 2;   // INT16_MAX less the largest matrix entry (align_matrix.py:15): parasail's head-room
    for (int32_t p = 0; p < n_pairs; ++p) {
        const int64_t n1 = s1_off[p + 1] - s1_off[p], n2 = s2_off[p + 1] - s2_off[p];
        if (n1 < 0 || n2 < 0) return fail(STRK_E_INVALID, "pair %d: negative length", p);
        int32_t f = 0;
        if (2 * std::min(n1, n2) > kLimit) f |= STRK_I16_CELL_MAY_SATURATE;   // no cell of an alignment exceeds 2 * min(rows, columns)
        if (scores[p] > kLimit) f |= STRK_I16_SCORE_SATURATES | STRK_I16_CELL_MAY_SATURATE;
        out_flags[p] = f;
    }
    return 0;
}

#include "strk_host_files.inc"

}  // extern "C"

#include "strk_dbam.inc"
#include "strk_lines.inc"
#include "strk_phase_inputs.inc"
#include "strk_snv_discover.inc"
#include "strk_methyl.inc"
#include "strk_vcf.inc"
#include "strk_gff.inc"
#include "strk_select.inc"
#include "strk_host_mi.inc"
