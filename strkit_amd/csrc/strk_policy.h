// strk_policy.h — the three adaptive policies of the host side, as plain state machines: the process-wide default candidate
// window (WindowPolicy), and per context the band gate (BandGate) and the grid history (GridHistory).  strk_api.hip feeds
// them the counters of every finished call (finish_device) and asks them when it submits the next one (submit_device,
// make_args, enqueue_scoring).  Nothing of HIP in here: the header compiles with the host compiler alone
// (tests/test_host.py drives the three through scripted call sequences).
#pragma once

#include <algorithm>
#include <atomic>
#include <cstdint>

namespace strk_policy {

constexpr int kWinBuckets = 5;   // motif-length buckets (= strk::kWinBuckets of strk_kernels.h; strk_api.hip asserts it)
constexpr int kWinStartLevel = 3, kWinLevels = 6;   // kWindowLevels below: a process starts at 8 sizes either side of the estimate
// default half-widths of the candidate window, see WindowPolicy.  A search that converges at once scores start +- 4, so +-4 is
// the floor of the TABLE; tools/window_need.py (BASELINE config 4): motifs of 11+ bases never need more, 7-10 bases in 0.7 % of
// the loci, 5-6 bases in 6 %, 3-4 in 27 %.  Levels 4 and 5 exist for the long-motif buckets but are switched off (kWinMinLevel):
// measured in round 4 on config 4's shard (tools/cfg_probe.py, windows pinned per bucket), a narrower TABLE puts the band into a
// narrower class, and what that class lacks is the slack the certificate needs — +-6 everywhere 6.40 ms per call, +-5 for motifs
// of 7+ bases 6.34 ms (15 000 certificate failures per call instead of 500), +-4: 8.08 ms (62 000 failures).  The cells a narrow
// window saves are taken by laying the BAND around the table's inner candidates instead (strk_search.h: BandTune), which keeps
// the table's outer entries for the searches that the caller's feedback moves.
// The short-motif buckets stop at +-6: +-5 was tried there in round 3 (the search from a start the feedback moved by one size
// then ends at the window's edge, 780 reads per 10 000-locus call turn out uncertain: 205 M reads/s instead of 221 M).
constexpr int kWindowLevels[kWinLevels] = {4, 5, 6, 8, 11, 15};
// narrowest level a motif-length bucket may settle at.  Motifs of 1-2 bases stay at +-8: their estimate is off by a size for every
// second base of indel drift (tools/window_need.py, config 4: 0.3 % of those loci need more than +-6, none more than +-8), a miss is
// a host round of about a millisecond (config 4's shard: 7 missed reads, 2 ms of an 8.2 ms call), and the wider window costs such
// short motifs four more fork rows and no wider band class.
constexpr int kWinMinLevel[kWinBuckets] = {3, 2, 2, 2, 2};

// Default candidate window of this process (one sample, whatever context a call runs on): level into kWindowLevels,
// and the number of consecutive default-window calls without a window miss since the level last changed.
// Misses cost extra rounds on the host: a call with more than a handful (> 0.4 % of its loci) moves a level up at
// once; eight (from the two widest levels: sixty-four) calls in a row with at most one miss per thousand loci move
// a level down — a probe, whose failures space the later ones out (failed).
// One level per motif-length bucket (win_bucket): the estimate round(|tr| / |motif|) is off by the read's indel drift divided
// by the motif length, so the reads of long motifs stay inside narrow windows that those of short ones leave.  The two
// narrowest levels (+-4, +-5) are open to the long-motif buckets only (kWinMinLevel).
// Lock-free: contexts on several threads read and update it with relaxed atomics.
struct WindowPolicy {
    std::atomic<int> level[kWinBuckets], quiet[kWinBuckets];
    // A step down is a probe: the call after it either stays quiet or pays a window-miss round for every locus the narrower window
    // does not hold (config 3, 3-4-base motifs at +-6: 111 loci, 18 ms on top of an 8 ms call) and steps up again.  Every failed
    // probe doubles the number of quiet calls before the next one (64, 128, ... 4 096), per bucket; reset() clears it.
    std::atomic<int> probing[kWinBuckets];   // 1: the level was last changed by a step down
    std::atomic<int> failed[kWinBuckets];    // probes that failed since the reset

    WindowPolicy() { reset(); }

    void reset() {   // strk_adaptive_reset
        for (int k = 0; k < kWinBuckets; ++k) {
            level[k].store(kWinStartLevel, std::memory_order_relaxed);
            quiet[k].store(0, std::memory_order_relaxed);
            probing[k].store(0, std::memory_order_relaxed);
            failed[k].store(0, std::memory_order_relaxed);
        }
    }

    // the window a call with the default window gives bucket k: what the sample needs, and never less than the search can
    // step in one iteration (reach = local_search_range + step_size), up to the widest level
    int window(int k, int reach) const {
        const int w = kWindowLevels[std::min(kWinLevels - 1, std::max(kWinMinLevel[k], level[k].load(std::memory_order_relaxed)))];
        return std::max(w, std::min(kWindowLevels[kWinLevels - 1], reach));
    }

    // one finished default-window call: the loci of bucket k it held and how many of them left their window
    void update(int k, int n_loci, int n_miss) {
        if (n_loci == 0) return;
        const int lvl = std::max(kWinMinLevel[k], level[k].load(std::memory_order_relaxed));
        // a handful of misses costs less (one short extra round) than a wider window for every read does
        // (small calls: two loci of 250 already are 0.8 %, and a window-miss round on long windows costs as much as the call)
        const int n_failed = failed[k].load(std::memory_order_relaxed);
        const int quiet_calls = n_failed > 0 ? 64 << std::min(n_failed - 1, 6) : (lvl > kWinStartLevel ? 64 : 8);
        if (n_miss > std::max(1, n_loci / 250)) {
            if (lvl < kWinLevels - 1) level[k].store(lvl + 1, std::memory_order_relaxed);
            if (probing[k].exchange(0, std::memory_order_relaxed)) failed[k].store(std::min(n_failed + 1, 16), std::memory_order_relaxed);
            quiet[k].store(0, std::memory_order_relaxed);
        } else if (n_miss > n_loci / 1000) {   // more than one locus in a thousand: not a quiet call
            quiet[k].store(0, std::memory_order_relaxed);
        } else if (quiet[k].fetch_add(1, std::memory_order_relaxed) + 1 >= quiet_calls && lvl > kWinMinLevel[k]) {
            level[k].store(lvl - 1, std::memory_order_relaxed);
            quiet[k].store(0, std::memory_order_relaxed);
            probing[k].store(1, std::memory_order_relaxed);
        }
    }
};

// Band gate of one context.  Adaptive: noisy reads mostly fail the certificate and pay for both passes.  A context starts on
// probation (the band sees the first kBandProbationReads reads of a call only, so a failure is cheap); a call with fewer
// than half of its band reads falling back ends it, one with more switches the band off for a while and for
// twice as long every time a retry (again on probation) fails.
struct BandGate {
    int cooldown = 0;        // > 0: the band kernel is switched off for that many calls (too many certificates failed)
    int penalty = 32;        // length of the next cool-down (doubles while retries keep failing)
    bool probation = true;   // the band has not proved itself on this context's data yet: only a sample of the reads takes it

    // enough band reads to judge by, and more than half of them fell back to the exact kernels
    static bool mostly_failed(int band_reads, int fallbacks) { return band_reads >= 64 && 2 * fallbacks > band_reads; }

    void update(int band_reads, int fallbacks) {
        if (cooldown > 0) {
            --cooldown;
        } else if (band_reads >= 64) {
            if (mostly_failed(band_reads, fallbacks)) {
                cooldown = penalty;
                penalty = std::min(penalty * 2, 1 << 14);
                probation = true;
            } else {
                penalty = 32;
                probation = false;
            }
        }
    }
};

// work-queue lengths of the previous finished call (wave chunks), used to size the persistent grids of the
// kernels that usually have little or nothing to do: an idle block still claims its 70-80 KB of LDS on a CU
// and so delays the band blocks of the calls it overlaps with
struct GridHistory {
    bool valid = false;
    int band_mode = 0, reads = 1, exact_chunks = 0, wide_chunks = 0, n_long = 0;
    bool tail_heavy = false;   // the previous call had both band kernels busy (each more than a quarter of the other's cells)

    // does the history say anything about a call in `mode` (0: a whole batched call) with this band mode?
    bool usable(int mode, int band_mode_now) const { return mode == 0 && valid && band_mode == band_mode_now; }

    // expected chunks of the sparsely used kernels, from the previous call of this context (same band mode), scaled
    // to this batch with 50 % head-room; without history every grid is the full resident one.  A grid that turns
    // out too small only makes that kernel slower: every wave pulls chunks until the queue is empty.
    int predicted_blocks(bool usable_now, int chunks, int n_reads, int full) const {
        if (!usable_now) return full;
        const double scaled = (double)chunks * std::max(1, n_reads) / std::max(1, reads);
        const int blocks = chunks == 0 ? 1 : (int)(scaled * 1.5 / 4.0) + 2;
        return std::max(1, std::min(full, blocks));
    }

    // queue lengths of a finished call, for the grids of the next one
    void update(bool on_probation, int band_mode_ran, int n_reads, int n_exact_chunks, int n_wide_chunks, int n_long_items,
                uint64_t band_cells, uint64_t wide_cells) {
        // (a call on band probation sent all but its first reads to the exact kernels: its queue lengths say nothing about the
        // next call's — a one-block grid then crawled through 30 000 wide-band chunks in 46 ms, profiles/README.md round 3)
        valid = !on_probation;
        band_mode = band_mode_ran;
        reads = std::max(1, n_reads);
        exact_chunks = n_exact_chunks;
        wide_chunks = n_wide_chunks;
        n_long = n_long_items;
        // (cells, not event spans: with calls in flight a span includes the wait for the other call's kernels)
        tail_heavy = wide_cells > band_cells / 4 && band_cells > wide_cells / 4;
    }
};

}  // namespace strk_policy
