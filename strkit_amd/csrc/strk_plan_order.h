// strk_plan_order.h — how one block of k_plan orders the band items of its reads: a counting sort on (band class, prefix rows).
// Host and device share the constants and the bin of a key.  plan_order_host() RESTATES the block's steps one after the other for
// the host checks (tools/plan_order_asan.cpp, tests/test_band_scope_host.py): what runs under the sanitizers is that restatement —
// the bin arithmetic, the order rule, the slot bookkeeping — not k_plan's own shuffles, ballots and barriers.  Those are covered on
// the device only: tests/test_gpu_band_scope.py reads the class lists back and compares them with the order stated here.
//
// A block of k_plan covers a scope of consecutive reads: kPlanThreads threads, thread t takes the reads t, t + kPlanThreads, ...
// of the block (rpt of them, one after the other: plan_reads_per_thread).  The band kernel runs the 8 (4, 2, 1) items of a chunk in lock step for as many
// steps as the longest one needs, so a class list is best filled in the order of the prefix rows; the lists are filled block
// after block, and the more reads a block orders the less its chunks mix long items with short ones
// (tools/band_order_model.py: 256 reads 1.000, 1 024 reads 0.961, 2 048 reads 0.950, the whole call 0.938).
//
// Threads and reads per thread.  k_plan of one call runs NEXT to the band pass of the other call in flight: two band blocks per
// CU hold 2 x 168 of a SIMD's 512 VGPRs and all but 7 KB of the LDS (all but 4.5 KB until round 19), and a k_plan block that does not fit beside them waits for
// the band pass to end (the head of one call then no longer hides in the band pass of the other).  A block of 1 024 threads is
// four waves per SIMD and would have to live in 44 VGPRs; 512 threads x 4 reads are two waves per SIMD (88 VGPRs each), and
// the whole block state — histogram, class counters — stays under 4.5 KB of LDS.
// Four reads per thread are four times the serial depth of a thread, which a large call hides behind its many blocks and a
// small one does not: BASELINE config 5's 10 000 reads of up to 12 000 bases were 5 blocks where they had been 40, and the
// call got 2.5 % slower.  A call of fewer than kPlanSmallCall reads therefore runs one read per thread (a scope of 512 reads);
// its band pass is short anyway and a wider order would save it little.
//
// Order.  Items are listed by (class, bin of the prefix rows, read index).  The bins are as wide as the model says is free:
// 4 rows in the 8-lane layouts, 8 in the 16-lane ones (model: 0.950 -> 0.952 against exact rows); the two wide layouts, which
// k_sort_wide orders again across the call where that pays, get 64 and 128.  Inside a bin the order is the read index, never
// the order in which LDS atomics happen to arrive: list order decides which items share a chunk, and with it band_cells and
// the other statistics, which must not change from run to run.  The steps:
//   1  histogram: one LDS atomic per band item;
//   2  exclusive scan over the bins (each thread owns kPlanBinsPerThread bins; wave scan, then the wave totals);
//   3  slots: the 64 items of a wave's j-th reads find, by ballots, their rank among the wave's items of the same bin and the
//      first lane of that bin ("leader"); then the waves take turns in read order (j, wave) — one barrier per turn — and each
//      leader moves its bin's cursor by the size of its group.  slot = cursor before the move + rank in the group.
#pragma once
#include <stdint.h>

#include "strk_search.h"

namespace strk {

constexpr int kPlanThreads = 512;
constexpr int kPlanReadsPerThread = 4;   // large calls; 2: a block orders 1 024 reads, 4: 2 048 (the one that measured better)
constexpr int kPlanScope = kPlanThreads * kPlanReadsPerThread;   // the largest scope
constexpr int kPlanSmallCall = 16 * kPlanScope;   // below this many reads (16 blocks of the large scope: 128 waves on 1 024 SIMDs) one read per thread
STRK_HD constexpr int plan_reads_per_thread(int n_items) { return n_items < kPlanSmallCall ? 1 : kPlanReadsPerThread; }
STRK_HD constexpr int plan_scope_of(int n_items) { return kPlanThreads * plan_reads_per_thread(n_items); }
constexpr int kPlanWaves = kPlanThreads / 64;
static_assert(kPlanThreads % 64 == 0 && kPlanThreads <= 1024 && kPlanReadsPerThread >= 1, "whole waves, one block");

// bins of the prefix rows (|left flank| + (lo + n - 1) |motif|) per band class; a class holds rows up to band_max_db + kBandRowSlack
STRK_HD constexpr int plan_bin_shift(int c) { return (c & 3) == 0 ? 2 : ((c & 3) == 1 ? 3 : ((c & 3) == 2 ? 6 : 7)); }
STRK_HD constexpr int plan_class_bins(int c) { return ((band_max_db(c) + kBandRowSlack) >> plan_bin_shift(c)) + 1; }
// (classes c and c + 4 share a layout and its limits; a closed form, so that the device code holds no call)
STRK_HD constexpr int plan_layout_bin0(int l) {
    return l == 0 ? 0 : (l == 1 ? plan_class_bins(0) : (l == 2 ? plan_class_bins(0) + plan_class_bins(1) : plan_class_bins(0) + plan_class_bins(1) + plan_class_bins(2)));
}
constexpr int kPlanLayoutBins = plan_layout_bin0(3) + plan_class_bins(3);
STRK_HD constexpr int plan_class_bin0(int c) { return (c >= 4 ? kPlanLayoutBins : 0) + plan_layout_bin0(c & 3); }
constexpr int kPlanBins = 2 * kPlanLayoutBins;
static_assert(kNumBandClasses == 8, "two lane widths x four layouts");
static_assert(kPlanBins * 4 + 512 <= 4608, "k_plan: histogram and block counters in the 4.5 KB that two band blocks per CU leave free");
constexpr int kPlanBinsPerThread = (kPlanBins + kPlanThreads - 1) / kPlanThreads;
static_assert(kPlanBins <= (1 << 12) && kPlanScope <= (1 << 12), "k_plan keeps a band item's bin, then its slot, in 12 bits of one word");
STRK_HD int plan_bin(int c, int rows) {   // (band_geometry bounds the rows of an item it accepts; the clamp keeps any key inside the class)
    const int b = (rows < 0 ? 0 : rows) >> plan_bin_shift(c);
    return plan_class_bin0(c) + (b < plan_class_bins(c) ? b : plan_class_bins(c) - 1);
}

#if !defined(__HIP_DEVICE_COMPILE__)
// The block's steps on the host, for kPlanThreads * rpt keys: cls[i] = band class of read i of the block or -1 (no band item), rows[i] its
// prefix rows.  slot[i] = position of the item among the block's band items (-1: none); returns their number.  `hist` is the
// block's LDS histogram (kPlanBins ints).
inline int plan_order_host(const int* cls, const int* rows, int* slot, int* hist, int rpt = kPlanReadsPerThread) {
    for (int b = 0; b < kPlanBins; ++b) hist[b] = 0;
    for (int i = 0; i < kPlanThreads * rpt; ++i)
        if (cls[i] >= 0) ++hist[plan_bin(cls[i], rows[i])];
    // exclusive scan, thread by thread as the block does it: own bins, then the lanes in front, then the waves in front
    int wsum[kPlanWaves], own[kPlanThreads], incl[kPlanThreads];
    for (int t = 0; t < kPlanThreads; ++t) {
        own[t] = 0;
        for (int k = 0; k < kPlanBinsPerThread; ++k)
            if (t * kPlanBinsPerThread + k < kPlanBins) own[t] += hist[t * kPlanBinsPerThread + k];
        incl[t] = own[t] + ((t & 63) ? incl[t - 1] : 0);
        if ((t & 63) == 63) wsum[t >> 6] = incl[t];
    }
    int total = 0;
    for (int t = 0; t < kPlanThreads; ++t) {
        int pre = incl[t] - own[t];
        for (int w = 0; w < (t >> 6); ++w) pre += wsum[w];
        for (int k = 0; k < kPlanBinsPerThread; ++k) {
            const int b = t * kPlanBinsPerThread + k;
            if (b >= kPlanBins) break;
            const int c = hist[b];
            hist[b] = pre;
            pre += c;
        }
        if (t == kPlanThreads - 1) total = pre;
    }
    // slots: turn (j, wave); the wave's lanes group by bin with ballots
    for (int j = 0; j < rpt; ++j)
        for (int w = 0; w < kPlanWaves; ++w) {
            const int i0 = j * kPlanThreads + w * 64;
            int bin[64];
            uint64_t todo = 0;
            for (int l = 0; l < 64; ++l) {
                bin[l] = cls[i0 + l] >= 0 ? plan_bin(cls[i0 + l], rows[i0 + l]) : -1;
                slot[i0 + l] = -1;
                if (bin[l] >= 0) todo |= (uint64_t)1 << l;
            }
            while (todo) {
                const int first = __builtin_ctzll(todo);
                uint64_t same = 0;
                for (int l = 0; l < 64; ++l)
                    if (bin[l] == bin[first]) same |= (uint64_t)1 << l;
                const int base = hist[bin[first]];
                hist[bin[first]] = base + __builtin_popcountll(same);
                for (int l = 0; l < 64; ++l)
                    if (bin[l] == bin[first]) slot[i0 + l] = base + __builtin_popcountll(same & (((uint64_t)1 << l) - 1));
                todo &= ~same;
            }
        }
    return total;
}
#endif

}  // namespace strk
