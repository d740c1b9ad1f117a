// strk_realign_plan.h — what strk_realign decides on the host before any launch: the check of its input, the column class,
// tile count and padding of every pair, the cut of the call into chunks whose traces fit a budget, the order of the pairs
// inside a chunk and where each pair's trace, edge and CIGAR ranges lie in the chunk's workspaces.  Nothing of HIP in here:
// the header compiles with the host compiler alone (tools/realign_asan.cpp drives it; tests/test_host.py builds and runs
// that program).
#pragma once

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

#include "strk_groups.h"

namespace strk {

struct RealignPair {
    int64_t s1_off, s2_off;      // into the raw base arrays
    int64_t trace_off;           // bytes into the trace workspace
    int64_t edge_off;            // ints into the edge scratch (2 * 2 * n2 ints, tiles ping-pong), -1: single tile
    int64_t cig_off;             // uint32 units into the CIGAR buffer
    int32_t n1, n2;
    int32_t cl;                  // columns per lane: 4, 8, 16, 32
    int32_t ntiles;
    int32_t pad;                 // pad columns on the left of tile 0
    int32_t cig_cap;
    int32_t orig;                // caller's pair index
    int32_t reserved;
};

}  // namespace strk

namespace strk_realign_plan {

constexpr int kNoMem = -12;   // = STRK_E_NOMEM of include/strkit_amd.h (strk_api.hip asserts it)

// What the kernel's number format holds (derived next to kRealignNeg in strk_realign.h, which asserts that the two agree):
// a pair is exact if and only if 2 * open + (n1 - 2) * extend < kGapCostLimit.
constexpr int64_t kGapCostLimit = (int64_t)1 << 24;
inline int64_t gap_cost_reach(int64_t open, int64_t ext, int64_t n1) { return 2 * open + (n1 - 2) * ext; }

// Pairs [p0, p1) of the call, run together: as many pairs in caller order as fit the trace budget, and always at least one.
struct Chunk {
    int p0, p1;
    size_t tsum, esum, csum;   // trace bytes, edge ints and CIGAR words of the chunk's pairs
    double cells;              // DP cells with the pad columns, for the watchdog
};

struct Plan {
    // Every pair with n1, n2, cl, ntiles, pad and cig_cap.  Inside [p0, p1) of a chunk they stand in the order they run in
    // (widest class first, then most work first, stable), trace_off / edge_off / cig_off are laid out in that order and
    // `orig` is the caller's index less p0.
    std::vector<strk::RealignPair> pairs;
    std::vector<size_t> trace_bytes;   // per pair, by the caller's index; a multiple of 256
    std::vector<Chunk> chunks;         // consecutive, in caller order
};

inline int64_t pair_work(const strk::RealignPair& r) { return (int64_t)r.ntiles * (r.n2 + 63); }

// Returns 0 and the plan, or the code of a refusal (strk_groups::kInvalid; kNoMem for a trace beyond 128 GiB) with its text in
// `why`.  A call of no pairs is valid whatever its arrays are.
inline int plan(int32_t n_pairs, const int64_t* s1_off, const int64_t* s2_off, const int64_t* cigar_off, int32_t open, int32_t ext,
                int32_t gap_pref, size_t trace_budget, Plan* out, strk_groups::Message* why) {
    *out = Plan{};
    if (n_pairs < 0) return why->invalid("n_pairs < 0");
    if (n_pairs == 0) return 0;
    if (!s1_off || !s2_off || !cigar_off) return why->invalid("NULL argument");
    if (open < 0 || ext < 0 || open > 4096 || ext > open) return why->invalid("need 0 <= extend <= open <= 4096");
    if (gap_pref != 0 && gap_pref != 1) return why->invalid("bad gap_pref");
    std::vector<strk::RealignPair>& all = out->pairs;
    std::vector<size_t>& trace_bytes = out->trace_bytes;
    all.resize((size_t)n_pairs);
    trace_bytes.resize((size_t)n_pairs);
    for (int p = 0; p < n_pairs; ++p) {
        const int64_t n1 = s1_off[p + 1] - s1_off[p], n2 = s2_off[p + 1] - s2_off[p], cap = cigar_off[p + 1] - cigar_off[p];
        if (n1 < 1 || n2 < 1) return why->invalid("pair %d: empty sequence", p);
        if (n1 > (1 << 20) || n2 > (1 << 24))
            return why->invalid("pair %d: sequence too long (%lld x %lld)", p, (long long)n1, (long long)n2);
        if (gap_cost_reach(open, ext, n1) >= kGapCostLimit)
            return why->invalid("pair %d: gap costs beyond the number format (2*open + (n1 - 2)*extend = %lld, must be below %lld)", p,
                                (long long)gap_cost_reach(open, ext, n1), (long long)kGapCostLimit);
        if (cap < 0) return why->invalid("pair %d: negative CIGAR capacity", p);
        strk::RealignPair& r = all[p];
        r.s1_off = s1_off[p] - s1_off[0];
        r.s2_off = s2_off[p] - s2_off[0];
        r.n1 = (int32_t)n1;
        r.n2 = (int32_t)n2;
        r.cl = n1 <= 256 ? 4 : n1 <= 512 ? 8 : n1 <= 1024 ? 16 : 32;
        r.ntiles = (int32_t)((n1 + 64 * r.cl - 1) / (64 * r.cl));
        r.pad = r.ntiles * 64 * r.cl - (int32_t)n1;
        r.cig_cap = (int32_t)std::min<int64_t>(cap, 2 * n1 + 4);
        r.orig = p;
        r.reserved = 0;
        const size_t tb = (size_t)r.ntiles * (size_t)(n2 + 63) * 64 * (size_t)(r.cl / 2);
        trace_bytes[p] = (tb + 255) & ~(size_t)255;
        if (trace_bytes[p] > ((size_t)128 << 30)) {
            why->invalid("pair %d: trace of %zu bytes", p, trace_bytes[p]);
            return kNoMem;
        }
    }
    for (int p0 = 0; p0 < n_pairs;) {
        int p1 = p0;
        for (size_t sum = 0; p1 < n_pairs && (p1 == p0 || sum + trace_bytes[p1] <= trace_budget); ++p1) sum += trace_bytes[p1];
        std::stable_sort(all.begin() + p0, all.begin() + p1, [](const strk::RealignPair& x, const strk::RealignPair& y) {
            if (x.cl != y.cl) return x.cl > y.cl;
            return pair_work(x) > pair_work(y);
        });
        Chunk c{p0, p1, 0, 0, 0, 0.0};   // the sums: where the layout of each workspace ends
        for (int k = p0; k < p1; ++k) {
            strk::RealignPair& r = all[k];
            r.trace_off = (int64_t)c.tsum;
            c.tsum += trace_bytes[r.orig];
            r.edge_off = r.ntiles > 1 ? (int64_t)c.esum : -1;
            if (r.ntiles > 1) c.esum += (size_t)4 * r.n2;
            r.cig_off = (int64_t)c.csum;
            c.csum += (size_t)r.cig_cap;
            r.orig -= p0;
            c.cells += (double)r.ntiles * 64 * r.cl * (r.n2 + 63);
        }
        out->chunks.push_back(c);
        p0 = p1;
    }
    return 0;
}

}  // namespace strk_realign_plan
