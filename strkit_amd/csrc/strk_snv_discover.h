// strk_snv_discover.h — candidate SNVs of a locus from a pileup of its kept reads: the positions of a window on either side
// of the flanked locus at which two of the four bases A C G T each occur in enough reads.  What a read contributes at a position
// is the cell strk_phase_inputs.h's walk gives there (the same lo / hi with the clip take-in, the same handling of D, N, I,
// zero-length operations and a CIGAR longer than its bases); it counts when that byte is A, C, G or T and the read has no
// qualities or its quality there is >= min_base_qual.  The per-base test, the window and tile geometry and the thresholds are
// written once, for host and device (STRK_FE_HD); the host twin (host_discover_locus) and the kernels (k_snv_span,
// k_snv_pileup, k_snv_pick) call the same functions.  Without HIP the header compiles with the host compiler alone
// (tools/snv_discover_asan.cpp runs the walks, the checker and the host twin under the sanitizers).
//
// The reference has no such step (its candidate SNVs come from a VCF): the rule is this project's own and UNPINNED
// (DESIGN.md §21); its readable statement is strkit_amd/frontend/snv_discovery.py, and tests/test_snv_discover_host.py holds
// the two together.
#pragma once
#include <stdint.h>

#include <algorithm>
#include <vector>

#include "strk_phase_inputs.h"

namespace strk_sd {

constexpr int kTile = 4096;              // window positions of one workgroup of k_snv_pileup: 4 096 x 8 bytes of LDS
constexpr int kTileWords = kTile / 64;   // 64-bit words of a tile's candidate mask (512 bytes)
constexpr int kMaxWindow = 65536;        // window positions of a side: sixteen tiles
constexpr int kMaxKept = 65535;          // kept reads of a locus: a count has 16 bits of its position's LDS word
constexpr int64_t kMaxCoord = (int64_t)1 << 40;          // |left_coord|, |right_coord|: coordinate + window cannot wrap
constexpr int64_t kMaskBudget = (int64_t)512 << 20;      // bytes of the device's mask workspace: loci x 2 x tiles x 512

STRK_FE_HD int32_t tiles_per_side(int32_t window) { return (window + kTile - 1) / kTile; }

// The counter (0 .. 3 for A C G T) that the base at read position qi adds to, or -1: a position beyond the record's bases, one
// of the other twelve codes, or a quality below min_base_qual.
STRK_FE_HD int base_slot(const strk_fe::Rec& r, bool has_qual, int64_t qi, int32_t min_base_qual) {
    if (qi >= r.l_seq) return -1;
    const uint8_t byte = r.seq[qi >> 1];
    const uint32_t code = (qi & 1) ? (byte & 15u) : (uint32_t)(byte >> 4);
    const int slot = code == 1 ? 0 : code == 2 ? 1 : code == 4 ? 2 : code == 8 ? 3 : -1;
    if (slot < 0 || (has_qual && (int32_t)r.qual[qi] < min_base_qual)) return -1;
    return slot;
}

// Side 0 = left of the flanked locus, side 1 = right of it.  Bit b of a side stands for position side_base + b, b in
// [0, window); a position below 0 is never counted.
STRK_FE_HD int64_t side_base(int64_t left, int64_t right, int32_t window, int side) { return side == 0 ? left - window : right; }

// the positions [*c0, *t1) that tile k of a side counts; bit j of the tile = position *t0 + j
STRK_FE_HD void tile_range(int64_t left, int64_t right, int32_t window, int side, int32_t k, int64_t* t0, int64_t* c0, int64_t* t1) {
    const int64_t base = side_base(left, right, window, side);
    *t0 = base + (int64_t)k * kTile;
    const int64_t end = base + window;
    *t1 = *t0 + kTile < end ? *t0 + kTile : end;
    *c0 = *t0 > 0 ? *t0 : 0;
}

// whether at least two of the four 16-bit counts of a position's word reach a_thr
STRK_FE_HD bool is_candidate(uint64_t word, int32_t a_thr) {
    int n = 0;
    for (int k = 0; k < 4; ++k) n += (int32_t)((word >> (16 * k)) & 0xFFFFu) >= a_thr ? 1 : 0;
    return n >= 2;
}

// [lo, hi) of an alignment, one thread (the host twin of the wave of k_snv_span); false: no aligned pair
inline bool alignment_span(const uint8_t* cigar, int32_t n_cigar, int64_t start, int32_t clip_threshold, int32_t take_in, int64_t* lo, int64_t* hi) {
    int32_t clip_l, clip_r;
    strk_pi::cigar_clips(cigar, n_cigar, &clip_l, &clip_r);
    int64_t ref = start, e = 0;
    bool found = false;
    for (int32_t i = 0; i < n_cigar; ++i) {
        const uint32_t c = strk_fe::rd_u32(cigar + 4 * (size_t)i);
        int64_t dr, dq;
        strk_pi::op_advance(c, &dr, &dq);
        if (strk_fe::is_aligned(c & 15u) && (c >> 4) > 0) {
            if (!found) { found = true; *lo = ref + strk_pi::clip_take_in(clip_l, clip_threshold, take_in); }
            e = ref + (int64_t)(c >> 4);
        }
        ref += dr;
    }
    if (found) *hi = e - strk_pi::clip_take_in(clip_r, clip_threshold, take_in);
    return found;
}

// ---- input --------------------------------------------------------------------------------------------------------------------
struct DiscoverInput {
    int64_t n_bytes;                 // size of the buffer the records lie in
    int32_t n_items;
    const int64_t* rec_off;
    const int32_t* item_locus;
    int32_t n_loci;
    const int64_t* left_coord;       // per locus left_flank_coord and right_flank_coord
    const int64_t* right_coord;
    const int32_t* kept_off;
    const int32_t* kept_item;
    strk_fe::AltCigars alt;
    int32_t clip_threshold, take_in, window, min_base_qual, min_allele_reads;
};

// Returns 0, or strk_groups::kInvalid and in `msg` what is wrong.
inline int check_discover(const DiscoverInput& in, strk_groups::Message* msg) {
    if (in.n_items < 0 || in.n_loci < 0 || in.n_bytes < 0) return msg->invalid("n_items, n_loci or n_bytes < 0");
    if (in.clip_threshold < 0 || in.take_in < 0) return msg->invalid("clip_threshold and take_in must be >= 0");
    if (in.window < 1 || in.window > kMaxWindow) return msg->invalid("window must be in 1 .. %d: got %d", kMaxWindow, in.window);
    if (in.min_base_qual < 0 || in.min_base_qual > 255) return msg->invalid("min_base_qual must be in 0 .. 255: got %d", in.min_base_qual);
    if (in.min_allele_reads < 1) return msg->invalid("min_allele_reads must be >= 1");
    if (in.n_loci > INT32_MAX / strk_pi::kMaxCand) return msg->invalid("n_loci: at most %d loci in one call", INT32_MAX / strk_pi::kMaxCand);
    if (in.n_loci > 0 && (!in.left_coord || !in.right_coord)) return msg->invalid("NULL argument");
    for (int32_t l = 0; l < in.n_loci; ++l) {
        if (in.left_coord[l] > in.right_coord[l]) return msg->invalid("locus %d: left_coord > right_coord", l);
        if (in.left_coord[l] < -kMaxCoord || in.right_coord[l] > kMaxCoord) return msg->invalid("locus %d: coordinate outside +-2^40", l);
    }
    if (in.n_items > 0 && (!in.rec_off || !in.item_locus)) return msg->invalid("NULL argument");
    if (in.n_items > 0 && strk_fe::check_alt(in.n_items, in.alt, msg)) return strk_groups::kInvalid;
    for (int32_t i = 0; i < in.n_items; ++i) {
        if (in.rec_off[i] < 0 || in.rec_off[i] > in.n_bytes - 4) return msg->invalid("item %d: rec_off outside the buffer", i);
        if (in.item_locus[i] < 0 || in.item_locus[i] >= in.n_loci) return msg->invalid("item %d: item_locus out of range", i);
    }
    const strk_pi::UsefulInput kept{in.n_items, in.item_locus, in.n_loci, in.kept_off, in.kept_item, in.min_allele_reads};
    if (strk_pi::check_useful(kept, msg)) return strk_groups::kInvalid;
    for (int32_t l = 0; l < in.n_loci; ++l)
        if (in.kept_off[l + 1] - in.kept_off[l] > kMaxKept)
            return msg->invalid("locus %d: %d kept reads (at most %d: a count has 16 bits)", l, in.kept_off[l + 1] - in.kept_off[l], kMaxKept);
    return 0;
}

// ---- host twin ----------------------------------------------------------------------------------------------------------------
// The first of items [i0, i1) whose record is malformed, or -1.
inline int32_t host_first_bad(const uint8_t* buf, const DiscoverInput& in, int32_t i0, int32_t i1) {
    for (int32_t it = i0; it < i1; ++it) {
        strk_fe::Rec r;
        int64_t next = 0;
        if (!strk_fe::parse_rec(buf, in.n_bytes, in.rec_off[it], &r, &next)) return it;
    }
    return -1;
}

// The nearest-limit rule on the ascending candidates of a locus: beyond `limit`, the `limit` nearest to the flanked locus stay
// (distance left - p on the left, p - (right - 1) on the right; of two at one distance the left one first).  In place.
inline void keep_nearest(std::vector<int64_t>& cand, int64_t left, int64_t right, size_t limit) {
    if (cand.size() <= limit) return;
    int64_t i = (int64_t)(std::lower_bound(cand.begin(), cand.end(), left) - cand.begin()) - 1;   // the highest on the left
    int64_t j = i + 1;                                                                             // the lowest on the right
    for (size_t taken = 0; taken < limit; ++taken) {
        const int64_t dl = i >= 0 ? left - cand[(size_t)i] : INT64_MAX, dr = j < (int64_t)cand.size() ? cand[(size_t)j] - (right - 1) : INT64_MAX;
        if (dl <= dr) --i;
        else ++j;
    }
    cand.assign(cand.begin() + (i + 1), cand.begin() + j);
}

// Locus l of a checked call whose records all parse: its candidates, ascending, into `out`.  `counts`: scratch of the thread.
inline void host_discover_locus(const uint8_t* buf, const DiscoverInput& in, int32_t l, std::vector<uint32_t>& counts, std::vector<int64_t>& out) {
    out.clear();
    const int32_t k0 = in.kept_off[l], n = in.kept_off[l + 1] - k0, w = in.window;
    if (n == 0) return;
    const int64_t left = in.left_coord[l], right = in.right_coord[l];
    counts.assign((size_t)8 * w, 0u);   // [side][bit][4]
    for (int32_t k = 0; k < n; ++k) {
        const int32_t it = in.kept_item[k0 + k];
        strk_fe::Rec r;
        int64_t next = 0, start, lo = 0, hi = 0;
        if (!strk_fe::parse_rec(buf, in.n_bytes, in.rec_off[it], &r, &next)) continue;
        const uint8_t* cig;
        int32_t n_cig;
        strk_fe::item_alignment(r, it, in.alt, &cig, &n_cig, &start);
        if (!alignment_span(cig, n_cig, start, in.clip_threshold, in.take_in, &lo, &hi)) continue;
        const bool has_qual = !(r.l_seq > 0 && r.qual[0] == 0xFF);
        int64_t ref = start, q = 0;
        for (int32_t i = 0; i < n_cig; ++i) {
            const uint32_t c = strk_fe::rd_u32(cig + 4 * (size_t)i);
            int64_t dr, dq;
            strk_pi::op_advance(c, &dr, &dq);
            if (strk_fe::is_aligned(c & 15u) && (c >> 4) > 0) {
                for (int side = 0; side < 2; ++side) {
                    const int64_t base = side_base(left, right, w, side);
                    const int64_t a = std::max({ref, lo, base, (int64_t)0}), b = std::min({ref + (int64_t)(c >> 4), hi, base + w});
                    for (int64_t p = a; p < b; ++p) {
                        const int slot = base_slot(r, has_qual, q + (p - ref), in.min_base_qual);
                        if (slot >= 0) ++counts[((size_t)side * w + (size_t)(p - base)) * 4 + slot];
                    }
                }
            }
            ref += dr; q += dq;
        }
    }
    int32_t a_thr, t_thr;
    strk_pi::thresholds(n, in.min_allele_reads, &a_thr, &t_thr);
    for (int side = 0; side < 2; ++side)
        for (int32_t b = 0; b < w; ++b) {
            const uint32_t* c = &counts[((size_t)side * w + b) * 4];
            if ((c[0] >= (uint32_t)a_thr) + (c[1] >= (uint32_t)a_thr) + (c[2] >= (uint32_t)a_thr) + (c[3] >= (uint32_t)a_thr) >= 2)
                out.push_back(side_base(left, right, w, side) + b);
        }
    keep_nearest(out, left, right, (size_t)strk_pi::kMaxCand);
}

}  // namespace strk_sd

#if defined(__HIPCC__)
namespace strk_sd {

// One wave per item, four items per workgroup: [lo, hi) of the item's alignment into span[2 it], span[2 it + 1] (0, 0 for an
// alignment without an aligned pair and for a malformed record, which is also reported in `bad`).  The CIGAR is taken 64
// operations per pass with the two wave scans of k_dbam_phase_cells; only lane 0 writes.
__global__ void __launch_bounds__(256) k_snv_span(const uint8_t* data, int64_t n_data, int item0, int item1, const int64_t* rec_off,
                                                  strk_fe::AltCigars alt, int clip_threshold, int take_in, int64_t* span, int32_t* bad) {
    const int lane = threadIdx.x & 63;
    const int it = item0 + blockIdx.x * 4 + (threadIdx.x >> 6);
    if (it >= item1) return;
    strk_fe::Rec r;
    int64_t next = 0;
    if (!strk_fe::parse_rec(data, n_data, rec_off[it], &r, &next)) {
        if (lane == 0) {
            atomicMax(bad, INT32_MAX - it);
            span[2 * (size_t)it] = 0; span[2 * (size_t)it + 1] = 0;
        }
        return;
    }
    const uint8_t* cig;
    int32_t n_cig;
    int64_t car_r;
    strk_fe::item_alignment(r, it, alt, &cig, &n_cig, &car_r);
    int32_t clip_l, clip_r;
    strk_pi::cigar_clips(cig, n_cig, &clip_l, &clip_r);
    int64_t lo = 0, e = 0;
    bool found = false;
    for (int32_t i0 = 0; i0 < n_cig; i0 += 64) {
        const int32_t i = i0 + lane;
        const uint32_t c = i < n_cig ? strk_fe::rd_u32(cig + 4 * (size_t)i) : 0u;
        int64_t dr, dq;
        strk_pi::op_advance(c, &dr, &dq);
        const int64_t sr = strk_pi::wave_scan_incl(dr, lane);
        const int64_t r0 = car_r + sr - dr;
        const unsigned long long m = __ballot(strk_fe::is_aligned(c & 15u) && (c >> 4) > 0);
        if (m) {   // (the same for every lane)
            if (!found) {
                found = true;
                lo = (int64_t)__shfl((long long)r0, __ffsll((long long)m) - 1, 64) + strk_pi::clip_take_in(clip_l, clip_threshold, take_in);
            }
            e = (int64_t)__shfl((long long)(r0 + (int64_t)(c >> 4)), 63 - __clzll((long long)m), 64);
        }
        car_r += (int64_t)__shfl((long long)sr, 63, 64);
    }
    if (lane == 0) {
        span[2 * (size_t)it] = found ? lo : 0;
        span[2 * (size_t)it + 1] = found ? e - strk_pi::clip_take_in(clip_r, clip_threshold, take_in) : 0;
    }
}

// One workgroup per (locus, tile), block0 + blockIdx.x = locus * 2 T + side * T + tile (T tiles per side).  A position's four
// counts lie in one 64-bit LDS word, 16 bits each (a read adds at most 1 to a position and a locus has at most 65 535 kept
// reads, so no count carries into its neighbour): 32 KB per workgroup.  The four waves take the locus's kept reads in turn; a
// read whose [lo, hi) (k_snv_span) does not reach the tile is skipped before its record is touched.  A wave walks its read's
// CIGAR 64 operations per pass, lane i holding operation i; the part of an aligned operation inside the tile shorter than
// `long_op` bases is counted by its lane, a longer one by all 64 lanes (ballot, then one broadcast per long operation): the
// counts are sums, so the switch changes no result.  After the barrier thread t tests positions t, t + 256, ... and lane 0 of
// every wave writes the ballot: word 4 i + w of the tile's 64 mask words, a slot no other wave writes.
__global__ void __launch_bounds__(256) k_snv_pileup(const uint8_t* data, int64_t n_data, int block0, const int64_t* rec_off, strk_fe::AltCigars alt,
                                                    const int64_t* span, const int64_t* left_coord, const int64_t* right_coord,
                                                    const int32_t* kept_off, const int32_t* kept_item, int window, int n_tiles,
                                                    int min_base_qual, int min_allele_reads, int long_op, unsigned long long* masks) {
    __shared__ unsigned long long cnt[kTile];
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    const int64_t blk = (int64_t)block0 + blockIdx.x;
    const int l = (int)(blk / (2 * n_tiles)), tile = (int)(blk % (2 * n_tiles));
    int64_t t0, c0, t1;
    tile_range(left_coord[l], right_coord[l], window, tile / n_tiles, tile % n_tiles, &t0, &c0, &t1);
    for (int j = t; j < kTile; j += 256) cnt[j] = 0ull;
    __syncthreads();
    const int32_t k0 = kept_off[l], n = kept_off[l + 1] - k0;
    for (int32_t k = w; k < n; k += 4) {   // (everything that decides a branch below is the same for the lanes of a wave)
        const int32_t it = kept_item[k0 + k];
        const int64_t s_lo = span[2 * (size_t)it], s_hi = span[2 * (size_t)it + 1];
        const int64_t lo = s_lo > c0 ? s_lo : c0, hi = s_hi < t1 ? s_hi : t1;
        if (lo >= hi) continue;
        strk_fe::Rec r;
        int64_t next = 0;
        if (!strk_fe::parse_rec(data, n_data, rec_off[it], &r, &next)) continue;
        const uint8_t* cig;
        int32_t n_cig;
        int64_t car_r, car_q = 0;
        strk_fe::item_alignment(r, it, alt, &cig, &n_cig, &car_r);
        const bool has_qual = !(r.l_seq > 0 && r.qual[0] == 0xFF);
        for (int32_t i0 = 0; i0 < n_cig && car_r < hi; i0 += 64) {
            const int32_t i = i0 + lane;
            const uint32_t c = i < n_cig ? strk_fe::rd_u32(cig + 4 * (size_t)i) : 0u;
            int64_t dr, dq;
            strk_pi::op_advance(c, &dr, &dq);
            const int64_t sr = strk_pi::wave_scan_incl(dr, lane), sq = strk_pi::wave_scan_incl(dq, lane);
            const int64_t r0 = car_r + sr - dr, q0 = car_q + sq - dq;
            int64_t a = r0 > lo ? r0 : lo, b = r0 + (int64_t)(c >> 4) < hi ? r0 + (int64_t)(c >> 4) : hi;
            if (!strk_fe::is_aligned(c & 15u) || a >= b) a = b = 0;
            const bool spread = b - a >= long_op;
            if (!spread)
                for (int64_t p = a; p < b; ++p) {
                    const int slot = base_slot(r, has_qual, q0 + (p - r0), min_base_qual);
                    if (slot >= 0) atomicAdd(&cnt[p - t0], 1ull << (16 * slot));
                }
            for (unsigned long long m = __ballot(spread); m; m &= m - 1) {
                const int src = __ffsll((long long)m) - 1;
                const int64_t sa = (int64_t)__shfl((long long)a, src, 64), sb = (int64_t)__shfl((long long)b, src, 64);
                const int64_t sd = (int64_t)__shfl((long long)(q0 - r0), src, 64);
                for (int64_t p = sa + lane; p < sb; p += 64) {
                    const int slot = base_slot(r, has_qual, p + sd, min_base_qual);
                    if (slot >= 0) atomicAdd(&cnt[p - t0], 1ull << (16 * slot));
                }
            }
            car_r += (int64_t)__shfl((long long)sr, 63, 64);
            car_q += (int64_t)__shfl((long long)sq, 63, 64);
        }
    }
    __syncthreads();
    int32_t a_thr, t_thr;
    strk_pi::thresholds(n, min_allele_reads, &a_thr, &t_thr);
    for (int i = 0; i < kTile / 256; ++i) {
        const unsigned long long m = __ballot(is_candidate(cnt[i * 256 + t], a_thr));
        if (lane == 0) masks[(size_t)blk * kTileWords + 4 * i + w] = m;
    }
}

// the bits of word wi of a side's mask whose distance to the flanked locus is <= dist (left: bit >= window - dist; right: bit < dist)
__device__ inline unsigned long long near_bits(const unsigned long long* side_mask, int side, int wi, int window, int dist) {
    const int b0 = wi * 64;
    unsigned long long v = side_mask[wi];
    if (side == 0) {
        const int first = window - dist;
        if (b0 + 63 < first) return 0ull;
        if (b0 < first) v &= ~0ull << (first - b0);
    } else {
        if (b0 >= dist) return 0ull;
        if (b0 + 64 > dist) v &= ~0ull >> (b0 + 64 - dist);
    }
    return v;
}

// One workgroup per locus over the 2 T x 64 mask words of its tiles (left side first: the words are in position order).
// out_pos == NULL: counts the candidates; beyond 1 024 it finds, by bisection over the distance, the 1 024 nearest to the
// flanked locus (at one distance there is at most one position a side, the left one goes first), and writes n_cand[l] and the
// two distances kept (keep[2 l], keep[2 l + 1]).  out_pos given (after the host's prefix sum, cand_off): thread t takes a
// contiguous run of words, the runs' popcounts give it its place, and it writes its positions ascending.
__global__ void __launch_bounds__(256) k_snv_pick(const unsigned long long* masks, const int64_t* left_coord, const int64_t* right_coord, int window,
                                                  int n_tiles, const int32_t* cand_off, int32_t* n_cand, int32_t* keep, int64_t* out_pos) {
    __shared__ int32_t part[256];
    __shared__ int32_t total;
    const int l = blockIdx.x, t = threadIdx.x, wps = n_tiles * kTileWords;
    const unsigned long long* const m_left = masks + (size_t)l * 2 * wps;
    const unsigned long long* const m_right = m_left + wps;
    auto count_near = [&](int d_left, int d_right) -> int32_t {   // (called by every thread)
        int32_t mine = 0;
        for (int wi = t; wi < wps; wi += 256) mine += __popcll(near_bits(m_left, 0, wi, window, d_left)) + __popcll(near_bits(m_right, 1, wi, window, d_right));
        __syncthreads();
        if (t == 0) total = 0;
        __syncthreads();
        if (mine) atomicAdd(&total, mine);
        __syncthreads();
        return total;
    };
    if (!out_pos) {
        int32_t n = count_near(window, window);
        int d_left = window, d_right = window;
        if (n > strk_pi::kMaxCand) {
            int lo = 1, hi = window;   // the smallest distance within which kMaxCand or more lie
            while (lo < hi) {
                const int mid = (lo + hi) >> 1;
                if (count_near(mid, mid) >= strk_pi::kMaxCand) hi = mid;
                else lo = mid + 1;
            }
            const int32_t below = count_near(lo - 1, lo - 1);
            d_left = d_right = lo;
            if (strk_pi::kMaxCand - below < 2) {   // room for one of the (at most two) positions at distance lo: the left one if there is one
                if (count_near(lo, lo - 1) > below) d_right = lo - 1;
                else d_left = lo - 1;
            }
            n = strk_pi::kMaxCand;
        }
        if (t == 0) { n_cand[l] = n; keep[2 * l] = d_left; keep[2 * l + 1] = d_right; }
        return;
    }
    const int d_left = keep[2 * l], d_right = keep[2 * l + 1];
    const int per = (2 * wps + 255) / 256, w0 = t * per, w1 = w0 + per < 2 * wps ? w0 + per : 2 * wps;
    int32_t mine = 0;
    for (int wi = w0; wi < w1; ++wi) mine += __popcll(wi < wps ? near_bits(m_left, 0, wi, window, d_left) : near_bits(m_right, 1, wi - wps, window, d_right));
    part[t] = mine;
    __syncthreads();
    int64_t at = cand_off[l];
    for (int k = 0; k < t; ++k) at += part[k];
    for (int wi = w0; wi < w1; ++wi) {
        const int side = wi < wps ? 0 : 1, sw = side ? wi - wps : wi;
        const int64_t p0 = side_base(left_coord[l], right_coord[l], window, side) + (int64_t)sw * 64;
        for (unsigned long long v = near_bits(side ? m_right : m_left, side, sw, window, side ? d_right : d_left); v; v &= v - 1)
            out_pos[at++] = p0 + (__ffsll((long long)v) - 1);
    }
}

}  // namespace strk_sd
#endif
