// strk_consensus.h — best representative of every group of sequences on gfx950 (strk_best_representatives).
//
// Stands where the reference calls strkit_rust_ext.consensus_seq (strkit/call/call_locus.py:1602-1613) for the methods
// `single` and `best_rep`; partial-order alignment is strk_poa.h.  The definition (the CPU restatement
// that the tests compare against is tests/consensus_restatement.py): all strings of a group byte-identical -> string 0,
// `single`; otherwise the smallest i with minimal D(i) = sum_j lev(s_i, s_j), unit-cost Levenshtein on raw bytes.
//
// k_best_rep: one workgroup of sixteen waves per group.
//   1. every string's hash (a wave per string, lanes stride over its bytes) and the set of byte values of the group;
//   2. every string's first equal predecessor (hash and length first, then a wave-wide byte comparison): the distinct
//      strings u_0..u_{d-1} with multiplicities c_k, and the alphabet's code map (thread 0);
//   3. one wave per unordered pair of distinct strings: bit-parallel Levenshtein (Myers 1999 in Hyyrö's block form).
//      The shorter string is the pattern; lane l owns rows 64l..64l+63 of the DP column as the words Pv / Mv and works on
//      text position t - l at step t (the skew of the DP kernels), the block's horizontal delta and the text byte travel
//      to lane l + 1 in one word.  A pattern beyond 4 096 rows takes several passes; the deltas along the last row of a
//      pass wait in global memory (one byte per text position) for the next.  The match word Eq comes from bit planes
//      of the pattern's codes kept in registers: Eq = ~OR_k (plane_k ^ -(bit k of the text code)), three planes when
//      the group uses at most eight byte values (any DNA), eight planes of the raw bytes otherwise.
//      lev * multiplicity goes to both strings' sums by LDS atomics (a sum is at most 250 * 65 535, 32 bits hold it);
//   4. thread 0 picks the first minimum over the distinct strings in original order.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace strk {

constexpr int kConsMaxGroup = 250;      // max_reads of the caller
constexpr int kConsMaxLen = 65535;
constexpr int kConsThreads = 1024;
constexpr int kConsWaves = kConsThreads / 64;
constexpr int kConsPassRows = 64 * 64;  // rows one pass of a wave covers
constexpr int kConsNone = 0, kConsSingle = 1, kConsBestRep = 2;

struct ConsArgs {
    const int32_t* group_off;   // [n_groups + 1] into seq_start / seq_len
    const uint8_t* seqs;
    const int64_t* seq_start;
    const int32_t* seq_len;
    uint8_t* bound;             // kConsWaves * bound_stride bytes per group (nullptr when no pattern exceeds one pass)
    int64_t bound_stride;
    int32_t* out_index;
    int32_t* out_method;
    int64_t* out_dist;
    int32_t n_groups;
};

// Levenshtein distance of pat[0..m) and txt[0..n), 1 <= m <= n, by the 64 lanes of one wave.  NP: bit planes per code.
template <int NP>
__device__ inline int cons_lev_wave(const uint8_t* __restrict__ pat, int m, const uint8_t* __restrict__ txt, int n,
                                    const uint8_t* s_map, uint8_t* bound, int lane) {
    const int W = (m + 63) >> 6;
    int score = 0;
    for (int b0 = 0; b0 < W; b0 += 64) {
        const int nb = min(64, W - b0);
        const bool last_pass = b0 + 64 >= W;
        const bool act = lane < nb;
        uint64_t pl[NP];
#pragma unroll
        for (int k = 0; k < NP; ++k) pl[k] = 0;
        if (act) {
            const int r0 = (b0 + lane) << 6;
            const int nr = min(64, m - r0);
            for (int i = 0; i < nr; ++i) {
                unsigned c = pat[r0 + i];
                if (NP < 8) c = s_map[c];
#pragma unroll
                for (int k = 0; k < NP; ++k) pl[k] |= (uint64_t)((c >> k) & 1u) << i;
            }
        }
        const bool tail = last_pass && lane == nb - 1;   // the lane that holds row m
        const uint64_t hbit = 1ull << (tail ? ((m - 1) & 63) : 63);
        uint64_t Pv = ~0ull, Mv = 0;
        int sc = tail ? m : 0;   // D[m][0]
        int carry = 0;           // (text code << 2 | hout + 1) of this lane's last step
        int chunk_c = 0, chunk_h = 2;
        const int steps = n + nb - 1;
        for (int t = 0; t < steps; ++t) {
            const int k = t & 63;
            if (k == 0) {   // the next 64 text bytes (and the deltas along the previous pass's last row), one per lane
                const int p = t + lane;
                unsigned c = p < n ? txt[p] : 0u;
                if (NP < 8) c = s_map[c];
                chunk_c = (int)c;
                if (b0 > 0) chunk_h = p < n ? bound[p] : 2;
            }
            int in = __builtin_amdgcn_update_dpp(0, carry, 0x138, 0xf, 0xf, false);   // wave_shr:1, lane l takes lane l - 1's word
            const int c0 = __builtin_amdgcn_readlane(chunk_c, k);
            const int h0 = __builtin_amdgcn_readlane(chunk_h, k);
            if (lane == 0) in = (c0 << 2) | h0;   // row 0 of the matrix: delta +1
            const int j = t - lane;
            if (act && j >= 0 && j < n) {
                const unsigned c = (unsigned)in >> 2;
                const int hin = (in & 3) - 1;
                uint64_t ne = 0;
#pragma unroll
                for (int q = 0; q < NP; ++q) ne |= pl[q] ^ (0ull - (uint64_t)((c >> q) & 1u));
                uint64_t Eq = ~ne;
                const uint64_t hneg = hin < 0 ? 1ull : 0ull;
                const uint64_t Xv = Eq | Mv;
                Eq |= hneg;
                const uint64_t Xh = (((Eq & Pv) + Pv) ^ Pv) | Eq;
                uint64_t Ph = Mv | ~(Xh | Pv);
                uint64_t Mh = Pv & Xh;
                const int hout = (int)((Ph & hbit) != 0) - (int)((Mh & hbit) != 0);
                Ph = (Ph << 1) | (hin > 0 ? 1ull : 0ull);
                Mh = (Mh << 1) | hneg;
                Pv = Mh | ~(Xv | Ph);
                Mv = Ph & Xv;
                carry = (int)(c << 2) | (hout + 1);
                sc += hout;
                if (!last_pass && lane == 63) bound[j] = (uint8_t)(hout + 1);
            }
        }
        if (last_pass) score = __shfl(sc, nb - 1);
        else __threadfence();   // the next pass reads what lane 63 wrote
    }
    return score;
}

__global__ __launch_bounds__(kConsThreads) void k_best_rep(ConsArgs a) {
    __shared__ uint32_t s_hash[kConsMaxGroup];
    __shared__ int32_t s_rep[kConsMaxGroup];
    __shared__ int32_t s_uniq[kConsMaxGroup];
    __shared__ int32_t s_cnt[kConsMaxGroup];
    __shared__ uint32_t s_sum[kConsMaxGroup];
    __shared__ uint32_t s_pres[8];
    __shared__ uint8_t s_map[256];
    __shared__ int32_t s_d, s_sigma;

    const int g = blockIdx.x;
    if (g >= a.n_groups) return;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int q0 = a.group_off[g];
    const int m = a.group_off[g + 1] - q0;
    if (m <= 0) {
        if (tid == 0) {
            a.out_index[g] = -1;
            a.out_method[g] = kConsNone;
            a.out_dist[g] = 0;
        }
        return;
    }
    const int64_t* st = a.seq_start + q0;
    const int32_t* ln = a.seq_len + q0;
    for (int i = tid; i < m; i += kConsThreads) {
        s_hash[i] = 0;
        s_sum[i] = 0;
    }
    if (tid < 8) s_pres[tid] = 0;
    __syncthreads();
    // 1. hashes and the alphabet
    for (int i = wave; i < m; i += kConsWaves) {
        const uint8_t* s = a.seqs + st[i];
        const int len = ln[i];
        uint32_t h = 0;
        for (int p = lane; p < len; p += 64) {
            const uint32_t b = s[p];
            h += (b + 1u) * ((uint32_t)p * 2654435761u + 0x9E3779B9u);
            if (!((s_pres[b >> 5] >> (b & 31)) & 1u)) atomicOr(&s_pres[b >> 5], 1u << (b & 31));
        }
        if (len > 0) atomicAdd(&s_hash[i], h);
    }
    __syncthreads();
    // 2. first equal predecessor of every string
    for (int i = wave; i < m; i += kConsWaves) {
        const uint8_t* s = a.seqs + st[i];
        const int len = ln[i];
        const uint32_t h = s_hash[i];
        int rep = i;
        for (int j0 = 0; j0 < i && rep == i; j0 += 64) {
            const int j = j0 + lane;
            unsigned long long cand = __ballot(j < i && s_hash[j] == h && ln[j] == len);
            while (cand) {
                const int jj = j0 + __ffsll((long long)cand) - 1;
                cand &= cand - 1;
                const uint8_t* o = a.seqs + st[jj];
                bool diff = false;
                for (int p0 = 0; p0 < len && !diff; p0 += 64) {
                    const int p = p0 + lane;
                    diff = __any(p < len && s[p] != o[p]) != 0;
                }
                if (!diff) {
                    rep = jj;
                    break;
                }
            }
        }
        if (lane == 0) s_rep[i] = rep;
    }
    __syncthreads();
    if (tid == 0) {
        int d = 0;
        for (int i = 0; i < m; ++i) {
            const int r = s_rep[i];
            if (r == i) {
                s_uniq[d] = i;
                s_cnt[d] = 1;
                s_rep[i] = -1 - d;   // a distinct string keeps its slot, coded below zero
                ++d;
            } else {
                s_cnt[-1 - s_rep[r]] += 1;
            }
        }
        s_d = d;
        int sigma = 0;
        for (int b = 0; b < 256; ++b) {
            const bool on = (s_pres[b >> 5] >> (b & 31)) & 1u;
            s_map[b] = on ? (uint8_t)(sigma & 7) : 0;
            sigma += on;
        }
        s_sigma = sigma;
    }
    __syncthreads();
    const int d = s_d;
    if (d == 1) {
        if (tid == 0) {
            a.out_index[g] = 0;
            a.out_method[g] = kConsSingle;
            a.out_dist[g] = 0;
        }
        return;
    }
    // 3. one wave per pair (x < y) of distinct strings
    const bool small_alphabet = s_sigma <= 8;
    uint8_t* bound = a.bound ? a.bound + ((int64_t)g * kConsWaves + wave) * a.bound_stride : nullptr;
    int x = 0, y = 1 + wave;
    for (;;) {
        while (x < d - 1 && y >= d) {
            y = y - d + x + 2;
            ++x;
        }
        if (x >= d - 1) break;
        const int ix = s_uniq[x], iy = s_uniq[y];
        int lx = __builtin_amdgcn_readfirstlane(ln[ix]), ly = __builtin_amdgcn_readfirstlane(ln[iy]);
        const uint8_t* sx = a.seqs + st[ix];
        const uint8_t* sy = a.seqs + st[iy];
        if (lx > ly) {
            const uint8_t* ts = sx;
            sx = sy;
            sy = ts;
            const int tl = lx;
            lx = ly;
            ly = tl;
        }
        int dist;
        if (lx == 0) dist = ly;
        else if (small_alphabet) dist = cons_lev_wave<3>(sx, lx, sy, ly, s_map, bound, lane);
        else dist = cons_lev_wave<8>(sx, lx, sy, ly, s_map, bound, lane);
        if (lane == 0) {
            atomicAdd(&s_sum[x], (uint32_t)dist * (uint32_t)s_cnt[y]);
            atomicAdd(&s_sum[y], (uint32_t)dist * (uint32_t)s_cnt[x]);
        }
        y += kConsWaves;
    }
    __syncthreads();
    // 4. the first minimum in original order
    if (tid == 0) {
        int best = 0;
        for (int k = 1; k < d; ++k)
            if (s_sum[k] < s_sum[best]) best = k;
        a.out_index[g] = s_uniq[best];
        a.out_method[g] = kConsBestRep;
        a.out_dist[g] = (int64_t)s_sum[best];
    }
}

}  // namespace strk
