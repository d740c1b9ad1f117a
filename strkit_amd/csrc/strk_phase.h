// strk_phase.h — phased allele calls on gfx950: reads grouped by their haplotags or by the SNVs they carry, one single-allele
// call per group.
//
// Replaces STRkit's call_alleles_with_haplotags (call_locus.py:222-288), call_alleles_with_incorporated_snvs (:457-714) with
// calculate_read_distance (:91-174) and sklearn's average-linkage clustering, and call_and_filter_useful_snvs (snvs.py:63-171),
// as rule A-F of DESIGN.md §13; the CPU restatement that the tests compare against is tests/phase_restatement.py.
//
// k_phase_group   one workgroup per locus: the haplotag decision (B), else the SNV decision (C): per-read masks of the cells that
//                 count, the float64 distance matrix over the clustered reads (parallel over pairs; in LDS up to kPhaseLdsReads
//                 reads, beyond that in the locus's global workspace), scipy's nearest-neighbour chain on it (wave 0: every row
//                 arg-min a wave reduction over (value, index), every Lance-Williams update parallel over lanes), the cut at two
//                 clusters.  Leaves the reads of the locus's groups as a permutation, the group sizes and the group seeds.
// k_phase_pack    the groups' reads (cn, renormalised w) packed one group behind the other, with the CSR offsets and workspace
//                 offsets that k_alleles takes.  A block's base offset is the sum of the sizes in front of it, which every block
//                 forms for itself: no block waits for another.
// k_alleles       (strk_alleles.h: k_alleles_w<2>) over the 2 L groups as single-allele loci.
// k_phase_finish  one workgroup per locus: peak order, the combined call, every read's peak, the SNV calls (E).
// Nothing here counts with an atomic where the order of the reads decides a tie; the LDS atomics of k_phase_group form sums,
// minima and maxima only.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "strk_alleles.h"

namespace strk {

constexpr int kPhaseMaxReads = 1024;
constexpr int kPhaseMaxSnvs = 64;
// the distance matrix of up to this many clustered reads lies in LDS: 80 * 80 * 8 = 51 200 bytes, with the per-read arrays
// 61.1 KiB (62 528 bytes) per workgroup, so that two workgroups share a CU's 160 KiB
constexpr int kPhaseLdsReads = 80;
constexpr int kPhaseThreads = 256;
constexpr int kPhasePackLoci = 128;       // loci (= 256 groups) per block of k_phase_pack
constexpr int kPhaseFinishThreads = 128;  // one thread per (SNV, peak)
constexpr int kPhaseOutI = kAlleleOutI + 3;   // the 14 of k_alleles, then method, reason, ps
constexpr int kPhaseMeta = 4;                 // per locus between the kernels: method, reason, ps, status

enum { kAssignNone = 0, kAssignHp = 1, kAssignSnv = 2, kAssignSnvDist = 3 };
enum { kReasonNone = 0, kReasonNoTags, kReasonTagThresholds, kReasonFewSnvReads, kReasonGroupNotCalled, kReasonNoSnvCalled };
enum { kSnvNotEvaluated = -1, kSnvCalled = 0, kSnvZeroTotal, kSnvOnlyOutOfRange, kSnvCrossTalk, kSnvSameBase };
constexpr int kStatusCalled = 0, kStatusTooFew = 1, kStatusNotPhased = 3;
constexpr uint8_t kSnvOutOfRange = '-', kSnvGap = '_';

struct PhaseArgs {
    // the piece as the caller gave it (offsets relative to the piece)
    const int32_t* read_off;   // [n_loci + 1]
    const int32_t* cn;
    const double* w;
    const int32_t* n_alleles;
    const uint64_t* seed;
    const int32_t *hp, *ps;      // [n_reads], or both NULL
    const int32_t* snv_off;      // [n_loci + 1], or NULL (no locus has an SNV)
    const int64_t* cell_off;     // [n_loci]: the locus's first cell in snv_base / snv_qual
    const uint8_t *snv_base, *snv_qual;
    const int64_t* ws_off;       // bytes into ws per locus (k_phase_group's workspace)
    char* ws;
    const int64_t* aws_base;     // [n_loci]: bytes into k_alleles' workspace for the locus's two groups
    // k_phase_group -> k_phase_pack, k_phase_finish
    int32_t* perm;     // [n_reads]: per locus, the reads of group 0 then of group 1 (indices inside the locus)
    int32_t* gsz;      // [2 n_loci]
    int32_t* meta;     // [n_loci][kPhaseMeta]
    uint64_t* gseed;   // [2 n_loci]
    int32_t* gone;     // [2 n_loci]: n_alleles of every group, 1
    // k_phase_pack -> k_alleles
    int32_t* goff;     // [2 n_loci + 1]
    int64_t* gws_off;  // [2 n_loci]
    int32_t* gcn;      // [n_reads]
    double* gw;
    // k_alleles -> k_phase_finish
    const int32_t* g_oi;   // [2 n_loci][kAlleleOutI]
    const double* g_od;    // [2 n_loci][kAlleleOutD]
    // k_phase_finish
    int32_t* out_i;        // [n_loci][kPhaseOutI]
    double* out_d;         // [n_loci][kAlleleOutD]
    int32_t* read_peak;    // [n_reads]
    int32_t* snv_status;   // [n_snvs]
    uint8_t* snv_call;     // [n_snvs][2]
    int32_t* snv_rcs;      // [n_snvs][2]
    int32_t n_loci;
    int32_t min_reads, min_allele_reads, B;
    int32_t min_hp_cov, qual_thr, many_snvs;
    double w_few, w_many;
};

// k_phase_group's workspace of one locus: the masks of its reads, and the matrix when it does not fit LDS
__host__ __device__ inline size_t phase_ws_bytes(int n, int n_snvs, int n_alleles, int min_reads) {
    if (n < min_reads || n_snvs < 1 || n_alleles != 2) return 0;
    size_t b = 8 * (size_t)n;
    if (n > kPhaseLdsReads) b += 8 * (size_t)n * (size_t)n;
    return (b + 255) & ~(size_t)255;
}

// dynamic LDS of k_phase_group for a piece whose largest locus has max_n reads
__host__ __device__ inline size_t phase_lds_matrix_bytes(int max_n) {
    const size_t m = (size_t)(max_n < kPhaseLdsReads ? max_n : kPhaseLdsReads);
    return (8 * m * m + 15) & ~(size_t)15;
}
constexpr size_t kPhaseLdsFixed = 64 + 5 * 2 * (size_t)kPhaseMaxReads + kPhaseMaxReads;   // scalars, five int16 arrays, one byte array
inline size_t phase_lds_bytes(int max_n) { return phase_lds_matrix_bytes(max_n) + kPhaseLdsFixed; }

// what one wave has written to LDS or to its workspace is seen by its other lanes behind this
__device__ inline void phase_wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// Average linkage cut at two clusters by scipy's nearest-neighbour chain (rule C), run by one wave on the m x m matrix D.
// size, chain, mx, my: m entries each; lab[i] receives 0 for the cluster of point 0 and 1 for the other.
__device__ inline void phase_chain(double* D, int m, int16_t* size, int16_t* chain, int16_t* mx, int16_t* my, uint8_t* lab, int lane) {
    for (int i = lane; i < m; i += 64) size[i] = 1;
    phase_wave_sync();
    int len = 0, k_last = 0;
    double d_last = -INFINITY;
    for (int k = 0; k < m - 1; ++k) {
        if (len == 0) {   // the lowest-index live cluster
            int first = -1;
            for (int i0 = 0; i0 < m && first < 0; i0 += 64) {
                const int i = i0 + lane;
                const unsigned long long live = __ballot(i < m && size[i] > 0);
                if (live) first = i0 + __builtin_ctzll(live);
            }
            chain[0] = (int16_t)first;
            len = 1;
            phase_wave_sync();
        }
        int x, y;
        double cur;
        for (;;) {
            x = chain[len - 1];
            const int prev = len > 1 ? chain[len - 2] : -1;
            const double* row = D + (size_t)x * m;
            double best = INFINITY;
            int bi = INT32_MAX;
            for (int i = lane; i < m; i += 64) {
                if (i == x || size[i] == 0) continue;
                const double v = row[i];
                if (v < best) { best = v; bi = i; }
            }
            for (int o = 32; o > 0; o >>= 1) {
                const double ov = __shfl_xor(best, o);
                const int oi = __shfl_xor(bi, o);
                if (ov < best || (ov == best && oi < bi)) { best = ov; bi = oi; }
            }
            cur = best;
            y = bi;
            if (prev >= 0 && row[prev] == cur) y = prev;   // the previous chain element wins ties
            if (prev >= 0 && y == prev) break;
            if (len >= m) { y = prev; break; }   // the chain holds every cluster: cannot be (a chain never revisits one), kept as the array's bound
            chain[len] = (int16_t)y;
            ++len;
            phase_wave_sync();
        }
        len -= 2;
        if (x > y) { const int t = x; x = y; y = t; }
        const int nx = size[x], ny = size[y];
        mx[k] = (int16_t)x;
        my[k] = (int16_t)y;
        if (cur >= d_last) { d_last = cur; k_last = k; }   // the merge that a stable sort by distance puts last
        const double fx = (double)nx, fy = (double)ny, ft = (double)(nx + ny);
        for (int i = lane; i < m; i += 64) {
            if (i == x || i == y || size[i] == 0) continue;
            const double nd = (fx * D[(size_t)i * m + x] + fy * D[(size_t)i * m + y]) / ft;
            D[(size_t)i * m + y] = nd;
            D[(size_t)y * m + i] = nd;
        }
        phase_wave_sync();
        size[x] = 0;
        size[y] = (int16_t)(nx + ny);
        phase_wave_sync();
    }
    // every merge but the last-sorted one, as unions over the points (chain is free now: the parents)
    int16_t* parent = chain;
    for (int i = lane; i < m; i += 64) parent[i] = (int16_t)i;
    phase_wave_sync();
    if (lane == 0) {
        auto find = [&](int a) {
            while (parent[a] != a) {
                parent[a] = parent[parent[a]];
                a = parent[a];
            }
            return a;
        };
        for (int k = 0; k < m - 1; ++k) {
            if (k == k_last) continue;
            const int a = find(mx[k]), b = find(my[k]);
            parent[a] = (int16_t)b;
        }
        const int root0 = find(0);
        for (int i = 0; i < m; ++i) lab[i] = find(i) == root0 ? 0 : 1;
    }
    phase_wave_sync();
}

__global__ void __launch_bounds__(kPhaseThreads) k_phase_group(PhaseArgs a, int lds_matrix_bytes) {
    const int l = blockIdx.x;
    if (l >= a.n_loci) return;
    const int tid = threadIdx.x, nt = blockDim.x;
    const int r0 = a.read_off[l], n = a.read_off[l + 1] - r0;
    const int n_alleles = a.n_alleles[l];
    const int S = a.snv_off ? a.snv_off[l + 1] - a.snv_off[l] : 0;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    double* lds_D = reinterpret_cast<double*>(smem);
    int32_t* sc = reinterpret_cast<int32_t*>(smem + lds_matrix_bytes);   // 16 scalars
    int16_t* s_idx = reinterpret_cast<int16_t*>(smem + lds_matrix_bytes + 64);
    int16_t* s_size = s_idx + kPhaseMaxReads;
    int16_t* s_chain = s_size + kPhaseMaxReads;
    int16_t* s_mx = s_chain + kPhaseMaxReads;
    int16_t* s_my = s_mx + kPhaseMaxReads;
    uint8_t* s_lab = reinterpret_cast<uint8_t*>(s_my + kPhaseMaxReads);
    enum { cTagged = 0, cHpMin, cHpMax, cHpOther, cTopKey, cMany, cOne, cDone, cReason, cM, cPure };
    int32_t* perm = a.perm + r0;
    int32_t* meta = a.meta + (size_t)l * kPhaseMeta;

    if (tid < 2) {
        a.gseed[2 * l + tid] = mix64(a.seed[l] + kGolden * (uint64_t)(tid + 1));
        a.gone[2 * l + tid] = 1;
    }
    if (n < a.min_reads) {
        if (tid == 0) {
            a.gsz[2 * l] = a.gsz[2 * l + 1] = 0;
            meta[0] = kAssignNone;
            meta[1] = kReasonNone;
            meta[2] = -1;
            meta[3] = kStatusTooFew;
        }
        return;
    }
    if (tid == 0) {
        sc[cTagged] = 0;
        sc[cHpMin] = INT32_MAX;
        sc[cHpMax] = -1;
        sc[cHpOther] = 0;
        sc[cTopKey] = -1;
        sc[cMany] = sc[cOne] = 0;
        sc[cDone] = 0;
        sc[cReason] = kReasonNoTags;
        sc[cM] = 0;
        sc[cPure] = 0;
    }
    __syncthreads();

    // B. haplotags
    if (a.hp) {
        const int32_t* hp = a.hp + r0;
        const int32_t* ps = a.ps + r0;
        for (int r = tid; r < n; r += nt) {
            if (hp[r] < 0 || ps[r] < 0) continue;
            atomicAdd(&sc[cTagged], 1);
            atomicMin(&sc[cHpMin], hp[r]);
            atomicMax(&sc[cHpMax], hp[r]);
            // the phase set of r among the tagged reads: its count, and whether r is the first read that carries it
            int c = 0, first = 1;
            for (int q = 0; q < n; ++q) {
                if (hp[q] < 0 || ps[q] != ps[r]) continue;
                ++c;
                if (q < r) first = 0;
            }
            if (first) atomicMax(&sc[cTopKey], (c << 10) | (kPhaseMaxReads - 1 - r));   // most reads, then met first
        }
        __syncthreads();
        for (int r = tid; r < n; r += nt)
            if (hp[r] >= 0 && ps[r] >= 0 && hp[r] != sc[cHpMin] && hp[r] != sc[cHpMax]) atomicOr(&sc[cHpOther], 1);
        __syncthreads();
        if (tid == 0) {
            int reason = kReasonTagThresholds;
            const int tagged = sc[cTagged];
            if (tagged > 0) {
                const int key = sc[cTopKey];
                const int top_cnt = key >> 10, top = ps[kPhaseMaxReads - 1 - (key & (kPhaseMaxReads - 1))];
                const int distinct = sc[cHpOther] ? 3 : (sc[cHpMin] == sc[cHpMax] ? 1 : 2);
                if (tagged >= a.min_hp_cov && distinct == n_alleles && top_cnt >= a.min_hp_cov) {
                    int pos = 0, ok = 1;
                    for (int g = 0; g < 2; ++g) {
                        const int h = g == 0 ? sc[cHpMin] : sc[cHpMax];
                        int cnt = 0;
                        if (g < n_alleles)
                            for (int r = 0; r < n; ++r)
                                if (hp[r] == h && ps[r] == top) { perm[pos++] = r; ++cnt; }
                        a.gsz[2 * l + g] = cnt;
                        if (g < n_alleles && cnt < a.min_allele_reads) ok = 0;
                    }
                    if (ok) {
                        meta[0] = kAssignHp;
                        meta[1] = kReasonNone;
                        meta[2] = top;
                        meta[3] = kStatusCalled;
                        sc[cDone] = 1;
                    } else {
                        reason = kReasonGroupNotCalled;
                    }
                }
            }
            sc[cReason] = reason;
        }
        __syncthreads();
    }

    // C. SNVs
    if (!sc[cDone] && n_alleles == 2 && S >= 1) {
        const uint8_t* base = a.snv_base + a.cell_off[l];
        const uint8_t* qual = a.snv_qual + a.cell_off[l];
        char* wsl = a.ws + a.ws_off[l];
        unsigned long long* mask = reinterpret_cast<unsigned long long*>(wsl);
        for (int r = tid; r < n; r += nt) {
            unsigned long long mk = 0;
            int real = 0;
            for (int s = 0; s < S; ++s) {
                const uint8_t b = base[(size_t)r * S + s];
                const bool hq = qual[(size_t)r * S + s] >= a.qual_thr;
                if (b != kSnvOutOfRange && (b == kSnvGap || hq)) mk |= 1ull << s;
                if (b != kSnvOutOfRange && b != kSnvGap && hq) ++real;
            }
            mask[r] = mk;
            s_lab[r] = (uint8_t)(real > 2 ? 2 : real);
            if (real >= 2) atomicAdd(&sc[cMany], 1);
            if (real >= 1) atomicAdd(&sc[cOne], 1);
        }
        __syncthreads();
        if (tid == 0) {
            const int n_many = sc[cMany], n_one = sc[cOne], n_none = n - n_one;
            const bool pure = n_many + n_none == n;
            const bool go = (pure && (double)n_many >= fmin((double)n * 0.68, 16.0)) || (double)n_one >= fmin((double)n * 0.8, 16.0);
            sc[cPure] = pure;
            if (go && n_one >= 2) {
                int m = 0;
                for (int r = 0; r < n; ++r)
                    if (s_lab[r] >= 1) s_idx[m++] = (int16_t)r;
                sc[cM] = m;
            } else {
                sc[cReason] = kReasonFewSnvReads;
            }
        }
        __syncthreads();
        const int m = sc[cM];
        if (m >= 2) {
            const bool pure = sc[cPure] != 0;
            double* D = m <= kPhaseLdsReads ? lds_D : reinterpret_cast<double*>(wsl + 8 * (size_t)n);
            const int32_t* cn = a.cn + r0;
            for (int e = tid; e < m * m; e += nt) {
                const int i = e / m, j = e - i * m;
                const int ri = s_idx[i], rj = s_idx[j];
                unsigned long long both = mask[ri] & mask[rj];
                const int n_comparable = __popcll(both);
                const uint8_t *bi = base + (size_t)ri * S, *bj = base + (size_t)rj * S;
                int diff = 0;
                while (both) {
                    const int s = __builtin_ctzll(both);
                    both &= both - 1;
                    diff += bi[s] != bj[s];
                }
                double d = (double)diff;
                if (!pure) {
                    const int dc = cn[ri] > cn[rj] ? cn[ri] - cn[rj] : cn[rj] - cn[ri];
                    d = d + (double)dc * (n_comparable >= a.many_snvs ? a.w_many : a.w_few);
                }
                D[e] = i == j ? 0.0 : d;
            }
            __syncthreads();
            if (tid < 64) phase_chain(D, m, s_size, s_chain, s_mx, s_my, s_lab, tid);
            __syncthreads();
            if (tid == 0) {
                int pos = 0, ok = 1;
                for (int g = 0; g < 2; ++g) {
                    int cnt = 0;
                    for (int i = 0; i < m; ++i)
                        if (s_lab[i] == g) { perm[pos++] = s_idx[i]; ++cnt; }
                    a.gsz[2 * l + g] = cnt;
                    if (cnt < a.min_allele_reads) ok = 0;
                }
                if (ok) {
                    meta[0] = pure ? kAssignSnv : kAssignSnvDist;
                    meta[1] = kReasonNone;
                    meta[2] = -1;
                    meta[3] = kStatusCalled;
                    sc[cDone] = 1;
                } else {
                    sc[cReason] = kReasonGroupNotCalled;
                }
            }
            __syncthreads();
        }
    }
    if (tid == 0 && !sc[cDone]) {
        a.gsz[2 * l] = a.gsz[2 * l + 1] = 0;
        meta[0] = kAssignNone;
        meta[1] = sc[cReason];
        meta[2] = -1;
        meta[3] = kStatusNotPhased;
    }
}

// The reads of the groups, one group behind the other: goff, gws_off, gcn, gw.
__global__ void __launch_bounds__(256) k_phase_pack(PhaseArgs a) {
    const int tid = threadIdx.x;
    const int l_begin = blockIdx.x * kPhasePackLoci;
    const int l_end = min(l_begin + kPhasePackLoci, a.n_loci);
    const int g_begin = 2 * l_begin, ng = 2 * (l_end - l_begin);
    __shared__ int s_part[256];
    __shared__ int s_off[257];
    __shared__ double s_sum[256];
    // the reads of every group in front of this block
    int part = 0;
    for (int g = tid; g < g_begin; g += 256) part += a.gsz[g];
    s_part[tid] = part;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (tid < o) s_part[tid] += s_part[tid + o];
        __syncthreads();
    }
    if (tid == 0) {
        int run = s_part[0];
        for (int g = 0; g < ng; ++g) {
            s_off[g] = run;
            run += a.gsz[g_begin + g];
        }
        s_off[ng] = run;
    }
    __syncthreads();
    if (tid < ng) {
        const int g = g_begin + tid, l = g >> 1;
        const int r0 = a.read_off[l];
        const int sz = a.gsz[g], p0 = (g & 1) ? a.gsz[g - 1] : 0;
        a.goff[g] = s_off[tid];
        if (g == 2 * a.n_loci - 1) a.goff[g + 1] = s_off[tid + 1];
        a.gws_off[g] = a.aws_base[l] + ((g & 1) ? (int64_t)allele_ws_layout(nullptr, a.gsz[g - 1], a.B, 2, nullptr) : 0);
        double s = 0.0;   // the group's weights, summed in group order
        for (int j = 0; j < sz; ++j) s = s + a.w[r0 + a.perm[r0 + p0 + j]];
        s_sum[tid] = s;
    }
    __syncthreads();
    const int rb = a.read_off[l_begin], re = a.read_off[l_end];
    for (int p = rb + tid; p < re; p += 256) {
        int lo = l_begin, hi = l_end - 1;   // the locus whose slot holds p
        while (lo < hi) {
            const int mid = (lo + hi + 1) >> 1;
            if (a.read_off[mid] <= p) lo = mid; else hi = mid - 1;
        }
        const int r0 = a.read_off[lo], j = p - r0;
        const int n0 = a.gsz[2 * lo], n1 = a.gsz[2 * lo + 1];
        if (j >= n0 + n1) continue;
        const int gl = 2 * (lo - l_begin) + (j < n0 ? 0 : 1);
        const int dst = s_off[gl] + (j < n0 ? j : j - n0);
        const int src = r0 + a.perm[p];
        a.gcn[dst] = a.cn[src];
        a.gw[dst] = a.w[src] / s_sum[gl];
    }
}

// Step E for one SNV and one peak: the eligible cells of the peak's reads (in read order), their most common byte with ties to
// the byte met first, '-' passed over for the second most common.  Returns the total; *byte = -1 when only '-' occurs.
__device__ inline int phase_snv_pick(const uint8_t* base, const uint8_t* qual, int S, int s, const int32_t* reads, int k, int thr,
                                     int* byte, int* count) {
    int total = 0;
    int all_b = -1, all_c = 0, real_b = -1, real_c = 0;   // the best over all bytes; over all but '-'
    for (int i = 0; i < k; ++i) {
        const size_t ci = (size_t)reads[i] * S + s;
        const uint8_t b = base[ci];
        if (!(b == kSnvGap || qual[ci] >= thr)) continue;
        ++total;
        int c = 0, first = 1;
        for (int j = 0; j < k; ++j) {
            const size_t cj = (size_t)reads[j] * S + s;
            if (base[cj] != b || !(b == kSnvGap || qual[cj] >= thr)) continue;
            if (j < i) { first = 0; break; }
            ++c;
        }
        if (!first) continue;
        if (c > all_c) { all_c = c; all_b = b; }
        if (b != kSnvOutOfRange && c > real_c) { real_c = c; real_b = b; }
    }
    const bool second = all_b == kSnvOutOfRange;
    *byte = total ? (second ? real_b : all_b) : -1;
    *count = total ? (second ? real_c : all_c) : 0;
    return total;
}

__device__ inline int phase_snv_count(const uint8_t* base, const uint8_t* qual, int S, int s, const int32_t* reads, int k, int thr, int byte) {
    int c = 0;
    for (int i = 0; i < k; ++i) {
        const size_t ci = (size_t)reads[i] * S + s;
        c += (base[ci] == byte && (byte == kSnvGap || qual[ci] >= thr)) ? 1 : 0;
    }
    return c;
}

__global__ void __launch_bounds__(kPhaseFinishThreads) k_phase_finish(PhaseArgs a) {
    const int l = blockIdx.x;
    if (l >= a.n_loci) return;
    const int tid = threadIdx.x, nt = blockDim.x;
    const int r0 = a.read_off[l], n = a.read_off[l + 1] - r0;
    const int S = a.snv_off ? a.snv_off[l + 1] - a.snv_off[l] : 0;
    const int s0 = a.snv_off ? a.snv_off[l] : 0;
    const int32_t* meta = a.meta + (size_t)l * kPhaseMeta;
    int32_t* oi = a.out_i + (size_t)l * kPhaseOutI;
    double* od = a.out_d + (size_t)l * kAlleleOutD;
    int32_t* rp = a.read_peak + r0;
    const int32_t* perm = a.perm + r0;
    __shared__ int s_total[kPhaseMaxSnvs][2], s_byte[kPhaseMaxSnvs][2], s_count[kPhaseMaxSnvs][2], s_cross[kPhaseMaxSnvs][2];
    __shared__ int s_any;
    int method = meta[0], reason = meta[1], status = meta[3];
    const int n_groups = a.n_alleles[l];
    const int gs0 = a.gsz[2 * l], gs1 = a.gsz[2 * l + 1];
    const int32_t* gi0 = a.g_oi + (size_t)(2 * l) * kAlleleOutI;
    const double* gd0 = a.g_od + (size_t)(2 * l) * kAlleleOutD;
    bool swap = false;
    if (method == kAssignSnv || method == kAssignSnvDist) {
        // peaks by (mean, low end of the 95 % interval) ascending, group 0 first on a tie
        const double m0 = gd0[0], m1 = gd0[kAlleleOutD];
        const int lo0 = gi0[4], lo1 = gi0[kAlleleOutI + 4];
        swap = m1 < m0 || (m1 == m0 && lo1 < lo0);
        // E. SNV calls: thread (s, peak)
        if (tid == 0) s_any = 0;
        __syncthreads();
        const uint8_t* base = a.snv_base + a.cell_off[l];
        const uint8_t* qual = a.snv_qual + a.cell_off[l];
        const int s = tid >> 1, pk = tid & 1;
        const int ga = swap ? 1 - pk : pk, gb = 1 - ga;
        const int32_t* reads_a = perm + (ga ? gs0 : 0);
        const int32_t* reads_b = perm + (gb ? gs0 : 0);
        if (s < S) {
            int byte, count;
            s_total[s][pk] = phase_snv_pick(base, qual, S, s, reads_a, ga ? gs1 : gs0, a.qual_thr, &byte, &count);
            s_byte[s][pk] = byte;
            s_count[s][pk] = count;
            s_cross[s][pk] = byte >= 0 ? phase_snv_count(base, qual, S, s, reads_b, gb ? gs1 : gs0, a.qual_thr, byte) : 0;
        }
        __syncthreads();
        if (s < S && pk == 0) {
            int st = kSnvCalled;
            for (int p = 0; p < 2 && st == kSnvCalled; ++p) {
                const int q = 1 - p;
                if (s_total[s][p] == 0) st = kSnvZeroTotal;
                else if (s_byte[s][p] < 0) st = kSnvOnlyOutOfRange;
                else if (s_total[s][q] == 0) st = kSnvZeroTotal;
                else if ((double)s_cross[s][p] / (double)s_total[s][q] > (double)s_count[s][p] / (double)s_total[s][p] / 2.0) st = kSnvCrossTalk;
            }
            if (st == kSnvCalled && s_byte[s][0] == s_byte[s][1]) st = kSnvSameBase;
            a.snv_status[s0 + s] = st;
            for (int p = 0; p < 2; ++p) {
                a.snv_call[2 * (size_t)(s0 + s) + p] = st == kSnvCalled ? (uint8_t)s_byte[s][p] : 0;
                a.snv_rcs[2 * (size_t)(s0 + s) + p] = st == kSnvCalled ? s_count[s][p] : 0;
            }
            if (st == kSnvCalled) atomicOr(&s_any, 1);
        }
        __syncthreads();
        if (!s_any) {
            method = kAssignNone;
            reason = kReasonNoSnvCalled;
            status = kStatusNotPhased;
        }
    } else {
        for (int s = tid; s < S; s += nt) {
            a.snv_status[s0 + s] = kSnvNotEvaluated;
            a.snv_call[2 * (size_t)(s0 + s)] = a.snv_call[2 * (size_t)(s0 + s) + 1] = 0;
            a.snv_rcs[2 * (size_t)(s0 + s)] = a.snv_rcs[2 * (size_t)(s0 + s) + 1] = 0;
        }
    }
    // every read's peak: each read is written once
    if (method == kAssignNone) {
        for (int j = tid; j < n; j += nt) rp[j] = -1;
    } else {
        for (int j = tid; j < n; j += nt) rp[j] = -1;
        __syncthreads();
        for (int j = tid; j < gs0 + gs1; j += nt) {
            const int g = j < gs0 ? 0 : 1;
            rp[perm[j]] = swap ? 1 - g : g;
        }
    }
    if (tid != 0) return;
    oi[kAlleleOutI] = method;
    oi[kAlleleOutI + 1] = reason;
    oi[kAlleleOutI + 2] = method == kAssignHp ? meta[2] : -1;
    if (method == kAssignNone) {
        oi[0] = status;
        oi[1] = 0;
        for (int e = 2; e < 12; ++e) oi[e] = -1;
        oi[12] = oi[13] = 0;
        for (int e = 0; e < kAlleleOutD; ++e) od[e] = NAN;
        return;
    }
    oi[0] = kStatusCalled;
    oi[1] = n_groups;
    for (int pk = 0; pk < 2; ++pk) {
        const int g = swap ? 1 - pk : pk;
        const bool used = pk < n_groups;
        const int32_t* gi = gi0 + (size_t)g * kAlleleOutI;
        const double* gd = gd0 + (size_t)g * kAlleleOutD;
        oi[2 + pk] = used ? gi[2] : -1;
        for (int e = 0; e < 2; ++e) {
            oi[4 + 2 * pk + e] = used ? gi[4 + e] : -1;
            oi[8 + 2 * pk + e] = used ? gi[8 + e] : -1;
        }
        oi[12 + pk] = used ? (g ? gs1 : gs0) : 0;
        od[pk] = used ? gd[0] : NAN;
        od[2 + pk] = used ? 1.0 / (double)n_groups : NAN;
        od[4 + pk] = used ? gd[4] : NAN;
    }
}

}  // namespace strk
