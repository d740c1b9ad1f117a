// strk_poa.h — allele sequences by partial-order alignment on gfx950 (strk_consensus, kernel k_poa).
//
// The definition is DESIGN.md §12; the CPU restatement that the tests compare against is tests/poa_restatement.py.  A
// group's distinct strings are added one after another to a graph of nodes (a byte each) and weighted edges; a string is
// aligned to the graph globally with linear gaps (match +5, mismatch -4, gap -8); the consensus is the heaviest path.
//
// k_poa: one workgroup of four waves per group, the whole group from its bytes to its consensus.
//   1. every string's hash, then its first equal predecessor (hash and length first, then a wave-wide comparison): the
//      distinct strings with their multiplicities, as k_best_rep finds them.  One distinct string: `single`.
//   2. per distinct string s of length L, one row H[v][0..L] per node v in topological order, in the group's piece of the
//      global workspace.  Thread t owns column j = 256 q + t of chunk q.  The predecessor part of a cell,
//      c[j] = max_p max(H[p][j-1] + sub, H[p][j] - 8), is elementwise; the horizontal closure H[v][j] = max_k<=j c[k] - 8 (j - k)
//      is a prefix maximum of c[j] + 8 j: shuffles inside a wave, the waves' totals through LDS, the chunk's total to the
//      next chunk in a register.
//   3. the end node by a workgroup-wide maximum over the sinks, then thread 0 alone: trace-back (ties by node id), the
//      graph's update, a new topological order (depth-first over the in-edges).  At most nodes + L steps each.
//   4. thread 0: the heaviest path and the consensus bytes, into the group's slice of the sequence pool.
// A graph that would outgrow the node limit marks its group for the best-representative path (host side) and stops.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace strk {

constexpr int kPoaThreads = 256;            // the workgroup's column span
constexpr int kPoaWaves = kPoaThreads / 64;
constexpr int kPoaMaxGroup = 250;
constexpr int kPoaMaxLen = 4096;            // a longer string sends its group to best_rep
constexpr int kPoaMaxNodes = 16384;         // the largest node limit
constexpr int kPoaMatch = 5, kPoaMismatch = -4, kPoaGap = -8;
constexpr int kPoaNeg = -(1 << 29);
constexpr int kConsPoa = 3;
constexpr int kPoaNodeArrays = 10, kPoaEdgeArrays = 3;
// states of a group after k_poa
constexpr int kPoaDone = 0, kPoaOverflow = 1, kPoaBroken = 2;

struct PoaArgs {
    const int32_t* list;        // [n_list] the groups of this launch
    const int32_t* group_off;   // [n_groups + 1] into seq_start / seq_len
    const uint8_t* seqs;
    const int64_t* seq_start;
    const int32_t* seq_len;
    int32_t* ws;                // the launch's workspace
    const int64_t* ws_off;      // [n_list] first int of a group's piece
    const int32_t* node_cap;    // [n_list] nodes the piece has room for (the node limit, or fewer where the bytes cannot make more)
    const int32_t* edge_cap;    // [n_list]
    const int32_t* row_len;     // [n_list] the group's longest string + 1
    uint8_t* pool;              // consensus bytes of all groups
    const int64_t* pool_off;    // [n_list] a group's slice of the pool (node_cap bytes)
    int32_t* out_index;         // per group (indexed by the group's number)
    int32_t* out_method;
    int32_t* out_len;
    int32_t* out_state;
    unsigned long long* cells;  // DP cells of the launch
    int32_t n_list;
};

// (H + 2^30) << 32 | ~id: the largest H wins, then the smallest id
__device__ inline unsigned long long poa_key(int h, int id) {
    return ((unsigned long long)(unsigned)(h + (1 << 30)) << 32) | (unsigned)(0x7fffffff - id);
}

__global__ __launch_bounds__(kPoaThreads) void k_poa(PoaArgs a) {
    __shared__ uint32_t s_hash[kPoaMaxGroup];
    __shared__ int32_t s_rep[kPoaMaxGroup];
    __shared__ int32_t s_uniq[kPoaMaxGroup];
    __shared__ int32_t s_cnt[kPoaMaxGroup];
    __shared__ int32_t s_wmax[2][kPoaWaves];
    __shared__ unsigned long long s_best;
    __shared__ int32_t s_d, s_nn, s_ne, s_state;

    const int li = blockIdx.x;
    if (li >= a.n_list) return;
    const int g = a.list[li];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int q0 = a.group_off[g];
    const int m = a.group_off[g + 1] - q0;
    const int64_t* st = a.seq_start + q0;
    const int32_t* ln = a.seq_len + q0;
    if (m <= 0) {   // (the host sends no empty group; kept for safety)
        if (tid == 0) {
            a.out_index[g] = -1;
            a.out_method[g] = kConsNone;
            a.out_len[g] = 0;
            a.out_state[g] = kPoaDone;
        }
        return;
    }
    for (int i = tid; i < m; i += kPoaThreads) s_hash[i] = 0;
    __syncthreads();
    // 1. hashes, first equal predecessors, the distinct strings
    for (int i = wave; i < m; i += kPoaWaves) {
        const uint8_t* s = a.seqs + st[i];
        const int len = ln[i];
        uint32_t h = 0;
        for (int p = lane; p < len; p += 64) h += ((uint32_t)s[p] + 1u) * ((uint32_t)p * 2654435761u + 0x9E3779B9u);
        if (len > 0) atomicAdd(&s_hash[i], h);
    }
    __syncthreads();
    for (int i = wave; i < m; i += kPoaWaves) {
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
                s_rep[i] = -1 - d;
                ++d;
            } else {
                s_cnt[-1 - s_rep[r]] += 1;
            }
        }
        s_d = d;
        s_nn = 0;
        s_ne = 0;
        s_state = kPoaDone;
    }
    __syncthreads();
    const int d = s_d;
    if (d == 1) {
        if (tid == 0) {
            a.out_index[g] = 0;
            a.out_method[g] = kConsSingle;
            a.out_len[g] = ln[0];
            a.out_state[g] = kPoaDone;
        }
        return;
    }
    // the group's piece of the workspace
    const int ncap = a.node_cap[li], ecap = a.edge_cap[li], rl = a.row_len[li];
    int32_t* base = a.ws + a.ws_off[li];
    int32_t* n_byte = base;
    int32_t* n_st = n_byte + ncap;
    int32_t* n_en = n_st + ncap;
    int32_t* n_head = n_en + ncap;      // first in-edge, -1: none
    int32_t* n_ring = n_head + ncap;    // the next node of the column (a ring; itself when alone)
    int32_t* n_out = n_ring + ncap;     // out-degree
    int32_t* topo = n_out + ncap;
    int32_t* t_a = topo + ncap;         // scratch of thread 0: visited | score
    int32_t* t_b = t_a + ncap;          // stack nodes | back
    int32_t* t_c = t_b + ncap;          // stack edges
    int32_t* e_src = t_c + ncap;
    int32_t* e_w = e_src + ecap;
    int32_t* e_next = e_w + ecap;
    int32_t* match = e_next + ecap;     // [rl] node matched to byte j (1-based), -1: inserted
    int32_t* H = match + rl;            // [ncap][rl]

    int n_empty = 0;   // (thread 0's copy is the one used)
    unsigned long long cells = 0;
    for (int k = 0; k < d; ++k) {
        const int i = s_uniq[k];
        const uint8_t* s = a.seqs + st[i];
        const int L = ln[i];
        const int c = s_cnt[k];
        if (L == 0) {
            n_empty += c;
            continue;
        }
        int nn = s_nn;
        __syncthreads();   // (thread 0 writes s_nn below)
        if (nn == 0) {   // the first non-empty string: a chain
            if (L > ncap) {
                if (tid == 0) s_state = kPoaOverflow;
                __syncthreads();
                break;
            }
            for (int v = tid; v < L; v += kPoaThreads) {
                n_byte[v] = s[v];
                n_st[v] = v == 0 ? c : 0;
                n_en[v] = v == L - 1 ? c : 0;
                n_head[v] = v - 1;            // edge v - 1 is (v - 1 -> v)
                n_ring[v] = v;
                n_out[v] = v < L - 1;
                topo[v] = v;
                if (v > 0) {
                    e_src[v - 1] = v - 1;
                    e_w[v - 1] = c;
                    e_next[v - 1] = -1;
                }
            }
            if (tid == 0) {
                s_nn = L;
                s_ne = L - 1;
            }
            __syncthreads();
            continue;
        }
        // 2. the rows
        if (tid == 0) s_best = 0;
        int par = 0;
        for (int r = 0; r < nn; ++r) {
            const int v = topo[r];
            const int vb = n_byte[v];
            const int e0 = n_head[v];
            int32_t* Hv = H + (int64_t)v * rl;
            int carry = kPoaNeg;
            for (int j0 = 0; j0 <= L; j0 += kPoaThreads) {
                const int j = j0 + tid;
                const bool valid = j <= L;
                int x = kPoaNeg;
                if (valid) {
                    const int sub = j >= 1 ? (s[j - 1] == vb ? kPoaMatch : kPoaMismatch) : 0;
                    int cand;
                    if (e0 < 0) {   // row 0 is the only predecessor
                        cand = kPoaGap * j + kPoaGap;
                        if (j >= 1) cand = max(cand, kPoaGap * (j - 1) + sub);
                    } else {
                        cand = kPoaNeg;
                        for (int e = e0; e >= 0; e = e_next[e]) {
                            const int32_t* Hp = H + (int64_t)e_src[e] * rl;
                            cand = max(cand, Hp[j] + kPoaGap);
                            if (j >= 1) cand = max(cand, Hp[j - 1] + sub);
                        }
                    }
                    x = cand - kPoaGap * j;
                }
#pragma unroll
                for (int o = 1; o < 64; o <<= 1) {
                    const int y = __shfl_up(x, o);
                    if (lane >= o) x = max(x, y);
                }
                if (lane == 63) s_wmax[par][wave] = x;
                __syncthreads();
                int pre = carry;
#pragma unroll
                for (int w = 0; w < kPoaWaves; ++w) {
                    const int t = s_wmax[par][w];
                    if (w < wave) pre = max(pre, t);
                    carry = max(carry, t);
                }
                x = max(x, pre);
                if (valid) Hv[j] = x + kPoaGap * j;
                if (j == L && n_out[v] == 0) atomicMax(&s_best, poa_key(x + kPoaGap * j, v));
                par ^= 1;
            }
            __syncthreads();   // the row is complete before a successor reads it
        }
        cells += (unsigned long long)nn * (unsigned long long)L;
        // 3. thread 0: trace-back, update, topological order
        if (tid == 0) {
            int v = 0x7fffffff - (int)(unsigned)(s_best & 0xffffffffu);
            int j = L;
            int steps = nn + L + 2;
            bool broken = s_best == 0;   // (no sink: cannot happen in an acyclic graph)
            while (!broken && (v >= 0 || j > 0)) {
                if (--steps < 0) {
                    broken = true;
                    break;
                }
                if (v < 0) {
                    match[j] = -1;
                    --j;
                    continue;
                }
                const int32_t* Hv = H + (int64_t)v * rl;
                const int h = Hv[j];
                const int e0 = n_head[v];
                int p_found = 0x7fffffff;
                if (j > 0) {
                    const int sub = s[j - 1] == n_byte[v] ? kPoaMatch : kPoaMismatch;
                    if (e0 < 0) {
                        if (kPoaGap * (j - 1) + sub == h) p_found = -1;
                    } else {
                        for (int e = e0; e >= 0; e = e_next[e]) {
                            const int p = e_src[e];
                            if (p < p_found && H[(int64_t)p * rl + j - 1] + sub == h) p_found = p;
                        }
                    }
                    if (p_found != 0x7fffffff) {
                        match[j] = v;
                        v = p_found;
                        --j;
                        continue;
                    }
                }
                if (e0 < 0) {
                    if (kPoaGap * j + kPoaGap == h) p_found = -1;
                } else {
                    for (int e = e0; e >= 0; e = e_next[e]) {
                        const int p = e_src[e];
                        if (p < p_found && H[(int64_t)p * rl + j] + kPoaGap == h) p_found = p;
                    }
                }
                if (p_found != 0x7fffffff) {
                    v = p_found;
                    continue;
                }
                if (j == 0) {
                    broken = true;
                    break;
                }
                match[j] = -1;
                --j;
            }
            int ne = s_ne;
            bool over = false;
            if (!broken) {
                int prev = -1;
                for (int q = 1; q <= L; ++q) {
                    const int b = s[q - 1];
                    const int mv = match[q];
                    int cur = -1;
                    if (mv >= 0) {
                        if (n_byte[mv] == b) cur = mv;
                        else
                            for (int t = n_ring[mv]; t != mv; t = n_ring[t])
                                if (n_byte[t] == b) {
                                    cur = t;
                                    break;
                                }
                    }
                    if (cur < 0) {
                        if (nn >= ncap) {
                            over = true;
                            break;
                        }
                        cur = nn++;
                        n_byte[cur] = b;
                        n_st[cur] = 0;
                        n_en[cur] = 0;
                        n_head[cur] = -1;
                        n_out[cur] = 0;
                        if (mv >= 0) {
                            n_ring[cur] = n_ring[mv];
                            n_ring[mv] = cur;
                        } else {
                            n_ring[cur] = cur;
                        }
                    }
                    if (prev >= 0) {
                        int e = n_head[cur];
                        while (e >= 0 && e_src[e] != prev) e = e_next[e];
                        if (e >= 0) {
                            e_w[e] += c;
                        } else {
                            if (ne >= ecap) {   // (cannot happen: a byte adds at most one edge)
                                broken = true;
                                break;
                            }
                            e = ne++;
                            e_src[e] = prev;
                            e_w[e] = c;
                            e_next[e] = n_head[cur];
                            n_head[cur] = e;
                            n_out[prev] += 1;
                        }
                    } else {
                        n_st[cur] += c;
                    }
                    prev = cur;
                }
                if (!over && !broken) n_en[prev] += c;
            }
            if (broken) s_state = kPoaBroken;
            else if (over) s_state = kPoaOverflow;
            else {
                // depth-first over the in-edges: a node follows all its predecessors
                for (int u = 0; u < nn; ++u) t_a[u] = 0;
                int n_done = 0;
                for (int root = 0; root < nn; ++root) {
                    if (t_a[root]) continue;
                    int sp = 0;
                    t_b[0] = root;
                    t_c[0] = n_head[root];
                    t_a[root] = 1;
                    while (sp >= 0) {
                        const int e = t_c[sp];
                        if (e < 0) {
                            topo[n_done++] = t_b[sp];
                            --sp;
                            continue;
                        }
                        t_c[sp] = e_next[e];
                        const int p = e_src[e];
                        if (!t_a[p]) {
                            t_a[p] = 1;
                            ++sp;
                            t_b[sp] = p;
                            t_c[sp] = n_head[p];
                        }
                    }
                }
                s_nn = nn;
                s_ne = ne;
            }
        }
        __syncthreads();
        if (s_state != kPoaDone) break;
    }
    // 4. the heaviest path
    if (tid == 0) {
        if (cells) atomicAdd(a.cells, cells);
        const int state = s_state;
        a.out_state[g] = state;
        if (state == kPoaDone) {
            const int nn = s_nn;
            int32_t* score = t_a;
            int32_t* back = t_b;
            for (int r = 0; r < nn; ++r) {
                const int v = topo[r];
                int bw = -1, bs = 0, bp = 0;
                if (n_st[v] > 0) {
                    bw = n_st[v];
                    bs = 0;
                    bp = -1;
                }
                for (int e = n_head[v]; e >= 0; e = e_next[e]) {
                    const int w = e_w[e], p = e_src[e], sc = score[p];
                    if (w > bw || (w == bw && (sc > bs || (sc == bs && p < bp)))) {
                        bw = w;
                        bs = sc;
                        bp = p;
                    }
                }
                score[v] = bw + bs;
                back[v] = bp;
            }
            int bw = -1, bs = 0, bv = -1;
            if (n_empty > 0) {
                bw = n_empty;
                bs = 0;
                bv = -1;
            }
            for (int v = 0; v < nn; ++v) {
                const int w = n_en[v];
                if (w <= 0) continue;
                const int sc = score[v];
                if (w > bw || (w == bw && sc > bs)) {   // (ascending v: an equal candidate never replaces an earlier one)
                    bw = w;
                    bs = sc;
                    bv = v;
                }
            }
            int len = 0;
            for (int v = bv; v >= 0; v = back[v]) ++len;
            uint8_t* out = a.pool + a.pool_off[li];
            int q = len;
            for (int v = bv; v >= 0; v = back[v]) out[--q] = (uint8_t)n_byte[v];
            a.out_index[g] = -1;
            a.out_method[g] = kConsPoa;
            a.out_len[g] = len;
        }
    }
}

// The sequence bytes of every group into one buffer: group g's out_len[g] bytes at out_off[g], from its string
// `index` (single / best_rep) or from its slice of the pool (poa).
struct PoaGatherArgs {
    const int32_t* group_off;
    const uint8_t* seqs;
    const int64_t* seq_start;
    const int32_t* index;
    const int32_t* method;
    const int64_t* out_off;     // [n_groups + 1]
    const uint8_t* pool;
    const int64_t* pool_of;     // [n_groups] a group's slice of the pool (-1: none)
    uint8_t* out;
    int32_t n_groups;
};

__global__ __launch_bounds__(256) void k_poa_gather(PoaGatherArgs a) {
    const int g = blockIdx.x;
    if (g >= a.n_groups) return;
    const int64_t o0 = a.out_off[g];
    const int64_t n = a.out_off[g + 1] - o0;
    if (n <= 0) return;
    const int meth = a.method[g];
    const uint8_t* src;
    if (meth == kConsPoa) src = a.pool + a.pool_of[g];
    else src = a.seqs + a.seq_start[a.group_off[g] + a.index[g]];
    for (int64_t p = threadIdx.x; p < n; p += blockDim.x) a.out[o0 + p] = src[p];
}

}  // namespace strk
