// strk_kmers.h — the distinct windows of every group of sequences, counted, on gfx950 (strk_count_kmers).
//
// Stands where the reference counts motif-sized k-mers per read (strkit/call/call_locus.py:1287) and per peak (:1526-1593,
// :1635).  The definition (the CPU restatement that the tests compare against is tests/kmers_restatement.py):
// a group's windows are the s[i : i + k] of all its strings; one entry per distinct window with its count and the place of its
// first occurrence (smallest string index, then smallest i), entries in ascending unsigned byte order.  Raw bytes, exact.
//
// Both kernels start with the set of byte values of the group (as k_best_rep does): a value's code is its rank in the set,
// b = the bits of the largest code (at least 1), so that code order is byte order.  With k * b <= 64 a window is ONE 64-bit key
// (first byte in the highest bits: key order is lexicographic order), rolled from window to window.
//
// k_kmers_hash<T>: one workgroup of four waves per group, a table of T slots in LDS (key | count | first place).  A slot is
//   claimed by a 64-bit compare-and-swap on the key; the count grows by an LDS atomic add, the first place (string index << 16
//   | i) shrinks by an LDS atomic min, so neither depends on the order in which the lanes arrive.  The key of all ones is the
//   empty mark, a window that packs to it is counted in a slot of its own.  More than 3T/4 distinct keys: the group is marked
//   kKmerSpilled and left to k_kmers_sort; k * b > 64: kKmerGeneral, likewise.  The host calls it twice: to count the entries
//   of every group and, with the prefix sums, to write them (rank of an entry = the number of smaller keys in the table).
// k_kmers_sort: one workgroup of sixteen waves per group, for the groups the table could not take.  Every window becomes an
//   element (key, place) of the group's piece of a global workspace, padded to a power of two; a bitonic sort orders them by
//   (key, place) — on the general path by (the k bytes, place), compared byte by byte: slow, and exact —; the first element of
//   every run is an entry, its place the first occurrence, the run's length the count.  The first call counts the runs and
//   leaves every run's start in the workspace, the second (kKmerWrite, once the host knows where the group's entries go) writes.
// No result depends on launch geometry: keys and places are unique, sums and minima commute.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace strk {

constexpr int kKmerMaxGroup = 250;
constexpr int kKmerMaxLen = 65535;
constexpr int kKmerHashThreads = 256;
constexpr int kKmerSortThreads = 1024;
constexpr int kKmerSmallSlots = 512;     // groups of at most 3/4 of this many windows: the table cannot fill up
constexpr int kKmerLargeSlots = 2048;
constexpr int kKmerRun = 8;              // consecutive windows a lane rolls through
constexpr int kKmerHashed = 0, kKmerSpilled = 1, kKmerGeneral = 2;   // KmerArgs::state
constexpr int kKmerCount = 0, kKmerWrite = 1;                        // KmerArgs::mode (k_kmers_sort: sort + count | emit)
constexpr uint64_t kKmerEmpty = ~0ull;
constexpr uint32_t kKmerPad = 0xFFFFFFFFu;   // place of a padding element (a real one is below 250 << 16)

struct KmerElem {
    uint64_t key;
    uint32_t place;   // string index << 16 | i
    uint32_t run;     // element r: where run r starts (written after the sort)
};

struct KmerArgs {
    const int32_t* group_off;   // [n_groups + 1] into seq_start / seq_len
    const uint8_t* seqs;
    const int64_t* seq_start;
    const int32_t* seq_len;
    const int32_t* k;           // [n_groups]
    const int32_t* list;        // [n_list] the groups of this launch, one workgroup each
    int32_t* cnt;               // [n_groups] entries of the group (-1 until k_kmers_sort has counted a group left to it)
    int32_t* state;             // [n_groups] kKmerHashed / kKmerSpilled / kKmerGeneral
    const int64_t* entry_off;   // [n_groups] first entry of the group (kKmerWrite)
    int64_t* out_pos;
    int32_t* out_count;
    KmerElem* ws;               // k_kmers_sort: the workspace ...
    const int64_t* ws_off;      // ... and [n_list] the first element of every listed group's piece
    int32_t n_list;
    int32_t mode;
};

// Code map of the group's byte values into s_map; returns the bits per code.  All NT threads of the workgroup call it.
template <int NT>
__device__ inline int kmer_code_bits(const uint8_t* __restrict__ seqs, const int64_t* st, const int32_t* ln, int m,
                                     uint32_t* s_pres, uint8_t* s_map, int* s_bits, int tid) {
    if (tid < 8) s_pres[tid] = 0;
    __syncthreads();
    for (int i = 0; i < m; ++i) {
        const uint8_t* s = seqs + st[i];
        const int len = ln[i];
        for (int p = tid; p < len; p += NT) {
            const uint32_t b = s[p];
            if (!((s_pres[b >> 5] >> (b & 31)) & 1u)) atomicOr(&s_pres[b >> 5], 1u << (b & 31));
        }
    }
    __syncthreads();
    if (tid == 0) {
        int sigma = 0;
        for (int b = 0; b < 256; ++b) {
            const bool on = (s_pres[b >> 5] >> (b & 31)) & 1u;
            s_map[b] = on ? (uint8_t)sigma : 0;
            sigma += on;
        }
        int bits = 1;
        while ((1 << bits) < sigma) ++bits;
        *s_bits = bits;
    }
    __syncthreads();
    return *s_bits;
}

template <int T>
__global__ __launch_bounds__(kKmerHashThreads) void k_kmers_hash(KmerArgs a) {
    __shared__ uint64_t s_key[T];
    __shared__ uint32_t s_cnt[T];
    __shared__ uint32_t s_first[T];
    __shared__ uint16_t s_idx[T];
    __shared__ uint32_t s_pres[8];
    __shared__ uint8_t s_map[256];
    __shared__ int s_bits, s_d, s_over, s_n;
    __shared__ uint32_t s_ones_cnt, s_ones_first;
    constexpr int NT = kKmerHashThreads;
    constexpr int kCap = T - T / 4;

    if ((int)blockIdx.x >= a.n_list) return;
    const int g = a.list[blockIdx.x];
    const int tid = threadIdx.x;
    if (a.mode == kKmerWrite && (a.state[g] != kKmerHashed || a.cnt[g] <= 0)) return;
    const int q0 = a.group_off[g];
    const int m = a.group_off[g + 1] - q0;
    const int k = a.k[g];
    const int64_t* st = a.seq_start + q0;
    const int32_t* ln = a.seq_len + q0;
    const int bits = kmer_code_bits<NT>(a.seqs, st, ln, m, s_pres, s_map, &s_bits, tid);
    const int64_t kb = (int64_t)k * bits;
    if (kb > 64) {
        if (tid == 0) {
            a.cnt[g] = -1;
            a.state[g] = kKmerGeneral;
        }
        return;
    }
    for (int s = tid; s < T; s += NT) {
        s_key[s] = kKmerEmpty;
        s_cnt[s] = 0;
        s_first[s] = kKmerPad;
    }
    if (tid == 0) {
        s_d = 0;
        s_over = 0;
        s_n = 0;
        s_ones_cnt = 0;
        s_ones_first = kKmerPad;
    }
    __syncthreads();
    const uint64_t mask = kb == 64 ? ~0ull : (1ull << kb) - 1;
    for (int si = 0; si < m; ++si) {
        const int nw = ln[si] - k + 1;
        if (nw <= 0) continue;
        const uint8_t* s = a.seqs + st[si];
        for (int i0 = tid * kKmerRun; i0 < nw; i0 += NT * kKmerRun) {
            if (*(volatile int*)&s_over) break;
            uint64_t key = 0;
            for (int j = 0; j < k - 1; ++j) key = (key << bits) | s_map[s[i0 + j]];
            const int i1 = min(i0 + kKmerRun, nw);
            for (int i = i0; i < i1; ++i) {
                key = ((key << bits) | s_map[s[i + k - 1]]) & mask;
                const uint32_t place = ((uint32_t)si << 16) | (uint32_t)i;
                if (key == kKmerEmpty) {
                    atomicAdd(&s_ones_cnt, 1u);
                    atomicMin(&s_ones_first, place);
                    continue;
                }
                uint32_t h = (uint32_t)((key * 0x9E3779B97F4A7C15ull) >> 40) & (T - 1);
                int probe = 0;
                for (; probe < T; ++probe, h = (h + 1) & (T - 1)) {
                    uint64_t seen = *(volatile uint64_t*)&s_key[h];
                    if (seen != key) {
                        if (seen != kKmerEmpty) continue;
                        seen = atomicCAS((unsigned long long*)&s_key[h], (unsigned long long)kKmerEmpty, (unsigned long long)key);
                        if (seen == kKmerEmpty) {
                            if (atomicAdd(&s_d, 1) + 1 > kCap) s_over = 1;
                        } else if (seen != key) {
                            continue;
                        }
                    }
                    atomicAdd(&s_cnt[h], 1u);
                    atomicMin(&s_first[h], place);
                    break;
                }
                if (probe == T) s_over = 1;
            }
        }
    }
    __syncthreads();
    if (s_over) {   // (never in kKmerWrite: whether a group spills depends on its distinct windows alone)
        if (tid == 0 && a.mode == kKmerCount) {
            a.cnt[g] = -1;
            a.state[g] = kKmerSpilled;
        }
        return;
    }
    const int d = s_d;
    if (a.mode == kKmerCount) {
        if (tid == 0) {
            a.cnt[g] = d + (s_ones_cnt > 0 ? 1 : 0);
            a.state[g] = kKmerHashed;
        }
        return;
    }
    // the occupied slots, then every entry's rank among them
    for (int s = tid; s < T; s += NT)
        if (s_key[s] != kKmerEmpty) s_idx[atomicAdd(&s_n, 1)] = (uint16_t)s;
    __syncthreads();
    const int64_t base = a.entry_off[g];
    for (int e = tid; e < d; e += NT) {
        const int slot = s_idx[e];
        const uint64_t key = s_key[slot];
        int rank = 0;
        for (int o = 0; o < d; ++o) rank += s_key[s_idx[o]] < key ? 1 : 0;
        const uint32_t f = s_first[slot];
        a.out_pos[base + rank] = st[f >> 16] + (int64_t)(f & 0xFFFFu);
        a.out_count[base + rank] = (int32_t)s_cnt[slot];
    }
    if (tid == 0 && s_ones_cnt > 0) {   // all ones: the largest key
        const uint32_t f = s_ones_first;
        a.out_pos[base + d] = st[f >> 16] + (int64_t)(f & 0xFFFFu);
        a.out_count[base + d] = (int32_t)s_ones_cnt;
    }
}

// a > b in the order of the sort: (window, place); padding last
__device__ inline bool kmer_greater(const KmerElem& x, const KmerElem& y, bool general, const uint8_t* __restrict__ seqs,
                                    const int64_t* st, int k) {
    if (!general) return x.key > y.key || (x.key == y.key && x.place > y.place);
    if (x.place == kKmerPad) return y.place != kKmerPad;
    if (y.place == kKmerPad) return false;
    const uint8_t* p = seqs + st[x.place >> 16] + (x.place & 0xFFFFu);
    const uint8_t* q = seqs + st[y.place >> 16] + (y.place & 0xFFFFu);
    for (int j = 0; j < k; ++j)
        if (p[j] != q[j]) return p[j] > q[j];
    return x.place > y.place;
}

__device__ inline bool kmer_same_window(const KmerElem& x, const KmerElem& y, bool general, const uint8_t* __restrict__ seqs,
                                        const int64_t* st, int k) {
    if (!general) return x.key == y.key;
    const uint8_t* p = seqs + st[x.place >> 16] + (x.place & 0xFFFFu);
    const uint8_t* q = seqs + st[y.place >> 16] + (y.place & 0xFFFFu);
    for (int j = 0; j < k; ++j)
        if (p[j] != q[j]) return false;
    return true;
}

__global__ __launch_bounds__(kKmerSortThreads) void k_kmers_sort(KmerArgs a) {
    __shared__ int32_t s_woff[kKmerMaxGroup + 1];
    __shared__ int32_t s_heads[kKmerSortThreads];
    __shared__ uint32_t s_pres[8];
    __shared__ uint8_t s_map[256];
    __shared__ int s_bits;
    constexpr int NT = kKmerSortThreads;

    if ((int)blockIdx.x >= a.n_list) return;
    const int g = a.list[blockIdx.x];
    const int tid = threadIdx.x;
    KmerElem* e = a.ws + a.ws_off[blockIdx.x];
    const int q0 = a.group_off[g];
    const int m = a.group_off[g + 1] - q0;
    const int k = a.k[g];
    const int64_t* st = a.seq_start + q0;
    const int32_t* ln = a.seq_len + q0;
    if (tid == 0) {
        int w = 0;
        for (int i = 0; i < m; ++i) {
            s_woff[i] = w;
            w += max(ln[i] - k + 1, 0);
        }
        s_woff[m] = w;
    }
    __syncthreads();
    const uint32_t W = (uint32_t)s_woff[m];
    if (a.mode == kKmerWrite) {   // run r starts at element e[r].run; its first element holds the first occurrence
        const uint32_t d = (uint32_t)a.cnt[g];
        const int64_t base = a.entry_off[g];
        for (uint32_t r = tid; r < d; r += NT) {
            const uint32_t i = e[r].run;
            const uint32_t end = r + 1 < d ? e[r + 1].run : W;
            const uint32_t f = e[i].place;
            a.out_pos[base + r] = st[f >> 16] + (int64_t)(f & 0xFFFFu);
            a.out_count[base + r] = (int32_t)(end - i);
        }
        return;
    }
    const int bits = kmer_code_bits<NT>(a.seqs, st, ln, m, s_pres, s_map, &s_bits, tid);
    const int64_t kb = (int64_t)k * bits;
    const bool general = kb > 64;
    uint32_t P = 1;
    while (P < W) P <<= 1;
    // 1. one element per window
    const uint64_t mask = kb >= 64 ? ~0ull : (1ull << kb) - 1;
    for (int si = 0; si < m; ++si) {
        const int nw = ln[si] - k + 1;
        if (nw <= 0) continue;
        const uint8_t* s = a.seqs + st[si];
        KmerElem* es = e + s_woff[si];
        for (int i0 = tid * kKmerRun; i0 < nw; i0 += NT * kKmerRun) {
            const int i1 = min(i0 + kKmerRun, nw);
            uint64_t key = 0;
            if (!general)
                for (int j = 0; j < k - 1; ++j) key = (key << bits) | s_map[s[i0 + j]];
            for (int i = i0; i < i1; ++i) {
                if (!general) key = ((key << bits) | s_map[s[i + k - 1]]) & mask;
                es[i].key = key;
                es[i].place = ((uint32_t)si << 16) | (uint32_t)i;
            }
        }
    }
    for (uint32_t i = W + tid; i < P; i += NT) {
        e[i].key = kKmerEmpty;
        e[i].place = kKmerPad;
    }
    __syncthreads();
    // 2. bitonic sort by (window, place)
    for (uint32_t size = 2; size <= P; size <<= 1) {
        for (uint32_t stride = size >> 1; stride > 0; stride >>= 1) {
            for (uint32_t t = tid; t < (P >> 1); t += NT) {
                const uint32_t lo = 2 * t - (t & (stride - 1));
                const uint32_t hi = lo + stride;
                const bool ascending = (lo & size) == 0;
                const KmerElem x = e[lo], y = e[hi];
                if (kmer_greater(x, y, general, a.seqs, st, k) == ascending) {
                    e[lo].key = y.key;
                    e[lo].place = y.place;
                    e[hi].key = x.key;
                    e[hi].place = x.place;
                }
            }
            __syncthreads();
        }
    }
    // 3. the runs: every thread takes a stretch of elements, counts the run starts in it, and numbers them after a scan
    const uint32_t per = (W + NT - 1) / NT;
    const uint32_t b0 = min(W, (uint32_t)tid * per), b1 = min(W, b0 + per);
    int heads = 0;
    for (uint32_t i = b0; i < b1; ++i) heads += (i == 0 || !kmer_same_window(e[i - 1], e[i], general, a.seqs, st, k)) ? 1 : 0;
    s_heads[tid] = heads;
    __syncthreads();
    if (tid == 0) {
        int sum = 0;
        for (int t = 0; t < NT; ++t) {
            const int h = s_heads[t];
            s_heads[t] = sum;
            sum += h;
        }
        a.cnt[g] = sum;
    }
    __syncthreads();
    uint32_t r = (uint32_t)s_heads[tid];
    for (uint32_t i = b0; i < b1; ++i)
        if (i == 0 || !kmer_same_window(e[i - 1], e[i], general, a.seqs, st, k)) e[r++].run = i;
}

}  // namespace strk
