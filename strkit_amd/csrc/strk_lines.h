// strk_lines.h — the lines of a text, for host and device: where every line of t[start, n) begins, how many lines a reader may
// take and where the next piece resumes (split_host; on the device k_lines_count / k_lines_scan / k_lines_starts, launched by
// dbam_lines in strk_lines.inc).  The VCF reader (strk_vcf.h) and the annotation reader (strk_gff.h) stand on it.
//
// The rule: a line start is `start` itself and the byte after every '\n' in [start, n).  n_nl = the '\n's; the bytes behind the
// last one are a line of their own only in the text that ends its file (`final`) and only when there are any.  end_off = where
// the first line not taken begins (n when all were).
#pragma once
#include <stdint.h>
#include <string.h>

#include <vector>

namespace strk_lines {

constexpr int kTileBytes = 1024;    // text bytes one wave walks in the line-split passes (a multiple of kStepBytes)
constexpr int kStepBytes = 256;     // one aligned 32-bit word per lane and step

inline bool tile_bytes_ok(int32_t tile_bytes) { return tile_bytes >= kStepBytes && tile_bytes % kStepBytes == 0 && tile_bytes <= (1 << 20); }

struct Lines {
    std::vector<int64_t> starts;   // [n_nl + 1]
    int32_t n_nl, n_lines;         // line i = [starts[i], starts[i + 1] - 1) for i < n_nl; line n_nl (n_lines == n_nl + 1) = [starts[n_nl], n)
    int64_t end_off;
};

// one memchr walk (it runs at memory speed)
inline Lines split_host(const uint8_t* t, int64_t n, int64_t start, int32_t final) {
    Lines l{{start}, 0, 0, 0};
    for (int64_t p = start; p < n;) {
        const void* nl = memchr(t + p, '\n', (size_t)(n - p));
        if (!nl) break;
        p = (const uint8_t*)nl - t + 1;
        l.starts.push_back(p);
    }
    l.n_nl = (int32_t)l.starts.size() - 1;
    l.n_lines = l.n_nl + ((final && l.starts.back() < n) ? 1 : 0);
    l.end_off = l.n_lines > l.n_nl ? n : l.starts.back();
    return l;
}

#if defined(__HIPCC__)

// ---- line split: count, scan, scatter ---------------------------------------------------------------------------------------
// Tile w = the tile_bytes text bytes from t0 + w * tile_bytes on (t0 = the start offset rounded down to kStepBytes, so that every
// word load is aligned); one wave per tile, a lane reads one aligned word per step and the wave ballots each of its four bytes.
// Only '\n' at offsets in [start, n) count.  A line start is the byte after a '\n'; starts[0] = start itself.
__device__ inline uint32_t text_word(const uint8_t* data, int64_t n, int64_t p) {
    return p < n ? *reinterpret_cast<const uint32_t*>(data + p) : 0u;   // (the stream's buffer is padded by 16 bytes)
}

__global__ void __launch_bounds__(256) k_lines_count(const uint8_t* data, int64_t n, int64_t start, int32_t tile_bytes, int32_t n_tiles,
                                                     int32_t* counts) {
    const int32_t w = (int32_t)(blockIdx.x * 4 + (threadIdx.x >> 6)), lane = threadIdx.x & 63;
    if (w >= n_tiles) return;
    const int64_t base = (start & ~(int64_t)(kStepBytes - 1)) + (int64_t)w * tile_bytes;
    int32_t cnt = 0;
    for (int32_t o = 0; o < tile_bytes; o += kStepBytes) {
        const int64_t p = base + o + 4 * lane;
        const uint32_t word = text_word(data, n, p);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const bool hit = ((word >> (8 * k)) & 0xffu) == '\n' && p + k >= start && p + k < n;
            cnt += __popcll(__ballot(hit));
        }
    }
    if (lane == 0) counts[w] = cnt;
}

// exclusive sums of n counts (one workgroup): off[i] = counts[0] + ... + counts[i - 1], off[n] = the total.  The readers use it
// for every count they turn into offsets, not for tiles only.
__global__ void __launch_bounds__(256) k_lines_scan(const int32_t* counts, int32_t n, int64_t* off) {
    __shared__ int64_t part[256];
    const int32_t t = threadIdx.x, per = (n + 255) / 256;
    const int32_t a = min(n, t * per), b = min(n, a + per);
    int64_t s = 0;
    for (int32_t i = a; i < b; ++i) s += counts[i];
    part[t] = s;
    __syncthreads();
    if (t == 0) {
        int64_t run = 0;
        for (int i = 0; i < 256; ++i) { const int64_t x = part[i]; part[i] = run; run += x; }
        off[n] = run;
    }
    __syncthreads();
    int64_t run = part[t];
    for (int32_t i = a; i < b; ++i) { off[i] = run; run += counts[i]; }
}

__global__ void __launch_bounds__(256) k_lines_starts(const uint8_t* data, int64_t n, int64_t start, int32_t tile_bytes, int32_t n_tiles,
                                                      const int64_t* tile_off, int64_t n_starts, int64_t* starts) {
    const int32_t w = (int32_t)(blockIdx.x * 4 + (threadIdx.x >> 6)), lane = threadIdx.x & 63;
    if (w >= n_tiles) return;
    if (w == 0 && lane == 0) starts[0] = start;
    const int64_t base = (start & ~(int64_t)(kStepBytes - 1)) + (int64_t)w * tile_bytes;
    const unsigned long long lower = (1ull << lane) - 1ull;
    int64_t run = 1 + tile_off[w];
    for (int32_t o = 0; o < tile_bytes; o += kStepBytes) {
        const int64_t p = base + o + 4 * lane;
        const uint32_t word = text_word(data, n, p);
        bool hit[4];
        int32_t before = 0, total = 0;   // '\n's of the step in lower lanes (all four of their bytes); all of the step's
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            hit[k] = ((word >> (8 * k)) & 0xffu) == '\n' && p + k >= start && p + k < n;
            const unsigned long long m = __ballot(hit[k]);
            before += __popcll(m & lower);
            total += __popcll(m);
        }
        int64_t at = run + before;
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (hit[k]) {
                if (at < n_starts) starts[at] = p + k + 1;
                ++at;
            }
        run += total;
    }
}

#endif  // __HIPCC__

}  // namespace strk_lines
