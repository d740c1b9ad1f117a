// strk_vcf.h — candidate SNVs out of VCF text, for host and device: the rule of one line (parse_line), the host walk over the
// lines in slices (snvs_host), what both entry points do with the kept lines afterwards (finish: one record per position,
// sortedness, capacities), and the kernels that parse the lines of a text resident in HBM.  The lines themselves: strk_lines.h.
// strk_vcf.inc has the buffers and the launches.
//
// Reference: the reader strkit_rust_ext wraps around htslib's tabix access (STRkitVCFReader.get_candidate_snvs, call site
// strkit/call/call_sample.py:124) — not in the tree.  The rule is the one frontend/snv_vcf.py::read_snv_vcf states
// (DESIGN.md §18 lists the stated differences); tests/vcf_cases.py pins both entry points against it.
#pragma once
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <mutex>
#include <utility>
#include <vector>

#include "strk_bamrec.h"   // STRK_FE_HD
#include "strk_lines.h"

namespace strk_vcf {

constexpr int kLinesPerWave = 64;   // parse / compaction: one lane per line

// what a line is to the query
enum : int32_t {
    kSkip = 0,      // header, fewer than five fields, REF or ALT not single bases
    kKeep = 1,      // a single-base record of the contig inside [beg, end)
    kBadPos = 2,    // base-valid, POS not 1..18 decimal digits: the call fails
    kPast = 3,      // of the contig, at or beyond end
    kOther = 4,     // of another contig
    kBefore = 5,    // of the contig, in front of beg
};

struct Line {
    int32_t status;
    uint8_t ref;        // upper-case
    int64_t pos;        // 0-based
    int64_t id_a;       // offset of the ID bytes in the text
    int32_t id_len;     // 0 where the column is "."
};

STRK_FE_HD uint8_t upper(uint8_t c) { return (c >= 'a' && c <= 'z') ? (uint8_t)(c - 32) : c; }
STRK_FE_HD bool is_base(uint8_t c) { return c == 'A' || c == 'C' || c == 'G' || c == 'T' || c == 'N'; }

// One line [a, e) of the text t (e excludes the '\n').  Touches the first five fields only.
STRK_FE_HD Line parse_line(const uint8_t* t, int64_t a, int64_t e, const uint8_t* contig, int32_t contig_len, int64_t beg, int64_t end) {
    Line r{kSkip, 0, 0, 0, 0};
    if (a >= e || t[a] == '#') return r;
    int64_t f[5], g[5];   // field k = [f[k], g[k])
    int64_t i = a;
    for (int k = 0; k < 5; ++k) {
        f[k] = i;
        while (i < e && t[i] != '\t') ++i;
        g[k] = i;
        if (k < 4) {
            if (i >= e) return r;   // fewer than five fields
            ++i;
        }
    }
    if (g[4] == e)   // ALT is the line's last field: trailing '\r's are no part of it
        while (g[4] > f[4] && t[g[4] - 1] == '\r') --g[4];
    if (g[3] - f[3] != 1 || !is_base(upper(t[f[3]]))) return r;
    const int64_t n_alt = g[4] - f[4];
    if (n_alt < 1 || !(n_alt & 1)) return r;   // B(,B)*
    for (int64_t k = 0; k < n_alt; ++k) {
        const uint8_t c = t[f[4] + k];
        if ((k & 1) ? c != ',' : !is_base(upper(c))) return r;
    }
    // POS only now, on a line that passed the base check
    const int64_t n_pos = g[1] - f[1];
    r.status = kBadPos;
    if (n_pos < 1 || n_pos > 18) return r;
    int64_t v = 0;
    for (int64_t k = f[1]; k < g[1]; ++k) {
        if (t[k] < '0' || t[k] > '9') return r;
        v = v * 10 + (t[k] - '0');
    }
    r.pos = v - 1;
    r.ref = upper(t[f[3]]);
    r.status = kOther;
    if (g[0] - f[0] != contig_len) return r;
    for (int32_t k = 0; k < contig_len; ++k)
        if (t[f[0] + k] != contig[k]) return r;
    r.status = r.pos < beg ? kBefore : (r.pos >= end ? kPast : kKeep);
    if (r.status == kKeep && !(g[2] - f[2] == 1 && t[f[2]] == '.')) {
        r.id_a = f[2];
        r.id_len = (int32_t)(g[2] - f[2]);
    }
    return r;
}

// The kept lines of a call, in file order: what the host walk collects and what the device hands back.
struct Kept {
    std::vector<int64_t> pos, line, id_off;   // id_off: [n + 1] into ids
    std::vector<uint8_t> ref, ids;
};

// What the host walk gives back, before finish() looks at the capacities.
struct Walk {
    Kept kept;
    int64_t bad_off = -1;   // the first line with a malformed POS
    int64_t end_off = 0;
    int32_t past = 0;       // the contig's part of the file is over
};

// The host walk over t[start, n): lines by strk_lines::split_host, their fields by `par` (a parallel for over [0, n) in slices, in
// any order, on any threads), then the slices merged in file order.
template <class Par>
void snvs_host(const uint8_t* t, int64_t n, int64_t start, const char* contig, int64_t beg, int64_t end, int32_t final, int32_t contig_seen,
               Walk* out, Par&& par) {
    const strk_lines::Lines l = strk_lines::split_host(t, n, start, final);
    out->end_off = l.end_off;
    const int32_t contig_len = (int32_t)strlen(contig);
    struct Slice { Kept k; int64_t bad = -1, first_on = -1, last_other = -1; bool past = false; };
    std::mutex mu;
    std::vector<std::pair<int32_t, Slice>> slices;
    par(l.n_lines, [&](int32_t i0, int32_t i1) {
        Slice s;
        s.k.id_off.push_back(0);
        for (int32_t i = i0; i < i1; ++i) {
            const int64_t a = l.starts[(size_t)i], e = i < l.n_nl ? l.starts[(size_t)i + 1] - 1 : n;
            const Line r = parse_line(t, a, e, (const uint8_t*)contig, contig_len, beg, end);
            switch (r.status) {
            case kBadPos: if (s.bad < 0) s.bad = a; break;
            case kOther: s.last_other = i; break;
            case kPast: s.past = true; [[fallthrough]];
            case kBefore: if (s.first_on < 0) s.first_on = i; break;
            case kKeep:
                if (s.first_on < 0) s.first_on = i;
                s.k.pos.push_back(r.pos); s.k.line.push_back(a); s.k.ref.push_back(r.ref);
                s.k.ids.insert(s.k.ids.end(), t + r.id_a, t + r.id_a + r.id_len);
                s.k.id_off.push_back((int64_t)s.k.ids.size());
                break;
            default: break;
            }
        }
        std::lock_guard<std::mutex> lk(mu);
        slices.emplace_back(i0, std::move(s));
    });
    std::sort(slices.begin(), slices.end(), [](const auto& x, const auto& y) { return x.first < y.first; });
    Kept& all = out->kept;
    all.id_off.push_back(0);
    int64_t bad = -1, first_on = contig_seen ? 0 : -1, last_other = -1;
    bool any_past = false;
    for (auto& [i0, s] : slices) {
        if (bad < 0) bad = s.bad;
        if (first_on < 0) first_on = s.first_on;
        if (s.last_other >= 0) last_other = s.last_other;
        any_past = any_past || s.past;
        const int64_t id0 = (int64_t)all.ids.size();
        all.pos.insert(all.pos.end(), s.k.pos.begin(), s.k.pos.end());
        all.line.insert(all.line.end(), s.k.line.begin(), s.k.line.end());
        all.ref.insert(all.ref.end(), s.k.ref.begin(), s.k.ref.end());
        all.ids.insert(all.ids.end(), s.k.ids.begin(), s.k.ids.end());
        for (size_t j = 1; j < s.k.id_off.size(); ++j) all.id_off.push_back(id0 + s.k.id_off[j]);
    }
    out->bad_off = bad;
    out->past = (any_past || (first_on >= 0 && (contig_seen ? last_other >= 0 : last_other > first_on))) ? 1 : 0;
}

struct Message { char text[200]; };

// One record per position (the first in the file stays), sortedness, the first malformed POS (bad_off >= 0: its line), the
// capacities.  Returns the record count, or -1 with `msg` (invalid input) or -2 with `msg` (ID buffer too small).
inline int64_t finish(const Kept& k, int64_t bad_off, int64_t prev_pos, int64_t cap, int64_t* pos, uint8_t* ref, int64_t* id_off,
                      uint8_t* ids, int64_t ids_cap, int64_t* id_bytes, Message* msg) {
    const size_t n_in = k.pos.size();
    int64_t n = 0, w = 0, prev = prev_pos;
    // pass 1: the count and the ID bytes; pass 2 (when they fit): the arrays
    for (int pass = 0; pass < 2; ++pass) {
        n = 0; w = 0; prev = prev_pos;
        for (size_t i = 0; i < n_in; ++i) {
            if (bad_off >= 0 && k.line[i] > bad_off) break;
            const int64_t p = k.pos[i];
            if (prev >= 0 && p < prev) {
                snprintf(msg->text, sizeof msg->text, "line at byte %lld: position %lld after %lld: not coordinate-sorted: the index cannot belong to this file",
                         (long long)k.line[i], (long long)p + 1, (long long)prev + 1);
                return -1;
            }
            if (prev >= 0 && p == prev) continue;
            prev = p;
            const int64_t len = k.id_off[i + 1] - k.id_off[i];
            if (pass) {
                pos[n] = p;
                ref[n] = k.ref[i];
                id_off[n] = w;
                if (ids && len) memcpy(ids + w, k.ids.data() + k.id_off[i], (size_t)len);
            }
            ++n;
            w += len;
        }
        if (pass == 0) {
            if (bad_off >= 0) {
                snprintf(msg->text, sizeof msg->text, "line at byte %lld: POS is not 1 to 18 decimal digits", (long long)bad_off);
                return -1;
            }
            *id_bytes = w;
            if (n > cap) return n;
            if (ids && w > ids_cap) {
                snprintf(msg->text, sizeof msg->text, "ID buffer too small (%lld < %lld)", (long long)ids_cap, (long long)w);
                return -2;
            }
        }
    }
    id_off[n] = w;
    return n;
}

#if defined(__HIPCC__)

// ---- parse: one lane per line ---------------------------------------------------------------------------------------------
// Line i = [starts[i], starts[i + 1] - 1) for i < n_nl; line n_nl (only when n_lines == n_nl + 1: the text ends the file without
// a '\n') = [starts[n_nl], n).  st: [0] the lowest offset of a line with a malformed POS, [1] the first line of the contig,
// [2] 1 + the last line of another contig, [3] a line of the contig at or beyond `end` was seen.
__global__ void __launch_bounds__(256) k_vcf_parse(const uint8_t* data, int64_t n, const int64_t* starts, int32_t n_nl, int32_t n_lines,
                                                   const uint8_t* contig, int32_t contig_len, int64_t beg, int64_t end, int64_t* l_pos,
                                                   int64_t* l_id_a, int32_t* l_id_len, uint8_t* l_ref, uint8_t* l_status,
                                                   int32_t* keep_cnt, int32_t* id_cnt, unsigned long long* st) {
    const int32_t i = (int32_t)(blockIdx.x * blockDim.x + threadIdx.x), lane = threadIdx.x & 63;
    Line r{kSkip, 0, 0, 0, 0};
    int64_t a = 0;
    if (i < n_lines) {
        a = starts[i];
        const int64_t e = i < n_nl ? starts[i + 1] - 1 : n;
        if (a >= 0 && a <= e && e <= n) r = parse_line(data, a, e, contig, contig_len, beg, end);   // (line starts ascend by construction)
        l_pos[i] = r.pos; l_id_a[i] = r.id_a; l_id_len[i] = r.id_len; l_ref[i] = r.ref; l_status[i] = (uint8_t)r.status;
    }
    const unsigned long long keep = __ballot(r.status == kKeep);
    int32_t id_sum = r.status == kKeep ? r.id_len : 0;
    for (int d = 32; d > 0; d >>= 1) id_sum += __shfl_down(id_sum, d, 64);
    if (lane == 0 && i < n_lines) {
        const int32_t w = i >> 6;
        keep_cnt[w] = __popcll(keep);
        id_cnt[w] = id_sum;
    }
    if (r.status == kBadPos) atomicMin(&st[0], (unsigned long long)a);
    if (r.status == kKeep || r.status == kPast || r.status == kBefore) atomicMin(&st[1], (unsigned long long)i);
    if (r.status == kOther) atomicMax(&st[2], (unsigned long long)i + 1ull);
    if (r.status == kPast) atomicMax(&st[3], 1ull);
}

// ---- compaction: the kept lines, in file order, and their ID bytes -----------------------------------------------------------
__global__ void __launch_bounds__(256) k_vcf_compact(const uint8_t* data, const int64_t* starts, int32_t n_lines, const int64_t* l_pos,
                                                     const int64_t* l_id_a, const int32_t* l_id_len, const uint8_t* l_ref,
                                                     const uint8_t* l_status, const int64_t* keep_off, const int64_t* id_base,
                                                     int64_t n_keep, int64_t n_id_bytes, int64_t* o_pos, int64_t* o_line, int64_t* o_id_off,
                                                     uint8_t* o_ref, uint8_t* o_ids) {
    const int32_t i = (int32_t)(blockIdx.x * blockDim.x + threadIdx.x), lane = threadIdx.x & 63;
    const bool keep = i < n_lines && l_status[i] == kKeep;
    const int32_t len = keep ? l_id_len[i] : 0;
    const unsigned long long m = __ballot(keep);
    int32_t incl = len;   // inclusive sums of the ID lengths over the wave
    for (int d = 1; d < 64; d <<= 1) {
        const int32_t up = __shfl_up(incl, d, 64);
        if (lane >= d) incl += up;
    }
    if (!keep) return;
    const int32_t w = i >> 6;
    const int64_t k = keep_off[w] + __popcll(m & ((1ull << lane) - 1ull));
    const int64_t at = id_base[w] + (incl - len);
    if (k >= n_keep || at + len > n_id_bytes) return;   // (cannot happen: the sums come from the same flags)
    o_pos[k] = l_pos[i];
    o_line[k] = starts[i];
    o_id_off[k] = at;
    o_ref[k] = l_ref[i];
    const uint8_t* src = data + l_id_a[i];
    for (int32_t b = 0; b < len; ++b) o_ids[at + b] = src[b];
}

#endif  // __HIPCC__

}  // namespace strk_vcf
