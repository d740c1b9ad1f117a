// strk_gff.h — the genome features of GFF3 / GTF text that overlap the loci of one contig, for host and device: the rule of one line
// (parse_line), the key match of an attribute piece (match_key) and the id of a feature (find_id), the host walk with its join
// (overlaps_host), the closing pass with its capacities (emit), and the kernels that do the same over a text resident in HBM.
// strk_gff.inc has the buffers and the launches; the lines: strk_lines.h.
//
// Reference: strkit/call/loci.py:158-166 (get_feature_id), :209-214, :250-253 (one tabix fetch per locus through pysam's asGFF3 /
// asGTF, which are not in the tree).  The rule is the one frontend/annotations.py states; tests/annot_cases.py pins
// both entry points against it.
#pragma once
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "strk_bamrec.h"   // STRK_FE_HD
#include "strk_lines.h"

namespace strk_gff {

constexpr int kClasses = 64;        // length classes of the join: c = floor(log2(f_end - f_beg)); one lane per class
constexpr int kStepBytes = 64;      // attribute bytes one wave reads per step in k_gff_ids
constexpr int kLinesPerWave = 64;   // k_gff_coords: one lane per line

enum : int32_t {
    kSkip = 0,    // empty, or begins with '#'
    kBad = 1,     // fewer than nine fields, start / end not 1 to 18 digits, start < 1, end < start: the call fails
    kOther = 2,   // a feature of another contig
    kOn = 3,      // a feature of the contig
};
enum : int32_t { kIdAttr = 0, kIdExon = 1, kIdPosition = 2 };   // where a feature's id comes from

struct Line {
    int32_t status;
    int64_t f_beg, f_end;           // 0-based, half-open
    int64_t type_a, attr_a;         // offsets of field 3 and field 9 in the text
    int32_t type_len, attr_len;
};

// 1 to 18 decimal digits -> the value, otherwise -1
STRK_FE_HD int64_t digits(const uint8_t* t, int64_t a, int64_t e) {
    if (e - a < 1 || e - a > 18) return -1;
    int64_t v = 0;
    for (int64_t k = a; k < e; ++k) {
        if (t[k] < '0' || t[k] > '9') return -1;
        v = v * 10 + (t[k] - '0');
    }
    return v;
}

// One line [a, e) of the text t (e excludes the '\n').  Touches fields 1 to 5 and finds the ninth; the attributes are not walked.
STRK_FE_HD Line parse_line(const uint8_t* t, int64_t a, int64_t e, const uint8_t* contig, int32_t contig_len) {
    Line r{kSkip, 0, 0, 0, 0, 0, 0};
    while (e > a && t[e - 1] == '\r') --e;
    if (a >= e || t[a] == '#') return r;
    r.status = kBad;
    int64_t f[9], g[9];   // field k = [f[k], g[k])
    int64_t i = a;
    for (int k = 0; k < 9; ++k) {
        f[k] = i;
        while (i < e && t[i] != '\t') ++i;
        g[k] = i;
        if (k < 8) {
            if (i >= e) return r;   // fewer than nine fields
            ++i;
        }
    }
    const int64_t s = digits(t, f[3], g[3]), x = digits(t, f[4], g[4]);
    if (s < 1 || x < s) return r;
    r.f_beg = s - 1;
    r.f_end = x;
    r.type_a = f[2]; r.type_len = (int32_t)(g[2] - f[2]);
    r.attr_a = f[8]; r.attr_len = (int32_t)(g[8] - f[8]);
    r.status = kOther;
    if (g[0] - f[0] != contig_len) return r;
    for (int32_t k = 0; k < contig_len; ++k)
        if (t[f[0] + k] != contig[k]) return r;
    r.status = kOn;
    return r;
}

STRK_FE_HD int32_t length_class(int64_t f_beg, int64_t f_end) {
    uint64_t len = (uint64_t)(f_end - f_beg);   // >= 1
    int32_t c = 0;
    while (len >>= 1) ++c;
    return c;
}
// a locus [s, e) can overlap a class-c feature only when s - reach(c) < f_beg < e
STRK_FE_HD int64_t reach(int32_t c) { return (int64_t)1 << (c + 1 < 62 ? c + 1 : 62); }

STRK_FE_HD bool bytes_are(const uint8_t* t, int64_t a, int64_t len, const char* w, int32_t wl) {
    if (len != wl) return false;
    for (int32_t k = 0; k < wl; ++k)
        if (t[a + k] != (uint8_t)w[k]) return false;
    return true;
}
// the types whose id may come from exon_id (loci.py:155; `exon` is not among them)
STRK_FE_HD bool exon_id_type(const uint8_t* t, int64_t a, int64_t len) {
    return bytes_are(t, a, len, "5UTR", 4) || bytes_are(t, a, len, "3UTR", 4) || bytes_are(t, a, len, "CDS", 3) ||
           bytes_are(t, a, len, "start_codon", 11) || bytes_are(t, a, len, "stop_codon", 10);
}

// The piece of the attribute column that begins at p (the byte after a separator, or the column's first; the column ends at e):
// leading spaces, then the key as a whole, then '=' (GFF3) / ' ' (GTF) or the end of the piece.  Returns 0 for `ID`, 1 for
// `exon_id`, -1 otherwise; *value = where the value begins.  Reads no byte that a separator could hide: spaces and key bytes only.
STRK_FE_HD int32_t match_key(const uint8_t* t, int64_t p, int64_t e, int32_t gtf, int64_t* value) {
    while (p < e && t[p] == ' ') ++p;
    const char* keys[2] = {"ID", "exon_id"};
    const int32_t lens[2] = {2, 7};
    for (int32_t q = 0; q < 2; ++q) {
        if (p + lens[q] > e) continue;
        bool same = true;
        for (int32_t k = 0; k < lens[q]; ++k) same = same && t[p + k] == (uint8_t)keys[q][k];
        if (!same) continue;
        const int64_t r = p + lens[q];
        if (r == e || t[r] == ';') { *value = r; return q; }
        if (t[r] == (gtf ? ' ' : '=')) { *value = r + 1; return q; }
    }
    return -1;
}

// GTF: the value without the spaces around it and without one pair of double quotes
STRK_FE_HD void trim_gtf(const uint8_t* t, int64_t* a, int64_t* e) {
    while (*a < *e && t[*a] == ' ') ++*a;
    while (*e > *a && t[*e - 1] == ' ') --*e;
    if (*e - *a >= 2 && t[*a] == '"' && t[*e - 1] == '"') { ++*a; --*e; }
}

// The id of a feature from its attribute column [a, e), piece by piece (the host's way; k_gff_ids does the same 64 bytes a step):
// the kind and the span of the id's bytes (none for kIdPosition).
STRK_FE_HD int32_t find_id(const uint8_t* t, int64_t a, int64_t e, int32_t gtf, bool exon_type, int64_t* id_a, int32_t* id_len) {
    int64_t va[2] = {-1, -1}, ve[2] = {-1, -1};
    int64_t p = a;
    while (p <= e) {
        int64_t pe = p;   // the piece ends at the next ';' (GTF: outside double quotes) or at e
        bool quoted = false;
        while (pe < e && !(t[pe] == ';' && !quoted)) {
            if (gtf && t[pe] == '"') quoted = !quoted;
            ++pe;
        }
        int64_t v = 0;
        const int32_t q = p < e ? match_key(t, p, e, gtf, &v) : -1;
        if (q >= 0) { va[q] = v; ve[q] = pe; }   // (the last piece of a key wins)
        p = pe + 1;
    }
    const int32_t q = va[0] >= 0 ? 0 : ((exon_type && va[1] >= 0) ? 1 : -1);
    *id_a = 0; *id_len = 0;
    if (q < 0) return kIdPosition;
    if (gtf) trim_gtf(t, &va[q], &ve[q]);
    *id_a = va[q]; *id_len = (int32_t)(ve[q] - va[q]);
    return q == 0 ? kIdAttr : kIdExon;
}

struct Message { char text[200]; };

// What a call gives back, on the host, before the capacities are looked at.
struct Result {
    std::vector<int64_t> pair_off;    // [n_loci + 1]: the pairs of locus l are pair_feat[pair_off[l] .. pair_off[l + 1])
    std::vector<int32_t> pair_feat;   // indices into the hit features, ascending per locus (file order)
    std::vector<int64_t> f_beg, f_end, text_off;   // hit features in file order; text_off [2 n + 1]: type bytes, then id bytes
    std::vector<int32_t> kind;
    std::vector<uint8_t> text;
    int64_t last_beg = -1, end_off = 0;
    int32_t past = 0;
};

inline int bad_line(Message* msg, int64_t off) {
    snprintf(msg->text, sizeof msg->text, "line at byte %lld: not a feature line (nine tab-separated fields, start and end of 1 to 18 decimal digits, 1 <= start <= end)", (long long)off);
    return -1;
}
inline int unsorted_line(Message* msg, int64_t off) {
    snprintf(msg->text, sizeof msg->text, "line at byte %lld: its start lies in front of the feature before it: not coordinate-sorted: the index cannot belong to this file", (long long)off);
    return -1;
}

// The host walk over t[start, n): lines by strk_lines::split_host, the fields by `par` (a parallel for over [0, n) in slices), order, the join by
// length classes (two binary searches per class and locus), ids of the hit features only.  Returns 0, or -1 with msg.
template <class Par>
int overlaps_host(const uint8_t* t, int64_t n, int64_t start, const char* contig, int32_t gtf, int32_t final, int64_t prev_beg, int32_t n_loci,
                  const int64_t* ls, const int64_t* le, Result* out, Message* msg, Par&& par) {
    const strk_lines::Lines l = strk_lines::split_host(t, n, start, final);
    const std::vector<int64_t>& starts = l.starts;
    const int32_t n_nl = l.n_nl, n_lines = l.n_lines;
    out->end_off = l.end_off;
    const int32_t contig_len = (int32_t)strlen(contig);
    std::vector<Line> lines((size_t)n_lines);
    par(n_lines, [&](int32_t i0, int32_t i1) {
        for (int32_t i = i0; i < i1; ++i)
            lines[(size_t)i] = parse_line(t, starts[(size_t)i], i < n_nl ? starts[(size_t)i + 1] - 1 : n, (const uint8_t*)contig, contig_len);
    });
    // in file order: the first line that breaks a rule; the contig's features; whether the contig's part of the file is over
    std::vector<int32_t> feat;
    int64_t prev = prev_beg;
    bool seen = prev_beg >= 0;
    for (int32_t i = 0; i < n_lines; ++i) {
        const Line& r = lines[(size_t)i];
        if (r.status == kBad) return bad_line(msg, starts[(size_t)i]);
        if (r.status == kOther && seen) out->past = 1;
        if (r.status != kOn) continue;
        if (r.f_beg < prev) return unsorted_line(msg, starts[(size_t)i]);
        prev = r.f_beg;
        seen = true;
        feat.push_back(i);
    }
    out->last_beg = prev;
    // the join: features by length class, each class in file order, hence ascending in f_beg
    std::vector<int64_t> cb[kClasses], ce[kClasses];
    std::vector<int32_t> co[kClasses];
    for (size_t k = 0; k < feat.size(); ++k) {
        const Line& r = lines[(size_t)feat[k]];
        const int32_t c = length_class(r.f_beg, r.f_end);
        cb[c].push_back(r.f_beg); ce[c].push_back(r.f_end); co[c].push_back((int32_t)k);
    }
    std::vector<std::vector<int32_t>> hits((size_t)n_loci);
    par(n_loci, [&](int32_t l0, int32_t l1) {
        for (int32_t l = l0; l < l1; ++l) {
            const int64_t s = ls[l], e = le[l];
            std::vector<int32_t>& h = hits[(size_t)l];
            for (int32_t c = 0; c < kClasses; ++c) {
                if (cb[c].empty()) continue;
                const size_t lo = (size_t)(std::lower_bound(cb[c].begin(), cb[c].end(), s - reach(c) + 1) - cb[c].begin());
                const size_t hi = (size_t)(std::lower_bound(cb[c].begin(), cb[c].end(), e) - cb[c].begin());
                for (size_t k = lo; k < hi; ++k)
                    if (ce[c][k] > s) h.push_back(co[c][k]);
            }
            std::sort(h.begin(), h.end());
        }
    });
    std::vector<int32_t> rank(feat.size(), -1);
    for (const auto& h : hits)
        for (int32_t k : h) rank[(size_t)k] = 0;
    out->text_off.push_back(0);
    for (size_t k = 0; k < feat.size(); ++k) {
        if (rank[k] < 0) continue;
        rank[k] = (int32_t)out->f_beg.size();
        const Line& r = lines[(size_t)feat[k]];
        int64_t id_a = 0;
        int32_t id_len = 0;
        const int32_t kind = find_id(t, r.attr_a, r.attr_a + r.attr_len, gtf, exon_id_type(t, r.type_a, r.type_len), &id_a, &id_len);
        out->f_beg.push_back(r.f_beg); out->f_end.push_back(r.f_end); out->kind.push_back(kind);
        out->text.insert(out->text.end(), t + r.type_a, t + r.type_a + r.type_len);
        out->text_off.push_back((int64_t)out->text.size());
        out->text.insert(out->text.end(), t + id_a, t + id_a + id_len);
        out->text_off.push_back((int64_t)out->text.size());
    }
    out->pair_off.assign((size_t)n_loci + 1, 0);
    for (int32_t l = 0; l < n_loci; ++l) {
        for (int32_t k : hits[(size_t)l]) out->pair_feat.push_back(rank[(size_t)k]);
        out->pair_off[(size_t)l + 1] = (int64_t)out->pair_feat.size();
    }
    return 0;
}

// The capacities: sizes[0..2] = pairs, hit features, text bytes (always), sizes[3] = the last f_beg of the contig; the arrays are
// filled when all three fit.  Returns the number of pairs.
inline int64_t emit(const Result& r, int32_t n_loci, int64_t pair_cap, int32_t* pair_locus, int32_t* pair_feat, int64_t feat_cap, int64_t* f_beg,
                    int64_t* f_end, int32_t* f_kind, int64_t* f_text_off, int64_t text_cap, uint8_t* text, int64_t* sizes) {
    const int64_t n_pairs = (int64_t)r.pair_feat.size(), n_feat = (int64_t)r.f_beg.size(), n_text = (int64_t)r.text.size();
    sizes[0] = n_pairs; sizes[1] = n_feat; sizes[2] = n_text; sizes[3] = r.last_beg;
    if (n_pairs > pair_cap || n_feat > feat_cap || n_text > text_cap) return n_pairs;
    for (int32_t l = 0; l < n_loci; ++l)
        for (int64_t i = r.pair_off[(size_t)l]; i < r.pair_off[(size_t)l + 1]; ++i) { pair_locus[i] = l; pair_feat[i] = r.pair_feat[(size_t)i]; }
    for (int64_t k = 0; k < n_feat; ++k) { f_beg[k] = r.f_beg[(size_t)k]; f_end[k] = r.f_end[(size_t)k]; f_kind[k] = r.kind[(size_t)k]; }
    if (feat_cap > 0 || n_feat > 0)
        for (int64_t k = 0; k <= 2 * n_feat; ++k) f_text_off[k] = r.text_off[(size_t)k];
    if (n_text) memcpy(text, r.text.data(), (size_t)n_text);
    return n_pairs;
}

#if defined(__HIPCC__)

// ---- the fields: one lane per line ------------------------------------------------------------------------------------------
// Lines as strk_lines.h numbers them.  st: [0] the lowest offset of a line that breaks a rule, [1] the first line of the contig, [2] 1 + the
// last line of another contig, [3] the lowest offset of a line whose start descends (k_gff_gather).
__global__ void __launch_bounds__(256) k_gff_coords(const uint8_t* data, int64_t n, const int64_t* starts, int32_t n_nl, int32_t n_lines,
                                                    const uint8_t* contig, int32_t contig_len, int64_t* l_beg, int64_t* l_end, int64_t* l_type_a,
                                                    int32_t* l_type_len, int64_t* l_attr_a, int32_t* l_attr_len, uint8_t* l_status,
                                                    int32_t* on_cnt, unsigned long long* st) {
    const int32_t i = (int32_t)(blockIdx.x * blockDim.x + threadIdx.x), lane = threadIdx.x & 63;
    Line r{kSkip, 0, 0, 0, 0, 0, 0};
    int64_t a = 0;
    if (i < n_lines) {
        a = starts[i];
        const int64_t e = i < n_nl ? starts[i + 1] - 1 : n;
        if (a >= 0 && a <= e && e <= n) r = parse_line(data, a, e, contig, contig_len);
        l_beg[i] = r.f_beg; l_end[i] = r.f_end; l_type_a[i] = r.type_a; l_type_len[i] = r.type_len;
        l_attr_a[i] = r.attr_a; l_attr_len[i] = r.attr_len; l_status[i] = (uint8_t)r.status;
    }
    const unsigned long long on = __ballot(r.status == kOn);
    if (lane == 0 && i < n_lines) on_cnt[i >> 6] = __popcll(on);
    if (r.status == kBad) atomicMin(&st[0], (unsigned long long)a);
    if (r.status == kOn) atomicMin(&st[1], (unsigned long long)i);
    if (r.status == kOther) atomicMax(&st[2], (unsigned long long)i + 1ull);
}

// the contig's features in file order: feature k = the k-th kOn line
__global__ void __launch_bounds__(256) k_gff_gather(int32_t n_lines, const uint8_t* l_status, const int64_t* l_beg, const int64_t* l_end,
                                                    const int64_t* on_off, int32_t n_feat, int64_t* fb, int64_t* fe, int32_t* f_line) {
    const int32_t i = (int32_t)(blockIdx.x * blockDim.x + threadIdx.x), lane = threadIdx.x & 63;
    const bool on = i < n_lines && l_status[i] == kOn;
    const unsigned long long m = __ballot(on);
    if (!on) return;
    const int64_t k = on_off[i >> 6] + __popcll(m & ((1ull << lane) - 1ull));
    if (k >= n_feat) return;   // (cannot happen: the sums come from the same flags)
    fb[k] = l_beg[i]; fe[k] = l_end[i]; f_line[k] = i;
}

// order (against the feature before, or the piece before), and the wave's features per length class: cnt[c * n_waves + w]
__global__ void __launch_bounds__(256) k_gff_classes(int32_t n_feat, const int64_t* fb, const int64_t* fe, const int32_t* f_line, const int64_t* starts,
                                                     int64_t prev_beg, int32_t n_waves, int32_t* cnt, const int64_t* coff, int64_t* p_beg,
                                                     int64_t* p_end, int32_t* p_ord, unsigned long long* st) {
    const int32_t k = (int32_t)(blockIdx.x * blockDim.x + threadIdx.x), lane = threadIdx.x & 63, w = k >> 6;
    const bool live = k < n_feat;
    int32_t c = 0;
    if (live) {
        c = length_class(fb[k], fe[k]);
        if (!coff && fb[k] < (k > 0 ? fb[k - 1] : prev_beg)) atomicMin(&st[3], (unsigned long long)starts[f_line[k]]);
    }
    // the lanes of this lane's class: six ballots, one per bit of the class
    unsigned long long peers = __ballot(live);
#pragma unroll
    for (int b = 0; b < 6; ++b) {
        const unsigned long long m = __ballot(live && ((c >> b) & 1));
        peers &= ((c >> b) & 1) ? m : ~m;
    }
    if (!live) return;
    const int32_t before = __popcll(peers & ((1ull << lane) - 1ull));
    const size_t slot = (size_t)c * (size_t)n_waves + (size_t)w;
    if (!coff) {                       // count pass
        if (before == 0) cnt[slot] = __popcll(peers);
    } else {                           // fill pass: a stable partition, class by class, file order within a class
        const int64_t at = coff[slot] + before;
        if (at < n_feat) { p_beg[at] = fb[k]; p_end[at] = fe[k]; p_ord[at] = k; }
    }
}

__device__ inline int32_t lower_bound_i64(const int64_t* v, int32_t lo, int32_t hi, int64_t x) {   // first index in [lo, hi) with v >= x
    while (lo < hi) {
        const int32_t mid = lo + ((hi - lo) >> 1);
        if (v[mid] < x) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// ---- the join: one wave per locus ------------------------------------------------------------------------------------------
// Lane c bounds the candidates of class c by two binary searches over the class's f_beg; the wave then tests f_end > s over each
// class's candidates, 64 a step.  Count pass (pair_off == NULL): cnt[l] = the hits.  Fill pass: the hits' feature ordinals in class
// order at tmp[pair_off[l] ..], and flag[ordinal] = 1.
__global__ void __launch_bounds__(256) k_gff_join(int32_t n_loci, const int64_t* ls, const int64_t* le, int32_t n_feat, int32_t n_waves, const int64_t* coff,
                                                  const int64_t* p_beg, const int64_t* p_end, const int32_t* p_ord, int32_t* cnt, const int64_t* pair_off,
                                                  int64_t n_pairs, int32_t* tmp, uint8_t* flag) {
    const int32_t l = (int32_t)(blockIdx.x * 4 + (threadIdx.x >> 6)), lane = threadIdx.x & 63;
    if (l >= n_loci) return;
    const int64_t s = ls[l], e = le[l];
    int32_t lo = 0, hi = 0;
    {
        const int32_t c0 = (int32_t)min(coff[(size_t)lane * n_waves], (int64_t)n_feat), c1 = (int32_t)min(coff[(size_t)(lane + 1) * n_waves], (int64_t)n_feat);
        if (c1 > c0) {
            lo = lower_bound_i64(p_beg, c0, c1, s - reach(lane) + 1);
            hi = lower_bound_i64(p_beg, c0, c1, e);
        }
    }
    const unsigned long long lower = (1ull << lane) - 1ull;
    const int64_t base = pair_off ? pair_off[l] : 0;
    int32_t run = 0;
    unsigned long long todo = __ballot(hi > lo);
    while (todo) {
        const int c = __ffsll((long long)todo) - 1;
        todo &= todo - 1;
        const int32_t clo = __shfl(lo, c, 64), chi = __shfl(hi, c, 64);
        for (int32_t k0 = clo; k0 < chi; k0 += 64) {
            const int32_t k = k0 + lane;
            const bool hit = k < chi && p_end[k] > s;
            const unsigned long long m = __ballot(hit);
            if (hit && pair_off) {
                const int64_t at = base + run + __popcll(m & lower);
                const int32_t ord = p_ord[k];
                if (at < n_pairs && ord >= 0 && ord < n_feat) { tmp[at] = ord; flag[ord] = 1; }
            }
            run += __popcll(m);
        }
    }
    if (!pair_off && lane == 0) cnt[l] = run;
}

// the distinct hit features: count pass (hit_off == NULL) and fill pass
__global__ void __launch_bounds__(256) k_gff_hits(int32_t n_feat, const uint8_t* flag, int32_t* hit_cnt, const int64_t* hit_off, int32_t n_hit,
                                                  int32_t* hit_rank, int32_t* hit_ord) {
    const int32_t k = (int32_t)(blockIdx.x * blockDim.x + threadIdx.x), lane = threadIdx.x & 63;
    const bool on = k < n_feat && flag[k];
    const unsigned long long m = __ballot(on);
    if (!hit_off) {
        if (lane == 0 && k < n_feat) hit_cnt[k >> 6] = __popcll(m);
        return;
    }
    if (!on) return;
    const int64_t j = hit_off[k >> 6] + __popcll(m & ((1ull << lane) - 1ull));
    if (j >= n_hit) return;
    hit_rank[k] = (int32_t)j; hit_ord[j] = k;
}

// a locus's hits into file order: the rank of an ordinal is the number of smaller ones among the locus's hits (they are distinct)
__global__ void __launch_bounds__(256) k_gff_order(int32_t n_loci, const int64_t* pair_off, int64_t n_pairs, const int32_t* tmp, int32_t n_feat,
                                                   const int32_t* hit_rank, int32_t* pair_feat) {
    const int32_t l = (int32_t)(blockIdx.x * 4 + (threadIdx.x >> 6)), lane = threadIdx.x & 63;
    if (l >= n_loci) return;
    const int64_t b = pair_off[l], h = pair_off[l + 1] - b;
    if (b < 0 || h < 0 || b + h > n_pairs) return;
    for (int64_t i0 = 0; i0 < h; i0 += 64) {
        const int64_t i = i0 + lane;
        if (i >= h) continue;
        const int32_t x = tmp[b + i];
        int64_t r = 0;
        for (int64_t j = 0; j < h; ++j) r += tmp[b + j] < x;
        if (x >= 0 && x < n_feat) pair_feat[b + r] = hit_rank[x];
    }
}

// ---- ids: one wave per distinct hit feature ----------------------------------------------------------------------------------
// The attribute column 64 bytes a step: ballots for ';' and '"' (GTF: a ';' counts when the quotes in front of it, a carried parity
// plus a prefix popcount, are even); the lane on the first byte of a piece does the whole-key compare (match_key); the value ends
// at the first separator behind it, in this step or a later one; of several pieces with a key the last wins.
__global__ void __launch_bounds__(256) k_gff_ids(const uint8_t* data, int64_t n, int32_t n_hit, const int32_t* hit_ord, int32_t n_feat, int32_t n_lines, const int32_t* f_line,
                                                 const int64_t* fb, const int64_t* fe, const int64_t* l_type_a, const int32_t* l_type_len,
                                                 const int64_t* l_attr_a, const int32_t* l_attr_len, int32_t gtf, int64_t* h_beg, int64_t* h_end,
                                                 int32_t* h_kind, int64_t* h_type_a, int32_t* h_type_len, int64_t* h_id_a, int32_t* h_id_len,
                                                 int32_t* h_text) {
    const int32_t j = (int32_t)(blockIdx.x * 4 + (threadIdx.x >> 6)), lane = threadIdx.x & 63;
    if (j >= n_hit) return;
    const int32_t k = hit_ord[j];
    if (k < 0 || k >= n_feat) return;   // (cannot happen: the list comes from the flags of these features)
    const int32_t i = f_line[k];
    if (i < 0 || i >= n_lines) return;
    const int64_t a = l_attr_a[i], e = a + l_attr_len[i], type_a = l_type_a[i];
    const int32_t type_len = l_type_len[i];
    int64_t va[2] = {-1, -1}, ve[2] = {-1, -1};
    bool open[2] = {false, false};
    if (a >= 0 && e <= n && type_a >= 0 && type_a + type_len <= n) {
        const unsigned long long lower = (1ull << lane) - 1ull;
        uint32_t parity = 0;
        bool prev_sep = true;   // the column's first byte begins a piece
        for (int64_t o = a; o < e; o += kStepBytes) {
            const int64_t p = o + lane;
            const bool valid = p < e;
            const uint8_t ch = valid ? data[p] : 0;
            const unsigned long long quote = gtf ? __ballot(valid && ch == '"') : 0ull;
            const bool outside = ((parity + __popcll(quote & lower)) & 1u) == 0;
            const unsigned long long sep = __ballot(valid && ch == ';' && outside);
            parity = (parity + __popcll(quote)) & 1u;
            const bool first = valid && (lane == 0 ? prev_sep : ((sep >> (lane - 1)) & 1ull) != 0);
            prev_sep = (sep >> 63) & 1ull;
            int64_t v = 0;
            const int32_t which = first ? match_key(data, p, e, gtf, &v) : -1;
            if (sep) {   // a value left open by an earlier step ends at this step's first separator
                const int64_t at = o + __ffsll((long long)sep) - 1;
                for (int q = 0; q < 2; ++q)
                    if (open[q]) { ve[q] = at; open[q] = false; }
            }
            for (int q = 0; q < 2; ++q) {
                const unsigned long long m = __ballot(which == q);
                if (!m) continue;
                const int L = 63 - __clzll((long long)m);
                va[q] = __shfl(v, L, 64);
                const unsigned long long behind = L == 63 ? 0ull : (sep & ~((2ull << L) - 1ull));
                open[q] = behind == 0;
                if (behind) ve[q] = o + __ffsll((long long)behind) - 1;
            }
        }
        for (int q = 0; q < 2; ++q)
            if (open[q]) ve[q] = e;
    }
    if (lane != 0) return;
    const bool exon_type = type_a >= 0 && type_a + type_len <= n && exon_id_type(data, type_a, type_len);
    const int q = va[0] >= 0 ? 0 : ((exon_type && va[1] >= 0) ? 1 : -1);
    int64_t id_a = 0, id_e = 0;
    if (q >= 0) {
        id_a = va[q]; id_e = ve[q];
        if (id_e < id_a) id_e = id_a;
        if (gtf) trim_gtf(data, &id_a, &id_e);
    }
    h_beg[j] = fb[k]; h_end[j] = fe[k];
    h_kind[j] = q < 0 ? kIdPosition : (q == 0 ? kIdAttr : kIdExon);
    h_type_a[j] = type_a; h_type_len[j] = type_len;
    h_id_a[j] = id_a; h_id_len[j] = (int32_t)(id_e - id_a);
    h_text[j] = type_len + (int32_t)(id_e - id_a);
}

// ---- compaction: the type and id bytes of the hit features, one wave per feature ---------------------------------------------
__global__ void __launch_bounds__(256) k_gff_text(const uint8_t* data, int64_t n, int32_t n_hit, const int64_t* h_type_a, const int32_t* h_type_len,
                                                  const int64_t* h_id_a, const int32_t* h_id_len, const int64_t* text_off, int64_t n_text,
                                                  uint8_t* text) {
    const int32_t j = (int32_t)(blockIdx.x * 4 + (threadIdx.x >> 6)), lane = threadIdx.x & 63;
    if (j >= n_hit) return;
    const int64_t at = text_off[j], ta = h_type_a[j], ia = h_id_a[j];
    const int32_t tl = h_type_len[j], il = h_id_len[j];
    if (at < 0 || tl < 0 || il < 0 || at + tl + il > n_text || ta < 0 || ta + tl > n || ia < 0 || ia + il > n) return;
    for (int32_t b = lane; b < tl; b += 64) text[at + b] = data[ta + b];
    for (int32_t b = lane; b < il; b += 64) text[at + tl + b] = data[ia + b];
}

#endif  // __HIPCC__

}  // namespace strk_gff
