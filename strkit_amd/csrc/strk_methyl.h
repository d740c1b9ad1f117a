// strk_methyl.h — 5-methyl CpG calls of a read inside a locus's tract, from the record's MM / ML tags (SAM tags specification):
// per item (record, locus boundaries) the number of CpG sites of the tract, how many of them the tags speak about, and how
// many of those carry a probability above the threshold.  The walks are written once, for host and device (strk_bamrec.h's
// STRK_FE_HD): the scan of one MM entry head and of
// one MM number, the target masks of sixteen bases and the site test; the auxiliary-chain finder is strk_aux.h's.  The host twin (host_methyl) and the kernel
// (k_dbam_methyl) call the same functions.  Without HIP the header compiles with the host compiler alone (tools/methyl_asan.cpp
// runs the walks and the checker under the sanitizers).
//
// Reference: STRkitAlignedSegment.get_methylation_prop of strkit_rust_ext (call site strkit/call/call_locus.py:1301-1305), which
// is not in the reference's tree: the rule is this project's own and UNPINNED; its readable statement is
// strkit_amd/frontend/methyl.py, and tests/test_methyl_host.py holds the two together.
#pragma once
#include <stdint.h>

#include <algorithm>
#include <vector>

#include "strk_aux.h"
#include "strk_bamrec.h"
#include "strk_groups.h"

namespace strk_me {

// status of an item
constexpr int kOk = 0, kNotSpanning = 1, kNoTags = 2, kClipped = 3, kMalformed = 4, kNoSites = 5;
constexpr int kBadChain = -1;          // item_prepare: the record's auxiliary chain is broken (STRK_E_INVALID for the call)

// the size constants of k_dbam_methyl (strk_methyl_constants hands them to the tests)
constexpr int kChunkBases = 16;        // bases a lane takes per sequence pass (8 packed bytes)
constexpr int kSeqPassBases = 64 * kChunkBases;
constexpr int kMmPassBytes = 64;       // bytes of the MM string per pass, one per lane
constexpr int kWindow = 2048;          // target ordinals per LDS window of a wave

// the auxiliary-chain walk (strk_aux.h), under the names this file uses
using strk_fe::aux_find;
using strk_fe::AuxWant;
using strk_fe::kAuxB;
using strk_fe::kAuxInt;
using strk_fe::kAuxInt32;
using strk_fe::kAuxZ;

// ---- what an item brings ----------------------------------------------------------------------------------------------------
struct Item {
    int64_t q_l, q_r;        // the tract [q_l, q_r) in positions of the stored SEQ
    const uint8_t* mm;       // the MM string (without its NUL) and the ML bytes; ml_count = 0 without ML
    int64_t mm_len;
    const uint8_t* ml;
    int64_t ml_count;
    char ml_sub;             // 'C' without ML
    bool reverse;
};

// The tract of an alignment: the bases strk_extract_reads returns as `tr` (the same one-pass walk, strk_fe::read_coords_linear).
// false: extraction would refuse the item, whatever its flank size, for a reason other than base quality.  Extraction cuts its
// flanks to flank_size before it asks whether they lie inside the record's bases, so an alignment that points past them is kept
// by a small flank size and refused by a large one; the test here is extraction's with a flank size of 0 (the four positions
// ordered, the tract inside the bases), which every item that extraction keeps with any flank size passes.
STRK_FE_HD bool tract_interval(const uint8_t* cigar, int32_t n_cigar, int64_t start, const int64_t* coords, int32_t l_seq, int64_t* q_l,
                               int64_t* q_r) {
    int64_t q[4];
    if (!strk_fe::read_coords_linear(cigar, n_cigar, start, coords[0], coords[1], coords[2], coords[3], q)) return false;
    if (q[0] < 0 || q[0] > q[1] || q[1] > q[2] || q[2] > q[3] || q[2] > l_seq) return false;
    *q_l = q[1]; *q_r = q[2];
    return true;
}

STRK_FE_HD bool has_hard_clip(const uint8_t* cigar, int32_t n_cigar) {
    for (int32_t i = 0; i < n_cigar; ++i)
        if ((strk_fe::rd_u32(cigar + 4 * (size_t)i) & 15u) == 5) return true;
    return false;
}

// Everything of an item that is one serial walk: the tract, the tags, the hard clips.  Returns kBadChain, the item's status
// (kNotSpanning, kNoTags, kClipped), or kOk with `it` filled: the MM grammar and the bases are the caller's.
// cig / n_cig / start: the alignment to walk (the record's own, its CG tag's, or the substitute one).
STRK_FE_HD int item_prepare(const uint8_t* buf, int64_t rec_off, const strk_fe::Rec& r, const uint8_t* cig, int32_t n_cig, int64_t start,
                            const int64_t* coords, Item* it) {
    const uint8_t* const end = buf + rec_off + 4 + strk_fe::rd_i32(buf + rec_off);
    const uint8_t* const aux = r.qual + r.l_seq;
    const AuxWant want[5] = {{'M', 'M', kAuxZ}, {'M', 'L', kAuxB}, {'M', 'm', kAuxZ}, {'M', 'l', kAuxB}, {'M', 'N', kAuxInt}};
    int64_t off[5], size[5], val[5];
    if (!aux_find(aux, (int64_t)(end - aux), want, 5, off, size, val)) return kBadChain;
    if (!tract_interval(cig, n_cig, start, coords, r.l_seq, &it->q_l, &it->q_r)) return kNotSpanning;
    const int k = (off[0] < 0 && off[1] < 0) ? 2 : 0;   // neither MM nor ML: Mm / Ml may stand in
    if (off[k] < 0) return kNoTags;
    if (has_hard_clip(r.cigar, r.n_cigar) || (off[4] >= 0 && val[4] != (int64_t)r.l_seq)) return kClipped;
    it->mm = aux + off[k];
    it->mm_len = size[k] - 1;
    it->ml = nullptr; it->ml_count = 0; it->ml_sub = 'C';
    if (off[k + 1] >= 0) {
        it->ml = aux + off[k + 1] + 5;
        it->ml_count = (int64_t)strk_fe::rd_u32(aux + off[k + 1] + 1);
        it->ml_sub = (char)aux[off[k + 1]];
    }
    it->reverse = (r.flag & 0x10) != 0;
    return kOk;
}

// ---- the MM string ------------------------------------------------------------------------------------------------------------
// Entries are separated by ';' (the last may be missing).  An entry: a base of ACGTUN, '+' or '-', one or more lower-case
// letters (each a code) or a decimal number (one code), an optional '.' or '?', then zero or more ",<1-10 digits, <= 2^31 - 1>".
struct Head {
    int32_t n_codes;
    int32_t j;          // index of the code 'm' among the letter codes of a C+ entry, -1: this entry is not taken
    char mode;          // '.', '?' or 0
    int64_t end;        // where the head ends: at a ',', a ';' or the end of the string
};

// The head of the entry that starts at mm[p] (p < len).  false: not of the grammar.
STRK_FE_HD bool parse_head(const uint8_t* mm, int64_t len, int64_t p, Head* h) {
    const uint8_t base = mm[p];
    if (!(base == 'A' || base == 'C' || base == 'G' || base == 'T' || base == 'U' || base == 'N')) return false;
    if (p + 1 >= len || (mm[p + 1] != '+' && mm[p + 1] != '-')) return false;
    const bool c_plus = base == 'C' && mm[p + 1] == '+';
    int64_t e = p + 2;
    h->n_codes = 0; h->j = -1; h->mode = 0;
    if (e < len && mm[e] >= 'a' && mm[e] <= 'z') {
        for (; e < len && mm[e] >= 'a' && mm[e] <= 'z'; ++e) {
            if (c_plus && mm[e] == 'm' && h->j < 0) h->j = h->n_codes;
            ++h->n_codes;
        }
    } else if (e < len && mm[e] >= '0' && mm[e] <= '9') {
        while (e < len && mm[e] >= '0' && mm[e] <= '9') ++e;
        h->n_codes = 1;
    } else {
        return false;
    }
    if (e < len && (mm[e] == '.' || mm[e] == '?')) h->mode = (char)mm[e++];
    if (e < len && mm[e] != ',' && mm[e] != ';') return false;
    h->end = e;
    return true;
}

// The number behind the ',' at mm[p]: its value, and where it ends (at a ',', a ';' or the end of the string).
STRK_FE_HD bool parse_number(const uint8_t* mm, int64_t len, int64_t p, int64_t* value, int64_t* end) {
    int64_t e = p + 1, v = 0;
    while (e < len && e - p <= 11 && mm[e] >= '0' && mm[e] <= '9') v = v * 10 + (mm[e++] - '0');
    const int64_t digits = e - p - 1;
    if (digits < 1 || digits > 10 || v > (int64_t)INT32_MAX) return false;
    if (e < len && mm[e] != ',' && mm[e] != ';') return false;
    *value = v; *end = e;
    return true;
}

// ---- bases ----------------------------------------------------------------------------------------------------------------------
// Chunk ch = the stored bases [16 ch, 16 ch + 16).  Bit i of *c / *g: base 16 ch + i is a C (code 2) / a G (code 4); bit 16 of
// *g: the first base of the next chunk is a G.  Positions at or past l_seq have no bit.
STRK_FE_HD void chunk_masks(const uint8_t* seq, int32_t l_seq, int64_t ch, uint32_t* c, uint32_t* g) {
    uint32_t cm = 0, gm = 0;
    const int64_t p0 = ch * kChunkBases;
    const int64_t n = (int64_t)l_seq - p0 < kChunkBases + 1 ? (int64_t)l_seq - p0 : kChunkBases + 1;
    for (int64_t i = 0; i < n; i += 2) {
        const uint8_t byte = seq[(p0 + i) >> 1];
        const uint32_t hi = byte >> 4, lo = byte & 15u;
        cm |= (uint32_t)(hi == 2) << i; gm |= (uint32_t)(hi == 4) << i;
        if (i + 1 < n) { cm |= (uint32_t)(lo == 2) << (i + 1); gm |= (uint32_t)(lo == 4) << (i + 1); }
    }
    *c = cm & 0xFFFFu; *g = gm & 0x1FFFFu;
}

STRK_FE_HD int popc32(uint32_t x) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __popc(x);
#else
    return __builtin_popcount(x);
#endif
}

// The sites of chunk ch: bit i = position p = 16 ch + i has q_l <= p < q_r, a C at p and a G at p + 1 (which exists).
STRK_FE_HD uint32_t chunk_sites(uint32_t c, uint32_t g, int64_t ch, int64_t q_l, int64_t q_r) {
    uint32_t m = c & (g >> 1);
    const int64_t p0 = ch * kChunkBases;
    if (q_l > p0) m &= q_l - p0 >= 16 ? 0u : ~0u << (q_l - p0);
    if (q_r < p0 + 16) m &= q_r <= p0 ? 0u : (1u << (q_r - p0)) - 1u;
    return m;
}

// The ordinal of the site at bit i of its chunk among the targets of the read as sequenced.  before = the targets of the stored
// bases in front of the chunk (Cs of a forward read, Gs of a reverse one), total = those of the whole SEQ.
STRK_FE_HD int64_t site_ordinal(bool reverse, uint32_t c, uint32_t g, int i, int64_t before, int64_t total) {
    if (!reverse) return before + popc32(c & ((1u << i) - 1u));        // the Cs in front of p
    return total - (before + popc32(g & ((1u << (i + 2)) - 1u)));      // the Gs behind p + 1 = all - those up to p + 1
}

// ---- inputs -------------------------------------------------------------------------------------------------------------------
struct Input {
    int64_t n_bytes;                 // size of the buffer the records lie in
    int32_t n_items;
    const int64_t* rec_off;
    const int64_t* coords;
    strk_fe::AltCigars alt;          // optional, as in strk_extract_reads
    int32_t threshold;
};

// Returns 0, or strk_groups::kInvalid and in `msg` what is wrong.
inline int check_input(const Input& in, strk_groups::Message* msg) {
    if (in.n_items < 0 || in.n_bytes < 0) return msg->invalid("n_items or n_bytes < 0");
    if (in.threshold < 0 || in.threshold > 255) return msg->invalid("threshold %d outside 0 .. 255", in.threshold);
    if (in.n_items == 0) return 0;
    if (!in.rec_off || !in.coords) return msg->invalid("NULL argument");
    if (strk_fe::check_alt(in.n_items, in.alt, msg)) return strk_groups::kInvalid;
    for (int32_t i = 0; i < in.n_items; ++i)
        if (in.rec_off[i] < 0 || in.rec_off[i] > in.n_bytes - 4) return msg->invalid("item %d: rec_off outside the buffer", i);
    return 0;
}

// ---- host twin ------------------------------------------------------------------------------------------------------------------
// One item of a checked call, one thread.  Returns the status (or kBadChain); sites / known / mc are zero unless it is kOk or
// kNoSites (which still has its sites).
inline int host_item(const uint8_t* buf, const Input& in, int32_t it, int32_t* sites, int32_t* known, int32_t* mc) {
    *sites = 0; *known = 0; *mc = 0;
    strk_fe::Rec r;
    int64_t next = 0;
    if (!strk_fe::parse_rec(buf, in.n_bytes, in.rec_off[it], &r, &next)) return kBadChain;
    const uint8_t* cig;
    int32_t n_cig;
    int64_t start;
    strk_fe::item_alignment(r, it, in.alt, &cig, &n_cig, &start);
    Item x;
    const int st = item_prepare(buf, in.rec_off[it], r, cig, n_cig, start, in.coords + 4 * (size_t)it, &x);
    if (st != kOk) return st;
    // the MM string: every entry for the grammar and for its share of ML, the numbers of the first C+m entry
    int64_t total = 0, t_off = 0;
    int32_t t_c = 0, t_j = 0;
    char t_mode = 0;
    bool found = false;
    std::vector<int64_t> ord;
    int64_t p = 0;
    while (p < x.mm_len) {
        Head h;
        if (!parse_head(x.mm, x.mm_len, p, &h)) return kMalformed;
        const bool take = !found && h.j >= 0;
        if (take) { found = true; t_off = total; t_c = h.n_codes; t_j = h.j; t_mode = h.mode; }
        int64_t e = h.end, o = -1;
        while (e < x.mm_len && x.mm[e] == ',') {
            int64_t d;
            if (!parse_number(x.mm, x.mm_len, e, &d, &e)) return kMalformed;
            total += h.n_codes;
            if (take) ord.push_back(o += d + 1);
        }
        p = e + 1;   // behind the ';' (or past the end)
    }
    if (x.ml_sub != 'C' || total != x.ml_count) return kMalformed;
    if (!found) return kNoTags;
    // the bases: the targets of the whole SEQ, then the sites of the tract's chunks
    const int64_t n_chunks = ((int64_t)r.l_seq + kChunkBases - 1) / kChunkBases;
    int64_t n_targets = 0;
    for (int64_t ch = 0; ch < n_chunks; ++ch) {
        uint32_t c, g;
        chunk_masks(r.seq, r.l_seq, ch, &c, &g);
        n_targets += popc32(x.reverse ? g & 0xFFFFu : c);
    }
    if (!ord.empty() && ord.back() >= n_targets) return kMalformed;
    int64_t before = 0;
    for (int64_t ch = 0; ch < n_chunks && ch * kChunkBases < x.q_r; ++ch) {
        uint32_t c, g;
        chunk_masks(r.seq, r.l_seq, ch, &c, &g);
        for (uint32_t m = (ch + 1) * kChunkBases > x.q_l ? chunk_sites(c, g, ch, x.q_l, x.q_r) : 0u; m; m &= m - 1) {
            const int64_t k = site_ordinal(x.reverse, c, g, __builtin_ctz(m), before, n_targets);
            const auto f = std::lower_bound(ord.begin(), ord.end(), k);
            ++*sites;
            if (f != ord.end() && *f == k) {
                ++*known;
                *mc += (int32_t)x.ml[t_off + (int64_t)(f - ord.begin()) * t_c + t_j] > in.threshold ? 1 : 0;
            } else if (t_mode != '?') {
                ++*known;
            }
        }
        before += popc32(x.reverse ? g & 0xFFFFu : c);
    }
    return *known > 0 ? kOk : kNoSites;
}

// Items [i0, i1) of a checked call.  Returns -1, or the first item of the slice whose record or auxiliary chain is malformed.
inline int32_t host_methyl(const uint8_t* buf, const Input& in, int32_t i0, int32_t i1, int32_t* out_status, int32_t* out_sites,
                           int32_t* out_known, int32_t* out_mc) {
    int32_t bad = -1;
    for (int32_t it = i0; it < i1; ++it) {
        const int st = host_item(buf, in, it, &out_sites[it], &out_known[it], &out_mc[it]);
        if (st == kBadChain && bad < 0) bad = it;
        out_status[it] = st == kBadChain ? kNotSpanning : st;
        if (st != kOk && st != kNoSites) out_sites[it] = 0;
    }
    return bad;
}

}  // namespace strk_me

#if defined(__HIPCC__)
namespace strk_me {

__device__ inline int64_t wave_scan_incl64(int64_t v, int lane) {
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int64_t o = (int64_t)__shfl_up((long long)v, d, 64);
        if (lane >= d) v += o;
    }
    return v;
}
__device__ inline int64_t wave_sum64(int64_t v) {
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) v += (int64_t)__shfl_xor((long long)v, d, 64);
    return v;
}
__device__ inline unsigned long long below(int lane) { return (1ull << lane) - 1ull; }   // the lanes in front of `lane` (lane < 64)

// One wave per item, four items per workgroup.  Every lane runs the item's serial walks (record, auxiliary chain, CIGAR: the
// item is wave-uniform, so these are scalar work), then the wave shares:
//   the MM string, 64 bytes per pass, lane i holding byte i: the lane at an entry's first byte scans its head, the lane at a
//     ',' its number (both read on past the pass where they must), ballots of the two give every entry its numbers, a wave
//     scan every entry the ML bytes in front of it;
//   the bases, 16 per lane and pass: a popcount of the target mask per lane, summed into the targets of the whole SEQ, of what
//     lies in front of the tract's first chunk and of the tract's chunks;
//   per window of kWindow ordinals of the tract: the taken entry's numbers once more (an inclusive scan of d + 1 with a carry
//     gives the ordinals, the walk resumes at the pass where the window before it ended) into the wave's LDS bytes (0 = no
//     call, 1 = a call, 2 = a call above the threshold), then the tract's chunks, each lane testing its sites against them.
// No floating point, no atomics but atomicMax(bad, INT32_MAX - item) for a broken record (the first such item wins); the counts
// are wave sums.
// item0: the first item of this launch (a call is cut into pieces of items).
__global__ void __launch_bounds__(256) k_dbam_methyl(const uint8_t* data, int64_t n_data, int item0, int item1, const int64_t* rec_off,
                                                     const int64_t* coords, strk_fe::AltCigars alt, int threshold, int32_t* out_status,
                                                     int32_t* out_sites, int32_t* out_known, int32_t* out_mc, int32_t* bad) {
    // win_mem[w] belongs to wave w alone: its lanes store bytes into it and other lanes of the SAME wave load them afterwards.  A
    // wave issues its LDS operations in order and the loops around them are wave-uniform (every lane is at the same store and at
    // the same load), so __threadfence_block(), which keeps the compiler and the memory counters from moving a load in front of a
    // store, is all the ordering there is and no barrier stands between them.  A window shared by several waves would need one.
    __shared__ uint32_t win_mem[4][kWindow / 4];
    const int lane = threadIdx.x & 63;
    const int it = __builtin_amdgcn_readfirstlane(item0 + (int)blockIdx.x * 4 + (int)(threadIdx.x >> 6));
    if (it >= item1) return;
    uint8_t* const win = reinterpret_cast<uint8_t*>(win_mem[threadIdx.x >> 6]);
    const auto finish = [&](int st, int32_t s, int32_t k, int32_t m) {
        if (lane == 0) { out_status[it] = st; out_sites[it] = s; out_known[it] = k; out_mc[it] = m; }
    };
    strk_fe::Rec r;
    int64_t next = 0;
    Item x;
    int st = kBadChain;
    if (strk_fe::parse_rec(data, n_data, rec_off[it], &r, &next)) {
        const uint8_t* cig;
        int32_t n_cig;
        int64_t start;
        strk_fe::item_alignment(r, it, alt, &cig, &n_cig, &start);
        st = item_prepare(data, rec_off[it], r, cig, n_cig, start, coords + 4 * (size_t)it, &x);
    }
    if (st == kBadChain) {
        if (lane == 0) atomicMax(bad, INT32_MAX - it);
        return finish(kNotSpanning, 0, 0, 0);
    }
    if (st != kOk) return finish(st, 0, 0, 0);

    // ---- the MM string: grammar, every entry's share of ML, the first C+m entry
    int64_t total = 0, t_off = 0, t_num = 0, t_sum = 0;   // t_sum: the sum of d + 1 over the taken entry's numbers
    int32_t cur_c = 0, t_c = 0, t_j = 0, t_mode = 0;
    bool found = false, open_taken = false, malformed = false;
    for (int64_t p0 = 0; p0 < x.mm_len; p0 += kMmPassBytes) {
        const int64_t p = p0 + lane;
        const bool in = p < x.mm_len;
        const uint8_t b = in ? x.mm[p] : (uint8_t)0;
        const bool is_start = in && (p == 0 || x.mm[p - 1] == ';'), is_comma = b == ',';
        Head h = {0, -1, 0, 0};
        int64_t d = 0, e = 0;
        bool ok = true;
        if (is_start) ok = parse_head(x.mm, x.mm_len, p, &h);
        if (is_comma) ok = parse_number(x.mm, x.mm_len, p, &d, &e);
        if (__any(!ok)) { malformed = true; break; }
        const unsigned long long starts = __ballot(is_start), commas = __ballot(is_comma);
        // the commas in front of the pass's first entry belong to the entry that was open when the pass began
        const unsigned long long head_part = starts ? below(__ffsll((long long)starts) - 1) : ~0ull;
        const int64_t n0 = __popcll(commas & head_part);
        const int64_t sum_d1 = wave_scan_incl64(is_comma ? d + 1 : 0, lane);   // (inclusive, over the pass)
        if (open_taken) t_sum += starts ? (int64_t)__shfl((long long)sum_d1, __ffsll((long long)starts) - 1, 64) : (int64_t)__shfl((long long)sum_d1, 63, 64);
        if (starts) open_taken = false;
        // a lane at an entry's first byte: the commas up to the next entry's first byte are its numbers (so far)
        const unsigned long long later = starts & ~below(lane) & ~(1ull << lane);
        const unsigned long long mine = later ? below(__ffsll((long long)later) - 1) & ~below(lane) : ~below(lane);
        const int64_t share = is_start ? (int64_t)__popcll(commas & mine) * h.n_codes : 0;
        const int64_t share_incl = wave_scan_incl64(share, lane);
        const unsigned long long takes = found ? 0ull : __ballot(is_start && h.j >= 0);
        if (takes) {
            const int f = __ffsll((long long)takes) - 1;
            found = true;
            t_off = total + n0 * cur_c + (int64_t)__shfl((long long)(share_incl - share), f, 64);
            t_c = __shfl(h.n_codes, f, 64); t_j = __shfl(h.j, f, 64); t_mode = __shfl((int)h.mode, f, 64);
            t_num = (int64_t)__shfl((long long)h.end, f, 64);
            // its numbers inside this pass: up to the next entry's first byte, or the pass's end (then it stays open)
            const unsigned long long after = starts & ~below(f) & ~(1ull << f);
            const int last = after ? __ffsll((long long)after) - 1 : 63;
            t_sum = (int64_t)__shfl((long long)sum_d1, last, 64) - (int64_t)__shfl((long long)sum_d1, f, 64);
            open_taken = !after;
        }
        total += n0 * cur_c + (int64_t)__shfl((long long)share_incl, 63, 64);
        if (starts) cur_c = __shfl(h.n_codes, 63 - __clzll((long long)starts), 64);
    }
    if (malformed || x.ml_sub != 'C' || total != x.ml_count) return finish(kMalformed, 0, 0, 0);
    if (!found) return finish(kNoTags, 0, 0, 0);

    // ---- the bases: targets of the whole SEQ, of what lies in front of the tract's first chunk, of the tract's chunks
    const int64_t n_chunks = ((int64_t)r.l_seq + kChunkBases - 1) / kChunkBases;
    const int64_t ch_lo = x.q_l / kChunkBases, ch_hi = x.q_r / kChunkBases;   // (ch_hi holds position q_r: the G of a last site)
    int64_t n_targets = 0, n_before = 0, n_tract = 0;
    for (int64_t ch = lane; ch < n_chunks; ch += 64) {
        uint32_t c, g;
        chunk_masks(r.seq, r.l_seq, ch, &c, &g);
        const int n = popc32(x.reverse ? g & 0xFFFFu : c);
        n_targets += n;
        if (ch < ch_lo) n_before += n;
        else if (ch <= ch_hi) n_tract += n;
    }
    n_targets = wave_sum64(n_targets); n_before = wave_sum64(n_before); n_tract = wave_sum64(n_tract);
    if (t_sum > 0 && t_sum - 1 >= n_targets) return finish(kMalformed, 0, 0, 0);   // (t_sum - 1 = the last ordinal)

    // ---- the windows of the tract's ordinals: [w_lo, w_lo + n_tract) holds every site's
    const int64_t w_lo = x.reverse ? n_targets - n_before - n_tract : n_before;
    const int64_t site_chunks_end = x.q_r > x.q_l ? (x.q_r - 1) / kChunkBases + 1 : ch_lo;   // one past the last chunk with a site
    int32_t n_sites = 0, n_known = 0, n_mc = 0;
    int64_t res_p0 = t_num, res_o = 0, res_t = 0;   // where the walk of the numbers resumes: a pass, the sum of d + 1 and the numbers before it
    for (int64_t w0 = w_lo; w0 < w_lo + n_tract && site_chunks_end > ch_lo; w0 += kWindow) {
        for (int k = lane; k < kWindow / 4; k += 64) win_mem[threadIdx.x >> 6][k] = 0u;
        __threadfence_block();
        bool res_set = false;
        int64_t car_o = res_o, car_t = res_t;
        for (int64_t p0 = res_p0; p0 < x.mm_len; p0 += kMmPassBytes) {
            const int64_t p = p0 + lane;
            const uint8_t b = p < x.mm_len ? x.mm[p] : (uint8_t)';';
            const unsigned long long ends = __ballot(b == ';');
            const unsigned long long live = ends ? below(__ffsll((long long)ends) - 1) : ~0ull;
            const bool is_comma = b == ',' && ((live >> lane) & 1ull);
            int64_t d = 0, e = 0;
            if (is_comma) (void)parse_number(x.mm, x.mm_len, p, &d, &e);   // (of the grammar: the first scan has seen it)
            const unsigned long long commas = __ballot(is_comma);
            const int64_t sum_d1 = wave_scan_incl64(is_comma ? d + 1 : 0, lane);
            const int64_t o = car_o + sum_d1 - 1, t = car_t + __popcll(commas & below(lane));
            if (is_comma && o >= w0 && o < w0 + kWindow)
                win[o - w0] = (int)x.ml[t_off + t * t_c + t_j] > threshold ? (uint8_t)2 : (uint8_t)1;
            const bool beyond = __any(is_comma && o >= w0 + kWindow);
            if (beyond && !res_set) { res_set = true; res_p0 = p0; res_o = car_o; res_t = car_t; }
            if (beyond || ends) break;
            car_o += (int64_t)__shfl((long long)sum_d1, 63, 64);
            car_t += __popcll(commas);
        }
        if (!res_set) res_p0 = x.mm_len;   // every number lies in front of the next window
        __threadfence_block();
        int64_t car = n_before;
        for (int64_t c0 = ch_lo; c0 < site_chunks_end; c0 += 64) {
            const int64_t ch = c0 + lane;
            uint32_t c = 0, g = 0;
            if (ch < site_chunks_end) chunk_masks(r.seq, r.l_seq, ch, &c, &g);
            const int n = popc32(x.reverse ? g & 0xFFFFu : c);
            const int64_t incl = wave_scan_incl64(n, lane);
            for (uint32_t m = ch < site_chunks_end ? chunk_sites(c, g, ch, x.q_l, x.q_r) : 0u; m; m &= m - 1) {
                const int64_t k = site_ordinal(x.reverse, c, g, __ffs((int)m) - 1, car + incl - n, n_targets);
                if (k < w0 || k >= w0 + kWindow) continue;
                const uint8_t v = win[k - w0];
                ++n_sites;
                n_known += (v || t_mode != '?') ? 1 : 0;
                n_mc += v == 2 ? 1 : 0;
            }
            car += (int64_t)__shfl((long long)incl, 63, 64);
        }
        __threadfence_block();
    }
    n_sites = (int32_t)wave_sum64(n_sites); n_known = (int32_t)wave_sum64(n_known); n_mc = (int32_t)wave_sum64(n_mc);
    finish(n_known > 0 ? kOk : kNoSites, n_sites, n_known, n_mc);
}

}  // namespace strk_me
#endif
