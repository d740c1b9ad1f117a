// strk_phase_inputs.h — what the phased allele call (strk_call_alleles_phased, strk_phase.h) needs from an alignment file:
// per read its HP / PS tags, per read and candidate SNV position the base and quality under the read's alignment (a "cell"),
// per locus the choice of the useful SNVs and their cells packed read-major.  The walks are written once, for host and device
// (strk_bamrec.h's STRK_FE_HD); the host twins (strk_phase_cells, strk_useful_snvs) and the kernels (k_dbam_phase_cells,
// k_snv_useful, k_snv_gather) call the same functions.  Without HIP the header compiles with the host compiler alone
// (tools/phase_inputs_asan.cpp runs the walks and the checkers under the sanitizers).
//
// Reference: process_read_snvs_for_locus_and_calculate_useful_snvs and STRkitAlignedSegment.hp / .ps of strkit_rust_ext, which
// is not in the reference's tree: the rule is this project's own; its readable statement is
// strkit_amd/frontend/phase_inputs.py, and tests/test_phase_inputs_host.py holds the two together.
#pragma once
#include <math.h>
#include <stdint.h>

#include <vector>

#include "strk_bamrec.h"
#include "strk_groups.h"
#include "strk_aux.h"

namespace strk_pi {

constexpr int kMaxCand = 1024;   // candidate positions of a locus (the front end keeps the nearest 1 024)
constexpr int kMaxSnvs = 64;     // useful SNVs of a locus (the limit of k_phase_group)
constexpr int64_t kCellBudget = (int64_t)512 << 20;   // bytes of the device's cell workspace (base + quality), DESIGN.md §9

// ---- tags ---------------------------------------------------------------------------------------------------------------
// Walks the auxiliary fields aux[0 .. n_aux) of one record.  HP and PS count when their type is one of c C s S i I and the
// value fits an int32 (the first occurrence that counts); a read is tagged only with both, otherwise both come out -1.
// false: the chain runs past the end of the record (or holds a type the format does not know) — nothing outside
// aux[0 .. n_aux) is read in either case.  (The walk itself is strk_aux.h's aux_find.)
STRK_FE_HD bool aux_tags(const uint8_t* aux, int64_t n_aux, int32_t* hp, int32_t* ps) {
    *hp = -1; *ps = -1;
    const strk_fe::AuxWant want[2] = {{'H', 'P', strk_fe::kAuxInt32}, {'P', 'S', strk_fe::kAuxInt32}};
    int64_t off[2], size[2], val[2];
    if (!strk_fe::aux_find(aux, n_aux, want, 2, off, size, val)) return false;
    if (off[0] >= 0 && off[1] >= 0) { *hp = (int32_t)val[0]; *ps = (int32_t)val[1]; }
    return true;
}

// The auxiliary fields of a parsed record: from behind its qualities to the end of its block.
STRK_FE_HD bool rec_tags(const uint8_t* buf, int64_t rec_off, const strk_fe::Rec& r, int32_t* hp, int32_t* ps) {
    const uint8_t* const end = buf + rec_off + 4 + strk_fe::rd_i32(buf + rec_off);
    const uint8_t* const aux = r.qual + r.l_seq;
    return aux_tags(aux, (int64_t)(end - aux), hp, ps);
}

// ---- cells --------------------------------------------------------------------------------------------------------------
STRK_FE_HD void op_advance(uint32_t c, int64_t* dr, int64_t* dq) {
    const uint32_t op = c & 15u;
    const int64_t len = c >> 4;
    *dr = strk_fe::consumes_ref(op) ? len : 0;
    *dq = strk_fe::consumes_query(op) ? len : 0;
}

// first index k of the ascending a[0 .. n) with a[k] >= x
STRK_FE_HD int32_t lower_bound(const int64_t* a, int32_t n, int64_t x) {
    int32_t lo = 0, hi = n;
    while (lo < hi) {
        const int32_t mid = (lo + hi) >> 1;
        if (a[mid] < x) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

STRK_FE_HD int32_t clip_take_in(int32_t clip, int32_t clip_threshold, int32_t take_in) { return clip >= clip_threshold ? take_in : 0; }

// The cells of one CIGAR operation that starts at reference coordinate r0 and read position q0: the candidates inside
// [max(r0, lo), r0 + len).  An aligned operation writes the read's base and quality (a read position beyond the record's
// bases — a CIGAR longer than its sequence — writes nothing), a deletion '_'; every other operation leaves the pre-filled '-'.
STRK_FE_HD void op_cells(uint32_t c, int64_t r0, int64_t q0, int64_t lo, const int64_t* cand, int32_t n_cand, const strk_fe::Rec& r,
                         bool has_qual, uint8_t* base, uint8_t* qual) {
    const uint32_t op = c & 15u;
    const int64_t len = c >> 4;
    const bool aligned = strk_fe::is_aligned(op);
    if (len == 0 || !(aligned || op == 2)) return;
    const int32_t k1 = lower_bound(cand, n_cand, r0 + len);
    for (int32_t k = lower_bound(cand, n_cand, r0 > lo ? r0 : lo); k < k1; ++k) {
        if (!aligned) { base[k] = (uint8_t)'_'; qual[k] = 0; continue; }
        const int64_t qi = q0 + (cand[k] - r0);
        if (qi >= r.l_seq) continue;
        const uint8_t byte = r.seq[qi >> 1];
        base[k] = (uint8_t)"=ACMGRSVTWYHKDBN"[(qi & 1) ? (byte & 15) : (byte >> 4)];
        qual[k] = has_qual ? r.qual[qi] : (uint8_t)0;
    }
}

STRK_FE_HD void cigar_clips(const uint8_t* cigar, int32_t n_cigar, int32_t* clip_l, int32_t* clip_r) {
    *clip_l = 0; *clip_r = 0;
    if (n_cigar <= 0) return;
    const uint32_t c0 = strk_fe::rd_u32(cigar), c1 = strk_fe::rd_u32(cigar + 4 * (size_t)(n_cigar - 1));
    if ((c0 & 15u) == 4) *clip_l = (int32_t)(c0 >> 4);
    if ((c1 & 15u) == 4) *clip_r = (int32_t)(c1 >> 4);
}

// One item, one thread: the n_cand cells of an alignment (the host twin of a wave of k_dbam_phase_cells).
inline void item_cells(const strk_fe::Rec& r, const uint8_t* cigar, int32_t n_cigar, int64_t start, int32_t clip_threshold,
                       int32_t take_in, const int64_t* cand, int32_t n_cand, uint8_t* base, uint8_t* qual) {
    for (int32_t k = 0; k < n_cand; ++k) { base[k] = (uint8_t)'-'; qual[k] = 0; }
    const bool has_qual = !(r.l_seq > 0 && r.qual[0] == 0xFF);
    int32_t clip_l, clip_r;
    cigar_clips(cigar, n_cigar, &clip_l, &clip_r);
    int64_t ref = start, q = 0, lo = 0, e = 0;
    bool found = false;
    for (int32_t i = 0; i < n_cigar; ++i) {
        const uint32_t c = strk_fe::rd_u32(cigar + 4 * (size_t)i);
        int64_t dr, dq;
        op_advance(c, &dr, &dq);
        if (strk_fe::is_aligned(c & 15u) && (c >> 4) > 0) {
            if (!found) { found = true; lo = ref + clip_take_in(clip_l, clip_threshold, take_in); }
            e = ref + (int64_t)(c >> 4);
        }
        if (found) op_cells(c, ref, q, lo, cand, n_cand, r, has_qual, base, qual);
        ref += dr; q += dq;
    }
    if (!found) return;
    for (int32_t k = lower_bound(cand, n_cand, e - clip_take_in(clip_r, clip_threshold, take_in)); k < n_cand; ++k) { base[k] = (uint8_t)'-'; qual[k] = 0; }
}

// ---- useful SNVs --------------------------------------------------------------------------------------------------------
// a cell's byte -> its counter (the sixteen 4-bit base codes), -1 for '-' and '_'
STRK_FE_HD int code_of(uint8_t b) {
    switch (b) {
        case '=': return 0; case 'A': return 1; case 'C': return 2; case 'M': return 3; case 'G': return 4; case 'R': return 5;
        case 'S': return 6; case 'V': return 7; case 'T': return 8; case 'W': return 9; case 'Y': return 10; case 'H': return 11;
        case 'K': return 12; case 'D': return 13; case 'B': return 14; case 'N': return 15;
        default: return -1;
    }
}

// float64, round half to even: n = 10 gives t_thr 6, n = 30 gives 16
STRK_FE_HD void thresholds(int32_t n, int32_t min_allele_reads, int32_t* a_thr, int32_t* t_thr) {
    const int32_t a = (int32_t)rint((double)n / 5.0), t = (int32_t)rint((double)n * 0.55);
    *a_thr = a > min_allele_reads ? a : min_allele_reads;
    *t_thr = t > 5 ? t : 5;
}

STRK_FE_HD bool useful_counts(const uint32_t cnt[16], int32_t a_thr, int32_t t_thr) {
    uint32_t total = 0;
    int distinct = 0;
    for (int k = 0; k < 16; ++k) {
        total += cnt[k];
        distinct += cnt[k] >= (uint32_t)a_thr ? 1 : 0;
    }
    return distinct >= 2 && total >= (uint32_t)t_thr;
}

// ---- inputs ---------------------------------------------------------------------------------------------------------------
struct CellsInput {
    int64_t n_bytes;                 // size of the buffer the records lie in
    int32_t n_items;
    const int64_t* rec_off;
    const int32_t* item_locus;
    int32_t n_loci;
    const int32_t* cand_off;
    const int64_t* cand_pos;
    strk_fe::AltCigars alt;          // optional, as in strk_extract_reads
    int32_t clip_threshold, take_in;
};

// Returns 0, or strk_groups::kInvalid and in `msg` what is wrong.  cell_off (n_items + 1 entries) = the cells in front of every
// item: the sum of the candidates of the loci of the items before it.
inline int check_cells(const CellsInput& in, std::vector<int64_t>& cell_off, strk_groups::Message* msg) {
    cell_off.clear();
    if (in.n_items < 0 || in.n_loci < 0 || in.n_bytes < 0) return msg->invalid("n_items, n_loci or n_bytes < 0");
    if (in.clip_threshold < 0 || in.take_in < 0) return msg->invalid("clip_threshold and take_in must be >= 0");
    if (in.n_loci > 0 && (!in.cand_off || in.cand_off[0] != 0)) return msg->invalid("cand_off must be given and start at 0");
    for (int32_t l = 0; l < in.n_loci; ++l) {
        const int64_t n = (int64_t)in.cand_off[l + 1] - in.cand_off[l];
        if (n < 0) return msg->invalid("locus %d: cand_off is decreasing", l);
        if (n > kMaxCand) return msg->invalid("locus %d: %lld candidates (at most %d)", l, (long long)n, kMaxCand);
        if (n > 0 && !in.cand_pos) return msg->invalid("cand_pos is NULL");
        for (int32_t k = in.cand_off[l] + 1; k < in.cand_off[l + 1]; ++k)
            if (in.cand_pos[k] <= in.cand_pos[k - 1]) return msg->invalid("locus %d: candidates must be ascending and distinct", l);
    }
    cell_off.reserve((size_t)in.n_items + 1);
    cell_off.push_back(0);
    if (in.n_items == 0) return 0;
    if (!in.rec_off || !in.item_locus) return msg->invalid("NULL argument");
    if (strk_fe::check_alt(in.n_items, in.alt, msg)) return strk_groups::kInvalid;
    for (int32_t i = 0; i < in.n_items; ++i) {
        if (in.rec_off[i] < 0 || in.rec_off[i] > in.n_bytes - 4) return msg->invalid("item %d: rec_off outside the buffer", i);
        if (in.item_locus[i] < 0 || in.item_locus[i] >= in.n_loci) return msg->invalid("item %d: item_locus out of range", i);
        cell_off.push_back(cell_off.back() + (in.cand_off[in.item_locus[i] + 1] - in.cand_off[in.item_locus[i]]));
    }
    return 0;
}

struct UsefulInput {
    int32_t n_items;                 // the items of the cells call
    const int32_t* item_locus;
    int32_t n_loci;
    const int32_t* kept_off;
    const int32_t* kept_item;
    int32_t min_allele_reads;
};

inline int check_useful(const UsefulInput& in, strk_groups::Message* msg) {
    if (in.n_items < 0 || in.n_loci < 0) return msg->invalid("n_items or n_loci < 0");
    if (in.min_allele_reads < 1) return msg->invalid("min_allele_reads must be >= 1");
    if (in.n_loci == 0) return 0;
    if (!in.kept_off || in.kept_off[0] != 0) return msg->invalid("kept_off must be given and start at 0");
    for (int32_t l = 0; l < in.n_loci; ++l) {
        if (in.kept_off[l + 1] < in.kept_off[l]) return msg->invalid("locus %d: kept_off is decreasing", l);
        if (in.kept_off[l + 1] > in.kept_off[l] && (!in.kept_item || !in.item_locus)) return msg->invalid("NULL argument");
        for (int32_t k = in.kept_off[l]; k < in.kept_off[l + 1]; ++k) {
            const int32_t it = in.kept_item[k];
            if (it < 0 || it >= in.n_items) return msg->invalid("kept read %d: item out of range", k);
            if (in.item_locus[it] != l) return msg->invalid("kept read %d: item %d belongs to locus %d, not %d", k, it, in.item_locus[it], l);
        }
    }
    return 0;
}

// ---- host twins -------------------------------------------------------------------------------------------------------------
// Items [i0, i1) of a checked call.  Returns -1, or the first item whose record or auxiliary chain is malformed.
inline int32_t host_cells(const uint8_t* buf, const CellsInput& in, const int64_t* cell_off, int32_t i0, int32_t i1, int32_t* out_hp,
                          int32_t* out_ps, uint8_t* out_base, uint8_t* out_qual) {
    for (int32_t it = i0; it < i1; ++it) {
        strk_fe::Rec r;
        int64_t next = 0;
        out_hp[it] = -1; out_ps[it] = -1;
        if (!strk_fe::parse_rec(buf, in.n_bytes, in.rec_off[it], &r, &next)) return it;
        if (!rec_tags(buf, in.rec_off[it], r, &out_hp[it], &out_ps[it])) return it;
        const int32_t l = in.item_locus[it];
        const uint8_t* cig;
        int32_t n_cig;
        int64_t start;
        strk_fe::item_alignment(r, it, in.alt, &cig, &n_cig, &start);
        item_cells(r, cig, n_cig, start, in.clip_threshold, in.take_in, in.cand_pos + in.cand_off[l], in.cand_off[l + 1] - in.cand_off[l],
                   out_base + cell_off[it], out_qual + cell_off[it]);
    }
    return -1;
}

// The useful SNVs of locus l of a checked call: their candidate indices (ascending, at most kMaxSnvs) into sel; returns their number.
inline int32_t host_useful_locus(const UsefulInput& in, const int32_t* cand_off, const int64_t* cell_off, const uint8_t* cells_base, int32_t l,
                                 int32_t* sel) {
    const int32_t nc = cand_off[l + 1] - cand_off[l], k0 = in.kept_off[l], n = in.kept_off[l + 1] - k0;
    int32_t a_thr, t_thr, s = 0;
    thresholds(n, in.min_allele_reads, &a_thr, &t_thr);
    for (int32_t c = 0; c < nc && s < kMaxSnvs; ++c) {
        uint32_t cnt[16] = {0};
        for (int32_t r = 0; r < n; ++r) {
            const int code = code_of(cells_base[cell_off[in.kept_item[k0 + r]] + c]);
            if (code >= 0) ++cnt[code];
        }
        if (useful_counts(cnt, a_thr, t_thr)) sel[s++] = c;
    }
    return s;
}

}  // namespace strk_pi

#if defined(__HIPCC__)
namespace strk_pi {

__device__ inline int64_t wave_scan_incl(int64_t v, int lane) {
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int64_t o = (int64_t)__shfl_up((long long)v, d, 64);
        if (lane >= d) v += o;
    }
    return v;
}

// One wave per item, four items per workgroup.  The CIGAR is taken 64 operations per pass: lane i loads operation i, two
// inclusive wave scans and the totals of the passes before give it the operation's reference and read position, and the lane
// writes the cells of the candidates inside its operation (op_cells: two binary searches in the locus's sorted candidates).
// The cells are pre-filled with ('-', 0); what lies at or right of `hi` is put back to that once the last aligned pair is
// known.  A cell is stored up to three times, by different lanes of this wave: the pre-fill (lane k % 64), the cell itself (the
// lane that holds the operation) and the put-back (lane (k - first) % 64).  The first fence stands between the pre-fill and the
// cells, the second between the cells and the put-back: stores of one lane are ordered, those of different lanes to one address
// only across a fence.  Inside the loop no two lanes write one cell (operations cover disjoint reference ranges).  Lane 0 walks
// the auxiliary fields.
// item0: the first item of this launch (a call is cut into pieces of items).
__global__ void __launch_bounds__(256) k_dbam_phase_cells(const uint8_t* data, int64_t n_data, int item0, int item1, const int64_t* rec_off,
                                                          const int32_t* item_locus, const int32_t* cand_off, const int64_t* cand_pos,
                                                          const int64_t* cell_off, strk_fe::AltCigars alt, int clip_threshold, int take_in,
                                                          int32_t* hp, int32_t* ps, uint8_t* cells_base, uint8_t* cells_qual,
                                                          int32_t* bad) {
    const int lane = threadIdx.x & 63;
    const int it = item0 + blockIdx.x * 4 + (threadIdx.x >> 6);
    if (it >= item1) return;
    const int32_t l = item_locus[it];
    const int32_t n_cand = cand_off[l + 1] - cand_off[l];
    const int64_t* const cand = cand_pos + cand_off[l];
    uint8_t* const base = cells_base + cell_off[it];
    uint8_t* const qual = cells_qual + cell_off[it];
    for (int32_t k = lane; k < n_cand; k += 64) { base[k] = (uint8_t)'-'; qual[k] = 0; }
    strk_fe::Rec r;
    int64_t next = 0;
    const bool ok = strk_fe::parse_rec(data, n_data, rec_off[it], &r, &next);
    if (lane == 0) {
        int32_t h = -1, p = -1;
        if (!ok || !rec_tags(data, rec_off[it], r, &h, &p)) atomicMax(bad, INT32_MAX - it);
        hp[it] = h; ps[it] = p;
    }
    if (!ok) return;
    __threadfence_block();
    const uint8_t* cig;
    int32_t n_cig;
    int64_t car_r, car_q = 0;
    strk_fe::item_alignment(r, it, alt, &cig, &n_cig, &car_r);
    const bool has_qual = !(r.l_seq > 0 && r.qual[0] == 0xFF);
    int32_t clip_l, clip_r;
    cigar_clips(cig, n_cig, &clip_l, &clip_r);
    int64_t lo = 0, e = 0;
    bool found = false;
    for (int32_t i0 = 0; i0 < n_cig; i0 += 64) {
        const int32_t i = i0 + lane;
        const uint32_t c = i < n_cig ? strk_fe::rd_u32(cig + 4 * (size_t)i) : 0u;   // (0 = 0M: no advance, no cell)
        int64_t dr, dq;
        op_advance(c, &dr, &dq);
        const int64_t sr = wave_scan_incl(dr, lane), sq = wave_scan_incl(dq, lane);
        const int64_t r0 = car_r + sr - dr, q0 = car_q + sq - dq;
        const unsigned long long m = __ballot(strk_fe::is_aligned(c & 15u) && (c >> 4) > 0);
        if (m) {   // (the same for every lane)
            if (!found) {
                found = true;
                lo = (int64_t)__shfl((long long)r0, __ffsll((long long)m) - 1, 64) + clip_take_in(clip_l, clip_threshold, take_in);
            }
            e = (int64_t)__shfl((long long)(r0 + (int64_t)(c >> 4)), 63 - __clzll((long long)m), 64);
        }
        if (found) op_cells(c, r0, q0, lo, cand, n_cand, r, has_qual, base, qual);
        car_r += (int64_t)__shfl((long long)sr, 63, 64);
        car_q += (int64_t)__shfl((long long)sq, 63, 64);
    }
    if (!found) return;
    __threadfence_block();
    for (int32_t k = lower_bound(cand, n_cand, e - clip_take_in(clip_r, clip_threshold, take_in)) + lane; k < n_cand; k += 64) {
        base[k] = (uint8_t)'-';
        qual[k] = 0;
    }
}

// One workgroup per locus.  Thread t takes candidates t, t + 256, ...: it counts the bytes of the candidate's cells over the
// locus's kept reads in sixteen counters of its own in LDS (column t: no two threads share a bank line's word), tests the two
// thresholds, and the workgroup compacts the useful candidates in order (ballot + the waves' totals), the first 64.
__global__ void __launch_bounds__(256) k_snv_useful(const int32_t* cand_off, const int32_t* kept_off, const int32_t* kept_item,
                                                    const int64_t* cell_off, const uint8_t* cells_base, int min_allele_reads, int32_t* out_n,
                                                    int32_t* out_sel /* [n_loci][kMaxSnvs] */) {
    __shared__ uint32_t cnt[16][256];
    __shared__ int32_t wave_tot[4];
    const int l = blockIdx.x, t = threadIdx.x, lane = t & 63, w = t >> 6;
    const int32_t nc = cand_off[l + 1] - cand_off[l], k0 = kept_off[l], n = kept_off[l + 1] - k0;
    int32_t a_thr, t_thr, n_sel = 0;
    thresholds(n, min_allele_reads, &a_thr, &t_thr);
    for (int32_t c0 = 0; c0 < nc; c0 += 256) {
        const int32_t c = c0 + t;
        bool useful = false;
        if (c < nc) {
            for (int k = 0; k < 16; ++k) cnt[k][t] = 0;
            for (int32_t r = 0; r < n; ++r) {
                const int code = code_of(cells_base[cell_off[kept_item[k0 + r]] + c]);
                if (code >= 0) ++cnt[code][t];
            }
            uint32_t mine[16];
            for (int k = 0; k < 16; ++k) mine[k] = cnt[k][t];
            useful = useful_counts(mine, a_thr, t_thr);
        }
        const unsigned long long m = __ballot(useful);
        if (lane == 0) wave_tot[w] = __popcll(m);
        __syncthreads();
        int32_t pos = n_sel + __popcll(m & ((1ull << lane) - 1ull));
        for (int k = 0; k < w; ++k) pos += wave_tot[k];
        if (useful && pos < kMaxSnvs) out_sel[(size_t)l * kMaxSnvs + pos] = c;
        n_sel += wave_tot[0] + wave_tot[1] + wave_tot[2] + wave_tot[3];
        __syncthreads();
        if (n_sel >= kMaxSnvs) break;   // (the same for every thread) the first 64 are taken: the later candidates need no count
    }
    if (t == 0) out_n[l] = n_sel < kMaxSnvs ? n_sel : kMaxSnvs;
}

// The n x S cells of every locus into the packed read-major layout strk_call_alleles_phased takes (pack_off[l] = the cells of
// the loci before l: known only when every locus has chosen, hence a launch of its own).
__global__ void __launch_bounds__(256) k_snv_gather(const int32_t* kept_off, const int32_t* kept_item, const int64_t* cell_off,
                                                    const uint8_t* cells_base, const uint8_t* cells_qual, const int32_t* n_sel,
                                                    const int32_t* sel, const int64_t* pack_off, uint8_t* out_base, uint8_t* out_qual) {
    const int l = blockIdx.x;
    const int32_t k0 = kept_off[l], n = kept_off[l + 1] - k0, s = n_sel[l];
    for (int32_t idx = threadIdx.x; idx < n * s; idx += 256) {   // (s <= 64: n * s fits an int32 up to 33 million kept reads)
        const int64_t src = cell_off[kept_item[k0 + idx / s]] + sel[(size_t)l * kMaxSnvs + idx % s];
        out_base[pack_off[l] + idx] = cells_base[src];
        out_qual[pack_off[l] + idx] = cells_qual[src];
    }
}

}  // namespace strk_pi
#endif
