// strk_select.h — which of the records fetched for a locus are used: one record per read name, the skip flags, the read cap, and
// the reads that are chimeric in the region.  The rule once, for host and device (STRK_FE_HD, on strk_fe::parse_rec), the input
// check, the host twin and the two kernels.
//
// Reference: block_segments.get_segments_for_locus of strkit_rust_ext (not in the tree; call sites strkit/call/call_locus.py:
// 1044-1057,1277-1285, call_sample.py:86-87; --skip-supplementary / --skip-secondary entry.py:237-245; chimeric_in_region
// types.py:35-37).  The statement below is this project's own (unpinned, §2).
//
// One locus has items 0 .. n-1 (the overlapping mapped records, coordinate order, equal positions in file order).  A read name is
// the l_read_name - 1 bytes behind the fixed part of the record (none when l_read_name is 0); names are equal when their lengths
// and all their bytes are.  `rules`: 1 = skip supplementary, 2 = skip secondary, 4 = one record per name.
//   1. status of a name = OR over ALL items of that name at the locus of (flag & 0x800 ? 2 : 1), whatever becomes of them;
//   2. an item is flag-skipped with reason 1 when rules & 1 and flag & 0x800, else with reason 2 when rules & 2 and flag & 0x100;
//   3. with rules & 4, an item that is not flag-skipped is a duplicate (reason 3) when an earlier item of its name at the locus is
//      not flag-skipped either (a flag-skipped first occurrence shadows nothing);
//   4. of the items without a reason the first max_reads are kept (reason 0), the others get reason 4;
//   5. out: reason and status per item, the number kept per locus.  A kept read is chimeric in the region when its status is 3.
//
// The table.  Names are found through an open-addressing table of two slots per item (a power of two), a slot = {representative
// item, first item that is not flag-skipped, status}.  An item hashes its name, then walks the slots from there: atomicCAS on the
// representative claims an empty slot; a slot that is taken is the item's when the representative's name has the same BYTES
// (never the hash alone: no hash is kept), else the walk goes on.  Then atomicOr on the slot's status and, for an item that is
// not flag-skipped, atomicMin on its first item.
//
// Why the result does not depend on which thread wins a CAS: a slot is written once (empty -> an item) and never changes, so
// every item of a name walks past the same foreign names and ends in the one slot that holds its name: WHICH slot that is, and
// which item represents it, depends on the race; that all items of a name and no others meet in it does not.  What is read
// after the barrier is the OR and the minimum over exactly those items, and both are independent of order.  Which item is kept
// of a name is the minimum, not the CAS winner.  The cap is a prefix sum in item order.
#pragma once
#include <stdint.h>

#include <vector>

#include "strk_bamrec.h"
#include "strk_groups.h"

namespace strk_sel {

constexpr int kSmallItems = 1024;              // items of a locus that k_select_small takes (table in LDS)
constexpr int kSmallSlots = 2 * kSmallItems;   // its table
constexpr int kThreads = 256;                  // threads per workgroup, both kernels
constexpr int kCmpStep = 4;                    // bytes per step of the name compare

constexpr int kRuleSkipSupplementary = 1, kRuleSkipSecondary = 2, kRuleUnique = 4;
constexpr int kKept = 0, kSupplementary = 1, kSecondary = 2, kDuplicate = 3, kOverCap = 4;

constexpr uint32_t kNoItem = 0xFFFFFFFFu;      // a slot's first item while it has none
constexpr int kMaxLocusItems = 1 << 27;        // a slot number and a reason share one word (kWhyShift)
constexpr int kFixed = 36;                    // block_size + the fixed part of a record: what check_input wants inside the stream

STRK_FE_HD uint32_t name_status(int32_t flag) { return (flag & 0x800) ? 2u : 1u; }

STRK_FE_HD int flag_reason(int32_t flag, int32_t rules) {
    if ((rules & kRuleSkipSupplementary) && (flag & 0x800)) return kSupplementary;
    if ((rules & kRuleSkipSecondary) && (flag & 0x100)) return kSecondary;
    return kKept;
}

// the name of a record that parse_rec has accepted (its bytes lie inside the record)
struct Name {
    const uint8_t* p;
    int32_t len;
};
STRK_FE_HD Name name_of(const strk_fe::Rec& r) { return Name{r.name, r.l_name > 0 ? r.l_name - 1 : 0}; }
// ... of a record that parse_rec has accepted before: parsed again (the layout is stated once, in strk_bamrec.h)
STRK_FE_HD Name name_at(const uint8_t* buf, int64_t n_bytes, int64_t rec_off) {
    strk_fe::Rec r;
    int64_t next = 0;
    if (!strk_fe::parse_rec(buf, n_bytes, rec_off, &r, &next)) return Name{buf, 0};
    return name_of(r);
}

// where a name's walk through the table starts (FNV-1a and a last fold: the low bits are what the table uses)
STRK_FE_HD uint32_t name_hash(Name a) {
    uint32_t h = 2166136261u;
    for (int32_t i = 0; i < a.len; ++i) h = (h ^ a.p[i]) * 16777619u;
    return h ^ (h >> 15);
}

STRK_FE_HD bool names_equal(Name a, Name b) {
    if (a.len != b.len) return false;
    int32_t i = 0;
    for (; i + kCmpStep <= a.len; i += kCmpStep)      // (records lie at any address: rd_u32 reads bytes)
        if (strk_fe::rd_u32(a.p + i) != strk_fe::rd_u32(b.p + i)) return false;
    for (; i < a.len; ++i)
        if (a.p[i] != b.p[i]) return false;
    return true;
}

// slots of the table of a locus of n items: two per item, a power of two
STRK_FE_HD int64_t slots_for(int64_t n) {
    int64_t s = 2;
    while (s < 2 * n) s <<= 1;
    return s;
}

// ---- inputs ---------------------------------------------------------------------------------------------------------------------
struct Input {
    int64_t n_bytes;                 // size of the stream the records lie in
    int32_t n_loci;
    const int64_t* item_off;         // [n_loci + 1]
    const int64_t* rec_off;          // [item_off[n_loci]]
    int32_t rules, max_reads;
};

// Returns 0, or strk_groups::kInvalid and in `msg` what is wrong.  Afterwards every rec_off leaves room for a record's fixed
// part inside the stream; whether a record starts there is parse_rec's to say.
inline int check_input(const Input& in, strk_groups::Message* msg) {
    if (in.n_loci < 0 || in.n_bytes < 0) return msg->invalid("n_loci or n_bytes < 0");
    if (in.rules < 0 || in.rules > 7) return msg->invalid("rules %d outside 0 .. 7", in.rules);
    if (in.max_reads < 1) return msg->invalid("max_reads %d: must be >= 1", in.max_reads);
    if (!in.item_off) return msg->invalid("NULL argument");
    if (in.item_off[0] != 0) return msg->invalid("item_off must ascend from 0");
    for (int32_t l = 0; l < in.n_loci; ++l) {
        if (in.item_off[l + 1] < in.item_off[l]) return msg->invalid("locus %d: item_off must ascend from 0", l);
        if (in.item_off[l + 1] - in.item_off[l] > kMaxLocusItems)
            return msg->invalid("locus %d: %lld items (at most %d)", l, (long long)(in.item_off[l + 1] - in.item_off[l]), kMaxLocusItems);
    }
    const int64_t n = in.item_off[in.n_loci];
    if (n > INT32_MAX) return msg->invalid("%lld items (at most 2^31 - 1)", (long long)n);
    if (n > 0 && !in.rec_off) return msg->invalid("NULL argument");
    for (int64_t i = 0; i < n; ++i)
        if (in.rec_off[i] < 0 || in.rec_off[i] > in.n_bytes - kFixed)
            return msg->invalid("item %lld: record offset %lld outside the stream", (long long)i, (long long)in.rec_off[i]);
    return 0;
}

// ---- host twin ------------------------------------------------------------------------------------------------------------------
// The first item of [i0, i1) whose record parse_rec refuses, or -1.
inline int64_t host_first_bad(const uint8_t* buf, const Input& in, int64_t i0, int64_t i1) {
    for (int64_t i = i0; i < i1; ++i) {
        strk_fe::Rec r;
        int64_t next = 0;
        if (!strk_fe::parse_rec(buf, in.n_bytes, in.rec_off[i], &r, &next)) return i;
    }
    return -1;
}

struct HostTable {   // scratch of host_locus, kept between loci
    std::vector<int32_t> rep, slot_of;
    std::vector<uint32_t> first, status;
};

// One locus of a checked call whose records all parse: items in order, one thread.
inline void host_locus(const uint8_t* buf, const Input& in, int32_t l, HostTable& t, uint8_t* out_reason, uint8_t* out_status, int32_t* out_n_kept) {
    const int64_t i0 = in.item_off[l], n = in.item_off[l + 1] - i0;
    const int64_t slots = slots_for(n);
    t.rep.assign((size_t)slots, -1);
    t.first.assign((size_t)slots, kNoItem);
    t.status.assign((size_t)slots, 0u);
    t.slot_of.resize((size_t)n);
    for (int64_t i = 0; i < n; ++i) {
        strk_fe::Rec r;
        int64_t next = 0;
        (void)strk_fe::parse_rec(buf, in.n_bytes, in.rec_off[i0 + i], &r, &next);      // (accepted by the pre-pass)
        const Name a = name_of(r);
        const int32_t flag = r.flag;
        int64_t s = name_hash(a) & (uint32_t)(slots - 1);
        for (;; s = (s + 1) & (slots - 1)) {
            if (t.rep[(size_t)s] < 0) { t.rep[(size_t)s] = (int32_t)i; break; }
            if (names_equal(a, name_at(buf, in.n_bytes, in.rec_off[i0 + t.rep[(size_t)s]]))) break;
        }
        t.slot_of[(size_t)i] = (int32_t)s;
        t.status[(size_t)s] |= name_status(flag);
        const int why = flag_reason(flag, in.rules);
        out_reason[i0 + i] = (uint8_t)why;
        if (why == kKept && t.first[(size_t)s] == kNoItem) t.first[(size_t)s] = (uint32_t)i;
    }
    int64_t survivors = 0;
    for (int64_t i = 0; i < n; ++i) {
        const size_t s = (size_t)t.slot_of[(size_t)i];
        out_status[i0 + i] = (uint8_t)t.status[s];
        if (out_reason[i0 + i] != kKept) continue;
        if ((in.rules & kRuleUnique) && t.first[s] != (uint32_t)i) { out_reason[i0 + i] = kDuplicate; continue; }
        if (survivors++ >= in.max_reads) out_reason[i0 + i] = kOverCap;
    }
    out_n_kept[l] = (int32_t)(survivors < in.max_reads ? survivors : in.max_reads);
}

}  // namespace strk_sel

#if defined(__HIPCC__)
namespace strk_sel {

// What an item leaves for its own thread between the two passes: its slot, and its flag-skip reason in the top bits.
constexpr int kWhyShift = 28;
constexpr int32_t kBadItem = -1;

// One locus by one workgroup of kThreads.  rep / first / status: the table of `slots` slots (LDS or global memory), rep all -1,
// first all kNoItem, status all 0 on entry; slot_why: one int per item.  kGlobal: the table lies in global memory (its words are
// read back past the L1).  *bad: max over refused records of n_items_all - item.
template <bool kGlobal>
__device__ __forceinline__ void select_locus(const uint8_t* data, int64_t n_data, const int64_t* rec_off, int64_t item0, int32_t n,
                                             int32_t n_items_all, int32_t rules, int32_t max_reads, int32_t* rep, uint32_t* first,
                                             uint32_t* status, uint32_t slots, int32_t* slot_why, int32_t* wave_sum, uint8_t* out_reason,
                                             uint8_t* out_status, int32_t* out_n_kept, int32_t* bad) {
    const int tid = threadIdx.x;
    for (int32_t i = tid; i < n; i += kThreads) {
        const int64_t off = rec_off[item0 + i];
        strk_fe::Rec r;
        int64_t next = 0;
        if (!strk_fe::parse_rec(data, n_data, off, &r, &next)) {   // no byte of it is read further, it claims no slot
            atomicMax(bad, (int32_t)(n_items_all - (item0 + i)));
            slot_why[i] = kBadItem;
            continue;
        }
        const Name a = name_of(r);
        uint32_t s = name_hash(a) & (slots - 1);
        for (;; s = (s + 1) & (slots - 1)) {                        // (two slots per item: an empty one is always met)
            const int32_t owner = atomicCAS(&rep[s], -1, i);
            if (owner == -1 || owner == i) break;
            if (names_equal(a, name_at(data, n_data, rec_off[item0 + owner]))) break;   // (the owner parsed its record before it claimed)
        }
        const int why = flag_reason(r.flag, rules);
        atomicOr(&status[s], name_status(r.flag));
        if (why == kKept) atomicMin(&first[s], (uint32_t)i);
        slot_why[i] = (int32_t)s | (why << kWhyShift);
    }
    if (kGlobal) __threadfence();
    __syncthreads();
    // pass 2, a workgroup's worth of items at a time, in item order: duplicates, then the cap by a prefix sum over the survivors
    const int lane = tid & 63, wave = tid >> 6;
    int32_t carry = 0;
    for (int32_t c0 = 0; c0 < n; c0 += kThreads) {
        const int32_t i = c0 + tid;
        int why = kKept;
        uint32_t st = 0;
        bool survives = false;
        if (i < n && slot_why[i] != kBadItem) {
            const uint32_t s = (uint32_t)slot_why[i] & ((1u << kWhyShift) - 1u);
            why = slot_why[i] >> kWhyShift;
            uint32_t f;
            if (kGlobal) {
                st = __hip_atomic_load(&status[s], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                f = __hip_atomic_load(&first[s], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            } else {
                st = status[s];
                f = first[s];
            }
            if (why == kKept && (rules & kRuleUnique) && f != (uint32_t)i) why = kDuplicate;
            survives = why == kKept;
        }
        const unsigned long long votes = __ballot(survives);
        if (lane == 0) wave_sum[wave] = __popcll(votes);
        __syncthreads();
        int32_t before = carry, total = 0;
        for (int w = 0; w < kThreads / 64; ++w) {
            if (w < wave) before += wave_sum[w];
            total += wave_sum[w];
        }
        if (i < n) {
            const int32_t rank = before + __popcll(votes & ((1ull << lane) - 1ull));
            if (survives && rank >= max_reads) why = kOverCap;
            out_reason[item0 + i] = (uint8_t)why;
            out_status[item0 + i] = (uint8_t)st;
        }
        carry += total;
        __syncthreads();
    }
    if (tid == 0) *out_n_kept = carry < max_reads ? carry : max_reads;
}

// One workgroup per locus of `loci` (each of at most kSmallItems items): the table in LDS.
__global__ void __launch_bounds__(kThreads) k_select_small(const uint8_t* data, int64_t n_data, const int32_t* loci, const int64_t* item_off,
                                                           const int64_t* rec_off, int32_t n_items_all, int32_t rules, int32_t max_reads,
                                                           uint8_t* out_reason, uint8_t* out_status, int32_t* out_n_kept, int32_t* bad) {
    __shared__ int32_t rep[kSmallSlots];
    __shared__ uint32_t first[kSmallSlots], status[kSmallSlots];
    __shared__ int32_t slot_why[kSmallItems];
    __shared__ int32_t wave_sum[kThreads / 64];
    const int32_t l = loci[blockIdx.x];
    const int64_t item0 = item_off[l];
    const int64_t n64 = item_off[l + 1] - item0;
    const int32_t n = (int32_t)(n64 < kSmallItems ? n64 : kSmallItems);   // (the host sorts larger loci into the other launch)
    const uint32_t slots = (uint32_t)slots_for(n);
    for (uint32_t s = threadIdx.x; s < slots; s += kThreads) { rep[s] = -1; first[s] = kNoItem; status[s] = 0u; }
    __syncthreads();
    select_locus<false>(data, n_data, rec_off, item0, n, n_items_all, rules, max_reads, rep, first, status, slots, slot_why, wave_sum,
                        out_reason, out_status, out_n_kept + l, bad);
}

// One workgroup per locus of `loci`, of any size: locus k's table of slots_for(n) slots starts at slot table_off[k] of the
// workspace (rep | first, both 0xFF bytes on entry, and status, zero on entry: memsets on the stream), slot_why at its items.
__global__ void __launch_bounds__(kThreads) k_select_large(const uint8_t* data, int64_t n_data, const int32_t* loci, const int64_t* table_off,
                                                           const int64_t* item_off, const int64_t* rec_off, int32_t n_items_all, int32_t rules,
                                                           int32_t max_reads, int32_t* ws_rep, uint32_t* ws_first, uint32_t* ws_status,
                                                           int32_t* ws_slot_why, uint8_t* out_reason, uint8_t* out_status,
                                                           int32_t* out_n_kept, int32_t* bad) {
    __shared__ int32_t wave_sum[kThreads / 64];
    const int32_t l = loci[blockIdx.x];
    const int64_t item0 = item_off[l], t0 = table_off[blockIdx.x];
    const int32_t n = (int32_t)(item_off[l + 1] - item0);
    select_locus<true>(data, n_data, rec_off, item0, n, n_items_all, rules, max_reads, ws_rep + t0, ws_first + t0, ws_status + t0,
                       (uint32_t)slots_for(n), ws_slot_why + item0, wave_sum, out_reason, out_status, out_n_kept + l, bad);
}

}  // namespace strk_sel
#endif
