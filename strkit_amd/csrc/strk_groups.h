// strk_groups.h — the input that strk_best_representatives, strk_count_kmers and strk_consensus share: groups of byte strings
// addressed as group_off[G + 1], seq_start[S], seq_len[S] into one buffer of n_seq_bytes.  The view of it, the one function
// that checks it, and the rule by which a list is cut into pieces that fit a workspace (the same three calls and
// strk_call_alleles).  Nothing of HIP in here: the header compiles with the host compiler alone (tests/test_host.py drives the
// checker and the cutter over scripted cases).
#pragma once

#include <cstdarg>
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <vector>

namespace strk_groups {

constexpr int kInvalid = -22;   // = STRK_E_INVALID of include/strkit_amd.h (strk_api.hip asserts it)

// Group g owns sequences group_off[g] .. group_off[g + 1]; sequence i is seq_len[i] bytes at offset seq_start[i] of the buffer.
struct View {
    int32_t n_groups;
    const int32_t* group_off;
    int64_t n_seq_bytes;
    const int64_t* seq_start;
    const int32_t* seq_len;
};

struct Totals {
    int32_t n_seqs = 0;      // group_off[n_groups]
    int32_t max_len = 0;     // the longest sequence
    int64_t total_len = 0;   // the sum of the lengths
};

struct Message {   // room for the text of a refusal
    char text[256];
    int invalid(const char* fmt, ...) __attribute__((format(printf, 2, 3))) {
        va_list ap;
        va_start(ap, fmt);
        vsnprintf(text, sizeof text, fmt, ap);
        va_end(ap);
        return kInvalid;
    }
};

// Everything about a view that does not depend on the call: counts, the offsets' order, the groups' sizes, every slice
// inside the buffer.  Returns 0 and the totals, or kInvalid, no totals and in `msg` what is wrong (the caller puts the
// function's name in front).  A view of no groups is valid whatever its pointers are.
inline int check(const View& v, int max_group, int max_len, Totals* t, Message* msg) {
    *t = Totals{};
    if (v.n_groups < 0) return msg->invalid("n_groups < 0");
    if (v.n_seq_bytes < 0) return msg->invalid("n_seq_bytes < 0");
    if (v.n_groups == 0) return 0;
    if (!v.group_off) return msg->invalid("NULL argument");
    if (v.group_off[0] != 0) return msg->invalid("group_off[0] must be 0");
    for (int32_t g = 0; g < v.n_groups; ++g) {
        const int64_t n = (int64_t)v.group_off[g + 1] - v.group_off[g];
        if (n < 0) return msg->invalid("group %d: group_off is decreasing", g);
        if (n > max_group) return msg->invalid("group %d: %lld sequences (at most %d)", g, (long long)n, max_group);
    }
    Totals sum;
    sum.n_seqs = v.group_off[v.n_groups];
    if (sum.n_seqs > 0 && (!v.seq_start || !v.seq_len)) return msg->invalid("NULL argument");
    for (int32_t i = 0; i < sum.n_seqs; ++i) {
        const int32_t len = v.seq_len[i];
        const int64_t start = v.seq_start[i];
        if (len < 0 || len > max_len) return msg->invalid("sequence %d: length %d is outside 0..%d", i, len, max_len);
        if (start < 0 || start > v.n_seq_bytes - len)
            return msg->invalid("sequence %d: bytes %lld..%lld lie outside the %lld given", i, (long long)start,
                                (long long)(start + len), (long long)v.n_seq_bytes);
        if (len > sum.max_len) sum.max_len = len;
        sum.total_len += len;
    }
    *t = sum;
    return 0;
}

constexpr size_t kNoItemCap = ~(size_t)0;

// One piece of items p0 .. n of a list: items in order while their costs fit `budget`, at most max_items of them, and always
// at least one (an item beyond the budget runs alone).  Returns p1, the end of the piece; `off` holds the running sum of the
// costs in front of every item of the piece, *used their total.
template <class Cost>
size_t cut_piece(size_t p0, size_t n, Cost&& cost, int64_t budget, size_t max_items, std::vector<int64_t>& off, int64_t* used) {
    off.clear();
    *used = 0;
    size_t p1 = p0;
    while (p1 < n && p1 - p0 < max_items) {
        const int64_t c = cost(p1);
        if (p1 > p0 && *used + c > budget) break;
        off.push_back(*used);
        *used += c;
        ++p1;
    }
    return p1;
}

}  // namespace strk_groups
