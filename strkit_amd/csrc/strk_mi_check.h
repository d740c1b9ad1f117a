// strk_mi_check.h — the input that strk_mi_trio and strk_mi_trio_host share, and the one check of it.  Nothing of HIP in
// here: the header compiles with the host compiler alone (tools/mi_asan.cpp drives it; tests/test_mi_tool.py builds and runs
// that program).
#pragma once

#include <cstdint>

#include "../../include/strkit_amd.h"
#include "strk_groups.h"

namespace strk_mi_check {

struct Input {
    int32_t n_loci;
    const int64_t* grp_off;   // [6 n + 1]
    const int32_t* cn;
    int64_t n_cn;
    const int32_t *gt, *ci95, *ci99, *seq_id, *seq_len;
    const strk_mi_params* p;
};

// Returns 0, or strk_groups::kInvalid and in `msg` what is wrong (the caller puts the function's name in front): the
// parameters, then every locus.  A call of no loci is valid whatever its arrays are, but not without its parameters.
inline int check(const Input& in, int max_group, strk_groups::Message* msg) {
    if (in.n_loci < 0) return msg->invalid("n_loci < 0");
    if (!in.p) return msg->invalid("params is NULL");
    const strk_mi_params* p = in.p;
    if (p->test < STRK_MI_TEST_NONE || p->test > STRK_MI_TEST_WMW_GT) return msg->invalid("test %d is outside 0..3", p->test);
    if (!(p->sig_level > 0.0) || !(p->sig_level < 1.0)) return msg->invalid("sig_level %g is outside (0, 1)", p->sig_level);
    if (!(p->widen >= 0.0) || p->widen > 1e300) return msg->invalid("widen %g must be finite and >= 0", p->widen);
    if (p->piece_loci < 0 || p->ws_budget < 0) return msg->invalid("piece_loci and ws_budget must be >= 0");
    if (in.n_loci == 0) return 0;
    if (!in.gt || !in.ci95) return msg->invalid("NULL argument");
    if (in.seq_id && !in.seq_len) return msg->invalid("seq_id is given without seq_len");
    if (in.seq_len && !in.seq_id) return msg->invalid("seq_len is given without seq_id");
    const bool reads = p->test != STRK_MI_TEST_NONE;
    if (reads) {
        if (!in.grp_off || in.n_cn < 0 || (in.n_cn > 0 && !in.cn)) return msg->invalid("NULL argument");
        if (in.grp_off[0] != 0) return msg->invalid("grp_off[0] must be 0");
    }
    for (int32_t l = 0; l < in.n_loci; ++l) {
        for (int k = 0; k < 6; ++k) {
            const int32_t *a = in.ci95 + 12 * (size_t)l + 2 * k, *b = in.ci99 ? in.ci99 + 12 * (size_t)l + 2 * k : nullptr;
            if (a[0] > a[1]) return msg->invalid("locus %d: ci95 of allele %d has its lower bound %d above its upper bound %d", l, k, a[0], a[1]);
            if (b && b[0] > b[1]) return msg->invalid("locus %d: ci99 of allele %d has its lower bound %d above its upper bound %d", l, k, b[0], b[1]);
        }
        if (!reads) continue;
        for (int g = 0; g < 6; ++g) {
            const int64_t r0 = in.grp_off[6 * (size_t)l + g], r1 = in.grp_off[6 * (size_t)l + g + 1];
            if (r1 < r0) return msg->invalid("locus %d: grp_off is decreasing at group %d", l, g);
            if (r1 > in.n_cn) return msg->invalid("locus %d: group %d ends at read %lld of %lld", l, g, (long long)r1, (long long)in.n_cn);
            if (r1 - r0 > max_group) return msg->invalid("locus %d: group %d has %lld reads (at most %d)", l, g, (long long)(r1 - r0), max_group);
            for (int64_t r = r0; r < r1; ++r)
                if (in.cn[r] < 0) return msg->invalid("locus %d: read %lld has the copy number %d", l, (long long)r, in.cn[r]);
        }
    }
    return 0;
}

}  // namespace strk_mi_check
