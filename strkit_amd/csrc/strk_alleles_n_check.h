// strk_alleles_n_check.h — the check of strk_call_alleles_n's input: that of strk_call_alleles (strk_alleles_check.h, whose
// Input and Limits it takes) with one to max_alleles alleles per locus.  Nothing of HIP in here: the header compiles with the
// host compiler alone (tools/alleles_n_asan.cpp drives it).
#pragma once

#include "strk_alleles_check.h"

namespace strk_alleles_n_check {

// Returns 0, or strk_groups::kInvalid and in `msg` what is wrong.  The rule's parameters are checked by
// strk_alleles_check::check itself (on a call of one empty locus); the loci are then walked as there, in the same words,
// except that a count outside 1..max_alleles is what is refused, by locus and value.
inline int check(const strk_alleles_check::Input& in, const strk_alleles_check::Limits& lim, int max_alleles,
                 strk_groups::Message* msg) {
    if (in.n_loci < 0) return msg->invalid("n_loci < 0");
    if (!in.p) return msg->invalid("params is NULL");
    if (in.n_loci == 0) return 0;
    if (!in.read_off || !in.cn || !in.w || !in.n_alleles || !in.seed) return msg->invalid("NULL argument");
    // the parameters and read_off[0]: a call of one locus without reads
    static const int32_t kNoReads[2] = {0, 0}, kOne = 1;
    strk_alleles_check::Input head = in;
    head.n_loci = 1;
    head.read_off = kNoReads;
    head.n_alleles = &kOne;
    if (const int rc = strk_alleles_check::check(head, lim, msg)) return rc;
    if (in.read_off[0] != 0) return msg->invalid("read_off[0] must be 0");
    for (int32_t l = 0; l < in.n_loci; ++l) {
        const int64_t n = (int64_t)in.read_off[l + 1] - in.read_off[l];
        if (n < 0) return msg->invalid("locus %d: read_off is decreasing", l);
        if (n > lim.max_reads) return msg->invalid("locus %d: %lld reads (at most %d)", l, (long long)n, lim.max_reads);
        if (in.n_alleles[l] < 1 || in.n_alleles[l] > max_alleles)
            return msg->invalid("locus %d: n_alleles %d is outside 1..%d", l, in.n_alleles[l], max_alleles);
        for (int32_t r = in.read_off[l]; r < in.read_off[l + 1]; ++r)
            if (!std::isfinite(in.w[r]) || !(in.w[r] > 0.0)) return msg->invalid("locus %d: read %d has weight %g", l, r, in.w[r]);
    }
    return 0;
}

}  // namespace strk_alleles_n_check
