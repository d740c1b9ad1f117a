// strk_alleles_check.h — the input that strk_call_alleles, strk_call_alleles_n and strk_call_alleles_phased share (loci as
// read_off[L + 1] over cn / w, n_alleles and seed per locus, one strk_allele_params) and the one check of it.  Nothing of HIP
// in here: the header compiles with the host compiler alone (tools/phase_asan.cpp and tools/alleles_n_asan.cpp drive it;
// tests/test_host.py and tests/test_alleles_n_host.py build and run those programs).
#pragma once

#include <cmath>
#include <cstdint>

#include "../../include/strkit_amd.h"
#include "strk_groups.h"

namespace strk_alleles_check {

struct Input {
    int32_t n_loci;
    const int32_t* read_off;
    const int32_t* cn;
    const double* w;
    const int32_t* n_alleles;
    const uint64_t* seed;
    const strk_allele_params* p;
};

struct Limits {
    int max_reads, max_bootstrap, max_init, max_alleles;
};

// Returns 0, or strk_groups::kInvalid and in `msg` what is wrong (the caller puts the function's name in front): the rule's
// parameters, then every locus (its reads in order and at most max_reads, 1 .. max_alleles alleles, every weight finite and > 0).
// A call of no loci is valid whatever its arrays are, but not without its parameters.  min_allele_reads is not looked at:
// only the phased call needs it >= 1 (strk_phase_check.h).
inline int check(const Input& in, const Limits& lim, strk_groups::Message* msg) {
    if (in.n_loci < 0) return msg->invalid("n_loci < 0");
    if (!in.p) return msg->invalid("params is NULL");
    if (in.n_loci == 0) return 0;
    if (!in.read_off || !in.cn || !in.w || !in.n_alleles || !in.seed) return msg->invalid("NULL argument");
    const strk_allele_params* p = in.p;
    if (p->num_bootstrap < 2 || p->num_bootstrap > lim.max_bootstrap)
        return msg->invalid("num_bootstrap %d is outside 2..%d", p->num_bootstrap, lim.max_bootstrap);
    if (p->n_init < 1 || p->n_init > lim.max_init) return msg->invalid("n_init %d is outside 1..%d", p->n_init, lim.max_init);
    if (p->min_reads < 1) return msg->invalid("min_reads must be >= 1");
    if (p->max_iter < 1) return msg->invalid("max_iter must be >= 1");
    if (p->filter_factor < 1) return msg->invalid("filter_factor must be >= 1");
    // reg_covar > 0: without it a component that collapses onto one value gets a variance of 0 (or a rounding below 0)
    // and its precision is inf / NaN
    if (!(p->tol >= 0.0) || !(p->reg_covar > 0.0) || !std::isfinite(p->tol) || !std::isfinite(p->reg_covar) ||
        !std::isfinite(p->expansion_ratio))
        return msg->invalid("tol must be finite and >= 0, reg_covar finite and > 0, expansion_ratio finite");
    if (in.read_off[0] != 0) return msg->invalid("read_off[0] must be 0");
    for (int32_t l = 0; l < in.n_loci; ++l) {
        const int64_t n = (int64_t)in.read_off[l + 1] - in.read_off[l];
        if (n < 0) return msg->invalid("locus %d: read_off is decreasing", l);
        if (n > lim.max_reads) return msg->invalid("locus %d: %lld reads (at most %d)", l, (long long)n, lim.max_reads);
        if (in.n_alleles[l] < 1 || in.n_alleles[l] > lim.max_alleles)
            return lim.max_alleles == 2 ? msg->invalid("locus %d: n_alleles %d is not 1 or 2", l, in.n_alleles[l])
                                        : msg->invalid("locus %d: n_alleles %d is outside 1..%d", l, in.n_alleles[l], lim.max_alleles);
        for (int32_t r = in.read_off[l]; r < in.read_off[l + 1]; ++r)
            if (!std::isfinite(in.w[r]) || !(in.w[r] > 0.0)) return msg->invalid("locus %d: read %d has weight %g", l, r, in.w[r]);
    }
    return 0;
}

}  // namespace strk_alleles_check
