// strk_phase_check.h — what strk_call_alleles_phased decides before its first launch: the check of every input, and the
// cells and SNVs in front of every locus.  Nothing of HIP in here: the header compiles with the host compiler alone
// (tools/phase_asan.cpp runs it, and the piece cutter of strk_groups.h over its costs, under the sanitizers).
#pragma once

#include <cmath>
#include <cstdint>
#include <vector>

#include "../../include/strkit_amd.h"
#include "strk_groups.h"

namespace strk_phase_check {

struct Limits {
    int max_reads, max_snvs, max_bootstrap, max_init;
};

struct Input {
    int32_t n_loci;
    const int32_t* read_off;
    const int32_t* cn;
    const double* w;
    const int32_t* n_alleles;
    const uint64_t* seed;
    const strk_allele_params* p;
    const strk_phase_params* pp;
    const int32_t *hp, *ps;
    const int32_t* snv_off;
    int64_t n_snv_cells;
    const uint8_t *snv_base, *snv_qual;
};

// Returns 0, or strk_groups::kInvalid and in `msg` what is wrong.  cell_off[l] (n_loci + 1 entries, filled when the call has
// SNVs) is the number of cells in front of locus l: the sum of reads x SNVs of the loci before it.
inline int check(const Input& in, const Limits& lim, std::vector<int64_t>& cell_off, strk_groups::Message* msg) {
    cell_off.clear();
    if (in.n_loci < 0) return msg->invalid("n_loci < 0");
    if (!in.p || !in.pp) return msg->invalid("params is NULL");
    if (in.n_loci == 0) return 0;
    if (!in.read_off || !in.cn || !in.w || !in.n_alleles || !in.seed) return msg->invalid("NULL argument");
    const strk_allele_params* p = in.p;
    const strk_phase_params* pp = in.pp;
    if (p->num_bootstrap < 2 || p->num_bootstrap > lim.max_bootstrap)
        return msg->invalid("num_bootstrap %d is outside 2..%d", p->num_bootstrap, lim.max_bootstrap);
    if (p->n_init < 1 || p->n_init > lim.max_init) return msg->invalid("n_init %d is outside 1..%d", p->n_init, lim.max_init);
    if (p->min_reads < 1) return msg->invalid("min_reads must be >= 1");
    if (p->min_allele_reads < 1) return msg->invalid("min_allele_reads must be >= 1 (it is the min_reads of a group's call)");
    if (p->max_iter < 1) return msg->invalid("max_iter must be >= 1");
    if (p->filter_factor < 1) return msg->invalid("filter_factor must be >= 1");
    if (!(p->tol >= 0.0) || !(p->reg_covar > 0.0) || !std::isfinite(p->tol) || !std::isfinite(p->reg_covar) ||
        !std::isfinite(p->expansion_ratio))
        return msg->invalid("tol must be finite and >= 0, reg_covar finite and > 0, expansion_ratio finite");
    if (pp->min_hp_read_coverage < 0 || pp->snv_quality_threshold < 0 || pp->snv_quality_threshold > 255 || pp->many_snvs_quantity < 0)
        return msg->invalid("min_hp_read_coverage and many_snvs_quantity must be >= 0, snv_quality_threshold 0..255");
    if (!std::isfinite(pp->cn_weight_few) || !std::isfinite(pp->cn_weight_many) || pp->cn_weight_few < 0.0 || pp->cn_weight_many < 0.0)
        return msg->invalid("cn_weight_few and cn_weight_many must be finite and >= 0");
    if (pp->piece_loci < 0 || pp->ws_budget < 0) return msg->invalid("piece_loci and ws_budget must be >= 0 (0: the library's)");
    if ((in.hp == nullptr) != (in.ps == nullptr)) return msg->invalid("hp and ps must both be given or both be NULL");
    const bool snvs = in.snv_off || in.snv_base || in.snv_qual;
    if (snvs && (!in.snv_off || !in.snv_base || !in.snv_qual)) return msg->invalid("snv_off, snv_base and snv_qual must all be given or all be NULL");
    if (in.read_off[0] != 0) return msg->invalid("read_off[0] must be 0");
    if (snvs && in.snv_off[0] != 0) return msg->invalid("snv_off[0] must be 0");
    if (snvs && in.n_snv_cells < 0) return msg->invalid("n_snv_cells < 0");
    if (snvs) cell_off.reserve((size_t)in.n_loci + 1);
    int64_t cells = 0;
    for (int32_t l = 0; l < in.n_loci; ++l) {
        const int64_t n = (int64_t)in.read_off[l + 1] - in.read_off[l];
        if (n < 0) return msg->invalid("locus %d: read_off is decreasing", l);
        if (n > lim.max_reads) return msg->invalid("locus %d: %lld reads (at most %d)", l, (long long)n, lim.max_reads);
        if (in.n_alleles[l] != 1 && in.n_alleles[l] != 2) return msg->invalid("locus %d: n_alleles %d is not 1 or 2", l, in.n_alleles[l]);
        for (int32_t r = in.read_off[l]; r < in.read_off[l + 1]; ++r)
            if (!std::isfinite(in.w[r]) || !(in.w[r] > 0.0)) return msg->invalid("locus %d: read %d has weight %g", l, r, in.w[r]);
        if (snvs) {
            const int64_t s = (int64_t)in.snv_off[l + 1] - in.snv_off[l];
            if (s < 0) return msg->invalid("locus %d: snv_off is decreasing", l);
            if (s > lim.max_snvs) return msg->invalid("locus %d: %lld SNVs (at most %d)", l, (long long)s, lim.max_snvs);
            cell_off.push_back(cells);
            cells += n * s;
        }
    }
    if (snvs) {
        cell_off.push_back(cells);
        if (cells > in.n_snv_cells)
            return msg->invalid("snv_off and read_off imply %lld cells, snv_base and snv_qual hold %lld", (long long)cells, (long long)in.n_snv_cells);
    }
    return 0;
}

}  // namespace strk_phase_check
