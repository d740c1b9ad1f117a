// strk_phase_check.h — what strk_call_alleles_phased decides before its first launch: the check of every input (the part it
// shares with strk_call_alleles is strk_alleles_check.h), and the cells and SNVs in front of every locus.  Nothing of HIP in
// here: the header compiles with the host compiler alone (tools/phase_asan.cpp runs it, and the piece cutter of strk_groups.h
// over its costs, under the sanitizers).
#pragma once

#include <vector>

#include "strk_alleles_check.h"

namespace strk_phase_check {

struct Limits {
    int max_reads, max_snvs, max_bootstrap, max_init;
};

struct Input : strk_alleles_check::Input {
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
    if (const int rc = strk_alleles_check::check(in, {lim.max_reads, lim.max_bootstrap, lim.max_init, 2}, msg)) return rc;
    if (!in.pp) return msg->invalid("params is NULL");
    if (in.n_loci == 0) return 0;
    const strk_phase_params* pp = in.pp;
    if (in.p->min_allele_reads < 1) return msg->invalid("min_allele_reads must be >= 1 (it is the min_reads of a group's call)");
    if (pp->min_hp_read_coverage < 0 || pp->snv_quality_threshold < 0 || pp->snv_quality_threshold > 255 || pp->many_snvs_quantity < 0)
        return msg->invalid("min_hp_read_coverage and many_snvs_quantity must be >= 0, snv_quality_threshold 0..255");
    if (!std::isfinite(pp->cn_weight_few) || !std::isfinite(pp->cn_weight_many) || pp->cn_weight_few < 0.0 || pp->cn_weight_many < 0.0)
        return msg->invalid("cn_weight_few and cn_weight_many must be finite and >= 0");
    if (pp->piece_loci < 0 || pp->ws_budget < 0) return msg->invalid("piece_loci and ws_budget must be >= 0 (0: the library's)");
    if ((in.hp == nullptr) != (in.ps == nullptr)) return msg->invalid("hp and ps must both be given or both be NULL");
    if (!in.snv_off && !in.snv_base && !in.snv_qual) return 0;
    if (!in.snv_off || !in.snv_base || !in.snv_qual) return msg->invalid("snv_off, snv_base and snv_qual must all be given or all be NULL");
    if (in.snv_off[0] != 0) return msg->invalid("snv_off[0] must be 0");
    if (in.n_snv_cells < 0) return msg->invalid("n_snv_cells < 0");
    cell_off.reserve((size_t)in.n_loci + 1);
    int64_t cells = 0;
    for (int32_t l = 0; l < in.n_loci; ++l) {
        const int64_t s = (int64_t)in.snv_off[l + 1] - in.snv_off[l];
        if (s < 0) return msg->invalid("locus %d: snv_off is decreasing", l);
        if (s > lim.max_snvs) return msg->invalid("locus %d: %lld SNVs (at most %d)", l, (long long)s, lim.max_snvs);
        cell_off.push_back(cells);
        cells += ((int64_t)in.read_off[l + 1] - in.read_off[l]) * s;
    }
    cell_off.push_back(cells);
    if (cells > in.n_snv_cells)
        return msg->invalid("snv_off and read_off imply %lld cells, snv_base and snv_qual hold %lld", (long long)cells, (long long)in.n_snv_cells);
    return 0;
}

}  // namespace strk_phase_check
