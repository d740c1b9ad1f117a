// strk_phase_inputs.inc — the inputs of the phased allele call read from an alignment file (part of strk_api.hip, after
// strk_dbam.inc): strk_phase_cells / strk_useful_snvs over a host buffer (NativeBam, the regions of an IndexedBam) and
// strk_dbam_phase_cells / strk_dbam_useful_snvs over the file resident on the device.  The rule, the walks, the input checks and
// the kernels are strk_phase_inputs.h; here are the threads, the buffers and the launches.

namespace {

// snv_off and the packed offsets from the loci's choices; returns the number of packed cells
int64_t pi_offsets(int32_t n_loci, const int32_t* kept_off, const int32_t* n_sel, int32_t* snv_off, std::vector<int64_t>& pack_off) {
    pack_off.assign((size_t)n_loci + 1, 0);
    snv_off[0] = 0;
    for (int32_t l = 0; l < n_loci; ++l) {
        snv_off[l + 1] = snv_off[l] + n_sel[l];
        pack_off[(size_t)l + 1] = pack_off[(size_t)l] + (int64_t)(kept_off[l + 1] - kept_off[l]) * n_sel[l];
    }
    return pack_off[(size_t)n_loci];
}

}  // namespace

extern "C" {

int strk_phase_cells(const uint8_t* buf, int64_t n_bytes, int32_t n_items, const int64_t* rec_off, const int32_t* item_locus,
                     int32_t n_loci, const int32_t* cand_off, const int64_t* cand_pos, const uint32_t* alt_cigar,
                     const int64_t* alt_cigar_off, const int64_t* alt_start, int32_t clip_threshold, int32_t take_in, int32_t* out_hp,
                     int32_t* out_ps, uint8_t* out_base, uint8_t* out_qual, int64_t cell_cap) {
    const strk_pi::CellsInput in{n_bytes, n_items, rec_off, item_locus, n_loci, cand_off, cand_pos, {alt_cigar, alt_cigar_off, alt_start},
                                 clip_threshold, take_in};
    strk_groups::Message msg;
    std::vector<int64_t> cell_off;
    if (strk_pi::check_cells(in, cell_off, &msg)) return fail(STRK_E_INVALID, "strk_phase_cells: %s", msg.text);
    if (n_items == 0) return 0;
    if (!buf || !out_hp || !out_ps) return fail(STRK_E_INVALID, "strk_phase_cells: NULL argument");
    if (cell_off.back() > 0 && (!out_base || !out_qual)) return fail(STRK_E_INVALID, "strk_phase_cells: NULL argument");
    if (cell_cap < cell_off.back())
        return fail(STRK_E_NOMEM, "strk_phase_cells: cell buffers too small (%lld < %lld)", (long long)cell_cap, (long long)cell_off.back());
    strk_threads::FirstBad bad;
    strk_threads::parallel_slices(n_items, 1024, 32, [&](int32_t i0, int32_t i1) {
        const int32_t b = strk_pi::host_cells(buf, in, cell_off.data(), i0, i1, out_hp, out_ps, out_base, out_qual);
        if (b >= 0) bad.report(b);
    });
    if (bad.get() >= 0) return fail(STRK_E_INVALID, "strk_phase_cells: item %d: malformed BAM record or auxiliary fields", (int)bad.get());
    return 0;
}

int64_t strk_useful_snvs(int32_t n_items, const int32_t* item_locus, int32_t n_loci, const int32_t* cand_off, const uint8_t* cells_base,
                         const uint8_t* cells_qual, const int32_t* kept_off, const int32_t* kept_item, int32_t min_allele_reads,
                         int32_t* out_snv_off, int32_t* out_snv_cand, uint8_t* out_base, uint8_t* out_qual, int64_t cap) {
    const strk_pi::UsefulInput in{n_items, item_locus, n_loci, kept_off, kept_item, min_allele_reads};
    strk_groups::Message msg;
    if (n_loci < 0 || n_items < 0 || cap < 0) return fail(STRK_E_INVALID, "strk_useful_snvs: bad argument");
    if (!out_snv_off) return fail(STRK_E_INVALID, "strk_useful_snvs: NULL argument");
    out_snv_off[0] = 0;
    if (n_loci == 0) return 0;
    if (!cand_off || cand_off[0] != 0) return fail(STRK_E_INVALID, "strk_useful_snvs: cand_off must be given and start at 0");
    for (int32_t l = 0; l < n_loci; ++l)
        if (cand_off[l + 1] < cand_off[l] || cand_off[l + 1] - cand_off[l] > strk_pi::kMaxCand)
            return fail(STRK_E_INVALID, "strk_useful_snvs: locus %d: cand_off is decreasing, or more than %d candidates", l, strk_pi::kMaxCand);
    // (the candidates and the items as strk_phase_cells took them: the offsets of the cells follow from them)
    if (n_items > 0 && !item_locus) return fail(STRK_E_INVALID, "strk_useful_snvs: NULL argument");
    std::vector<int64_t> cell_off((size_t)n_items + 1, 0);
    for (int32_t i = 0; i < n_items; ++i) {
        if (item_locus[i] < 0 || item_locus[i] >= n_loci) return fail(STRK_E_INVALID, "strk_useful_snvs: item %d: item_locus out of range", i);
        cell_off[(size_t)i + 1] = cell_off[(size_t)i] + (cand_off[item_locus[i] + 1] - cand_off[item_locus[i]]);
    }
    if (strk_pi::check_useful(in, &msg)) return fail(STRK_E_INVALID, "strk_useful_snvs: %s", msg.text);
    if (!out_snv_cand || (cell_off.back() > 0 && (!cells_base || !cells_qual))) return fail(STRK_E_INVALID, "strk_useful_snvs: NULL argument");
    std::vector<int32_t> n_sel((size_t)n_loci), sel((size_t)n_loci * strk_pi::kMaxSnvs);
    strk_threads::parallel_slices(n_loci, 1024, 32, [&](int32_t l0, int32_t l1) {
        for (int32_t l = l0; l < l1; ++l)
            n_sel[(size_t)l] = strk_pi::host_useful_locus(in, cand_off, cell_off.data(), cells_base, l, sel.data() + (size_t)l * strk_pi::kMaxSnvs);
    });
    std::vector<int64_t> pack_off;
    const int64_t total = pi_offsets(n_loci, kept_off, n_sel.data(), out_snv_off, pack_off);
    for (int32_t l = 0; l < n_loci; ++l)
        for (int32_t j = 0; j < n_sel[(size_t)l]; ++j) out_snv_cand[out_snv_off[l] + j] = sel[(size_t)l * strk_pi::kMaxSnvs + j];
    if (total > cap) return total;   // size query: snv_off and the candidate indices are filled, no cell is written
    if (total > 0 && (!out_base || !out_qual)) return fail(STRK_E_INVALID, "strk_useful_snvs: NULL argument");
    for (int32_t l = 0; l < n_loci; ++l) {
        const int32_t k0 = kept_off[l], n = kept_off[l + 1] - k0, s = n_sel[(size_t)l];
        for (int32_t r = 0; r < n; ++r)
            for (int32_t j = 0; j < s; ++j) {
                const int64_t src = cell_off[(size_t)kept_item[k0 + r]] + sel[(size_t)l * strk_pi::kMaxSnvs + j];
                out_base[pack_off[(size_t)l] + (int64_t)r * s + j] = cells_base[src];
                out_qual[pack_off[(size_t)l] + (int64_t)r * s + j] = cells_qual[src];
            }
    }
    return total;
}

int strk_dbam_phase_cells(strk_dbam* d, int32_t n_items, const int64_t* rec_off, const int32_t* item_locus, int32_t n_loci,
                          const int32_t* cand_off, const int64_t* cand_pos, const uint32_t* alt_cigar, const int64_t* alt_cigar_off,
                          const int64_t* alt_start, int32_t clip_threshold, int32_t take_in, int32_t piece_items, int32_t* out_hp,
                          int32_t* out_ps) {
    if (!d || piece_items < 0) return fail(STRK_E_INVALID, "strk_dbam_phase_cells: bad argument");
    d->pc_valid = false;
    const strk_pi::CellsInput in{d->n_data, n_items, rec_off, item_locus, n_loci, cand_off, cand_pos, {alt_cigar, alt_cigar_off, alt_start},
                                 clip_threshold, take_in};
    strk_groups::Message msg;
    if (strk_pi::check_cells(in, d->pc_cell_off_h, &msg)) return fail(STRK_E_INVALID, "strk_dbam_phase_cells: %s", msg.text);
    const std::vector<int64_t>& cell_off = d->pc_cell_off_h;
    if (n_items > 0 && (!out_hp || !out_ps)) return fail(STRK_E_INVALID, "strk_dbam_phase_cells: NULL argument");
    const int64_t n_cells = cell_off.back();
    if (2 * n_cells > strk_pi::kCellBudget)
        return fail(STRK_E_NOMEM, "strk_dbam_phase_cells: %lld cells exceed the workspace of %lld bytes: call it for fewer loci at a time",
                    (long long)n_cells, (long long)strk_pi::kCellBudget);
    d->pc_item_locus.assign(item_locus, item_locus + n_items);
    d->pc_cand_off_h.assign(cand_off, cand_off + (n_loci > 0 ? n_loci + 1 : 0));
    if (n_items == 0) { d->pc_valid = true; return 0; }
    HIP_TRY(hipSetDevice(d->device));
    const size_t n = (size_t)n_items, n_cand = (size_t)cand_off[n_loci];
    // pc_in: rec_off | item_locus | cand_pos | cand_off | cell_off | alt | bad || hp | ps
    Staging st(d->stage);
    const size_t o_rec = st.put(rec_off, n * 8), o_loc = st.put(item_locus, n * 4), o_cand = st.put(cand_pos, n_cand * 8);
    d->pc_cand_off = st.put(cand_off, ((size_t)n_loci + 1) * 4);
    d->pc_cell_off = st.put(cell_off.data(), (n + 1) * 8);
    const StagedAlt s_alt = stage_alt(st, n, in.alt);
    const size_t o_bad = st.zero(4), o_hp = st.room(n * 4), o_ps = st.room(n * 4);
    int rc;
    if ((rc = st.upload(d->pc_in)) || (rc = d->pc_cells.ensure((size_t)(2 * n_cells) + 16))) return rc;
    uint8_t* const cells_base = d->pc_cells.as<uint8_t>();
    uint8_t* const cells_qual = cells_base + n_cells;
    // launches of at most piece_items items (0: all of them in one); every item's cells have their place, so the cut changes nothing
    d->tic();
    rc = strk_threads::for_pieces(n_items, piece_items, [&](int32_t i0, int32_t i1) {
        hipLaunchKernelGGL(strk_pi::k_dbam_phase_cells, dim3((unsigned)((i1 - i0 + 3) / 4)), dim3(256), 0, 0, d->data.as<uint8_t>(), d->n_data, i0,
                           i1, d->pc_in.at<int64_t>(o_rec), d->pc_in.at<int32_t>(o_loc), d->pc_in.at<int32_t>(d->pc_cand_off),
                           d->pc_in.at<int64_t>(o_cand), d->pc_in.at<int64_t>(d->pc_cell_off), s_alt.on(d->pc_in), clip_threshold, take_in,
                           d->pc_in.at<int32_t>(o_hp), d->pc_in.at<int32_t>(o_ps), cells_base, cells_qual, d->pc_in.at<int32_t>(o_bad));
        HIP_TRY(hipGetLastError());
        return 0;
    });
    if (rc) return rc;
    d->toc();
    if ((rc = st.download(d->pc_in, o_bad, st.cv.bytes))) return rc;
    const int64_t bad = strk_threads::first_bad_of_word(*st.at<int32_t>(o_bad), INT32_MAX);
    if (bad >= 0) return fail(STRK_E_INVALID, "strk_dbam_phase_cells: item %d: malformed BAM record or auxiliary fields", (int)bad);
    memcpy(out_hp, st.at<int32_t>(o_hp), n * 4);
    memcpy(out_ps, st.at<int32_t>(o_ps), n * 4);
    d->pc_valid = true;
    return 0;
}

// The cells of the last strk_dbam_phase_cells -> host (tests, the Python block path's comparison); n_cells of each.
int strk_dbam_download_cells(strk_dbam* d, int64_t n_cells, uint8_t* out_base, uint8_t* out_qual) {
    if (!d || !d->pc_valid || n_cells < 0 || n_cells != d->pc_cell_off_h.back()) return fail(STRK_E_INVALID, "strk_dbam_download_cells: bad argument (or no cells)");
    if (n_cells == 0) return 0;
    if (!out_base || !out_qual) return fail(STRK_E_INVALID, "strk_dbam_download_cells: NULL argument");
    HIP_TRY(hipSetDevice(d->device));
    HIP_TRY(hipMemcpy(out_base, d->pc_cells.p, (size_t)n_cells, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(out_qual, d->pc_cells.as<uint8_t>() + n_cells, (size_t)n_cells, hipMemcpyDeviceToHost));
    return 0;
}

int64_t strk_dbam_useful_snvs(strk_dbam* d, int32_t n_loci, const int32_t* kept_off, const int32_t* kept_item, int32_t min_allele_reads,
                              int32_t* out_snv_off, int32_t* out_snv_cand, uint8_t* out_base, uint8_t* out_qual, int64_t cap) {
    if (!d || cap < 0 || !out_snv_off) return fail(STRK_E_INVALID, "strk_dbam_useful_snvs: bad argument");
    if (!d->pc_valid) return fail(STRK_E_INVALID, "strk_dbam_useful_snvs: no cells (call strk_dbam_phase_cells first)");
    const int32_t n_have = d->pc_cand_off_h.empty() ? 0 : (int32_t)d->pc_cand_off_h.size() - 1;
    if (n_loci != n_have) return fail(STRK_E_INVALID, "strk_dbam_useful_snvs: %d loci, the cells are those of %d", n_loci, n_have);
    const strk_pi::UsefulInput in{(int32_t)d->pc_item_locus.size(), d->pc_item_locus.data(), n_loci, kept_off, kept_item, min_allele_reads};
    strk_groups::Message msg;
    if (strk_pi::check_useful(in, &msg)) return fail(STRK_E_INVALID, "strk_dbam_useful_snvs: %s", msg.text);
    out_snv_off[0] = 0;
    if (n_loci == 0) return 0;
    if (!out_snv_cand) return fail(STRK_E_INVALID, "strk_dbam_useful_snvs: NULL argument");
    if (d->pc_item_locus.empty()) {   // a cells call without items staged nothing: no locus has a read, none a useful SNV
        std::fill(out_snv_off, out_snv_off + n_loci + 1, 0);
        return 0;
    }
    HIP_TRY(hipSetDevice(d->device));
    const size_t nl = (size_t)n_loci, n_kept = (size_t)kept_off[n_loci];
    // w_a: kept_off | kept_item || n_sel | sel || pack_off
    Staging st(d->stage);
    const size_t o_koff = st.put(kept_off, (nl + 1) * 4), o_kit = st.put(kept_item, n_kept * 4);
    const size_t o_nsel = st.room(nl * 4), o_sel = st.room(nl * strk_pi::kMaxSnvs * 4), o_pack = st.room((nl + 1) * 8);
    int rc;
    if ((rc = st.upload(d->w_a))) return rc;
    const int64_t n_cells = d->pc_cell_off_h.back();
    const uint8_t* const cells_base = d->pc_cells.as<uint8_t>();
    const int64_t* const d_cell_off = d->pc_in.at<int64_t>(d->pc_cell_off);
    d->tic();
    hipLaunchKernelGGL(strk_pi::k_snv_useful, dim3((unsigned)n_loci), dim3(256), 0, 0, d->pc_in.at<int32_t>(d->pc_cand_off), d->w_a.at<int32_t>(o_koff),
                       d->w_a.at<int32_t>(o_kit), d_cell_off, cells_base, min_allele_reads, d->w_a.at<int32_t>(o_nsel), d->w_a.at<int32_t>(o_sel));
    HIP_TRY(hipGetLastError());
    d->toc();
    if ((rc = st.download(d->w_a, o_nsel, o_pack))) return rc;
    const int32_t* const n_sel = st.at<int32_t>(o_nsel);
    const int32_t* const sel = st.at<int32_t>(o_sel);
    std::vector<int64_t> pack_off;
    const int64_t total = pi_offsets(n_loci, kept_off, n_sel, out_snv_off, pack_off);
    for (int32_t l = 0; l < n_loci; ++l)
        for (int32_t j = 0; j < n_sel[(size_t)l]; ++j) out_snv_cand[out_snv_off[l] + j] = sel[(size_t)l * strk_pi::kMaxSnvs + j];
    if (total > cap || total == 0) return total;
    if (!out_base || !out_qual) return fail(STRK_E_INVALID, "strk_dbam_useful_snvs: NULL argument");
    if ((rc = d->w_f.ensure((size_t)(2 * total) + 16))) return rc;
    HIP_TRY(hipMemcpy(d->w_a.at<char>(o_pack), pack_off.data(), (nl + 1) * 8, hipMemcpyHostToDevice));
    d->tic();
    hipLaunchKernelGGL(strk_pi::k_snv_gather, dim3((unsigned)n_loci), dim3(256), 0, 0, d->w_a.at<int32_t>(o_koff), d->w_a.at<int32_t>(o_kit), d_cell_off,
                       cells_base, cells_base + n_cells, d->w_a.at<int32_t>(o_nsel), d->w_a.at<int32_t>(o_sel), d->w_a.at<int64_t>(o_pack),
                       d->w_f.as<uint8_t>(), d->w_f.as<uint8_t>() + total);
    HIP_TRY(hipGetLastError());
    d->toc();
    HIP_TRY(hipMemcpy(out_base, d->w_f.p, (size_t)total, hipMemcpyDeviceToHost));   // (straight into the caller's two arrays)
    HIP_TRY(hipMemcpy(out_qual, d->w_f.as<uint8_t>() + total, (size_t)total, hipMemcpyDeviceToHost));
    return total;
}

}  // extern "C"
