// strk_snv_discover.inc — candidate SNVs from a pileup of the kept reads (part of strk_api.hip, after strk_phase_inputs.inc):
// strk_discover_snvs over a host buffer and strk_dbam_discover_snvs over the file resident on the device.  The rule, the input
// check, the host twin and the kernels are strk_snv_discover.h; here are the threads, the buffers and the launches.

namespace {

// An aligned operation with this many bases or more inside a tile is counted by all 64 lanes of its wave, a shorter one by the
// lane that holds it (k_snv_pileup).  Not tuned: profiles/r32_snv_discover.txt.
constexpr int kSdLongOp = 64;

// out_cand_off from the loci's counts; returns the number of candidates
int64_t sd_offsets(int32_t n_loci, const int32_t* n_cand, int32_t* cand_off) {
    cand_off[0] = 0;
    for (int32_t l = 0; l < n_loci; ++l) cand_off[l + 1] = cand_off[l] + n_cand[l];
    return cand_off[n_loci];
}

}  // namespace

extern "C" {

int64_t strk_discover_snvs(const uint8_t* buf, int64_t n_bytes, int32_t n_items, const int64_t* rec_off, const int32_t* item_locus,
                           int32_t n_loci, const int64_t* left_coord, const int64_t* right_coord, const int32_t* kept_off,
                           const int32_t* kept_item, const uint32_t* alt_cigar, const int64_t* alt_cigar_off, const int64_t* alt_start,
                           int32_t clip_threshold, int32_t take_in, int32_t window, int32_t min_base_qual, int32_t min_allele_reads,
                           int32_t* out_cand_off, int64_t* out_cand_pos, int64_t cap) {
    const strk_sd::DiscoverInput in{n_bytes, n_items, rec_off, item_locus, n_loci, left_coord, right_coord, kept_off, kept_item,
                                    {alt_cigar, alt_cigar_off, alt_start}, clip_threshold, take_in, window, min_base_qual, min_allele_reads};
    strk_groups::Message msg;
    if (cap < 0 || !out_cand_off) return fail(STRK_E_INVALID, "strk_discover_snvs: bad argument");
    if (strk_sd::check_discover(in, &msg)) return fail(STRK_E_INVALID, "strk_discover_snvs: %s", msg.text);
    out_cand_off[0] = 0;
    if (n_loci == 0) return 0;
    if (n_items > 0 && !buf) return fail(STRK_E_INVALID, "strk_discover_snvs: NULL argument");
    strk_threads::FirstBad bad;
    strk_threads::parallel_slices(n_items, 1024, 32, [&](int32_t i0, int32_t i1) {
        const int32_t b = strk_sd::host_first_bad(buf, in, i0, i1);
        if (b >= 0) bad.report(b);
    });
    if (bad.get() >= 0) return fail(STRK_E_INVALID, "strk_discover_snvs: item %d: malformed BAM record", (int)bad.get());
    std::vector<std::vector<int64_t>> found((size_t)n_loci);
    struct Scratch { std::vector<uint32_t> counts; };
    strk_threads::parallel_chunks<Scratch>(n_loci, 16, std::min(strk_threads::host_cpus(), std::max(1, n_loci / 16)), [&](int64_t l0, int64_t l1, Scratch& s) {
        for (int64_t l = l0; l < l1; ++l) strk_sd::host_discover_locus(buf, in, (int32_t)l, s.counts, found[(size_t)l]);
    });
    for (int32_t l = 0; l < n_loci; ++l) out_cand_off[l + 1] = out_cand_off[l] + (int32_t)found[(size_t)l].size();
    const int64_t total = out_cand_off[n_loci];
    if (total > cap) return total;   // size query: the offsets are filled, no position is written
    if (total > 0 && !out_cand_pos) return fail(STRK_E_INVALID, "strk_discover_snvs: NULL argument");
    for (int32_t l = 0; l < n_loci; ++l) std::copy(found[(size_t)l].begin(), found[(size_t)l].end(), out_cand_pos + out_cand_off[l]);
    return total;
}

int64_t strk_dbam_discover_snvs(strk_dbam* d, int32_t n_items, const int64_t* rec_off, const int32_t* item_locus, int32_t n_loci,
                                const int64_t* left_coord, const int64_t* right_coord, const int32_t* kept_off, const int32_t* kept_item,
                                const uint32_t* alt_cigar, const int64_t* alt_cigar_off, const int64_t* alt_start, int32_t clip_threshold,
                                int32_t take_in, int32_t window, int32_t min_base_qual, int32_t min_allele_reads, int32_t piece_items,
                                int32_t* out_cand_off, int64_t* out_cand_pos, int64_t cap) {
    if (!d || piece_items < 0 || cap < 0 || !out_cand_off) return fail(STRK_E_INVALID, "strk_dbam_discover_snvs: bad argument");
    const strk_sd::DiscoverInput in{d->n_data, n_items, rec_off, item_locus, n_loci, left_coord, right_coord, kept_off, kept_item,
                                    {alt_cigar, alt_cigar_off, alt_start}, clip_threshold, take_in, window, min_base_qual, min_allele_reads};
    strk_groups::Message msg;
    if (strk_sd::check_discover(in, &msg)) return fail(STRK_E_INVALID, "strk_dbam_discover_snvs: %s", msg.text);
    out_cand_off[0] = 0;
    if (n_loci == 0) return 0;
    if (n_items == 0) {   // no read, no candidate: nothing is staged
        std::fill(out_cand_off, out_cand_off + n_loci + 1, 0);
        return 0;
    }
    const int32_t n_tiles = strk_sd::tiles_per_side(window);
    const int64_t n_blocks = (int64_t)n_loci * 2 * n_tiles, mask_bytes = n_blocks * strk_sd::kTileWords * 8;
    if (mask_bytes > strk_sd::kMaskBudget)
        return fail(STRK_E_NOMEM, "strk_dbam_discover_snvs: the masks of %d loci x %d tiles exceed the workspace of %lld bytes: call it for fewer loci at a time",
                    (int)n_loci, 2 * (int)n_tiles, (long long)strk_sd::kMaskBudget);
    HIP_TRY(hipSetDevice(d->device));
    const size_t n = (size_t)n_items, nl = (size_t)n_loci, n_kept = (size_t)kept_off[n_loci];
    // w_a: rec_off | left | right | kept_off | kept_item | alt | bad || span | n_cand | keep || cand_off
    Staging st(d->stage);
    const size_t o_rec = st.put(rec_off, n * 8), o_left = st.put(left_coord, nl * 8), o_right = st.put(right_coord, nl * 8);
    const size_t o_koff = st.put(kept_off, (nl + 1) * 4), o_kit = st.put(kept_item, n_kept * 4);
    const StagedAlt s_alt = stage_alt(st, n, in.alt);
    const size_t o_bad = st.zero(4), o_span = st.room(n * 16), o_ncand = st.room(nl * 4), o_keep = st.room(nl * 8), o_coff = st.room((nl + 1) * 4);
    int rc;
    if ((rc = st.upload(d->w_a)) || (rc = d->sd_masks.ensure((size_t)mask_bytes + 16))) return rc;
    unsigned long long* const masks = d->sd_masks.as<unsigned long long>();
    // piece_items > 0 cuts the launches: the span kernel into that many items, the pileup into that many tiles.  Every item's span
    // and every tile's mask has its place, so the cut changes nothing.
    d->tic();
    rc = strk_threads::for_pieces(n_items, piece_items, [&](int32_t i0, int32_t i1) {
        hipLaunchKernelGGL(strk_sd::k_snv_span, dim3((unsigned)((i1 - i0 + 3) / 4)), dim3(256), 0, 0, d->data.as<uint8_t>(), d->n_data, i0, i1,
                           d->w_a.at<int64_t>(o_rec), s_alt.on(d->w_a), clip_threshold, take_in, d->w_a.at<int64_t>(o_span), d->w_a.at<int32_t>(o_bad));
        HIP_TRY(hipGetLastError());
        return 0;
    });
    if (rc) return rc;
    d->toc();
    if ((rc = st.download(d->w_a, o_bad, o_bad + 4))) return rc;
    const int64_t bad = strk_threads::first_bad_of_word(*st.at<int32_t>(o_bad), INT32_MAX);
    if (bad >= 0) return fail(STRK_E_INVALID, "strk_dbam_discover_snvs: item %d: malformed BAM record", (int)bad);
    d->tic();
    rc = strk_threads::for_pieces((int32_t)n_blocks, piece_items, [&](int32_t b0, int32_t b1) {
        hipLaunchKernelGGL(strk_sd::k_snv_pileup, dim3((unsigned)(b1 - b0)), dim3(256), 0, 0, d->data.as<uint8_t>(), d->n_data, b0,
                           d->w_a.at<int64_t>(o_rec), s_alt.on(d->w_a), d->w_a.at<int64_t>(o_span), d->w_a.at<int64_t>(o_left),
                           d->w_a.at<int64_t>(o_right), d->w_a.at<int32_t>(o_koff), d->w_a.at<int32_t>(o_kit), window, n_tiles, min_base_qual,
                           min_allele_reads, kSdLongOp, masks);
        HIP_TRY(hipGetLastError());
        return 0;
    });
    if (rc) return rc;
    hipLaunchKernelGGL(strk_sd::k_snv_pick, dim3((unsigned)n_loci), dim3(256), 0, 0, masks, d->w_a.at<int64_t>(o_left), d->w_a.at<int64_t>(o_right), window,
                       n_tiles, (const int32_t*)nullptr, d->w_a.at<int32_t>(o_ncand), d->w_a.at<int32_t>(o_keep), (int64_t*)nullptr);
    HIP_TRY(hipGetLastError());
    d->toc();
    if ((rc = st.download(d->w_a, o_ncand, o_keep))) return rc;
    const int64_t total = sd_offsets(n_loci, st.at<int32_t>(o_ncand), out_cand_off);
    if (total > cap || total == 0) return total;   // size query: the offsets are filled, no position is written
    if (!out_cand_pos) return fail(STRK_E_INVALID, "strk_dbam_discover_snvs: NULL argument");
    if ((rc = d->w_f.ensure((size_t)total * 8 + 16))) return rc;
    HIP_TRY(hipMemcpy(d->w_a.at<char>(o_coff), out_cand_off, (nl + 1) * 4, hipMemcpyHostToDevice));
    d->tic();
    hipLaunchKernelGGL(strk_sd::k_snv_pick, dim3((unsigned)n_loci), dim3(256), 0, 0, masks, d->w_a.at<int64_t>(o_left), d->w_a.at<int64_t>(o_right), window,
                       n_tiles, d->w_a.at<int32_t>(o_coff), d->w_a.at<int32_t>(o_ncand), d->w_a.at<int32_t>(o_keep), d->w_f.as<int64_t>());
    HIP_TRY(hipGetLastError());
    d->toc();
    HIP_TRY(hipMemcpy(out_cand_pos, d->w_f.p, (size_t)total * 8, hipMemcpyDeviceToHost));
    return total;
}

}  // extern "C"
