// strk_methyl.inc — 5-methyl CpG calls from MM / ML tags (part of strk_api.hip, after strk_phase_inputs.inc): strk_methyl over a
// host buffer (NativeBam, the regions of an IndexedBam) and strk_dbam_methyl over the file resident on the device.  The rule,
// the walks, the input check and the kernel are strk_methyl.h; here are the threads, the buffers and the launches.

extern "C" {

void strk_methyl_constants(int32_t* out4) {
    out4[0] = strk_me::kChunkBases; out4[1] = strk_me::kSeqPassBases; out4[2] = strk_me::kMmPassBytes; out4[3] = strk_me::kWindow;
}

int strk_methyl(const uint8_t* buf, int64_t n_bytes, int32_t n_items, const int64_t* rec_off, const int64_t* coords, const uint32_t* alt_cigar,
                const int64_t* alt_cigar_off, const int64_t* alt_start, int32_t threshold, int32_t* out_status, int32_t* out_sites,
                int32_t* out_known, int32_t* out_mc) {
    const strk_me::Input in{n_bytes, n_items, rec_off, coords, {alt_cigar, alt_cigar_off, alt_start}, threshold};
    strk_groups::Message msg;
    if (strk_me::check_input(in, &msg)) return fail(STRK_E_INVALID, "strk_methyl: %s", msg.text);
    if (n_items == 0) return 0;
    if (!buf || !out_status || !out_sites || !out_known || !out_mc) return fail(STRK_E_INVALID, "strk_methyl: NULL argument");
    strk_threads::FirstBad bad;
    strk_threads::parallel_slices(n_items, 1024, 32, [&](int32_t i0, int32_t i1) {
        const int32_t b = strk_me::host_methyl(buf, in, i0, i1, out_status, out_sites, out_known, out_mc);
        if (b >= 0) bad.report(b);
    });
    if (bad.get() >= 0) return fail(STRK_E_INVALID, "strk_methyl: item %d: malformed BAM record or auxiliary fields", (int)bad.get());
    return 0;
}

int strk_dbam_methyl(strk_dbam* d, int32_t n_items, const int64_t* rec_off, const int64_t* coords, const uint32_t* alt_cigar,
                     const int64_t* alt_cigar_off, const int64_t* alt_start, int32_t threshold, int32_t piece_items, int32_t* out_status,
                     int32_t* out_sites, int32_t* out_known, int32_t* out_mc) {
    if (!d || piece_items < 0) return fail(STRK_E_INVALID, "strk_dbam_methyl: bad argument");
    const strk_me::Input in{d->n_data, n_items, rec_off, coords, {alt_cigar, alt_cigar_off, alt_start}, threshold};
    strk_groups::Message msg;
    if (strk_me::check_input(in, &msg)) return fail(STRK_E_INVALID, "strk_dbam_methyl: %s", msg.text);
    if (n_items == 0) return 0;
    if (!out_status || !out_sites || !out_known || !out_mc) return fail(STRK_E_INVALID, "strk_dbam_methyl: NULL argument");
    HIP_TRY(hipSetDevice(d->device));
    const size_t n = (size_t)n_items;
    // w_a: rec_off | coords | alt | bad || status, sites, known, mc
    Staging st(d->stage);
    const size_t o_rec = st.put(rec_off, n * 8), o_co = st.put(coords, n * 32);
    const StagedAlt s_alt = stage_alt(st, n, in.alt);
    const size_t o_bad = st.zero(4), o_out = st.room(n * 16);
    int rc;
    if ((rc = st.upload(d->w_a))) return rc;
    int32_t* const o = d->w_a.at<int32_t>(o_out);
    // launches of at most piece_items items (0: all of them in one); every item has its own outputs, so the cut changes nothing
    d->tic();
    rc = strk_threads::for_pieces(n_items, piece_items, [&](int32_t i0, int32_t i1) {
        hipLaunchKernelGGL(strk_me::k_dbam_methyl, dim3((unsigned)((i1 - i0 + 3) / 4)), dim3(256), 0, 0, d->data.as<uint8_t>(), d->n_data, i0, i1,
                           d->w_a.at<int64_t>(o_rec), d->w_a.at<int64_t>(o_co), s_alt.on(d->w_a), threshold, o, o + n, o + 2 * n, o + 3 * n,
                           d->w_a.at<int32_t>(o_bad));
        HIP_TRY(hipGetLastError());
        return 0;
    });
    if (rc) return rc;
    d->toc();
    if ((rc = st.download(d->w_a, o_bad, st.cv.bytes))) return rc;
    const int64_t bad = strk_threads::first_bad_of_word(*st.at<int32_t>(o_bad), INT32_MAX);
    if (bad >= 0) return fail(STRK_E_INVALID, "strk_dbam_methyl: item %d: malformed BAM record or auxiliary fields", (int)bad);
    int32_t* const outs[4] = {out_status, out_sites, out_known, out_mc};
    for (int j = 0; j < 4; ++j) memcpy(outs[j], st.at<int32_t>(o_out) + (size_t)j * n, n * 4);
    return 0;
}

}  // extern "C"
