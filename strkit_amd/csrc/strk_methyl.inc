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
    const strk_me::Input in{n_bytes, n_items, rec_off, coords, alt_cigar, alt_cigar_off, alt_start, threshold};
    strk_groups::Message msg;
    if (strk_me::check_input(in, &msg)) return fail(STRK_E_INVALID, "strk_methyl: %s", msg.text);
    if (n_items == 0) return 0;
    if (!buf || !out_status || !out_sites || !out_known || !out_mc) return fail(STRK_E_INVALID, "strk_methyl: NULL argument");
    std::atomic<int32_t> bad{-1};
    pi_parallel(n_items, [&](int32_t i0, int32_t i1) {
        const int32_t b = strk_me::host_methyl(buf, in, i0, i1, out_status, out_sites, out_known, out_mc);
        int32_t cur = bad.load();
        while (b > cur && !bad.compare_exchange_weak(cur, b)) {}
    });
    if (bad.load() >= 0) return fail(STRK_E_INVALID, "strk_methyl: item %d: malformed BAM record or auxiliary fields", bad.load());
    return 0;
}

int strk_dbam_methyl(strk_dbam* d, int32_t n_items, const int64_t* rec_off, const int64_t* coords, const uint32_t* alt_cigar,
                     const int64_t* alt_cigar_off, const int64_t* alt_start, int32_t threshold, int32_t piece_items, int32_t* out_status,
                     int32_t* out_sites, int32_t* out_known, int32_t* out_mc) {
    if (!d || piece_items < 0) return fail(STRK_E_INVALID, "strk_dbam_methyl: bad argument");
    const strk_me::Input in{d->n_data, n_items, rec_off, coords, alt_cigar, alt_cigar_off, alt_start, threshold};
    strk_groups::Message msg;
    if (strk_me::check_input(in, &msg)) return fail(STRK_E_INVALID, "strk_dbam_methyl: %s", msg.text);
    if (n_items == 0) return 0;
    if (!out_status || !out_sites || !out_known || !out_mc) return fail(STRK_E_INVALID, "strk_dbam_methyl: NULL argument");
    HIP_TRY(hipSetDevice(d->device));
    const size_t n = (size_t)n_items;
    const bool alt = alt_cigar_off && alt_cigar_off[n] > 0;
    const size_t n_ops = alt ? (size_t)alt_cigar_off[n] : 0;
    // me_in: rec_off | coords | alt_off | alt_start | alt ops | status, sites, known, mc | bad
    Carve cv;
    const size_t o_rec = cv.take(n * 8), o_co = cv.take(n * 32), o_aoff = cv.take((n + 1) * 8), o_astart = cv.take(n * 8),
                 o_ops = cv.take(n_ops * 4 + 4), o_out = cv.take(n * 16), o_bad = cv.take(4);
    int rc;
    if ((rc = d->me_in.ensure(cv.bytes))) return rc;
    HIP_TRY(hipMemcpy(d->me_in.at<char>(o_rec), rec_off, n * 8, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(d->me_in.at<char>(o_co), coords, n * 32, hipMemcpyHostToDevice));
    HIP_TRY(hipMemset(d->me_in.at<char>(o_bad), 0, 4));
    if (alt) {
        HIP_TRY(hipMemcpy(d->me_in.at<char>(o_ops), alt_cigar, n_ops * 4, hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(d->me_in.at<char>(o_aoff), alt_cigar_off, (n + 1) * 8, hipMemcpyHostToDevice));
        if (alt_start) HIP_TRY(hipMemcpy(d->me_in.at<char>(o_astart), alt_start, n * 8, hipMemcpyHostToDevice));
        else HIP_TRY(hipMemset(d->me_in.at<char>(o_astart), 0, n * 8));
    }
    int32_t* const o = d->me_in.at<int32_t>(o_out);
    // launches of at most piece_items items (0: all of them in one); every item has its own outputs, so the cut changes nothing
    const int32_t piece = piece_items > 0 ? piece_items : n_items;
    d->tic();
    for (int32_t i0 = 0; i0 < n_items; i0 += piece) {
        const int32_t i1 = (int32_t)std::min<int64_t>(n_items, (int64_t)i0 + piece);
        hipLaunchKernelGGL(strk_me::k_dbam_methyl, dim3((unsigned)((i1 - i0 + 3) / 4)), dim3(256), 0, 0, d->data.as<uint8_t>(), d->n_data, i0, i1,
                           d->me_in.at<int64_t>(o_rec), d->me_in.at<int64_t>(o_co), alt ? d->me_in.at<uint32_t>(o_ops) : (const uint32_t*)nullptr,
                           alt ? d->me_in.at<int64_t>(o_aoff) : (const int64_t*)nullptr, alt ? d->me_in.at<int64_t>(o_astart) : (const int64_t*)nullptr,
                           threshold, o, o + n, o + 2 * n, o + 3 * n, d->me_in.at<int32_t>(o_bad));
        HIP_TRY(hipGetLastError());
        if (i1 == n_items) break;   // (i0 + piece may pass INT32_MAX)
    }
    d->toc();
    int32_t bad = 0;
    HIP_TRY(hipMemcpy(&bad, d->me_in.at<char>(o_bad), 4, hipMemcpyDeviceToHost));
    if (bad) return fail(STRK_E_INVALID, "strk_dbam_methyl: item %d: malformed BAM record or auxiliary fields", bad - 1);
    HIP_TRY(hipMemcpy(out_status, o, n * 4, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(out_sites, o + n, n * 4, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(out_known, o + 2 * n, n * 4, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(out_mc, o + 3 * n, n * 4, hipMemcpyDeviceToHost));
    return 0;
}

}  // extern "C"
