// strk_select.inc — read selection over the file resident on the device (part of strk_api.hip, after strk_methyl.inc):
// strk_dbam_select_reads and strk_select_constants.  The rule, the input check and the kernels are strk_select.h; here are the
// buffers, the split of the loci into the two launches and the launches.  (strk_select_reads, the host entry, is in
// strk_host_files.inc.)

extern "C" {

void strk_select_constants(int32_t* out4) {
    out4[0] = strk_sel::kSmallItems; out4[1] = strk_sel::kSmallSlots; out4[2] = strk_sel::kThreads; out4[3] = strk_sel::kCmpStep;
}

int strk_dbam_select_reads(strk_dbam* d, int32_t n_loci, const int64_t* item_off, const int64_t* rec_off, int32_t rules, int32_t max_reads,
                           uint8_t* out_reason, uint8_t* out_status, int32_t* out_n_kept) {
    if (!d) return fail(STRK_E_INVALID, "strk_dbam_select_reads: bad argument");
    const strk_sel::Input in{d->n_data, n_loci, item_off, rec_off, rules, max_reads};
    strk_groups::Message msg;
    if (strk_sel::check_input(in, &msg)) return fail(STRK_E_INVALID, "strk_dbam_select_reads: %s", msg.text);
    if (n_loci == 0) return 0;
    const size_t n = (size_t)item_off[n_loci], nl = (size_t)n_loci;
    if (!out_n_kept || (n > 0 && (!out_reason || !out_status))) return fail(STRK_E_INVALID, "strk_dbam_select_reads: NULL argument");
    if (n == 0) { memset(out_n_kept, 0, nl * 4); return 0; }
    HIP_TRY(hipSetDevice(d->device));
    // the two launches: loci of at most kSmallItems items, and the others with their tables' places in the workspace
    std::vector<int32_t> lists, large;   // the small loci, then the large ones
    std::vector<int64_t> table_off;
    int64_t n_slots = 0;
    lists.reserve(nl);
    for (int32_t l = 0; l < n_loci; ++l) {
        const int64_t k = item_off[l + 1] - item_off[l];
        if (k <= strk_sel::kSmallItems) { lists.push_back(l); continue; }
        large.push_back(l);
        table_off.push_back(n_slots);
        n_slots += strk_sel::slots_for(k);
    }
    const size_t n_small = lists.size(), n_large = large.size();
    lists.insert(lists.end(), large.begin(), large.end());
    // w_a: item_off | rec_off | table_off | the lists | bad | n_kept || reason | status;
    // w_d: rep | first | status of the large tables;  w_f: slot_why of the large loci's items
    Staging st(d->stage);
    const size_t a_item = st.put(item_off, (nl + 1) * 8), a_rec = st.put(rec_off, n * 8), a_toff = st.put(table_off.data(), n_large * 8),
                 a_lists = st.put(lists.data(), nl * 4), b_bad = st.zero(4), b_kept = st.zero(nl * 4), b_reason = st.room(n), b_status = st.room(n);
    Carve cd;
    const size_t d_rep = cd.take((size_t)n_slots * 4), d_first = cd.take((size_t)n_slots * 4), d_status = cd.take((size_t)n_slots * 4);
    int rc;
    if ((rc = st.upload(d->w_a))) return rc;
    if (n_large) {
        if ((rc = d->w_d.ensure(cd.bytes)) || (rc = d->w_f.ensure(n * 4))) return rc;
        HIP_TRY(hipMemset(d->w_d.at<char>(d_rep), 0xFF, d_status - d_rep));              // rep = -1, first = kNoItem
        HIP_TRY(hipMemset(d->w_d.at<char>(d_status), 0, (size_t)n_slots * 4));
    }
    const uint8_t* const data = d->data.as<uint8_t>();
    const int64_t* const d_item = d->w_a.at<int64_t>(a_item);
    const int64_t* const d_rec = d->w_a.at<int64_t>(a_rec);
    const int32_t* const d_lists = d->w_a.at<int32_t>(a_lists);
    uint8_t* const o_reason = d->w_a.at<uint8_t>(b_reason);
    uint8_t* const o_status = d->w_a.at<uint8_t>(b_status);
    int32_t* const o_kept = d->w_a.at<int32_t>(b_kept);
    int32_t* const o_bad = d->w_a.at<int32_t>(b_bad);
    d->tic();
    if (n_small)
        hipLaunchKernelGGL(strk_sel::k_select_small, dim3((unsigned)n_small), dim3(strk_sel::kThreads), 0, 0, data, d->n_data, d_lists,
                           d_item, d_rec, (int32_t)n, rules, max_reads, o_reason, o_status, o_kept, o_bad);
    if (n_large)
        hipLaunchKernelGGL(strk_sel::k_select_large, dim3((unsigned)n_large), dim3(strk_sel::kThreads), 0, 0, data, d->n_data,
                           d_lists + n_small, d->w_a.at<int64_t>(a_toff), d_item, d_rec, (int32_t)n, rules, max_reads,
                           d->w_d.at<int32_t>(d_rep), d->w_d.at<uint32_t>(d_first), d->w_d.at<uint32_t>(d_status),
                           d->w_f.as<int32_t>(), o_reason, o_status, o_kept, o_bad);
    HIP_TRY(hipGetLastError());
    d->toc();
    if ((rc = st.download(d->w_a, b_bad, st.cv.bytes))) return rc;
    const int64_t bad = strk_threads::first_bad_of_word(*st.at<int32_t>(b_bad), (int64_t)n);
    if (bad >= 0) return fail(STRK_E_INVALID, "strk_dbam_select_reads: item %lld: malformed BAM record", (long long)bad);
    memcpy(out_n_kept, st.at<char>(b_kept), nl * 4);
    memcpy(out_reason, st.at<char>(b_reason), n);
    memcpy(out_status, st.at<char>(b_status), n);
    return 0;
}

}  // extern "C"
