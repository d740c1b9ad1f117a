// Host side of strk_best_representatives / strk_best_representatives_dseqs: input checks, pieces, launches.
// Part of strk_api.hip: included inside its anonymous namespace (uses fail(), HIP_TRY, DevBuf, strk_ctx, check_groups,
// side_stream and timed_launch defined there); not a stand-alone header.
// ---------------------------------------------------------------------------------------------
// Best representative of every group: strk_best_representatives
// ---------------------------------------------------------------------------------------------
constexpr size_t kConsBoundBudget = (size_t)256 << 20;   // bytes of last-row deltas of one piece (patterns beyond one pass only)
constexpr int kConsPieceGroups = 32768;

// `d_seqs` != nullptr: the bases are in device memory already and `seqs` is not read.  `fn`: the entry point, for messages
// (strk_consensus's own name when that call runs this pass on some of its groups).
int best_rep_impl(strk_ctx* c, const char* fn, int32_t n_groups, const int32_t* group_off, const uint8_t* seqs,
                  const uint8_t* d_seqs, int64_t n_seq_bytes, const int64_t* seq_start, const int32_t* seq_len,
                  int32_t* out_index, int32_t* out_method, int64_t* out_dist_sum, strk_stats* stats) {
    if (stats) memset(stats, 0, sizeof *stats);
    const strk_groups::View view{n_groups, group_off, n_seq_bytes, seq_start, seq_len};
    strk_groups::Totals tot;
    int rc;
    if ((rc = check_groups(fn, view, kConsMaxGroup, kConsMaxLen, &tot))) return rc;
    if (n_groups == 0) return 0;
    if (!out_index || !out_method || !out_dist_sum) return fail(STRK_E_INVALID, "%s: NULL argument", fn);
    const int32_t max_len = tot.max_len;
    if (n_seq_bytes > 0 && !seqs && !d_seqs && max_len > 0) return fail(STRK_E_INVALID, "%s: seqs is NULL", fn);
    HIP_TRY(hipSetDevice(c->device));
    hipStream_t st;
    if ((rc = side_stream(c, &st))) return rc;
    if ((rc = c->cs_out.ensure((size_t)n_groups * 16))) return rc;
    if ((rc = c->cs_in.upload(view, tot, seqs, d_seqs, st))) return rc;
    // a pattern (the shorter string of a pair) beyond one pass parks a row of deltas per wave; the row is as long as the text
    const size_t bound_stride = max_len > kConsPassRows ? ((size_t)max_len + 63) & ~(size_t)63 : 0;
    const int32_t piece = bound_stride ? (int32_t)std::max<size_t>(1, std::min<size_t>(kConsPieceGroups, kConsBoundBudget / (bound_stride * kConsWaves)))
                                       : kConsPieceGroups;
    if (bound_stride && (rc = c->cs_bound.ensure((size_t)std::min(piece, n_groups) * kConsWaves * bound_stride))) return rc;
    int64_t* d_dist = c->cs_out.as<int64_t>();
    int32_t* d_index = reinterpret_cast<int32_t*>(d_dist + n_groups);
    int32_t* d_method = d_index + n_groups;
    for (int32_t g0 = 0; g0 < n_groups; g0 += piece) {
        const int32_t ng = std::min(piece, n_groups - g0);
        ConsArgs a{};
        a.group_off = c->cs_in.off.as<int32_t>() + g0;
        a.seqs = c->cs_in.bases;
        a.seq_start = c->cs_in.start.as<int64_t>();
        a.seq_len = c->cs_in.len.as<int32_t>();
        a.bound = bound_stride ? c->cs_bound.as<uint8_t>() : nullptr;
        a.bound_stride = (int64_t)bound_stride;
        a.out_index = d_index + g0;
        a.out_method = d_method + g0;
        a.out_dist = d_dist + g0;
        a.n_groups = ng;
        if ((rc = timed_launch(c, st, stats, fn, "best-representative kernel", 1, [&] {
                hipLaunchKernelGGL(k_best_rep, dim3(ng), dim3(kConsThreads), 0, st, a);
            }))) return rc;
    }
    HIP_TRY(hipMemcpyAsync(out_dist_sum, d_dist, (size_t)n_groups * 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(out_index, d_index, (size_t)n_groups * 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(out_method, d_method, (size_t)n_groups * 4, hipMemcpyDeviceToHost, st));
    const hipError_t q = hipStreamSynchronize(st);
    if (q != hipSuccess) return fail(STRK_E_DEVICE, "%s: best-representative results: %s", fn, hipGetErrorString(q));
    return 0;
}
