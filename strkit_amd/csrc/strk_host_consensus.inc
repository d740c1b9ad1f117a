// Host side of strk_best_representatives / strk_best_representatives_dseqs: input checks, pieces, launches.
// Part of strk_api.hip: included inside its anonymous namespace (uses fail(), HIP_TRY, DevBuf, Staging, strk_ctx, check_groups,
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
    // the view and the results in one staged buffer, sized here once: the pieces below keep its pointers
    Staging sg(c->image);
    const StagedGroups s_in = stage_groups(sg, view, tot, seqs, d_seqs);
    const size_t o_dist = sg.get(out_dist_sum, (size_t)n_groups * 8), o_index = sg.get(out_index, (size_t)n_groups * 4),
                 o_method = sg.get(out_method, (size_t)n_groups * 4);
    if ((rc = sg.upload(c->cs_stage, st))) return rc;
    const DevBuf& d = c->cs_stage;
    const StagedGroups::Ptrs in = s_in.on(d);
    // a pattern (the shorter string of a pair) beyond one pass parks a row of deltas per wave; the row is as long as the text
    const size_t bound_stride = max_len > kConsPassRows ? ((size_t)max_len + 63) & ~(size_t)63 : 0;
    const int32_t piece = bound_stride ? (int32_t)std::max<size_t>(1, std::min<size_t>(kConsPieceGroups, kConsBoundBudget / (bound_stride * kConsWaves)))
                                       : kConsPieceGroups;
    if (bound_stride && (rc = c->cs_bound.ensure((size_t)std::min(piece, n_groups) * kConsWaves * bound_stride))) return rc;
    for (int32_t g0 = 0; g0 < n_groups; g0 += piece) {
        const int32_t ng = std::min(piece, n_groups - g0);
        ConsArgs a{};
        a.group_off = in.off + g0;
        a.seqs = in.seqs;
        a.seq_start = in.start;
        a.seq_len = in.len;
        a.bound = bound_stride ? c->cs_bound.as<uint8_t>() : nullptr;
        a.bound_stride = (int64_t)bound_stride;
        a.out_index = d.at<int32_t>(o_index) + g0;
        a.out_method = d.at<int32_t>(o_method) + g0;
        a.out_dist = d.at<int64_t>(o_dist) + g0;
        a.n_groups = ng;
        if ((rc = timed_launch(c, st, stats, fn, "best-representative kernel", 1, [&] {
                hipLaunchKernelGGL(k_best_rep, dim3(ng), dim3(kConsThreads), 0, st, a);
            }))) return rc;
    }
    if ((rc = sg.download(d, st))) return rc;
    const hipError_t q = hipStreamSynchronize(st);
    if (q != hipSuccess) return fail(STRK_E_DEVICE, "%s: best-representative results: %s", fn, hipGetErrorString(q));
    sg.scatter();
    return 0;
}
