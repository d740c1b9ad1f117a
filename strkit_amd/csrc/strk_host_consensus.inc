// Host side of strk_best_representatives / strk_best_representatives_dseqs: input checks, pieces, launches.
// Part of strk_api.hip: included inside its anonymous namespace (uses fail(), HIP_TRY, DevBuf, strk_ctx defined there);
// not a stand-alone header.
// ---------------------------------------------------------------------------------------------
// Best representative of every group: strk_best_representatives
// ---------------------------------------------------------------------------------------------
constexpr size_t kConsBoundBudget = (size_t)256 << 20;   // bytes of last-row deltas of one piece (patterns beyond one pass only)
constexpr int kConsPieceGroups = 32768;

// `d_seqs` != nullptr: the bases are in device memory already and `seqs` is not read
int best_rep_impl(strk_ctx* c, int32_t n_groups, const int32_t* group_off, const uint8_t* seqs, const uint8_t* d_seqs,
                  int64_t n_seq_bytes, const int64_t* seq_start, const int32_t* seq_len, int32_t* out_index,
                  int32_t* out_method, int64_t* out_dist_sum, strk_stats* stats) {
    if (stats) memset(stats, 0, sizeof *stats);
    if (n_groups < 0) return fail(STRK_E_INVALID, "n_groups < 0");
    if (n_seq_bytes < 0) return fail(STRK_E_INVALID, "n_seq_bytes < 0");
    if (n_groups == 0) return 0;
    if (!group_off || !out_index || !out_method || !out_dist_sum) return fail(STRK_E_INVALID, "NULL argument");
    if (group_off[0] != 0) return fail(STRK_E_INVALID, "group_off[0] must be 0");
    for (int32_t g = 0; g < n_groups; ++g) {
        const int64_t n = (int64_t)group_off[g + 1] - group_off[g];
        if (n < 0) return fail(STRK_E_INVALID, "group %d: group_off is decreasing", g);
        if (n > kConsMaxGroup) return fail(STRK_E_INVALID, "group %d: %lld sequences (at most %d)", g, (long long)n, kConsMaxGroup);
    }
    const int32_t n_seqs = group_off[n_groups];
    if (n_seqs > 0 && (!seq_start || !seq_len)) return fail(STRK_E_INVALID, "NULL argument");
    int32_t max_len = 0;
    for (int32_t i = 0; i < n_seqs; ++i) {
        if (seq_len[i] < 0 || seq_len[i] > kConsMaxLen)
            return fail(STRK_E_INVALID, "sequence %d: length %d is outside 0..%d", i, seq_len[i], kConsMaxLen);
        if (seq_start[i] < 0 || seq_start[i] > n_seq_bytes - seq_len[i])
            return fail(STRK_E_INVALID, "sequence %d: bytes %lld..%lld lie outside the %lld given", i, (long long)seq_start[i],
                        (long long)(seq_start[i] + seq_len[i]), (long long)n_seq_bytes);
        max_len = std::max(max_len, seq_len[i]);
    }
    if (n_seq_bytes > 0 && !seqs && !d_seqs && max_len > 0) return fail(STRK_E_INVALID, "seqs is NULL");
    HIP_TRY(hipSetDevice(c->device));
    if (!c->cs_stream) HIP_TRY(hipStreamCreateWithFlags(&c->cs_stream.h, hipStreamNonBlocking));
    hipStream_t st = c->cs_stream;
    int rc;
    if ((rc = c->cs_off.ensure(((size_t)n_groups + 1) * 4))) return rc;
    if ((rc = c->cs_start.ensure(std::max<size_t>(n_seqs, 1) * 8))) return rc;
    if ((rc = c->cs_len.ensure(std::max<size_t>(n_seqs, 1) * 4))) return rc;
    if ((rc = c->cs_out.ensure((size_t)n_groups * 16))) return rc;
    if (!d_seqs) {
        if ((rc = c->cs_seqs.ensure(std::max<size_t>((size_t)n_seq_bytes, 256)))) return rc;
        if (n_seq_bytes > 0 && max_len > 0) HIP_TRY(hipMemcpyAsync(c->cs_seqs.p, seqs, (size_t)n_seq_bytes, hipMemcpyHostToDevice, st));
    }
    HIP_TRY(hipMemcpyAsync(c->cs_off.p, group_off, ((size_t)n_groups + 1) * 4, hipMemcpyHostToDevice, st));
    if (n_seqs > 0) {
        HIP_TRY(hipMemcpyAsync(c->cs_start.p, seq_start, (size_t)n_seqs * 8, hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(c->cs_len.p, seq_len, (size_t)n_seqs * 4, hipMemcpyHostToDevice, st));
    }
    // a pattern (the shorter string of a pair) beyond one pass parks a row of deltas per wave; the row is as long as the text
    const size_t bound_stride = max_len > kConsPassRows ? ((size_t)max_len + 63) & ~(size_t)63 : 0;
    const int32_t piece = bound_stride ? (int32_t)std::max<size_t>(1, std::min<size_t>(kConsPieceGroups, kConsBoundBudget / (bound_stride * kConsWaves)))
                                       : kConsPieceGroups;
    if (bound_stride && (rc = c->cs_bound.ensure((size_t)std::min(piece, n_groups) * kConsWaves * bound_stride))) return rc;
    int64_t* d_dist = c->cs_out.as<int64_t>();
    int32_t* d_index = reinterpret_cast<int32_t*>(d_dist + n_groups);
    int32_t* d_method = d_index + n_groups;
    hipEvent_t ev0 = c->ev[0], ev1 = c->ev[kNumEvents - 1];
    for (int32_t g0 = 0; g0 < n_groups; g0 += piece) {
        const int32_t ng = std::min(piece, n_groups - g0);
        ConsArgs a{};
        a.group_off = c->cs_off.as<int32_t>() + g0;
        a.seqs = d_seqs ? d_seqs : c->cs_seqs.as<uint8_t>();
        a.seq_start = c->cs_start.as<int64_t>();
        a.seq_len = c->cs_len.as<int32_t>();
        a.bound = bound_stride ? c->cs_bound.as<uint8_t>() : nullptr;
        a.bound_stride = (int64_t)bound_stride;
        a.out_index = d_index + g0;
        a.out_method = d_method + g0;
        a.out_dist = d_dist + g0;
        a.n_groups = ng;
        HIP_TRY(hipEventRecord(ev0, st));
        hipLaunchKernelGGL(k_best_rep, dim3(ng), dim3(kConsThreads), 0, st, a);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipEventRecord(ev1, st));
        const hipError_t q = hipStreamSynchronize(st);
        if (q != hipSuccess) return fail(STRK_E_DEVICE, "best-representative kernel: %s", hipGetErrorString(q));
        float ms = 0.f;
        HIP_TRY(hipEventElapsedTime(&ms, ev0, ev1));
        if (stats) {
            stats->kernel_ms += ms;
            stats->n_dp_launches += 1;
        }
    }
    HIP_TRY(hipMemcpyAsync(out_dist_sum, d_dist, (size_t)n_groups * 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(out_index, d_index, (size_t)n_groups * 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(out_method, d_method, (size_t)n_groups * 4, hipMemcpyDeviceToHost, st));
    const hipError_t q = hipStreamSynchronize(st);
    if (q != hipSuccess) return fail(STRK_E_DEVICE, "best-representative results: %s", hipGetErrorString(q));
    return 0;
}
