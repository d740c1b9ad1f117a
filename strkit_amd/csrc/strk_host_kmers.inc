// Host side of strk_count_kmers / strk_count_kmers_dseqs / strk_count_kmers_ws: input checks, launch lists, pieces, prefix sums.
// Part of strk_api.hip: included inside its anonymous namespace (uses fail(), HIP_TRY, DevBuf, Staging, strk_ctx, check_groups,
// side_stream and timed_launch defined there); not a stand-alone header.
// ---------------------------------------------------------------------------------------------
// Distinct windows of every group: strk_count_kmers
// ---------------------------------------------------------------------------------------------
constexpr int64_t kKmerWsBytes = (int64_t)1 << 30;   // elements of one launch of k_kmers_sort (a group beyond it runs alone)

// `d_seqs` != nullptr: the bases are in device memory already and `seqs` is not read.  ws_bytes <= 0: kKmerWsBytes.
int64_t count_kmers_impl(strk_ctx* c, const char* fn, int32_t n_groups, const int32_t* group_off, const uint8_t* seqs,
                         const uint8_t* d_seqs, int64_t n_seq_bytes, const int64_t* seq_start, const int32_t* seq_len,
                         const int32_t* k, int64_t cap, int64_t* out_entry_off, int64_t* out_pos, int32_t* out_count,
                         int64_t ws_bytes, strk_stats* stats) {
    if (stats) memset(stats, 0, sizeof *stats);
    const strk_groups::View view{n_groups, group_off, n_seq_bytes, seq_start, seq_len};
    strk_groups::Totals tot;
    int rc;
    if ((rc = check_groups(fn, view, kKmerMaxGroup, kKmerMaxLen, &tot))) return rc;
    if (cap < 0) return fail(STRK_E_INVALID, "%s: cap < 0", fn);
    if (!out_entry_off) return fail(STRK_E_INVALID, "%s: out_entry_off is NULL", fn);
    if (cap > 0 && (!out_pos || !out_count)) return fail(STRK_E_INVALID, "%s: cap > 0 with a NULL output array", fn);
    if (n_groups > 0 && !k) return fail(STRK_E_INVALID, "%s: NULL argument", fn);
    for (int32_t g = 0; g < n_groups; ++g)
        if (k[g] < 1) return fail(STRK_E_INVALID, "%s: group %d: window length %d (at least 1)", fn, g, k[g]);
    // windows per group; the launch lists of the table kernel (a group without windows has no entries and no workgroup)
    std::vector<int64_t> windows((size_t)n_groups, 0);
    std::vector<int32_t> lists;   // small | large
    std::vector<int32_t> large;
    int64_t total_windows = 0;
    for (int32_t g = 0; g < n_groups; ++g) {
        int64_t w = 0;
        for (int32_t i = group_off[g]; i < group_off[g + 1]; ++i) w += std::max(seq_len[i] - k[g] + 1, 0);
        windows[(size_t)g] = w;
        total_windows += w;
        if (w > kKmerSmallSlots - kKmerSmallSlots / 4) large.push_back(g);
        else if (w > 0) lists.push_back(g);
    }
    const int32_t n_small = (int32_t)lists.size(), n_large = (int32_t)large.size();
    lists.insert(lists.end(), large.begin(), large.end());
    if (total_windows > 0 && !seqs && !d_seqs) return fail(STRK_E_INVALID, "%s: seqs is NULL", fn);
    out_entry_off[0] = 0;
    if (total_windows == 0) {
        for (int32_t g = 0; g < n_groups; ++g) out_entry_off[g + 1] = 0;
        return 0;
    }
    if (stats) stats->dp_cells = total_windows;
    if (ws_bytes <= 0) ws_bytes = kKmerWsBytes;
    const int64_t ws_elems = std::max<int64_t>(1, ws_bytes / (int64_t)sizeof(KmerElem));

    HIP_TRY(hipSetDevice(c->device));
    hipStream_t st;
    if ((rc = side_stream(c, &st))) return rc;
    const size_t ng = (size_t)n_groups;
    // what the whole call holds, in one staged buffer sized here once; cnt | state start as zeros, and the entry offsets go up
    // before each write pass (below)
    Staging sg(c->image);
    const StagedGroups s_in = stage_groups(sg, view, tot, seqs, d_seqs);
    const size_t i_k = sg.put(k, ng * 4), i_small = sg.put(lists.data(), (size_t)n_small * 4),
                 i_large = sg.put(lists.data() + n_small, (size_t)n_large * 4), i_cnt = sg.zero(ng * 4), i_state = sg.zero(ng * 4),
                 i_eoff = sg.room((ng + 1) * 8);
    if ((rc = sg.upload(c->km_call, st))) return rc;
    const DevBuf& d = c->km_call;
    const StagedGroups::Ptrs in = s_in.on(d);

    KmerArgs a{};
    a.group_off = in.off;
    a.seqs = in.seqs;
    a.seq_start = in.start;
    a.seq_len = in.len;
    a.k = d.at<int32_t>(i_k);
    a.cnt = d.at<int32_t>(i_cnt);
    a.state = d.at<int32_t>(i_state);
    a.entry_off = d.at<int64_t>(i_eoff);
    auto table_pass = [&](int mode) {
        KmerArgs t = a;
        t.mode = mode;
        if (n_small) {
            t.list = d.at<int32_t>(i_small);
            t.n_list = n_small;
            hipLaunchKernelGGL(k_kmers_hash<kKmerSmallSlots>, dim3(n_small), dim3(kKmerHashThreads), 0, st, t);
        }
        if (n_large) {
            t.list = d.at<int32_t>(i_large);
            t.n_list = n_large;
            hipLaunchKernelGGL(k_kmers_hash<kKmerLargeSlots>, dim3(n_large), dim3(kKmerHashThreads), 0, st, t);
        }
    };
    // pass 1: the entries of every group the table takes
    if ((rc = timed_launch(c, st, stats, fn, "table kernel (count)", (n_small > 0) + (n_large > 0), [&] { table_pass(kKmerCount); }))) return rc;
    std::vector<int32_t> cnt(ng), state(ng);
    HIP_TRY(hipMemcpyAsync(cnt.data(), a.cnt, ng * 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(state.data(), a.state, ng * 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    std::vector<int32_t> sorted;   // the groups left to k_kmers_sort, ascending
    for (int32_t i = n_small; i < n_small + n_large; ++i) {
        const int32_t g = lists[(size_t)i];
        if (cnt[(size_t)g] < 0) sorted.push_back(g);
        if (stats && state[g] == kKmerSpilled) stats->n_fallback += 1;
        if (stats && state[g] == kKmerGeneral) stats->n_miss_reads += 1;
    }
    for (int32_t i = 0; i < n_small; ++i) {   // (a small group is never spilled: long windows only)
        const int32_t g = lists[(size_t)i];
        if (cnt[(size_t)g] < 0) sorted.push_back(g);
        if (stats && state[g] == kKmerGeneral) stats->n_miss_reads += 1;
    }
    std::sort(sorted.begin(), sorted.end());
    // the output on the device: as many entries as the caller can take, and never more than there are windows
    const int64_t n_out = std::min(cap, total_windows);
    if (n_out > 0 && (rc = c->km_out.ensure((size_t)n_out * 12))) return rc;
    a.out_pos = c->km_out.as<int64_t>();
    a.out_count = c->km_out.at<int32_t>((size_t)n_out * 8);
    // pieces of the sorted groups: sort + count, and, while the entries still fit, write (the workspace holds the runs)
    int32_t done = 0;   // out_entry_off[0..done] is final
    auto prefix_to = [&](int32_t g_end) {
        for (; done < g_end; ++done) out_entry_off[done + 1] = out_entry_off[done] + cnt[(size_t)done];
    };
    std::vector<int64_t> ws_off;
    auto sort_elems = [&](size_t p) {   // the power of two above the group's window count
        int64_t pow2 = 1;
        while (pow2 < windows[(size_t)sorted[p]]) pow2 <<= 1;
        return pow2;
    };
    for (size_t p0 = 0, p1; p0 < sorted.size(); p0 = p1) {
        int64_t used = 0;
        p1 = strk_groups::cut_piece(p0, sorted.size(), sort_elems, ws_elems, strk_groups::kNoItemCap, ws_off, &used);
        const int32_t n_piece = (int32_t)(p1 - p0);
        if ((rc = c->km_ws.ensure((size_t)used * sizeof(KmerElem)))) return rc;
        Staging ps(c->image);   // (the stream has been waited on since the call's own upload)
        const size_t i_slist = ps.put(sorted.data() + p0, (size_t)n_piece * 4), i_wsoff = ps.put(ws_off.data(), (size_t)n_piece * 8);
        if ((rc = ps.upload(c->km_piece, st))) return rc;
        KmerArgs s = a;
        s.list = c->km_piece.at<int32_t>(i_slist);
        s.n_list = n_piece;
        s.ws = c->km_ws.as<KmerElem>();
        s.ws_off = c->km_piece.at<int64_t>(i_wsoff);
        s.mode = kKmerCount;
        if ((rc = timed_launch(c, st, stats, fn, "sort kernel", 1, [&] {
                hipLaunchKernelGGL(k_kmers_sort, dim3(n_piece), dim3(kKmerSortThreads), 0, st, s);
            }))) return rc;
        HIP_TRY(hipMemcpyAsync(cnt.data(), a.cnt, ng * 4, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        const int32_t g_end = sorted[p1 - 1] + 1;
        prefix_to(g_end);
        if (out_entry_off[g_end] <= n_out) {
            HIP_TRY(hipMemcpyAsync(d.at<int64_t>(i_eoff), out_entry_off, (size_t)g_end * 8, hipMemcpyHostToDevice, st));
            s.mode = kKmerWrite;
            if ((rc = timed_launch(c, st, stats, fn, "sort kernel (write)", 1, [&] {
                    hipLaunchKernelGGL(k_kmers_sort, dim3(n_piece), dim3(kKmerSortThreads), 0, st, s);
                }))) return rc;
        }
        if (stats) stats->n_sub_batches += 1;
    }
    prefix_to(n_groups);
    const int64_t n_entries = out_entry_off[n_groups];
    if (n_entries > cap) return n_entries;
    // pass 2: the table kernel writes its groups' entries
    HIP_TRY(hipMemcpyAsync(d.at<int64_t>(i_eoff), out_entry_off, ng * 8, hipMemcpyHostToDevice, st));
    if ((rc = timed_launch(c, st, stats, fn, "table kernel (write)", (n_small > 0) + (n_large > 0), [&] { table_pass(kKmerWrite); }))) return rc;
    HIP_TRY(hipMemcpyAsync(out_pos, a.out_pos, (size_t)n_entries * 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(out_count, a.out_count, (size_t)n_entries * 4, hipMemcpyDeviceToHost, st));
    const hipError_t q = hipStreamSynchronize(st);
    if (q != hipSuccess) return fail(STRK_E_DEVICE, "%s: results: %s", fn, hipGetErrorString(q));
    return n_entries;
}
