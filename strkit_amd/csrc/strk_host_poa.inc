// Host side of strk_consensus / strk_consensus_dseqs / strk_consensus_ws: input checks, the method of every group, launches
// of k_poa cut at a group count and at a workspace bound, the best-representative path for the rest, the bytes' gather.
// Part of strk_api.hip: included inside its anonymous namespace (uses fail(), HIP_TRY, DevBuf, Staging, strk_ctx, check_groups,
// side_stream, timed_launch and best_rep_impl defined there); not a stand-alone header.
// ---------------------------------------------------------------------------------------------
// Allele sequences by partial-order alignment: strk_consensus
// ---------------------------------------------------------------------------------------------
constexpr int64_t kPoaWsBytes = (int64_t)4 << 30;   // workspace of one launch of k_poa (a group beyond it runs alone)
constexpr int kPoaPieceGroups = 8192;               // groups of one launch

// `d_seqs` != nullptr: the bases are in device memory already and `seqs` is not read.  node_limit <= 0: kPoaMaxNodes;
// ws_bytes <= 0: kPoaWsBytes.
int64_t consensus_impl(strk_ctx* c, const char* fn, int32_t n_groups, const int32_t* group_off, const uint8_t* seqs,
                       const uint8_t* d_seqs, int64_t n_seq_bytes, const int64_t* seq_start, const int32_t* seq_len,
                       int32_t max_mdn, int64_t cap, int32_t* out_index, int32_t* out_method, int64_t* out_seq_off,
                       uint8_t* out_seqs, int32_t node_limit, int64_t ws_bytes, strk_stats* stats) {
    if (stats) memset(stats, 0, sizeof *stats);
    const strk_groups::View view{n_groups, group_off, n_seq_bytes, seq_start, seq_len};
    strk_groups::Totals tot;
    int rc;
    if ((rc = check_groups(fn, view, kConsMaxGroup, kConsMaxLen, &tot))) return rc;
    if (max_mdn < 0) return fail(STRK_E_INVALID, "%s: max_mdn_poa_length < 0", fn);
    if (cap < 0) return fail(STRK_E_INVALID, "%s: cap < 0", fn);
    if (node_limit > kPoaMaxNodes) return fail(STRK_E_INVALID, "%s: node_limit %d (at most %d)", fn, node_limit, kPoaMaxNodes);
    if (!out_seq_off) return fail(STRK_E_INVALID, "%s: out_seq_off is NULL", fn);
    if (cap > 0 && !out_seqs) return fail(STRK_E_INVALID, "%s: cap > 0 with out_seqs NULL", fn);
    if (n_groups > 0 && (!out_index || !out_method)) return fail(STRK_E_INVALID, "%s: NULL argument", fn);
    if (tot.total_len > 0 && !seqs && !d_seqs) return fail(STRK_E_INVALID, "%s: seqs is NULL", fn);
    static_assert(kPoaMaxGroup == kConsMaxGroup, "strk_poa.h <-> strk_consensus.h");
    out_seq_off[0] = 0;
    if (n_groups == 0) return 0;
    if (node_limit <= 0) node_limit = kPoaMaxNodes;
    if (ws_bytes <= 0) ws_bytes = kPoaWsBytes;
    const int64_t ws_ints = std::max<int64_t>(1, ws_bytes / 4);

    // The method of every group as far as lengths decide it.  route: 0 = k_poa, 1 = best representative by the median rule
    // (or no string at all), 2 = best representative because a string is beyond the kernel's rows.
    const size_t ng = (size_t)n_groups;
    std::vector<uint8_t> route(ng, 0);
    std::vector<int32_t> poa_list;
    std::vector<int32_t> sorted_len;
    struct Piece { int64_t ints; int32_t node_cap, edge_cap, row_len; };
    std::vector<Piece> need;          // per entry of poa_list
    std::vector<int64_t> pool_of(ng, -1);
    int64_t pool_bytes = 0;
    for (int32_t g = 0; g < n_groups; ++g) {
        const int32_t a = group_off[g], n = group_off[g + 1] - a;
        if (n == 0) {
            route[(size_t)g] = 1;
            continue;
        }
        sorted_len.assign(seq_len + a, seq_len + a + n);
        std::nth_element(sorted_len.begin(), sorted_len.begin() + n / 2, sorted_len.end());
        const int32_t mdn = sorted_len[(size_t)(n / 2)];
        int64_t sum = 0;
        int32_t longest = 0;
        for (int32_t i = a; i < a + n; ++i) {
            sum += seq_len[i];
            longest = std::max(longest, seq_len[i]);
        }
        if (mdn > max_mdn) route[(size_t)g] = 1;
        else if (longest > kPoaMaxLen) route[(size_t)g] = 2;
        else {
            Piece p;
            p.node_cap = (int32_t)std::max<int64_t>(1, std::min<int64_t>(sum, node_limit));
            p.edge_cap = (int32_t)std::max<int64_t>(1, sum);
            p.row_len = longest + 1;
            p.ints = (int64_t)p.node_cap * (kPoaNodeArrays + p.row_len) + (int64_t)p.edge_cap * kPoaEdgeArrays + p.row_len;
            p.ints = (p.ints + 63) & ~(int64_t)63;
            poa_list.push_back(g);
            need.push_back(p);
            pool_of[(size_t)g] = pool_bytes;
            pool_bytes += p.node_cap;
        }
    }

    HIP_TRY(hipSetDevice(c->device));
    hipStream_t st;
    if ((rc = side_stream(c, &st))) return rc;
    // What the whole call holds, in one staged buffer sized here once: the view, where each group's consensus lies in the pool,
    // and the results, which start as zeros.  Its image is the call's own (strk_ctx::po_image).
    Staging sg(c->po_image);
    const StagedGroups s_in = stage_groups(sg, view, tot, seqs, d_seqs);
    const size_t i_poolof = sg.put(pool_of.data(), ng * 8);
    const size_t o_cells = sg.zero(8), o_index = sg.zero(ng * 4), o_method = sg.zero(ng * 4), o_len = sg.zero(ng * 4), o_state = sg.zero(ng * 4);
    if ((rc = c->po_pool.ensure(std::max<size_t>((size_t)pool_bytes, 256)))) return rc;
    if ((rc = sg.upload(c->po_call, st))) return rc;
    const DevBuf& d = c->po_call;
    const StagedGroups::Ptrs in = s_in.on(d);

    // k_poa over its groups, in pieces
    std::vector<int64_t> ws_off, pool_off;
    std::vector<int32_t> caps;
    for (size_t p0 = 0, p1; p0 < poa_list.size(); p0 = p1) {
        int64_t used = 0;
        p1 = strk_groups::cut_piece(p0, poa_list.size(), [&](size_t p) { return need[p].ints; }, ws_ints, kPoaPieceGroups,
                                    ws_off, &used);
        const int32_t n_piece = (int32_t)(p1 - p0);
        pool_off.resize((size_t)n_piece);
        caps.resize((size_t)n_piece * 3);
        for (int32_t k = 0; k < n_piece; ++k) {
            pool_off[(size_t)k] = pool_of[(size_t)poa_list[p0 + k]];
            caps[(size_t)k] = need[p0 + k].node_cap;
            caps[(size_t)n_piece + k] = need[p0 + k].edge_cap;
            caps[(size_t)2 * n_piece + k] = need[p0 + k].row_len;
        }
        if ((rc = c->po_ws.ensure((size_t)used * 4, false))) return rc;
        Staging ps(c->image);
        const size_t i_wsoff = ps.put(ws_off.data(), (size_t)n_piece * 8), i_pooloff = ps.put(pool_off.data(), (size_t)n_piece * 8),
                     i_list = ps.put(poa_list.data() + p0, (size_t)n_piece * 4), i_ncap = ps.put(caps.data(), (size_t)n_piece * 4),
                     i_ecap = ps.put(caps.data() + n_piece, (size_t)n_piece * 4), i_rlen = ps.put(caps.data() + 2 * (size_t)n_piece, (size_t)n_piece * 4);
        if ((rc = ps.upload(c->po_piece, st))) return rc;
        const DevBuf& dp = c->po_piece;
        PoaArgs a{};
        a.list = dp.at<int32_t>(i_list);
        a.group_off = in.off;
        a.seqs = in.seqs;
        a.seq_start = in.start;
        a.seq_len = in.len;
        a.ws = c->po_ws.as<int32_t>();
        a.ws_off = dp.at<int64_t>(i_wsoff);
        a.node_cap = dp.at<int32_t>(i_ncap);
        a.edge_cap = dp.at<int32_t>(i_ecap);
        a.row_len = dp.at<int32_t>(i_rlen);
        a.pool = c->po_pool.as<uint8_t>();
        a.pool_off = dp.at<int64_t>(i_pooloff);
        a.out_index = d.at<int32_t>(o_index);
        a.out_method = d.at<int32_t>(o_method);
        a.out_len = d.at<int32_t>(o_len);
        a.out_state = d.at<int32_t>(o_state);
        a.cells = d.at<unsigned long long>(o_cells);
        a.n_list = n_piece;
        if ((rc = timed_launch(c, st, stats, fn, "POA kernel", 1, [&] {
                hipLaunchKernelGGL(k_poa, dim3(n_piece), dim3(kPoaThreads), 0, st, a);
            }))) return rc;
        if (stats) stats->n_sub_batches += 1;
    }
    if ((rc = sg.download(d, o_cells, o_state + ng * 4, st))) return rc;
    {
        const hipError_t q = hipStreamSynchronize(st);   // (the bases are on the device now as well)
        if (q != hipSuccess) return fail(STRK_E_DEVICE, "%s: POA results: %s", fn, hipGetErrorString(q));
    }
    if (stats) stats->dp_cells = (int64_t)*sg.at<unsigned long long>(o_cells);
    // the results where they came down: the best-representative pass below fills in its groups
    int32_t* r_index = sg.mut<int32_t>(o_index);
    int32_t* r_method = sg.mut<int32_t>(o_method);
    int32_t* r_len = sg.mut<int32_t>(o_len);
    const int32_t* r_state = sg.at<int32_t>(o_state);
    for (int32_t g : poa_list) {
        if (r_state[g] == kPoaBroken) return fail(STRK_E_DEVICE, "%s: group %d: the POA kernel lost its trace-back", fn, g);
        if (r_state[g] == kPoaOverflow) route[(size_t)g] = 2;
    }
    // the best representatives of the rest: the existing path, over a packed copy of those groups
    std::vector<int32_t> rest;
    for (int32_t g = 0; g < n_groups; ++g)
        if (route[(size_t)g]) rest.push_back(g);
    if (!rest.empty()) {
        std::vector<int32_t> b_off(rest.size() + 1, 0), b_len, b_index(rest.size()), b_method(rest.size());
        std::vector<int64_t> b_start, b_dist(rest.size());
        for (size_t k = 0; k < rest.size(); ++k) {
            const int32_t a = group_off[rest[k]], b = group_off[rest[k] + 1];
            b_start.insert(b_start.end(), seq_start + a, seq_start + b);
            b_len.insert(b_len.end(), seq_len + a, seq_len + b);
            b_off[k + 1] = (int32_t)b_len.size();
        }
        strk_stats bs;
        if ((rc = best_rep_impl(c, fn, (int32_t)rest.size(), b_off.data(), nullptr, in.seqs, n_seq_bytes, b_start.data(), b_len.data(),
                                b_index.data(), b_method.data(), b_dist.data(), &bs))) return rc;
        if (stats) {
            stats->kernel_ms += bs.kernel_ms;
            stats->n_dp_launches += bs.n_dp_launches;
        }
        for (size_t k = 0; k < rest.size(); ++k) {
            const int32_t g = rest[k];
            r_index[g] = b_index[k];
            r_method[g] = b_method[k];
            r_len[g] = b_method[k] == kConsNone ? 0 : seq_len[group_off[g] + b_index[k]];
            if (stats && route[(size_t)g] == 2 && b_method[k] == kConsBestRep) stats->n_fallback += 1;
        }
    }
    for (int32_t g = 0; g < n_groups; ++g) {
        out_index[g] = r_index[g];
        out_method[g] = r_method[g];
        out_seq_off[g + 1] = out_seq_off[g] + r_len[g];
    }
    const int64_t n_bytes = out_seq_off[n_groups];
    if (n_bytes > cap || n_bytes == 0) return n_bytes;
    // the bytes of every group, gathered on the device
    if ((rc = c->po_out.ensure((size_t)n_bytes))) return rc;
    Staging gs(c->image);
    const size_t i_outoff = gs.put(out_seq_off, (ng + 1) * 8), i_index = gs.put(r_index, ng * 4), i_method = gs.put(r_method, ng * 4);
    if ((rc = gs.upload(c->po_piece, st))) return rc;
    PoaGatherArgs ga{};
    ga.group_off = in.off;
    ga.seqs = in.seqs;
    ga.seq_start = in.start;
    ga.index = c->po_piece.at<int32_t>(i_index);
    ga.method = c->po_piece.at<int32_t>(i_method);
    ga.out_off = c->po_piece.at<int64_t>(i_outoff);
    ga.pool = c->po_pool.as<uint8_t>();
    ga.pool_of = d.at<int64_t>(i_poolof);
    ga.out = c->po_out.as<uint8_t>();
    ga.n_groups = n_groups;
    if ((rc = timed_launch(c, st, stats, fn, "gather kernel", 1, [&] {
            hipLaunchKernelGGL(k_poa_gather, dim3(n_groups), dim3(256), 0, st, ga);
        }))) return rc;
    HIP_TRY(hipMemcpyAsync(out_seqs, c->po_out.p, (size_t)n_bytes, hipMemcpyDeviceToHost, st));
    const hipError_t q = hipStreamSynchronize(st);
    if (q != hipSuccess) return fail(STRK_E_DEVICE, "%s: results: %s", fn, hipGetErrorString(q));
    return n_bytes;
}
