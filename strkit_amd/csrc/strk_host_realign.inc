// Host side of strk_realign (strkit/call/realign.py:56-72): what needs the device.  The input check, the chunks by trace budget
// and the layout of a chunk's workspaces are strk_realign_plan.h's.
// Part of strk_api.hip: included inside its anonymous namespace (uses fail(), HIP_TRY, DevBuf, Carve, strk_ctx, side_stream and
// timed_launch defined there); not a stand-alone header.
// ---------------------------------------------------------------------------------------------
// Realignment: strk_realign (strkit/call/realign.py:56-72)
// ---------------------------------------------------------------------------------------------
// Launches the DP kernel of one column class on pairs [first, first + count) of a.pairs (persistent grid).
template <int CL, bool EXT0>
void launch_realign_dp_t(const RealignArgs& a, int first, int count, int qslot, int device, hipStream_t st) {
    static int resident = 0;   // blocks that fit the device (queried once per instantiation)
    if (resident == 0) {
        int per_cu = 0, cus = 0;
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, k_realign_dp<CL, EXT0>, 256, 0) != hipSuccess) per_cu = 1;
        if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess) cus = 256;
        resident = std::max(1, per_cu) * std::max(1, cus);
    }
    const int blocks = std::min(resident, (count + 3) / 4);
    hipLaunchKernelGGL((k_realign_dp<CL, EXT0>), dim3(blocks), dim3(256), 0, st, a, first, count, qslot);
}
void launch_realign_dp(int cl, bool ext0, const RealignArgs& a, int first, int count, int qslot, int device, hipStream_t st) {
    switch (cl) {
        case 4: ext0 ? launch_realign_dp_t<4, true>(a, first, count, qslot, device, st) : launch_realign_dp_t<4, false>(a, first, count, qslot, device, st); break;
        case 8: ext0 ? launch_realign_dp_t<8, true>(a, first, count, qslot, device, st) : launch_realign_dp_t<8, false>(a, first, count, qslot, device, st); break;
        case 16: ext0 ? launch_realign_dp_t<16, true>(a, first, count, qslot, device, st) : launch_realign_dp_t<16, false>(a, first, count, qslot, device, st); break;
        default: ext0 ? launch_realign_dp_t<32, true>(a, first, count, qslot, device, st) : launch_realign_dp_t<32, false>(a, first, count, qslot, device, st); break;
    }
}

int realign_impl(strk_ctx* c, int32_t n_pairs, const uint8_t* s1, const int64_t* s1_off, const uint8_t* s2,
                 const int64_t* s2_off, int32_t open, int32_t ext, int32_t gap_pref, int32_t* out_score,
                 int32_t* out_end_ref, int32_t* out_n_cigar, uint32_t* cigar, const int64_t* cigar_off, strk_stats* stats) {
    if (stats) memset(stats, 0, sizeof *stats);
    if (n_pairs > 0 && (!s1 || !s2 || !out_score || !out_end_ref || !out_n_cigar || !cigar)) return fail(STRK_E_INVALID, "NULL argument");
    size_t trace_budget = (size_t)16 << 30;
    if (const char* e = getenv("STRKIT_AMD_TRACE_BYTES")) trace_budget = std::max<size_t>((size_t)strtoull(e, nullptr, 10), 1 << 20);
    strk_realign_plan::Plan plan;
    strk_groups::Message why;
    int rc;
    if ((rc = strk_realign_plan::plan(n_pairs, s1_off, s2_off, cigar_off, open, ext, gap_pref, trace_budget, &plan, &why)))
        return fail(rc, "%s", why.text);
    if (plan.chunks.empty()) return 0;
    HIP_TRY(hipSetDevice(c->device));
    hipStream_t st;
    if ((rc = side_stream(c, &st))) return rc;

    // what the call sizes once: the bases of both sides, and 64 bytes of queue counters (at 0) and the cell count (at 32)
    const size_t s1_bytes = (size_t)(s1_off[n_pairs] - s1_off[0]), s2_bytes = (size_t)(s2_off[n_pairs] - s2_off[0]);
    Carve call;
    const size_t at_s1 = call.take(s1_bytes + 16), at_s2 = call.take(s2_bytes + 16), at_queue = call.take(64);
    if ((rc = c->rl_call.ensure(call.bytes))) return rc;
    HIP_TRY(hipMemcpyAsync(c->rl_call.at<char>(at_s1), s1 + s1_off[0], s1_bytes, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(c->rl_call.at<char>(at_s2), s2 + s2_off[0], s2_bytes, hipMemcpyHostToDevice, st));

    for (const strk_realign_plan::Chunk& ch : plan.chunks) {
        const int p0 = ch.p0, n = ch.p1 - ch.p0;
        const RealignPair* chunk = plan.pairs.data() + p0;
        Carve cv;
        const size_t at_pairs = cv.take((size_t)n * sizeof(RealignPair)), at_trace = cv.take(ch.tsum + 256),
                     at_edge = cv.take(std::max<size_t>(ch.esum, 1) * 4), at_out = cv.take((size_t)n * 3 * 4),
                     at_cigar = cv.take(std::max<size_t>(ch.csum, 1) * 4);
        if ((rc = c->rl_chunk.ensure(cv.bytes))) return rc;
        RealignArgs a{};
        a.pairs = c->rl_chunk.at<RealignPair>(at_pairs); a.n_pairs = n; a.open = open; a.ext = ext; a.gap_pref = gap_pref;
        a.s1 = c->rl_call.at<uint8_t>(at_s1); a.s2 = c->rl_call.at<uint8_t>(at_s2);
        a.trace = c->rl_chunk.at<uint8_t>(at_trace); a.edge = c->rl_chunk.at<int32_t>(at_edge);
        a.score = c->rl_chunk.at<int32_t>(at_out); a.end2 = a.score + n; a.n_cigar = a.score + 2 * n;
        a.cigar = c->rl_chunk.at<uint32_t>(at_cigar);
        a.queue = c->rl_call.at<int32_t>(at_queue); a.cells = c->rl_call.at<unsigned long long>(at_queue + 32);
        HIP_TRY(hipMemcpyAsync(c->rl_chunk.at<char>(at_pairs), chunk, (size_t)n * sizeof(RealignPair), hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemsetAsync(a.queue, 0, 64, st));
        std::vector<int32_t> o((size_t)n * 3);
        std::vector<uint32_t> cg(std::max<size_t>(ch.csum, 1));
        unsigned long long cells = 0;
        // (the wait is a watchdog: the chunk's cells at a pessimistic 1 GCUPS, plus a minute)
        rc = timed_launch(c, st, stats, nullptr, "realignment kernels", 1, [&] {
            for (int first = 0, q = 0; first < n; ++q) {
                int cnt = 1;
                while (first + cnt < n && chunk[first + cnt].cl == chunk[first].cl) ++cnt;
                launch_realign_dp(chunk[first].cl, ext == 0, a, first, cnt, q, c->device, st);
                first += cnt;
            }
            hipLaunchKernelGGL(k_realign_trace, dim3((n + 63) / 64), dim3(64), 0, st, a);
        }, [&] {
            HIP_TRY(hipMemcpyAsync(o.data(), a.score, (size_t)n * 3 * 4, hipMemcpyDeviceToHost, st));
            HIP_TRY(hipMemcpyAsync(cg.data(), a.cigar, ch.csum * 4, hipMemcpyDeviceToHost, st));
            HIP_TRY(hipMemcpyAsync(&cells, a.cells, 8, hipMemcpyDeviceToHost, st));
            return 0;
        }, 60.0 + ch.cells / 1e9);
        if (rc) return rc;
        if (stats) {
            stats->dp_kernel_ms = stats->kernel_ms;   // (this call's kernels are all DP)
            stats->dp_cells += (int64_t)cells;
            stats->exact_bytes += (int64_t)ch.tsum;   // trace bytes written (the kernel's real HBM traffic)
        }
        for (int k = 0; k < n; ++k) {
            const RealignPair& r = chunk[k];
            const int p = r.orig + p0;
            out_score[p] = o[r.orig];
            out_end_ref[p] = o[(size_t)n + r.orig];
            const int32_t nc = o[(size_t)2 * n + r.orig];
            if (nc < 0) return fail(STRK_E_INVALID, "pair %d: CIGAR capacity %d too small", p, r.cig_cap);
            out_n_cigar[p] = nc;
            memcpy(cigar + cigar_off[p], cg.data() + r.cig_off, (size_t)nc * 4);
        }
    }
    return 0;
}
