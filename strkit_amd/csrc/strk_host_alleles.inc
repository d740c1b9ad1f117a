// Host side of strk_call_alleles (strkit/call/allele.py:176-336 + call_locus.py:1536-1600): input checks, pieces, launches.
// Part of strk_api.hip: included inside its anonymous namespace (uses fail(), HIP_TRY, DevBuf, strk_ctx and side_stream
// defined there); not a stand-alone header.
// ---------------------------------------------------------------------------------------------
// Allele calling: strk_call_alleles
// ---------------------------------------------------------------------------------------------
constexpr size_t kAlleleWsBudget = (size_t)512 << 20;   // workspace bytes of one piece (a larger single locus runs alone)
constexpr int kAllelePieceLoci = 32768;

int call_alleles_impl(strk_ctx* c, int32_t n_loci, const int32_t* read_off, const int32_t* cn, const double* w,
                      const int32_t* n_alleles, const uint64_t* seed, const strk_allele_params* p, int32_t* out_status,
                      int32_t* out_modal_n, int32_t* out_call, int32_t* out_ci95, int32_t* out_ci99, double* out_means,
                      double* out_weights, double* out_stdevs, int32_t* out_peak_n_reads, int32_t* out_read_peak,
                      strk_stats* stats) {
    if (stats) memset(stats, 0, sizeof *stats);
    if (n_loci < 0) return fail(STRK_E_INVALID, "n_loci < 0");
    if (!p) return fail(STRK_E_INVALID, "params is NULL");
    if (n_loci == 0) return 0;
    if (!read_off || !cn || !w || !n_alleles || !seed || !out_status || !out_modal_n || !out_call || !out_ci95 || !out_ci99 ||
        !out_means || !out_weights || !out_stdevs || !out_peak_n_reads || !out_read_peak)
        return fail(STRK_E_INVALID, "NULL argument");
    if (p->num_bootstrap < 2 || p->num_bootstrap > kAlleleMaxBootstrap)
        return fail(STRK_E_INVALID, "num_bootstrap %d is outside 2..%d", p->num_bootstrap, kAlleleMaxBootstrap);
    if (p->n_init < 1 || p->n_init > kAlleleMaxInit) return fail(STRK_E_INVALID, "n_init %d is outside 1..%d", p->n_init, kAlleleMaxInit);
    if (p->min_reads < 1) return fail(STRK_E_INVALID, "min_reads must be >= 1");
    if (p->max_iter < 1) return fail(STRK_E_INVALID, "max_iter must be >= 1");
    if (p->filter_factor < 1) return fail(STRK_E_INVALID, "filter_factor must be >= 1");
    // reg_covar > 0: without it a component that collapses onto one value gets a variance of 0 (or a rounding below 0)
    // and its precision is inf / NaN
    if (!(p->tol >= 0.0) || !(p->reg_covar > 0.0) || !std::isfinite(p->tol) || !std::isfinite(p->reg_covar) ||
        !std::isfinite(p->expansion_ratio))
        return fail(STRK_E_INVALID, "tol must be finite and >= 0, reg_covar finite and > 0, expansion_ratio finite");
    if (read_off[0] != 0) return fail(STRK_E_INVALID, "read_off[0] must be 0");
    for (int32_t l = 0; l < n_loci; ++l) {
        const int64_t n = (int64_t)read_off[l + 1] - read_off[l];
        if (n < 0) return fail(STRK_E_INVALID, "locus %d: read_off is decreasing", l);
        if (n > kAlleleMaxReads) return fail(STRK_E_INVALID, "locus %d: %lld reads (at most %d)", l, (long long)n, kAlleleMaxReads);
        if (n_alleles[l] != 1 && n_alleles[l] != 2) return fail(STRK_E_INVALID, "locus %d: n_alleles %d is not 1 or 2", l, n_alleles[l]);
        for (int32_t r = read_off[l]; r < read_off[l + 1]; ++r)
            if (!std::isfinite(w[r]) || !(w[r] > 0.0)) return fail(STRK_E_INVALID, "locus %d: read %d has weight %g", l, r, w[r]);
    }
    HIP_TRY(hipSetDevice(c->device));
    hipStream_t st;
    if (const int rc = side_stream(c, &st)) return rc;
    const int B = p->num_bootstrap;
    const int threads = std::min(256, (B + 63) / 64 * 64);
    std::vector<int64_t> ws_off;
    std::vector<int32_t> off_rel, oi;
    std::vector<double> od;
    hipEvent_t ev0 = c->ev[0], ev1 = c->ev[kNumEvents - 1];
    auto locus_ws = [&](size_t l) {
        const int n = read_off[l + 1] - read_off[l];
        return (int64_t)(n >= p->min_reads ? allele_ws_bytes(n, B) : 0);
    };
    for (int32_t l0 = 0, l1; l0 < n_loci; l0 = l1) {
        // one piece: loci in caller order while their workspace fits the budget
        int64_t wsum = 0;
        l1 = (int32_t)strk_groups::cut_piece((size_t)l0, (size_t)n_loci, locus_ws, (int64_t)kAlleleWsBudget, kAllelePieceLoci,
                                             ws_off, &wsum);
        const int32_t nl = l1 - l0, r0 = read_off[l0], nr = read_off[l1] - r0;
        off_rel.resize((size_t)nl + 1);
        for (int32_t l = 0; l <= nl; ++l) off_rel[l] = read_off[l0 + l] - r0;
        int rc;
        if ((rc = c->al_off.ensure(((size_t)nl + 1) * 4))) return rc;
        if ((rc = c->al_cn.ensure(std::max<size_t>(nr, 1) * 4))) return rc;
        if ((rc = c->al_w.ensure(std::max<size_t>(nr, 1) * 8))) return rc;
        const size_t nal_bytes = ((size_t)nl * 4 + 7) & ~(size_t)7;   // n_alleles, padded so that the seeds are 8-aligned
        if ((rc = c->al_meta.ensure(nal_bytes + (size_t)nl * 16))) return rc;
        if ((rc = c->al_ws.ensure(std::max<size_t>((size_t)wsum, 256)))) return rc;
        if ((rc = c->al_out.ensure((size_t)nl * (kAlleleOutI * 4 + kAlleleOutD * 8)))) return rc;
        if ((rc = c->al_rp.ensure(std::max<size_t>(nr, 1) * 4))) return rc;
        char* meta = c->al_meta.as<char>();
        int32_t* d_nal = reinterpret_cast<int32_t*>(meta);
        uint64_t* d_seed = reinterpret_cast<uint64_t*>(meta + nal_bytes);
        int64_t* d_wsoff = reinterpret_cast<int64_t*>(reinterpret_cast<char*>(d_seed) + (size_t)nl * 8);
        HIP_TRY(hipMemcpyAsync(c->al_off.p, off_rel.data(), ((size_t)nl + 1) * 4, hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(c->al_cn.p, cn + r0, (size_t)nr * 4, hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(c->al_w.p, w + r0, (size_t)nr * 8, hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(d_nal, n_alleles + l0, (size_t)nl * 4, hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(d_seed, seed + l0, (size_t)nl * 8, hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(d_wsoff, ws_off.data(), (size_t)nl * 8, hipMemcpyHostToDevice, st));
        AlleleArgs a{};
        a.read_off = c->al_off.as<int32_t>();
        a.cn = c->al_cn.as<int32_t>();
        a.w = c->al_w.as<double>();
        a.n_alleles = d_nal;
        a.seed = d_seed;
        a.ws_off = d_wsoff;
        a.ws = c->al_ws.as<char>();
        a.out_i = c->al_out.as<int32_t>();
        a.out_d = reinterpret_cast<double*>(c->al_out.as<char>() + (size_t)nl * kAlleleOutI * 4);
        a.read_peak = c->al_rp.as<int32_t>();
        a.n_loci = nl;
        a.min_reads = p->min_reads;
        a.min_allele_reads = p->min_allele_reads;
        a.B = B;
        a.n_init = p->n_init;
        a.max_iter = p->max_iter;
        a.filter_factor = p->filter_factor;
        a.force_gm_filter = p->force_gm_filter;
        a.tol = p->tol;
        a.reg_covar = p->reg_covar;
        a.expansion_ratio = p->expansion_ratio;
        HIP_TRY(hipEventRecord(ev0, st));
        hipLaunchKernelGGL(k_alleles, dim3(nl), dim3(threads), 0, st, a);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipEventRecord(ev1, st));
        oi.resize((size_t)nl * kAlleleOutI);
        od.resize((size_t)nl * kAlleleOutD);
        HIP_TRY(hipMemcpyAsync(oi.data(), a.out_i, oi.size() * 4, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipMemcpyAsync(od.data(), a.out_d, od.size() * 8, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipMemcpyAsync(out_read_peak + r0, a.read_peak, (size_t)nr * 4, hipMemcpyDeviceToHost, st));
        const hipError_t q = hipStreamSynchronize(st);
        if (q != hipSuccess) return fail(STRK_E_DEVICE, "allele kernel: %s", hipGetErrorString(q));
        float ms = 0.f;
        HIP_TRY(hipEventElapsedTime(&ms, ev0, ev1));
        if (stats) {
            stats->kernel_ms += ms;
            stats->n_dp_launches += 1;
        }
        for (int32_t l = 0; l < nl; ++l) {
            const int32_t* s = oi.data() + (size_t)l * kAlleleOutI;
            const double* t = od.data() + (size_t)l * kAlleleOutD;
            const size_t g = (size_t)(l0 + l);
            out_status[g] = s[0];
            out_modal_n[g] = s[1];
            for (int e = 0; e < 2; ++e) {
                out_call[2 * g + e] = s[2 + e];
                out_peak_n_reads[2 * g + e] = s[12 + e];
                out_means[2 * g + e] = t[e];
                out_weights[2 * g + e] = t[2 + e];
                out_stdevs[2 * g + e] = t[4 + e];
            }
            for (int e = 0; e < 4; ++e) {
                out_ci95[4 * g + e] = s[4 + e];
                out_ci99[4 * g + e] = s[8 + e];
            }
        }
    }
    return 0;
}
