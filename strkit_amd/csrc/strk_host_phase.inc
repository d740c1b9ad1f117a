// Host side of strk_call_alleles_phased (call_locus.py:1381-1495 without the file front end; DESIGN.md §13): input checks
// (strk_phase_check.h), pieces, launches.  What it shares with strk_call_alleles is in strk_host_alleles.inc.
// Part of strk_api.hip: included inside its anonymous namespace (uses fail(), HIP_TRY, DevBuf and Carve of strk_host.h, and
// strk_ctx, side_stream and timed_launch defined there); not a stand-alone header.
// ---------------------------------------------------------------------------------------------
// Phased allele calls: strk_call_alleles_phased
// ---------------------------------------------------------------------------------------------
struct PhaseOut {
    AlleleOut al;
    int32_t *method, *reason, *ps, *snv_status;
    uint8_t* snv_call;
    int32_t* snv_rcs;
};

int call_alleles_phased_impl(strk_ctx* c, const char* fn, const strk_phase_check::Input& in, const PhaseOut& out, strk_stats* stats) {
    if (stats) memset(stats, 0, sizeof *stats);
    std::vector<int64_t> cell_off;
    {
        strk_groups::Message m;
        const strk_phase_check::Limits lim{kPhaseMaxReads, kPhaseMaxSnvs, kAlleleMaxBootstrap, kAlleleMaxInit};
        if (const int rc = strk_phase_check::check(in, lim, cell_off, &m)) return fail(rc, "%s: %s", fn, m.text);
    }
    const int32_t n_loci = in.n_loci;
    if (n_loci == 0) return 0;
    const bool snvs = in.snv_off != nullptr, tags = in.hp != nullptr;
    if (!out.al.complete() || !out.method || !out.reason || !out.ps) return fail(STRK_E_INVALID, "%s: NULL argument", fn);
    if (snvs && in.snv_off[n_loci] > 0 && (!out.snv_status || !out.snv_call || !out.snv_rcs))
        return fail(STRK_E_INVALID, "%s: NULL argument (SNV outputs)", fn);
    const strk_allele_params* p = in.p;
    const strk_phase_params* pp = in.pp;
    const int32_t* read_off = in.read_off;
    HIP_TRY(hipSetDevice(c->device));
    hipStream_t st;
    if (const int rc = side_stream(c, &st)) return rc;
    const int B = p->num_bootstrap;
    const int64_t budget = pp->ws_budget > 0 ? pp->ws_budget : (int64_t)kAlleleWsBudget;
    const size_t piece_loci = pp->piece_loci > 0 ? (size_t)pp->piece_loci : (size_t)kAllelePieceLoci;
    std::vector<int64_t> ws_off, aws_base, cell_rel;
    std::vector<int32_t> off_rel, snv_rel, oi;
    std::vector<double> od;
    auto n_snvs_of = [&](size_t l) { return snvs ? in.snv_off[l + 1] - in.snv_off[l] : 0; };
    auto group_ws = [&](size_t l) {   // k_phase_group's workspace
        return (int64_t)phase_ws_bytes(read_off[l + 1] - read_off[l], n_snvs_of(l), in.n_alleles[l], p->min_reads);
    };
    auto locus_ws = [&](size_t l) {   // ... and k_alleles' for the locus's two groups, whose reads are at most the locus's
        const int n = read_off[l + 1] - read_off[l];
        return group_ws(l) + (int64_t)(n >= p->min_reads ? allele_ws_bytes(n, B, 2) + allele_ws_bytes(0, B, 2) + 1024 : 0);
    };
    for (int32_t l0 = 0, l1; l0 < n_loci; l0 = l1) {
        int64_t wsum = 0;
        l1 = (int32_t)strk_groups::cut_piece((size_t)l0, (size_t)n_loci, locus_ws, budget, piece_loci, ws_off, &wsum);
        const int32_t nl = l1 - l0, r0 = read_off[l0], nr = read_off[l1] - r0;
        const int32_t s0 = snvs ? in.snv_off[l0] : 0, ns = snvs ? in.snv_off[l1] - s0 : 0;
        const int64_t c0 = snvs ? cell_off[l0] : 0, nc = snvs ? cell_off[l1] - c0 : 0;
        piece_offsets(read_off, l0, nl, off_rel);
        aws_base.resize(nl);
        int max_n = 0;
        for (int32_t l = 0; l < nl; ++l) {
            const int64_t g = group_ws((size_t)l0 + l);
            aws_base[l] = ws_off[l] + g;
            if (g > 0) max_n = std::max(max_n, off_rel[l + 1] - off_rel[l]);
        }
        if (snvs) {
            piece_offsets(in.snv_off, l0, nl, snv_rel);
            cell_rel.resize(nl);
            for (int32_t l = 0; l < nl; ++l) cell_rel[l] = cell_off[l0 + l] - c0;
        }
        const size_t snl = (size_t)nl, snr = std::max<size_t>(nr, 1), sns = std::max<size_t>(ns, 1);
        Carve ci, cm, co;
        const size_t i_off = ci.take((snl + 1) * 4), i_cn = ci.take(snr * 4), i_w = ci.take(snr * 8), i_nal = ci.take(snl * 4),
                     i_seed = ci.take(snl * 8), i_hp = ci.take(snr * 4), i_ps = ci.take(snr * 4), i_soff = ci.take((snl + 1) * 4),
                     i_coff = ci.take(snl * 8), i_base = ci.take(std::max<size_t>((size_t)nc, 1)), i_qual = ci.take(std::max<size_t>((size_t)nc, 1)),
                     i_wsoff = ci.take(snl * 8), i_aws = ci.take(snl * 8);
        const size_t m_perm = cm.take(snr * 4), m_gsz = cm.take(2 * snl * 4), m_meta = cm.take(snl * kPhaseMeta * 4), m_gseed = cm.take(2 * snl * 8),
                     m_gone = cm.take(2 * snl * 4), m_goff = cm.take((2 * snl + 1) * 4), m_gws = cm.take(2 * snl * 8), m_gcn = cm.take(snr * 4),
                     m_gw = cm.take(snr * 8), m_goi = cm.take(2 * snl * kAlleleOutI * 4), m_god = cm.take(2 * snl * kAlleleOutD * 8),
                     m_grp = cm.take(snr * 4);
        const size_t o_i = co.take(snl * kPhaseOutI * 4), o_d = co.take(snl * kAlleleOutD * 8), o_rp = co.take(snr * 4),
                     o_sst = co.take(sns * 4), o_scall = co.take(sns * 2), o_srcs = co.take(sns * 8);
        int rc;
        if ((rc = c->ph_in.ensure(ci.bytes))) return rc;
        if ((rc = c->ph_mid.ensure(cm.bytes))) return rc;
        if ((rc = c->ph_out.ensure(co.bytes))) return rc;
        if ((rc = c->ph_ws.ensure(std::max<size_t>((size_t)wsum, 256)))) return rc;
        char* di = c->ph_in.as<char>();
        HIP_TRY(hipMemcpyAsync(di + i_off, off_rel.data(), (snl + 1) * 4, hipMemcpyHostToDevice, st));
        if (nr > 0) {
            HIP_TRY(hipMemcpyAsync(di + i_cn, in.cn + r0, (size_t)nr * 4, hipMemcpyHostToDevice, st));
            HIP_TRY(hipMemcpyAsync(di + i_w, in.w + r0, (size_t)nr * 8, hipMemcpyHostToDevice, st));
        }
        HIP_TRY(hipMemcpyAsync(di + i_nal, in.n_alleles + l0, snl * 4, hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(di + i_seed, in.seed + l0, snl * 8, hipMemcpyHostToDevice, st));
        if (tags && nr > 0) {
            HIP_TRY(hipMemcpyAsync(di + i_hp, in.hp + r0, (size_t)nr * 4, hipMemcpyHostToDevice, st));
            HIP_TRY(hipMemcpyAsync(di + i_ps, in.ps + r0, (size_t)nr * 4, hipMemcpyHostToDevice, st));
        }
        if (snvs) {
            HIP_TRY(hipMemcpyAsync(di + i_soff, snv_rel.data(), (snl + 1) * 4, hipMemcpyHostToDevice, st));
            HIP_TRY(hipMemcpyAsync(di + i_coff, cell_rel.data(), snl * 8, hipMemcpyHostToDevice, st));
            if (nc > 0) {
                HIP_TRY(hipMemcpyAsync(di + i_base, in.snv_base + c0, (size_t)nc, hipMemcpyHostToDevice, st));
                HIP_TRY(hipMemcpyAsync(di + i_qual, in.snv_qual + c0, (size_t)nc, hipMemcpyHostToDevice, st));
            }
        }
        HIP_TRY(hipMemcpyAsync(di + i_wsoff, ws_off.data(), snl * 8, hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(di + i_aws, aws_base.data(), snl * 8, hipMemcpyHostToDevice, st));
        PhaseArgs a{};
        a.read_off = c->ph_in.at<int32_t>(i_off);
        a.cn = c->ph_in.at<int32_t>(i_cn);
        a.w = c->ph_in.at<double>(i_w);
        a.n_alleles = c->ph_in.at<int32_t>(i_nal);
        a.seed = c->ph_in.at<uint64_t>(i_seed);
        a.hp = tags ? c->ph_in.at<int32_t>(i_hp) : nullptr;
        a.ps = tags ? c->ph_in.at<int32_t>(i_ps) : nullptr;
        a.snv_off = snvs ? c->ph_in.at<int32_t>(i_soff) : nullptr;
        a.cell_off = c->ph_in.at<int64_t>(i_coff);
        a.snv_base = c->ph_in.at<uint8_t>(i_base);
        a.snv_qual = c->ph_in.at<uint8_t>(i_qual);
        a.ws_off = c->ph_in.at<int64_t>(i_wsoff);
        a.ws = c->ph_ws.as<char>();
        a.aws_base = c->ph_in.at<int64_t>(i_aws);
        a.perm = c->ph_mid.at<int32_t>(m_perm);
        a.gsz = c->ph_mid.at<int32_t>(m_gsz);
        a.meta = c->ph_mid.at<int32_t>(m_meta);
        a.gseed = c->ph_mid.at<uint64_t>(m_gseed);
        a.gone = c->ph_mid.at<int32_t>(m_gone);
        a.goff = c->ph_mid.at<int32_t>(m_goff);
        a.gws_off = c->ph_mid.at<int64_t>(m_gws);
        a.gcn = c->ph_mid.at<int32_t>(m_gcn);
        a.gw = c->ph_mid.at<double>(m_gw);
        a.g_oi = c->ph_mid.at<int32_t>(m_goi);
        a.g_od = c->ph_mid.at<double>(m_god);
        a.out_i = c->ph_out.at<int32_t>(o_i);
        a.out_d = c->ph_out.at<double>(o_d);
        a.read_peak = c->ph_out.at<int32_t>(o_rp);
        a.snv_status = c->ph_out.at<int32_t>(o_sst);
        a.snv_call = c->ph_out.at<uint8_t>(o_scall);
        a.snv_rcs = c->ph_out.at<int32_t>(o_srcs);
        a.n_loci = nl;
        a.min_reads = p->min_reads;
        a.min_allele_reads = p->min_allele_reads;
        a.B = B;
        a.min_hp_cov = pp->min_hp_read_coverage;
        a.qual_thr = pp->snv_quality_threshold;
        a.many_snvs = pp->many_snvs_quantity;
        a.w_few = pp->cn_weight_few;
        a.w_many = pp->cn_weight_many;
        // the groups as 2 nl single-allele loci of k_alleles
        AlleleArgs g = allele_rule_args(p);
        g.read_off = a.goff;
        g.cn = a.gcn;
        g.w = a.gw;
        g.n_alleles = a.gone;
        g.seed = a.gseed;
        g.ws_off = a.gws_off;
        g.ws = a.ws;
        g.out_i = c->ph_mid.at<int32_t>(m_goi);
        g.out_d = c->ph_mid.at<double>(m_god);
        g.read_peak = c->ph_mid.at<int32_t>(m_grp);
        g.n_loci = 2 * nl;
        g.min_reads = p->min_allele_reads;
        g.min_allele_reads = p->min_allele_reads;
        const int lds_matrix = (int)phase_lds_matrix_bytes(max_n);
        oi.resize(snl * kPhaseOutI);
        od.resize(snl * kAlleleOutD);
        if ((rc = timed_launch(c, st, stats, fn, "phase kernels", 4, [&] {   // a launch that failed is the last one (timed_launch reports it)
                hipLaunchKernelGGL(k_phase_group, dim3(nl), dim3(kPhaseThreads), lds_matrix + kPhaseLdsFixed, st, a, lds_matrix);
                if (hipPeekAtLastError() != hipSuccess) return;
                hipLaunchKernelGGL(k_phase_pack, dim3((nl + kPhasePackLoci - 1) / kPhasePackLoci), dim3(256), 0, st, a);
                if (hipPeekAtLastError() != hipSuccess) return;
                hipLaunchKernelGGL(k_alleles, dim3(2 * nl), dim3(allele_threads(B)), 0, st, g);
                if (hipPeekAtLastError() != hipSuccess) return;
                hipLaunchKernelGGL(k_phase_finish, dim3(nl), dim3(kPhaseFinishThreads), 0, st, a);
            }, [&] {
                HIP_TRY(hipMemcpyAsync(oi.data(), a.out_i, oi.size() * 4, hipMemcpyDeviceToHost, st));
                HIP_TRY(hipMemcpyAsync(od.data(), a.out_d, od.size() * 8, hipMemcpyDeviceToHost, st));
                if (nr > 0) HIP_TRY(hipMemcpyAsync(out.al.read_peak + r0, a.read_peak, (size_t)nr * 4, hipMemcpyDeviceToHost, st));
                if (ns > 0) {
                    HIP_TRY(hipMemcpyAsync(out.snv_status + s0, a.snv_status, (size_t)ns * 4, hipMemcpyDeviceToHost, st));
                    HIP_TRY(hipMemcpyAsync(out.snv_call + 2 * (size_t)s0, a.snv_call, (size_t)ns * 2, hipMemcpyDeviceToHost, st));
                    HIP_TRY(hipMemcpyAsync(out.snv_rcs + 2 * (size_t)s0, a.snv_rcs, (size_t)ns * 8, hipMemcpyDeviceToHost, st));
                }
                return 0;
            }))) return rc;
        if (stats) stats->n_sub_batches += 1;
        scatter_alleles<2>(out.al, l0, nl, oi.data(), kPhaseOutI, od.data());
        for (int32_t l = 0; l < nl; ++l) {
            const int32_t* s = oi.data() + (size_t)l * kPhaseOutI + kAlleleOutI;
            out.method[l0 + l] = s[0];
            out.reason[l0 + l] = s[1];
            out.ps[l0 + l] = s[2];
        }
    }
    return 0;
}
