// Host side of strk_call_alleles and strk_call_alleles_n (strkit/call/allele.py:176-336 + call_locus.py:1536-1600; DESIGN.md
// §9, §15): input checks (strk_alleles_check.h), pieces, launches, for rows of W = 2 or kMaxAlleles allele slots; and what
// strk_call_alleles_phased (strk_host_phase.inc) shares with it: the piece constants, AlleleOut and its scatter, the rule's
// part of an AlleleArgs, the piece-relative offsets.
// Part of strk_api.hip: included inside its anonymous namespace (uses fail(), HIP_TRY, DevBuf and Staging of strk_host.h, and
// strk_ctx, side_stream and timed_launch defined there); not a stand-alone header.
// ---------------------------------------------------------------------------------------------
// Allele calling: strk_call_alleles, strk_call_alleles_n
// ---------------------------------------------------------------------------------------------
constexpr size_t kAlleleWsBudget = (size_t)512 << 20;   // workspace bytes of one piece (a larger single locus runs alone)
constexpr int kAllelePieceLoci = 32768;

// The caller's arrays, W allele slots per locus: status, modal_n [L]; call, means, weights, stdevs [L][W]; ci95, ci99 [L][W][2];
// peak_n_reads [L][2]; read_peak per read.
struct AlleleOut {
    int32_t *status, *modal_n, *call, *ci95, *ci99;
    double *means, *weights, *stdevs;
    int32_t *peak_n_reads, *read_peak;
    bool complete() const {
        return status && modal_n && call && ci95 && ci99 && means && weights && stdevs && peak_n_reads && read_peak;
    }
};

// The per-locus rows of a piece as they came down (`stride` ints of oi per locus, the first AlleleRow<W>::kOutI laid out as
// k_alleles_w<W> writes them; AlleleRow<W>::kOutD doubles of od) into the caller's arrays at loci l0 .. l0 + nl.
template <int W>
void scatter_alleles(const AlleleOut& out, int32_t l0, int32_t nl, const int32_t* oi, int stride, const double* od) {
    using R = AlleleRow<W>;
    for (int32_t l = 0; l < nl; ++l) {
        const int32_t* s = oi + (size_t)l * stride;
        const double* t = od + (size_t)l * R::kOutD;
        const size_t g = (size_t)(l0 + l);
        out.status[g] = s[0];
        out.modal_n[g] = s[1];
        for (int e = 0; e < W; ++e) {
            out.call[W * g + e] = s[R::kCall + e];
            out.means[W * g + e] = t[e];
            out.weights[W * g + e] = t[W + e];
            out.stdevs[W * g + e] = t[2 * W + e];
        }
        for (int e = 0; e < 2 * W; ++e) {
            out.ci95[2 * W * g + e] = s[R::kCi95 + e];
            out.ci99[2 * W * g + e] = s[R::kCi99 + e];
        }
        for (int e = 0; e < 2; ++e) out.peak_n_reads[2 * g + e] = s[R::kPeak + e];
    }
}

// The rule's part of k_alleles' arguments.  The caller sets the pointers, n_loci and the two read thresholds (a locus's call
// and a group's call differ in them on purpose).
AlleleArgs allele_rule_args(const strk_allele_params* p) {
    AlleleArgs a{};
    a.B = p->num_bootstrap;
    a.n_init = p->n_init;
    a.max_iter = p->max_iter;
    a.filter_factor = p->filter_factor;
    a.force_gm_filter = p->force_gm_filter;
    a.tol = p->tol;
    a.reg_covar = p->reg_covar;
    a.expansion_ratio = p->expansion_ratio;
    return a;
}

int allele_threads(int B) { return std::min(256, (B + 63) / 64 * 64); }   // block size of k_alleles_w

// off[l0 .. l0 + nl] of a call as the offsets of a piece that begins at l0
void piece_offsets(const int32_t* off, int32_t l0, int32_t nl, std::vector<int32_t>& rel) {
    rel.resize((size_t)nl + 1);
    for (int32_t l = 0; l <= nl; ++l) rel[l] = off[l0 + l] - off[l0];
}

// W = 2: k_alleles, at most two alleles per locus, two workspace rows.  W = kMaxAlleles: k_alleles_n, a locus's n_alleles rows.
template <int W>
int call_alleles_impl(strk_ctx* c, const char* fn, const strk_alleles_check::Input& in, const AlleleOut& out, strk_stats* stats) {
    if (stats) memset(stats, 0, sizeof *stats);
    {
        strk_groups::Message m;
        if (const int rc = strk_alleles_check::check(in, {kAlleleMaxReads, kAlleleMaxBootstrap, kAlleleMaxInit, W}, &m))
            return fail(rc, "%s: %s", fn, m.text);
    }
    const int32_t n_loci = in.n_loci;
    if (n_loci == 0) return 0;
    if (!out.complete()) return fail(STRK_E_INVALID, "%s: NULL argument", fn);
    const strk_allele_params* p = in.p;
    const int32_t* read_off = in.read_off;
    HIP_TRY(hipSetDevice(c->device));
    hipStream_t st;
    if (const int rc = side_stream(c, &st)) return rc;
    using R = AlleleRow<W>;
    const int B = p->num_bootstrap;
    std::vector<int64_t> ws_off;
    std::vector<int32_t> off_rel;
    auto locus_ws = [&](size_t l) {
        const int n = read_off[l + 1] - read_off[l];
        return (int64_t)(n >= p->min_reads ? allele_ws_bytes(n, B, W == 2 ? 2 : in.n_alleles[l]) : 0);
    };
    for (int32_t l0 = 0, l1; l0 < n_loci; l0 = l1) {
        // one piece: loci in caller order while their workspace fits the budget
        int64_t wsum = 0;
        l1 = (int32_t)strk_groups::cut_piece((size_t)l0, (size_t)n_loci, locus_ws, (int64_t)kAlleleWsBudget, kAllelePieceLoci,
                                             ws_off, &wsum);
        const int32_t nl = l1 - l0, r0 = read_off[l0], nr = read_off[l1] - r0;
        piece_offsets(read_off, l0, nl, off_rel);
        const size_t snl = (size_t)nl, snr = (size_t)nr;
        Staging sg(c->image);
        const size_t i_off = sg.put(off_rel.data(), (snl + 1) * 4), i_cn = sg.put(in.cn + r0, snr * 4), i_w = sg.put(in.w + r0, snr * 8),
                     i_nal = sg.put(in.n_alleles + l0, snl * 4), i_seed = sg.put(in.seed + l0, snl * 8), i_wsoff = sg.put(ws_off.data(), snl * 8);
        const size_t o_i = sg.get(nullptr, snl * R::kOutI * 4), o_d = sg.get(nullptr, snl * R::kOutD * 8), o_rp = sg.get(out.read_peak + r0, snr * 4);
        int rc;
        if ((rc = c->al_ws.ensure(std::max<size_t>((size_t)wsum, 256)))) return rc;
        if ((rc = sg.upload(c->al_stage, st))) return rc;
        const DevBuf& d = c->al_stage;
        AlleleArgs a = allele_rule_args(p);
        a.read_off = d.at<int32_t>(i_off);
        a.cn = d.at<int32_t>(i_cn);
        a.w = d.at<double>(i_w);
        a.n_alleles = d.at<int32_t>(i_nal);
        a.seed = d.at<uint64_t>(i_seed);
        a.ws_off = d.at<int64_t>(i_wsoff);
        a.ws = c->al_ws.as<char>();
        a.out_i = d.at<int32_t>(o_i);
        a.out_d = d.at<double>(o_d);
        a.read_peak = d.at<int32_t>(o_rp);
        a.n_loci = nl;
        a.min_reads = p->min_reads;
        a.min_allele_reads = p->min_allele_reads;
        if ((rc = timed_launch(c, st, stats, fn, "allele kernel", 1, [&] {
                hipLaunchKernelGGL(k_alleles_w<W>, dim3(nl), dim3(allele_threads(B)), 0, st, a);
            }, [&] { return sg.download(d, st); }))) return rc;
        sg.scatter();
        scatter_alleles<W>(out, l0, nl, sg.at<int32_t>(o_i), R::kOutI, sg.at<double>(o_d));
    }
    return 0;
}
