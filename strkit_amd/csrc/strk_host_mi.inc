// strk_host_mi.inc — Mendelian inheritance and the de novo test of a trio (part of strk_api.hip, after strk_methyl.inc):
// strk_mi_trio on the device and strk_mi_trio_host on the host's cores.  The rule, the statistics, the host twin and the kernels
// are strk_mi.h, the input check strk_mi_check.h; here are the threads, the pieces, the buffers and the launches.

namespace {

constexpr int64_t kMiWsBudget = (int64_t)512 << 20;   // workspace and read bytes of one piece (a larger single locus runs alone)
constexpr int32_t kMiPieceLoci = 262144;
constexpr int32_t kMiHostPieceLoci = 256;

static_assert(strk_mi::kTestWmwGt == STRK_MI_TEST_WMW_GT && strk_mi::kEmptyChild == STRK_MI_EMPTY_CHILD &&
              strk_mi::kFromBoth == STRK_MI_FROM_BOTH, "strk_mi.h <-> include/strkit_amd.h");

struct MiOut {
    int8_t* respects;
    double* p;
    int32_t *config, *from, *status;
};

int mi_check(const char* fn, const strk_mi_check::Input& in, const MiOut& out) {
    strk_groups::Message m;
    if (const int rc = strk_mi_check::check(in, strk_mi::kMaxGroup, &m)) return fail(rc, "%s: %s", fn, m.text);
    if (in.n_loci > 0 && (!out.respects || (in.p->test != STRK_MI_TEST_NONE && (!out.p || !out.config || !out.from || !out.status))))
        return fail(STRK_E_INVALID, "%s: NULL argument", fn);
    return 0;
}

strk_mi::Args mi_rule_args(const strk_mi_check::Input& in) {
    strk_mi::Args a{};
    a.test = in.p->test;
    a.sig_level = in.p->sig_level;
    a.widen = in.p->widen;
    return a;
}

}  // namespace

extern "C" {

void strk_mi_constants(int32_t* out3) {
    out3[0] = strk_mi::kSmallReads; out3[1] = strk_mi::kSmallWaves; out3[2] = strk_mi::kMaxGroup;
}

int strk_mi_trio_host(int32_t n_loci, const int64_t* grp_off, const int32_t* cn, int64_t n_cn, const int32_t* gt, const int32_t* ci95,
                      const int32_t* ci99, const int32_t* seq_id, const int32_t* seq_len, const strk_mi_params* params,
                      int8_t* out_respects, double* out_p, int32_t* out_config, int32_t* out_mutation_from, int32_t* out_status) {
    const strk_mi_check::Input in{n_loci, grp_off, cn, n_cn, gt, ci95, ci99, seq_id, seq_len, params};
    const MiOut out{out_respects, out_p, out_config, out_mutation_from, out_status};
    if (const int rc = mi_check("strk_mi_trio_host", in, out)) return rc;
    if (n_loci == 0) return 0;
    strk_mi::Args a = mi_rule_args(in);
    a.grp_off = grp_off; a.cn = cn; a.gt = gt; a.ci95 = ci95; a.ci99 = ci99; a.seq_id = seq_id; a.seq_len = seq_len;
    a.respects = out_respects; a.p = out_p; a.config = out_config; a.from = out_mutation_from; a.status = out_status;
    // threads take pieces of consecutive loci from a counter; every locus has its own outputs, so the cut changes nothing
    const int32_t piece = params->piece_loci > 0 ? params->piece_loci : kMiHostPieceLoci;
    const int64_t n_pieces = ((int64_t)n_loci + piece - 1) / piece;
    // threads: the CPUs this process may run on, at most OMP_NUM_THREADS where it is set and 16 where it is not (a machine
    // may show many more CPUs than a command is meant to use)
    int64_t cap = 16;
    if (const char* e = getenv("OMP_NUM_THREADS")) {
        const long v = strtol(e, nullptr, 10);
        if (v > 0) cap = std::min<long>(v, 256);
    }
    struct Scratch {
        std::vector<uint64_t> keys;
        std::vector<int32_t> tval, tcnt;
        std::vector<strk_mi::U128> ws;
    };
    strk_threads::parallel_chunks<Scratch>(n_loci, piece, (int)std::min<int64_t>({(int64_t)host_cpus(), cap, n_pieces}), [&](int64_t l0, int64_t l1, Scratch& s) {
        for (int64_t l = l0; l < l1; ++l) strk_mi::host_locus(a, l, s.keys, s.tval, s.tcnt, s.ws);
    });
    return 0;
}

int strk_mi_trio(strk_ctx* c, int32_t n_loci, const int64_t* grp_off, const int32_t* cn, int64_t n_cn, const int32_t* gt,
                 const int32_t* ci95, const int32_t* ci99, const int32_t* seq_id, const int32_t* seq_len, const strk_mi_params* params,
                 int8_t* out_respects, double* out_p, int32_t* out_config, int32_t* out_mutation_from, int32_t* out_status,
                 strk_stats* stats) {
    const char* const fn = "strk_mi_trio";
    if (stats) memset(stats, 0, sizeof *stats);
    if (!c) return fail(STRK_E_INVALID, "%s: ctx is NULL", fn);
    const strk_mi_check::Input in{n_loci, grp_off, cn, n_cn, gt, ci95, ci99, seq_id, seq_len, params};
    const MiOut out{out_respects, out_p, out_config, out_mutation_from, out_status};
    if (const int rc = mi_check(fn, in, out)) return rc;
    if (n_loci == 0) return 0;
    HIP_TRY(hipSetDevice(c->device));
    hipStream_t st;
    if (const int rc = side_stream(c, &st)) return rc;
    const bool reads = params->test != STRK_MI_TEST_NONE;
    const int64_t budget = params->ws_budget > 0 ? params->ws_budget : kMiWsBudget;
    const size_t max_loci = params->piece_loci > 0 ? (size_t)params->piece_loci : (size_t)kMiPieceLoci;
    const auto is_large = [&](size_t l) {
        return reads && (params->force_large || grp_off[6 * l + 6] - grp_off[6 * l] > strk_mi::kSmallReads);
    };
    // a locus's share of a piece: its workspace; its reads are counted too, so that the budget bounds what goes up as well
    const auto locus_ws = [&](size_t l) -> int64_t {
        if (!reads) return 0;
        int64_t n[strk_mi::kGroups];
        for (int g = 0; g < strk_mi::kGroups; ++g) n[g] = grp_off[6 * l + g + 1] - grp_off[6 * l + g];
        return strk_mi::locus_ws_bytes(n, is_large(l));
    };
    const auto locus_cost = [&](size_t l) -> int64_t {
        return locus_ws(l) + (reads ? strk_mi::round256((grp_off[6 * l + 6] - grp_off[6 * l]) * 4) : 0) + 256;
    };
    std::vector<int64_t> cost_off, ws_off, off_rel;
    std::vector<int32_t> small_list, large_list;
    for (size_t l0 = 0, l1; l0 < (size_t)n_loci; l0 = l1) {
        int64_t used = 0;
        l1 = strk_groups::cut_piece(l0, (size_t)n_loci, locus_cost, budget, max_loci, cost_off, &used);
        const size_t nl = l1 - l0;
        const int64_t r0 = reads ? grp_off[6 * l0] : 0, nr = reads ? grp_off[6 * l1] - r0 : 0;
        ws_off.resize(nl);
        small_list.clear(); large_list.clear();
        int64_t ws_bytes = 0;
        for (size_t l = 0; l < nl; ++l) {
            ws_off[l] = ws_bytes;
            ws_bytes += locus_ws(l0 + l);
            (is_large(l0 + l) ? large_list : small_list).push_back((int32_t)l);
        }
        if (reads) {
            off_rel.resize(6 * nl + 1);
            for (size_t k = 0; k <= 6 * nl; ++k) off_rel[k] = grp_off[6 * l0 + k] - r0;
        }
        // without a test no reads go up and only `respects` comes down; absent intervals and sequences are absent here as well
        Staging sg(c->image);
        const size_t i_gt = sg.put(gt + 6 * l0, nl * 24), i_c95 = sg.put(ci95 + 12 * l0, nl * 48);
        const size_t i_c99 = ci99 ? sg.put(ci99 + 12 * l0, nl * 48) : 0;
        const size_t i_sid = seq_id ? sg.put(seq_id + 6 * l0, nl * 24) : 0, i_slen = seq_id ? sg.put(seq_len + 6 * l0, nl * 24) : 0;
        const size_t i_off = reads ? sg.put(off_rel.data(), (6 * nl + 1) * 8) : 0, i_cn = reads ? sg.put(cn + r0, (size_t)nr * 4) : 0,
                     i_wsoff = reads ? sg.put(ws_off.data(), nl * 8) : 0, i_small = reads ? sg.put(small_list.data(), small_list.size() * 4) : 0,
                     i_large = reads ? sg.put(large_list.data(), large_list.size() * 4) : 0;
        const size_t o_res = sg.get(out_respects + 7 * l0, nl * 7);
        const size_t o_p = reads ? sg.get(out_p + l0, nl * 8) : 0, o_cfg = reads ? sg.get(out_config + l0, nl * 4) : 0,
                     o_from = reads ? sg.get(out_mutation_from + l0, nl * 4) : 0, o_st = reads ? sg.get(out_status + l0, nl * 4) : 0;
        int rc;
        if ((rc = c->mi_ws.ensure(std::max<size_t>((size_t)ws_bytes, 256)))) return rc;
        if ((rc = sg.upload(c->mi_stage, st))) return rc;
        const DevBuf& d = c->mi_stage;
        strk_mi::Args a = mi_rule_args(in);
        a.gt = d.at<int32_t>(i_gt);
        a.ci95 = d.at<int32_t>(i_c95);
        a.ci99 = ci99 ? d.at<int32_t>(i_c99) : nullptr;
        a.seq_id = seq_id ? d.at<int32_t>(i_sid) : nullptr;
        a.seq_len = seq_id ? d.at<int32_t>(i_slen) : nullptr;
        a.respects = d.at<int8_t>(o_res);
        if (reads) {
            a.grp_off = d.at<int64_t>(i_off);
            a.cn = d.at<int32_t>(i_cn);
            a.ws_off = d.at<int64_t>(i_wsoff);
            a.ws = c->mi_ws.as<char>();
            a.p = d.at<double>(o_p); a.config = d.at<int32_t>(o_cfg); a.from = d.at<int32_t>(o_from); a.status = d.at<int32_t>(o_st);
        }
        const int32_t ns = reads ? (int32_t)small_list.size() : (int32_t)nl, ng = (int32_t)large_list.size();
        if ((rc = timed_launch(c, st, stats, fn, "trio kernels", (ns > 0) + (ng > 0), [&] {
                if (ns > 0)
                    hipLaunchKernelGGL(strk_mi::k_mi_small, dim3((unsigned)((ns + strk_mi::kSmallWaves - 1) / strk_mi::kSmallWaves)),
                                       dim3(64 * strk_mi::kSmallWaves), 0, st, a, reads ? d.at<int32_t>(i_small) : (const int32_t*)nullptr, ns);
                if (ng > 0) hipLaunchKernelGGL(strk_mi::k_mi_large, dim3((unsigned)ng), dim3(256), 0, st, a, d.at<int32_t>(i_large));
            }, [&] { return sg.download(d, st); }))) return rc;
        sg.scatter();
        if (stats) { stats->n_fallback += ng; stats->n_sub_batches += 1; }
    }
    return 0;
}

}  // extern "C"
