// strk_gff.inc — locus annotations from GFF3 / GTF text (part of strk_api.hip, after strk_vcf.inc): strk_gff_overlaps over a
// decompressed host buffer and strk_dbam_gff_overlaps over the stream of a strk_dbam object.  The rule of a line and of an id, the
// host walk, the closing pass and the kernels are strk_gff.h, the lines strk_lines.h / strk_lines.inc; here are the argument checks,
// the buffers and the launches.

namespace {

int gff_check(const char* who, int64_t n_bytes, int64_t start, const char* contig, int64_t prev_beg, int32_t n_loci, const int64_t* ls, const int64_t* le,
              int64_t pair_cap, const int32_t* pair_locus, const int32_t* pair_feat, int64_t feat_cap, const int64_t* f_beg, const int64_t* f_end,
              const int32_t* f_kind, const int64_t* f_text_off, int64_t text_cap, const uint8_t* text, const int64_t* sizes, const int64_t* end_off,
              const int32_t* past) {
    if (const int rc = text_check(who, n_bytes, start, contig, sizes, end_off, past)) return rc;
    if (prev_beg < -1) return fail(STRK_E_INVALID, "%s: bad prev_beg", who);
    if (n_loci < 0 || (n_loci > 0 && (!ls || !le))) return fail(STRK_E_INVALID, "%s: bad loci", who);
    if (pair_cap < 0 || feat_cap < 0 || text_cap < 0 || (pair_cap > 0 && (!pair_locus || !pair_feat)) ||
        (feat_cap > 0 && (!f_beg || !f_end || !f_kind || !f_text_off)) || (text_cap > 0 && !text))
        return fail(STRK_E_INVALID, "%s: NULL output array", who);
    return 0;
}

}  // namespace

extern "C" {

void strk_gff_constants(int32_t* out3) {
    out3[0] = strk_gff::kClasses; out3[1] = strk_gff::kStepBytes; out3[2] = strk_gff::kLinesPerWave;
}

int64_t strk_gff_overlaps(const uint8_t* buf, int64_t n_bytes, int64_t start, const char* contig, int32_t gtf, int32_t final, int64_t prev_beg,
                          int32_t n_loci, const int64_t* l_start, const int64_t* l_end, int64_t pair_cap, int32_t* pair_locus, int32_t* pair_feat,
                          int64_t feat_cap, int64_t* f_beg, int64_t* f_end, int32_t* f_kind, int64_t* f_text_off, int64_t text_cap, uint8_t* text,
                          int64_t* sizes, int64_t* end_off, int32_t* past) {
    static const char who[] = "strk_gff_overlaps";
    int rc = gff_check(who, n_bytes, start, contig, prev_beg, n_loci, l_start, l_end, pair_cap, pair_locus, pair_feat, feat_cap, f_beg, f_end, f_kind,
                       f_text_off, text_cap, text, sizes, end_off, past);
    if (rc) return rc;
    if (!buf && n_bytes > 0) return fail(STRK_E_INVALID, "%s: NULL argument", who);
    strk_gff::Result r;
    strk_gff::Message msg;
    if (strk_gff::overlaps_host(buf, n_bytes, start, contig, gtf, final, prev_beg, n_loci, l_start, l_end, &r, &msg,
                                [](int32_t n, auto&& body) { strk_threads::parallel_slices(n, 1024, 32, body); }))
        return fail(STRK_E_INVALID, "%s: %s", who, msg.text);
    *end_off = r.end_off; *past = r.past;
    return strk_gff::emit(r, n_loci, pair_cap, pair_locus, pair_feat, feat_cap, f_beg, f_end, f_kind, f_text_off, text_cap, text, sizes);
}

int64_t strk_dbam_gff_overlaps(strk_dbam* d, int64_t start, const char* contig, int32_t gtf, int32_t final, int64_t prev_beg, int32_t tile_bytes,
                               int32_t n_loci, const int64_t* l_start, const int64_t* l_end, int64_t pair_cap, int32_t* pair_locus, int32_t* pair_feat,
                               int64_t feat_cap, int64_t* f_beg, int64_t* f_end, int32_t* f_kind, int64_t* f_text_off, int64_t text_cap, uint8_t* text,
                               int64_t* sizes, int64_t* end_off, int32_t* past) {
    static const char who[] = "strk_dbam_gff_overlaps";
    if (!d) return fail(STRK_E_INVALID, "%s: bad argument", who);
    // before any launch: the start offset lies inside the stream, the piece is below 2^31 bytes
    int rc = gff_check(who, d->n_data, start, contig, prev_beg, n_loci, l_start, l_end, pair_cap, pair_locus, pair_feat, feat_cap, f_beg, f_end, f_kind,
                       f_text_off, text_cap, text, sizes, end_off, past);
    if (rc) return rc;
    *end_off = start; *past = 0;
    DevLines l;
    if ((rc = dbam_lines(d, who, start, final, tile_bytes, &l))) return rc;
    const int64_t n = d->n_data;
    strk_gff::Result r;
    r.pair_off.assign((size_t)n_loci + 1, 0);
    r.text_off.push_back(0);
    r.last_beg = prev_beg; r.end_off = l.end_off;
    const auto done = [&]() {
        *end_off = r.end_off; *past = r.past;
        return strk_gff::emit(r, n_loci, pair_cap, pair_locus, pair_feat, feat_cap, f_beg, f_end, f_kind, f_text_off, text_cap, text, sizes);
    };
    if (start == n) return done();   // nothing to read, nothing launched
    const int32_t n_nl = l.n_nl, n_lines = l.n_lines;
    if (n_lines == 0) return done();
    const uint8_t* const data = d->data.as<uint8_t>();
    const int64_t* const starts = l.starts;
    const int32_t contig_len = (int32_t)strlen(contig);
    unsigned long long* st = nullptr;
    const uint8_t* name = nullptr;
    if ((rc = dbam_query(d, {~0ull, ~0ull, 0ull, ~0ull}, contig, contig_len, &st, &name))) return rc;
    // gf_lines: f_beg | f_end | type_a | attr_a | type_len | attr_len | status per line | features per wave, their offsets
    const size_t cap_lines = (size_t)n_nl + 1, n_lw = (cap_lines + 63) / 64;
    Carve cl;
    const size_t o_beg = cl.take(cap_lines * 8), o_end = cl.take(cap_lines * 8), o_ta = cl.take(cap_lines * 8), o_aa = cl.take(cap_lines * 8),
                 o_tl = cl.take(cap_lines * 4), o_al = cl.take(cap_lines * 4), o_stat = cl.take(cap_lines), o_oc = cl.take(n_lw * 4),
                 o_oo = cl.take((n_lw + 1) * 8);
    if ((rc = d->gf_lines.ensure(cl.bytes))) return rc;
    // ---- the fields, the contig's features in file order
    const int32_t n_line_waves = (n_lines + 63) / 64;
    const dim3 line_grid = l.line_grid;
    d->tic();
    hipLaunchKernelGGL(strk_gff::k_gff_coords, line_grid, dim3(256), 0, 0, data, n, starts, n_nl, n_lines, name, contig_len,
                       d->gf_lines.at<int64_t>(o_beg), d->gf_lines.at<int64_t>(o_end), d->gf_lines.at<int64_t>(o_ta), d->gf_lines.at<int32_t>(o_tl),
                       d->gf_lines.at<int64_t>(o_aa), d->gf_lines.at<int32_t>(o_al), d->gf_lines.at<uint8_t>(o_stat), d->gf_lines.at<int32_t>(o_oc), st);
    hipLaunchKernelGGL(strk_lines::k_lines_scan, dim3(1), dim3(256), 0, 0, d->gf_lines.at<int32_t>(o_oc), n_line_waves, d->gf_lines.at<int64_t>(o_oo));
    HIP_TRY(hipGetLastError());
    d->toc();
    int64_t n_feat64 = 0;
    HIP_TRY(hipMemcpy(&n_feat64, d->gf_lines.at<int64_t>(o_oo) + n_line_waves, 8, hipMemcpyDeviceToHost));
    if (n_feat64 < 0 || n_feat64 > n_lines) return fail(STRK_E_DEVICE, "%s: feature count out of range", who);
    const int32_t n_feat = (int32_t)n_feat64, n_fw = (n_feat + 63) / 64;
    // gf_feat: f_beg | f_end | line per feature | the same partitioned by class, with the ordinal | counts per class and wave, offsets | flags,
    // hit counts per wave, offsets, ranks
    Carve cf;
    const size_t nf = (size_t)std::max(n_feat, 1), n_slots = (size_t)strk_gff::kClasses * (size_t)std::max(n_fw, 1);
    const size_t o_fb = cf.take(nf * 8), o_fe = cf.take(nf * 8), o_fl = cf.take(nf * 4), o_pb = cf.take(nf * 8), o_pe = cf.take(nf * 8), o_po = cf.take(nf * 4),
                 o_cc = cf.take(n_slots * 4), o_co = cf.take((n_slots + 1) * 8), o_flag = cf.take(nf), o_hc = cf.take((size_t)std::max(n_fw, 1) * 4),
                 o_ho = cf.take(((size_t)n_fw + 1) * 8), o_hr = cf.take(nf * 4);
    if ((rc = d->gf_feat.ensure(cf.bytes))) return rc;
    int64_t* const fb = d->gf_feat.at<int64_t>(o_fb);
    int64_t* const fe = d->gf_feat.at<int64_t>(o_fe);
    int32_t* const f_line = d->gf_feat.at<int32_t>(o_fl);
    int64_t* const coff = d->gf_feat.at<int64_t>(o_co);
    if (n_feat > 0) {
        const dim3 feat_grid((unsigned)((n_feat + 255) / 256));
        HIP_TRY(hipMemset(d->gf_feat.at<char>(o_cc), 0, n_slots * 4));
        HIP_TRY(hipMemset(d->gf_feat.at<char>(o_flag), 0, nf));
        d->tic();
        hipLaunchKernelGGL(strk_gff::k_gff_gather, line_grid, dim3(256), 0, 0, n_lines, d->gf_lines.at<uint8_t>(o_stat), d->gf_lines.at<int64_t>(o_beg),
                           d->gf_lines.at<int64_t>(o_end), d->gf_lines.at<int64_t>(o_oo), n_feat, fb, fe, f_line);
        hipLaunchKernelGGL(strk_gff::k_gff_classes, feat_grid, dim3(256), 0, 0, n_feat, fb, fe, f_line, starts, prev_beg, n_fw, d->gf_feat.at<int32_t>(o_cc),
                           (const int64_t*)nullptr, (int64_t*)nullptr, (int64_t*)nullptr, (int32_t*)nullptr, st);
        hipLaunchKernelGGL(strk_lines::k_lines_scan, dim3(1), dim3(256), 0, 0, d->gf_feat.at<int32_t>(o_cc), (int32_t)n_slots, coff);
        hipLaunchKernelGGL(strk_gff::k_gff_classes, feat_grid, dim3(256), 0, 0, n_feat, fb, fe, f_line, starts, prev_beg, n_fw, d->gf_feat.at<int32_t>(o_cc),
                           (const int64_t*)coff, d->gf_feat.at<int64_t>(o_pb), d->gf_feat.at<int64_t>(o_pe), d->gf_feat.at<int32_t>(o_po), st);
        HIP_TRY(hipGetLastError());
        d->toc();
    }
    unsigned long long sth[4];
    HIP_TRY(hipMemcpy(sth, st, 32, hipMemcpyDeviceToHost));
    if (sth[0] != ~0ull || sth[3] != ~0ull) {
        strk_gff::Message msg;
        if (sth[0] < sth[3]) strk_gff::bad_line(&msg, (int64_t)sth[0]);
        else strk_gff::unsorted_line(&msg, (int64_t)sth[3]);
        return fail(STRK_E_INVALID, "%s: %s", who, msg.text);
    }
    r.past = (prev_beg >= 0 ? sth[2] > 0 : (sth[1] != ~0ull && sth[2] > sth[1] + 1)) ? 1 : 0;
    if (n_feat == 0) return done();
    HIP_TRY(hipMemcpy(&r.last_beg, fb + (n_feat - 1), 8, hipMemcpyDeviceToHost));
    if (n_loci == 0) return done();
    // ---- the join.  gf_join: loci | hits per locus, offsets | the hits in class order
    Carve cj;
    const size_t o_ls = cj.take((size_t)n_loci * 8), o_le = cj.take((size_t)n_loci * 8), o_pc = cj.take((size_t)n_loci * 4), o_pf = cj.take(((size_t)n_loci + 1) * 8);
    if ((rc = d->gf_join.ensure(cj.bytes))) return rc;
    HIP_TRY(hipMemcpy(d->gf_join.at<char>(o_ls), l_start, (size_t)n_loci * 8, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(d->gf_join.at<char>(o_le), l_end, (size_t)n_loci * 8, hipMemcpyHostToDevice));
    const dim3 locus_grid((unsigned)((n_loci + 3) / 4));
    int64_t* const pair_off = d->gf_join.at<int64_t>(o_pf);
    d->tic();
    hipLaunchKernelGGL(strk_gff::k_gff_join, locus_grid, dim3(256), 0, 0, n_loci, d->gf_join.at<int64_t>(o_ls), d->gf_join.at<int64_t>(o_le), n_feat, n_fw, coff,
                       d->gf_feat.at<int64_t>(o_pb), d->gf_feat.at<int64_t>(o_pe), d->gf_feat.at<int32_t>(o_po), d->gf_join.at<int32_t>(o_pc),
                       (const int64_t*)nullptr, (int64_t)0, (int32_t*)nullptr, (uint8_t*)nullptr);
    hipLaunchKernelGGL(strk_lines::k_lines_scan, dim3(1), dim3(256), 0, 0, d->gf_join.at<int32_t>(o_pc), n_loci, pair_off);
    HIP_TRY(hipGetLastError());
    d->toc();
    int64_t n_pairs = 0;
    HIP_TRY(hipMemcpy(&n_pairs, pair_off + n_loci, 8, hipMemcpyDeviceToHost));
    if (n_pairs < 0 || n_pairs > (int64_t)n_loci * n_feat) return fail(STRK_E_DEVICE, "%s: pair count out of range", who);
    if (n_pairs == 0) return done();
    if ((rc = d->gf_pairs.ensure((size_t)n_pairs * 4))) return rc;
    const dim3 feat_grid((unsigned)((n_feat + 255) / 256));
    d->tic();
    hipLaunchKernelGGL(strk_gff::k_gff_join, locus_grid, dim3(256), 0, 0, n_loci, d->gf_join.at<int64_t>(o_ls), d->gf_join.at<int64_t>(o_le), n_feat, n_fw, coff,
                       d->gf_feat.at<int64_t>(o_pb), d->gf_feat.at<int64_t>(o_pe), d->gf_feat.at<int32_t>(o_po), (int32_t*)nullptr,
                       (const int64_t*)pair_off, n_pairs, d->gf_pairs.as<int32_t>(), d->gf_feat.at<uint8_t>(o_flag));
    hipLaunchKernelGGL(strk_gff::k_gff_hits, feat_grid, dim3(256), 0, 0, n_feat, d->gf_feat.at<uint8_t>(o_flag), d->gf_feat.at<int32_t>(o_hc),
                       (const int64_t*)nullptr, 0, (int32_t*)nullptr, (int32_t*)nullptr);
    hipLaunchKernelGGL(strk_lines::k_lines_scan, dim3(1), dim3(256), 0, 0, d->gf_feat.at<int32_t>(o_hc), n_fw, d->gf_feat.at<int64_t>(o_ho));
    HIP_TRY(hipGetLastError());
    d->toc();
    int64_t n_hit64 = 0;
    HIP_TRY(hipMemcpy(&n_hit64, d->gf_feat.at<int64_t>(o_ho) + n_fw, 8, hipMemcpyDeviceToHost));
    if (n_hit64 < 1 || n_hit64 > n_feat) return fail(STRK_E_DEVICE, "%s: hit count out of range", who);
    const int32_t n_hit = (int32_t)n_hit64;
    // gf_out (one download): pair offsets | pairs | per hit feature f_beg | f_end | kind | type length | id length | text offsets; then device-only
    // spans and lengths; the text follows once its size is known
    Carve co;
    const size_t q_po = co.take(((size_t)n_loci + 1) * 8), q_pf = co.take((size_t)n_pairs * 4), q_hb = co.take((size_t)n_hit * 8), q_he = co.take((size_t)n_hit * 8),
                 q_hk = co.take((size_t)n_hit * 4), q_tl = co.take((size_t)n_hit * 4), q_il = co.take((size_t)n_hit * 4), q_to = co.take(((size_t)n_hit + 1) * 8);
    const size_t n_down = co.bytes;
    const size_t q_ord = co.take((size_t)n_hit * 4), q_ta = co.take((size_t)n_hit * 8), q_ia = co.take((size_t)n_hit * 8), q_ht = co.take((size_t)n_hit * 4);
    if ((rc = d->gf_out.ensure(co.bytes))) return rc;
    const dim3 hit_grid((unsigned)((n_hit + 3) / 4));
    d->tic();
    hipLaunchKernelGGL(strk_gff::k_gff_hits, feat_grid, dim3(256), 0, 0, n_feat, d->gf_feat.at<uint8_t>(o_flag), d->gf_feat.at<int32_t>(o_hc),
                       (const int64_t*)d->gf_feat.at<int64_t>(o_ho), n_hit, d->gf_feat.at<int32_t>(o_hr), d->gf_out.at<int32_t>(q_ord));
    hipLaunchKernelGGL(strk_gff::k_gff_order, locus_grid, dim3(256), 0, 0, n_loci, (const int64_t*)pair_off, n_pairs, d->gf_pairs.as<int32_t>(), n_feat,
                       d->gf_feat.at<int32_t>(o_hr), d->gf_out.at<int32_t>(q_pf));
    hipLaunchKernelGGL(strk_gff::k_gff_ids, hit_grid, dim3(256), 0, 0, data, n, n_hit, d->gf_out.at<int32_t>(q_ord), n_feat, n_lines, f_line, fb, fe, d->gf_lines.at<int64_t>(o_ta),
                       d->gf_lines.at<int32_t>(o_tl), d->gf_lines.at<int64_t>(o_aa), d->gf_lines.at<int32_t>(o_al), gtf ? 1 : 0, d->gf_out.at<int64_t>(q_hb),
                       d->gf_out.at<int64_t>(q_he), d->gf_out.at<int32_t>(q_hk), d->gf_out.at<int64_t>(q_ta), d->gf_out.at<int32_t>(q_tl),
                       d->gf_out.at<int64_t>(q_ia), d->gf_out.at<int32_t>(q_il), d->gf_out.at<int32_t>(q_ht));
    hipLaunchKernelGGL(strk_lines::k_lines_scan, dim3(1), dim3(256), 0, 0, d->gf_out.at<int32_t>(q_ht), n_hit, d->gf_out.at<int64_t>(q_to));
    HIP_TRY(hipMemcpyAsync(d->gf_out.at<char>(q_po), pair_off, ((size_t)n_loci + 1) * 8, hipMemcpyDeviceToDevice, 0));
    HIP_TRY(hipGetLastError());
    d->toc();
    int64_t n_text = 0;
    HIP_TRY(hipMemcpy(&n_text, d->gf_out.at<int64_t>(q_to) + n_hit, 8, hipMemcpyDeviceToHost));
    if (n_text < 0 || n_text > 2 * (n - start)) return fail(STRK_E_DEVICE, "%s: text size out of range", who);
    if ((rc = d->gf_text.ensure((size_t)n_text + 16))) return rc;
    d->tic();
    hipLaunchKernelGGL(strk_gff::k_gff_text, hit_grid, dim3(256), 0, 0, data, n, n_hit, d->gf_out.at<int64_t>(q_ta), d->gf_out.at<int32_t>(q_tl),
                       d->gf_out.at<int64_t>(q_ia), d->gf_out.at<int32_t>(q_il), d->gf_out.at<int64_t>(q_to), n_text, d->gf_text.as<uint8_t>());
    HIP_TRY(hipGetLastError());
    d->toc();
    std::vector<uint8_t> down(n_down);
    HIP_TRY(hipMemcpy(down.data(), d->gf_out.p, n_down, hipMemcpyDeviceToHost));
    r.text.resize((size_t)n_text);
    if (n_text) HIP_TRY(hipMemcpy(r.text.data(), d->gf_text.p, (size_t)n_text, hipMemcpyDeviceToHost));
    const int64_t* const h_po = (const int64_t*)(down.data() + q_po);
    const int32_t* const h_pf = (const int32_t*)(down.data() + q_pf);
    const int32_t *const h_tl = (const int32_t*)(down.data() + q_tl), *const h_il = (const int32_t*)(down.data() + q_il);
    const int64_t* const h_to = (const int64_t*)(down.data() + q_to);
    // (what came back is data like any other: emit() indexes with these offsets)
    for (int32_t l = 0; l < n_loci; ++l)
        if (h_po[l] < 0 || h_po[l] > h_po[l + 1] || h_po[l + 1] > n_pairs) return fail(STRK_E_DEVICE, "%s: pair offsets out of order", who);
    for (int64_t i = 0; i < n_pairs; ++i)
        if (h_pf[i] < 0 || h_pf[i] >= n_hit) return fail(STRK_E_DEVICE, "%s: pair %lld names no hit feature", who, (long long)i);
    r.pair_off.assign(h_po, h_po + n_loci + 1);
    r.pair_feat.assign(h_pf, h_pf + n_pairs);
    r.f_beg.assign((const int64_t*)(down.data() + q_hb), (const int64_t*)(down.data() + q_hb) + n_hit);
    r.f_end.assign((const int64_t*)(down.data() + q_he), (const int64_t*)(down.data() + q_he) + n_hit);
    r.kind.assign((const int32_t*)(down.data() + q_hk), (const int32_t*)(down.data() + q_hk) + n_hit);
    r.text_off.assign(1, 0);
    for (int32_t j = 0; j < n_hit; ++j) {
        if (h_tl[j] < 0 || h_il[j] < 0 || h_to[j] < 0 || h_to[j] + h_tl[j] + h_il[j] > n_text) return fail(STRK_E_DEVICE, "%s: text offsets out of order", who);
        r.text_off.push_back(h_to[j] + h_tl[j]);
        r.text_off.push_back(h_to[j] + h_tl[j] + h_il[j]);
    }
    return done();
}

}  // extern "C"
