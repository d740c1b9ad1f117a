// strk_vcf.inc — candidate SNVs from VCF text (part of strk_api.hip, after strk_lines.inc): strk_vcf_snvs over a decompressed host
// buffer (after strk_bgzf_inflate_range) and strk_dbam_vcf_snvs over the stream of a strk_dbam object (a BGZF file inflated in
// HBM: nothing in that object is BAM-specific).  The rule of a line, the host walk, the closing pass and the kernels are
// strk_vcf.h, the lines strk_lines.h / strk_lines.inc; here are the argument checks, the buffers and the launches.

namespace {

// the arguments both entry points share, checked before anything is read
int vcf_check(const char* who, int64_t n_bytes, int64_t start, const char* contig, int64_t beg, int64_t end, int64_t prev_pos, int64_t cap,
              const int64_t* pos, const uint8_t* ref, const int64_t* id_off, const uint8_t* ids, int64_t ids_cap, const int64_t* id_bytes,
              const int64_t* end_off, const int32_t* past) {
    if (const int rc = text_check(who, n_bytes, start, contig, id_bytes, end_off, past)) return rc;
    if (beg < 0 || end < beg) return fail(STRK_E_INVALID, "%s: bad window [%lld, %lld)", who, (long long)beg, (long long)end);
    if (prev_pos < -1) return fail(STRK_E_INVALID, "%s: bad prev_pos", who);
    if (cap < 0 || ids_cap < 0 || (cap > 0 && (!pos || !ref || !id_off))) return fail(STRK_E_INVALID, "%s: NULL output array", who);
    return 0;
}

int64_t vcf_finish(const char* who, const strk_vcf::Kept& k, int64_t bad_off, int64_t prev_pos, int64_t cap, int64_t* pos, uint8_t* ref,
                   int64_t* id_off, uint8_t* ids, int64_t ids_cap, int64_t* id_bytes) {
    strk_vcf::Message msg;
    int64_t one_off[1];
    const int64_t n = strk_vcf::finish(k, bad_off, prev_pos, cap, pos, ref, cap > 0 ? id_off : one_off, ids, ids_cap, id_bytes, &msg);
    if (n == -1) return fail(STRK_E_INVALID, "%s: %s", who, msg.text);
    if (n == -2) return fail(STRK_E_NOMEM, "%s: %s", who, msg.text);
    return n;
}

}  // namespace

extern "C" {

void strk_vcf_constants(int32_t* out3) {
    out3[0] = strk_lines::kTileBytes; out3[1] = strk_lines::kStepBytes; out3[2] = strk_vcf::kLinesPerWave;
}

int64_t strk_vcf_snvs(const uint8_t* buf, int64_t n_bytes, int64_t start, const char* contig, int64_t beg, int64_t end, int32_t final,
                      int64_t prev_pos, int32_t contig_seen, int64_t cap, int64_t* pos, uint8_t* ref, int64_t* id_off, uint8_t* ids,
                      int64_t ids_cap, int64_t* id_bytes, int64_t* end_off, int32_t* past) {
    static const char who[] = "strk_vcf_snvs";
    int rc = vcf_check(who, n_bytes, start, contig, beg, end, prev_pos, cap, pos, ref, id_off, ids, ids_cap, id_bytes, end_off, past);
    if (rc) return rc;
    if (!buf && n_bytes > 0) return fail(STRK_E_INVALID, "%s: NULL argument", who);
    strk_vcf::Walk w;
    strk_vcf::snvs_host(buf, n_bytes, start, contig, beg, end, final, contig_seen, &w, [](int32_t n, auto&& body) { strk_threads::parallel_slices(n, 1024, 32, body); });
    *end_off = w.end_off; *past = w.past;
    return vcf_finish(who, w.kept, w.bad_off, prev_pos, cap, pos, ref, id_off, ids, ids_cap, id_bytes);
}

int64_t strk_dbam_vcf_snvs(strk_dbam* d, int64_t start, const char* contig, int64_t beg, int64_t end, int32_t final, int64_t prev_pos,
                           int32_t contig_seen, int32_t tile_bytes, int64_t cap, int64_t* pos, uint8_t* ref, int64_t* id_off, uint8_t* ids,
                           int64_t ids_cap, int64_t* id_bytes, int64_t* end_off, int32_t* past) {
    static const char who[] = "strk_dbam_vcf_snvs";
    if (!d) return fail(STRK_E_INVALID, "%s: bad argument", who);
    // before any launch: the start offset lies inside the stream, the piece is below 2^31 bytes
    int rc = vcf_check(who, d->n_data, start, contig, beg, end, prev_pos, cap, pos, ref, id_off, ids, ids_cap, id_bytes, end_off, past);
    if (rc) return rc;
    *id_bytes = 0; *past = 0; *end_off = start;
    DevLines l;
    if ((rc = dbam_lines(d, who, start, final, tile_bytes, &l))) return rc;
    const int64_t n = d->n_data;
    *end_off = l.end_off;
    if (start == n) {   // nothing to read, nothing launched
        strk_vcf::Kept none;
        none.id_off.push_back(0);
        return vcf_finish(who, none, -1, prev_pos, cap, pos, ref, id_off, ids, ids_cap, id_bytes);
    }
    const uint8_t* const data = d->data.as<uint8_t>();
    const int64_t* const starts = l.starts;
    const int32_t n_nl = l.n_nl, n_lines = l.n_lines, contig_len = (int32_t)strlen(contig);
    strk_vcf::Kept k;
    k.id_off.push_back(0);
    int64_t bad = -1;
    if (n_lines > 0) {
        const int32_t n_waves = (n_lines + 63) / 64;
        const dim3 line_grid = l.line_grid;
        unsigned long long* st = nullptr;
        const uint8_t* name = nullptr;
        if ((rc = dbam_query(d, {~0ull, ~0ull, 0ull, 0ull}, contig, contig_len, &st, &name))) return rc;
        // vc_lines: pos | id_a | id_len | ref | status per line | kept lines and ID bytes per wave, their offsets
        const size_t cap_lines = (size_t)n_nl + 1, n_lw = (cap_lines + 63) / 64;
        Carve cl;
        const size_t o_pos = cl.take(cap_lines * 8), o_ida = cl.take(cap_lines * 8), o_idl = cl.take(cap_lines * 4), o_ref = cl.take(cap_lines),
                     o_stat = cl.take(cap_lines), o_kc = cl.take(n_lw * 4), o_ic = cl.take(n_lw * 4), o_ko = cl.take((n_lw + 1) * 8),
                     o_io = cl.take((n_lw + 1) * 8);
        if ((rc = d->vc_lines.ensure(cl.bytes))) return rc;
        d->tic();
        hipLaunchKernelGGL(strk_vcf::k_vcf_parse, line_grid, dim3(256), 0, 0, data, n, starts, n_nl, n_lines, name, contig_len,
                           beg, end, d->vc_lines.at<int64_t>(o_pos), d->vc_lines.at<int64_t>(o_ida), d->vc_lines.at<int32_t>(o_idl),
                           d->vc_lines.at<uint8_t>(o_ref), d->vc_lines.at<uint8_t>(o_stat), d->vc_lines.at<int32_t>(o_kc), d->vc_lines.at<int32_t>(o_ic), st);
        hipLaunchKernelGGL(strk_lines::k_lines_scan, dim3(1), dim3(256), 0, 0, d->vc_lines.at<int32_t>(o_kc), n_waves, d->vc_lines.at<int64_t>(o_ko));
        hipLaunchKernelGGL(strk_lines::k_lines_scan, dim3(1), dim3(256), 0, 0, d->vc_lines.at<int32_t>(o_ic), n_waves, d->vc_lines.at<int64_t>(o_io));
        HIP_TRY(hipGetLastError());
        d->toc();
        unsigned long long sth[4];
        int64_t n_keep = 0, n_idb = 0;
        HIP_TRY(hipMemcpy(sth, st, 32, hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(&n_keep, d->vc_lines.at<int64_t>(o_ko) + n_waves, 8, hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(&n_idb, d->vc_lines.at<int64_t>(o_io) + n_waves, 8, hipMemcpyDeviceToHost));
        if (n_keep < 0 || n_keep > n_lines || n_idb < 0 || n_idb > n - start) return fail(STRK_E_DEVICE, "%s: kept count out of range", who);
        if (sth[0] != ~0ull) bad = (int64_t)sth[0];
        const bool on_seen = contig_seen || sth[1] != ~0ull;
        *past = (sth[3] || (on_seen && (contig_seen ? sth[2] > 0 : sth[2] > sth[1] + 1))) ? 1 : 0;
        if (n_keep > 0) {
            // vc_out: pos | line | id_off | ref | ids of the kept lines
            Carve co;
            const size_t q_pos = co.take((size_t)n_keep * 8), q_line = co.take((size_t)n_keep * 8), q_ido = co.take((size_t)n_keep * 8),
                         q_ref = co.take((size_t)n_keep), q_ids = co.take((size_t)n_idb + 16);
            if ((rc = d->vc_out.ensure(co.bytes))) return rc;
            d->tic();
            hipLaunchKernelGGL(strk_vcf::k_vcf_compact, line_grid, dim3(256), 0, 0, data, starts, n_lines, d->vc_lines.at<int64_t>(o_pos),
                               d->vc_lines.at<int64_t>(o_ida), d->vc_lines.at<int32_t>(o_idl), d->vc_lines.at<uint8_t>(o_ref),
                               d->vc_lines.at<uint8_t>(o_stat), d->vc_lines.at<int64_t>(o_ko), d->vc_lines.at<int64_t>(o_io), n_keep, n_idb,
                               d->vc_out.at<int64_t>(q_pos), d->vc_out.at<int64_t>(q_line), d->vc_out.at<int64_t>(q_ido), d->vc_out.at<uint8_t>(q_ref),
                               d->vc_out.at<uint8_t>(q_ids));
            HIP_TRY(hipGetLastError());
            d->toc();
            k.pos.resize((size_t)n_keep); k.line.resize((size_t)n_keep); k.id_off.resize((size_t)n_keep + 1); k.ref.resize((size_t)n_keep);
            k.ids.resize((size_t)n_idb);
            HIP_TRY(hipMemcpy(k.pos.data(), d->vc_out.at<char>(q_pos), (size_t)n_keep * 8, hipMemcpyDeviceToHost));
            HIP_TRY(hipMemcpy(k.line.data(), d->vc_out.at<char>(q_line), (size_t)n_keep * 8, hipMemcpyDeviceToHost));
            HIP_TRY(hipMemcpy(k.id_off.data(), d->vc_out.at<char>(q_ido), (size_t)n_keep * 8, hipMemcpyDeviceToHost));
            HIP_TRY(hipMemcpy(k.ref.data(), d->vc_out.at<char>(q_ref), (size_t)n_keep, hipMemcpyDeviceToHost));
            if (n_idb) HIP_TRY(hipMemcpy(k.ids.data(), d->vc_out.at<char>(q_ids), (size_t)n_idb, hipMemcpyDeviceToHost));
            k.id_off[(size_t)n_keep] = n_idb;
            // (what came back is data like any other: finish() indexes ids with these offsets)
            for (int64_t i = 0; i < n_keep; ++i)
                if (k.id_off[(size_t)i] < 0 || k.id_off[(size_t)i] > k.id_off[(size_t)i + 1] || k.id_off[(size_t)i + 1] > n_idb)
                    return fail(STRK_E_DEVICE, "%s: ID offsets out of order", who);
        }
    }
    return vcf_finish(who, k, bad, prev_pos, cap, pos, ref, id_off, ids, ids_cap, id_bytes);
}

}  // extern "C"
