// strk_vcf.inc — candidate SNVs from VCF text (part of strk_api.hip, after strk_methyl.inc): strk_vcf_snvs over a decompressed host
// buffer (after strk_bgzf_inflate_range) and strk_dbam_vcf_snvs over the stream of a strk_dbam object (a BGZF file inflated in
// HBM: nothing in that object is BAM-specific).  The rule of a line, the closing pass and the kernels are strk_vcf.h; here are
// the threads, the buffers and the launches.

namespace {

// the arguments both entry points share, checked before anything is read
int vcf_check(const char* who, int64_t n_bytes, int64_t start, const char* contig, int64_t beg, int64_t end, int64_t prev_pos, int64_t cap,
              const int64_t* pos, const uint8_t* ref, const int64_t* id_off, const uint8_t* ids, int64_t ids_cap, const int64_t* id_bytes,
              const int64_t* end_off, const int32_t* past) {
    if (!contig || !contig[0]) return fail(STRK_E_INVALID, "%s: no contig name", who);
    if (!id_bytes || !end_off || !past) return fail(STRK_E_INVALID, "%s: NULL argument", who);
    if (n_bytes < 0 || start < 0 || start > n_bytes) return fail(STRK_E_INVALID, "%s: start offset %lld outside the text of %lld bytes", who, (long long)start, (long long)n_bytes);
    if (n_bytes - start >= ((int64_t)1 << 31)) return fail(STRK_E_INVALID, "%s: a piece of %lld bytes (at most 2^31 - 1)", who, (long long)(n_bytes - start));
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
    out3[0] = strk_vcf::kTileBytes; out3[1] = strk_vcf::kStepBytes; out3[2] = strk_vcf::kLinesPerWave;
}

int64_t strk_vcf_snvs(const uint8_t* buf, int64_t n_bytes, int64_t start, const char* contig, int64_t beg, int64_t end, int32_t final,
                      int64_t prev_pos, int32_t contig_seen, int64_t cap, int64_t* pos, uint8_t* ref, int64_t* id_off, uint8_t* ids,
                      int64_t ids_cap, int64_t* id_bytes, int64_t* end_off, int32_t* past) {
    static const char who[] = "strk_vcf_snvs";
    int rc = vcf_check(who, n_bytes, start, contig, beg, end, prev_pos, cap, pos, ref, id_off, ids, ids_cap, id_bytes, end_off, past);
    if (rc) return rc;
    if (!buf && n_bytes > 0) return fail(STRK_E_INVALID, "%s: NULL argument", who);
    // the lines: one memchr walk (it runs at memory speed); the fields of the lines are then read by all cores
    std::vector<int64_t> starts{start};
    for (int64_t p = start; p < n_bytes;) {
        const void* nl = memchr(buf + p, '\n', (size_t)(n_bytes - p));
        if (!nl) break;
        p = (const uint8_t*)nl - buf + 1;
        starts.push_back(p);
    }
    const int32_t n_nl = (int32_t)starts.size() - 1;
    const int32_t n_lines = n_nl + ((final && starts.back() < n_bytes) ? 1 : 0);
    *end_off = n_lines > n_nl ? n_bytes : starts.back();
    const int32_t contig_len = (int32_t)strlen(contig);
    struct Slice { strk_vcf::Kept k; int64_t bad = -1, first_on = -1, last_other = -1; bool past = false; };
    std::mutex mu;
    std::vector<std::pair<int32_t, Slice>> slices;
    pi_parallel(n_lines, [&](int32_t i0, int32_t i1) {
        Slice s;
        s.k.id_off.push_back(0);
        for (int32_t i = i0; i < i1; ++i) {
            const int64_t a = starts[(size_t)i], e = i < n_nl ? starts[(size_t)i + 1] - 1 : n_bytes;
            const strk_vcf::Line r = strk_vcf::parse_line(buf, a, e, (const uint8_t*)contig, contig_len, beg, end);
            switch (r.status) {
            case strk_vcf::kBadPos: if (s.bad < 0) s.bad = a; break;
            case strk_vcf::kOther: s.last_other = i; break;
            case strk_vcf::kPast: s.past = true; [[fallthrough]];
            case strk_vcf::kBefore: if (s.first_on < 0) s.first_on = i; break;
            case strk_vcf::kKeep:
                if (s.first_on < 0) s.first_on = i;
                s.k.pos.push_back(r.pos); s.k.line.push_back(a); s.k.ref.push_back(r.ref);
                s.k.ids.insert(s.k.ids.end(), buf + r.id_a, buf + r.id_a + r.id_len);
                s.k.id_off.push_back((int64_t)s.k.ids.size());
                break;
            default: break;
            }
        }
        std::lock_guard<std::mutex> lk(mu);
        slices.emplace_back(i0, std::move(s));
    });
    std::sort(slices.begin(), slices.end(), [](const auto& x, const auto& y) { return x.first < y.first; });
    strk_vcf::Kept all;
    all.id_off.push_back(0);
    int64_t bad = -1, first_on = contig_seen ? 0 : -1, last_other = -1;
    bool any_past = false;
    for (auto& [i0, s] : slices) {
        if (bad < 0) bad = s.bad;
        if (first_on < 0) first_on = s.first_on;
        if (s.last_other >= 0) last_other = s.last_other;
        any_past = any_past || s.past;
        const int64_t id0 = (int64_t)all.ids.size();
        all.pos.insert(all.pos.end(), s.k.pos.begin(), s.k.pos.end());
        all.line.insert(all.line.end(), s.k.line.begin(), s.k.line.end());
        all.ref.insert(all.ref.end(), s.k.ref.begin(), s.k.ref.end());
        all.ids.insert(all.ids.end(), s.k.ids.begin(), s.k.ids.end());
        for (size_t j = 1; j < s.k.id_off.size(); ++j) all.id_off.push_back(id0 + s.k.id_off[j]);
    }
    *past = (any_past || (first_on >= 0 && (contig_seen ? last_other >= 0 : last_other > first_on))) ? 1 : 0;
    return vcf_finish(who, all, bad, prev_pos, cap, pos, ref, id_off, ids, ids_cap, id_bytes);
}

int64_t strk_dbam_vcf_snvs(strk_dbam* d, int64_t start, const char* contig, int64_t beg, int64_t end, int32_t final, int64_t prev_pos,
                           int32_t contig_seen, int32_t tile_bytes, int64_t cap, int64_t* pos, uint8_t* ref, int64_t* id_off, uint8_t* ids,
                           int64_t ids_cap, int64_t* id_bytes, int64_t* end_off, int32_t* past) {
    static const char who[] = "strk_dbam_vcf_snvs";
    if (!d) return fail(STRK_E_INVALID, "%s: bad argument", who);
    // before any launch: the start offset lies inside the stream, the piece is below 2^31 bytes
    int rc = vcf_check(who, d->n_data, start, contig, beg, end, prev_pos, cap, pos, ref, id_off, ids, ids_cap, id_bytes, end_off, past);
    if (rc) return rc;
    if (tile_bytes == 0) tile_bytes = strk_vcf::kTileBytes;
    if (tile_bytes < strk_vcf::kStepBytes || tile_bytes % strk_vcf::kStepBytes || tile_bytes > (1 << 20))
        return fail(STRK_E_INVALID, "%s: tile_bytes must be a multiple of %d", who, strk_vcf::kStepBytes);
    const int64_t n = d->n_data;
    *id_bytes = 0; *past = 0; *end_off = start;
    if (start == n) {   // nothing to read, nothing launched
        strk_vcf::Kept none;
        none.id_off.push_back(0);
        return vcf_finish(who, none, -1, prev_pos, cap, pos, ref, id_off, ids, ids_cap, id_bytes);
    }
    HIP_TRY(hipSetDevice(d->device));
    const uint8_t* const data = d->data.as<uint8_t>();
    const int32_t contig_len = (int32_t)strlen(contig);
    // ---- the lines.  vc_tiles: counts | offsets | status words | the contig's name
    const int64_t t0 = start & ~(int64_t)(strk_vcf::kStepBytes - 1);
    const int32_t n_tiles = (int32_t)((n - t0 + tile_bytes - 1) / tile_bytes);
    Carve ct;
    const size_t o_cnt = ct.take((size_t)n_tiles * 4), o_off = ct.take(((size_t)n_tiles + 1) * 8), o_st = ct.take(32), o_name = ct.take((size_t)contig_len);
    if ((rc = d->vc_tiles.ensure(ct.bytes))) return rc;
    const unsigned long long st0[4] = {~0ull, ~0ull, 0ull, 0ull};
    HIP_TRY(hipMemcpy(d->vc_tiles.at<char>(o_st), st0, 32, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(d->vc_tiles.at<char>(o_name), contig, (size_t)contig_len, hipMemcpyHostToDevice));
    const dim3 tile_grid((unsigned)((n_tiles + 3) / 4));
    d->tic();
    hipLaunchKernelGGL(strk_vcf::k_vcf_count, tile_grid, dim3(256), 0, 0, data, n, start, tile_bytes, n_tiles, d->vc_tiles.at<int32_t>(o_cnt));
    hipLaunchKernelGGL(strk_vcf::k_vcf_scan, dim3(1), dim3(256), 0, 0, d->vc_tiles.at<int32_t>(o_cnt), n_tiles, d->vc_tiles.at<int64_t>(o_off));
    HIP_TRY(hipGetLastError());
    d->toc();
    int64_t n_nl64 = 0;
    HIP_TRY(hipMemcpy(&n_nl64, d->vc_tiles.at<int64_t>(o_off) + n_tiles, 8, hipMemcpyDeviceToHost));
    if (n_nl64 < 0 || n_nl64 > n - start) return fail(STRK_E_DEVICE, "%s: line count %lld out of range", who, (long long)n_nl64);
    const int32_t n_nl = (int32_t)n_nl64;
    // vc_lines: starts [n_nl + 1] | pos | id_a | id_len | ref | status per line | kept lines and ID bytes per wave, their offsets
    const size_t cap_lines = (size_t)n_nl + 1, n_lw = (cap_lines + 63) / 64;
    Carve cl;
    const size_t o_starts = cl.take(cap_lines * 8), o_pos = cl.take(cap_lines * 8), o_ida = cl.take(cap_lines * 8), o_idl = cl.take(cap_lines * 4),
                 o_ref = cl.take(cap_lines), o_stat = cl.take(cap_lines), o_kc = cl.take(n_lw * 4), o_ic = cl.take(n_lw * 4),
                 o_ko = cl.take((n_lw + 1) * 8), o_io = cl.take((n_lw + 1) * 8);
    if ((rc = d->vc_lines.ensure(cl.bytes))) return rc;
    int64_t* const starts = d->vc_lines.at<int64_t>(o_starts);
    d->tic();
    hipLaunchKernelGGL(strk_vcf::k_vcf_starts, tile_grid, dim3(256), 0, 0, data, n, start, tile_bytes, n_tiles, d->vc_tiles.at<int64_t>(o_off),
                       (int64_t)cap_lines, starts);
    HIP_TRY(hipGetLastError());
    d->toc();
    int64_t last_start = 0;
    HIP_TRY(hipMemcpy(&last_start, starts + n_nl, 8, hipMemcpyDeviceToHost));
    if (last_start < start || last_start > n) return fail(STRK_E_DEVICE, "%s: line start %lld out of range", who, (long long)last_start);
    const int32_t n_lines = n_nl + ((final && last_start < n) ? 1 : 0);
    *end_off = n_lines > n_nl ? n : last_start;
    strk_vcf::Kept k;
    k.id_off.push_back(0);
    int64_t bad = -1;
    if (n_lines > 0) {
        const int32_t n_waves = (n_lines + 63) / 64;
        const dim3 line_grid((unsigned)((n_lines + 255) / 256));
        unsigned long long* const st = d->vc_tiles.at<unsigned long long>(o_st);
        d->tic();
        hipLaunchKernelGGL(strk_vcf::k_vcf_parse, line_grid, dim3(256), 0, 0, data, n, starts, n_nl, n_lines, d->vc_tiles.at<uint8_t>(o_name), contig_len,
                           beg, end, d->vc_lines.at<int64_t>(o_pos), d->vc_lines.at<int64_t>(o_ida), d->vc_lines.at<int32_t>(o_idl),
                           d->vc_lines.at<uint8_t>(o_ref), d->vc_lines.at<uint8_t>(o_stat), d->vc_lines.at<int32_t>(o_kc), d->vc_lines.at<int32_t>(o_ic), st);
        hipLaunchKernelGGL(strk_vcf::k_vcf_scan, dim3(1), dim3(256), 0, 0, d->vc_lines.at<int32_t>(o_kc), n_waves, d->vc_lines.at<int64_t>(o_ko));
        hipLaunchKernelGGL(strk_vcf::k_vcf_scan, dim3(1), dim3(256), 0, 0, d->vc_lines.at<int32_t>(o_ic), n_waves, d->vc_lines.at<int64_t>(o_io));
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
