// strk_host_files.inc — the file front end on the CPU: record scan, read names, read extraction and BGZF inflation over host
// buffers (strk_bam_scan*, strk_bam_names, strk_extract_reads, strk_bgzf_inflate*).  No device work, no context.
// Part of strk_api.hip: included inside its extern "C" block (uses fail() defined there, the threads of strk_threads.h, the record parser
// of strk_frontend.h); not a stand-alone header.
static int64_t bam_scan_impl(const uint8_t* buf, int64_t n_bytes, int64_t first_rec, int64_t cap, int64_t* rec_off, int32_t* tid,
                             int32_t* pos, int32_t* end, int32_t* flag, int32_t* l_seq, int32_t* clip_l, int32_t* clip_r, int64_t* end_off) {
    if (!buf || n_bytes < 0 || first_rec < 0 || cap < 0) return fail(STRK_E_INVALID, "bad argument");
    if (cap > 0 && (!rec_off || !tid || !pos || !end || !flag || !l_seq || !clip_l || !clip_r)) return fail(STRK_E_INVALID, "NULL output array");
    int64_t off = first_rec, n = 0;
    while (off + 4 <= n_bytes) {
        strk_fe::Rec r;
        int64_t next = 0;
        if (end_off) {   // a piece of the stream: the last record may be cut off
            const int32_t block = strk_fe::rd_i32(buf + off);
            if (block >= 32 && off + 4 + block > n_bytes) break;
        }
        if (!strk_fe::parse_rec(buf, n_bytes, off, &r, &next)) return fail(STRK_E_INVALID, "malformed BAM record at byte %lld", (long long)off);
        if (n < cap) {
            int64_t ref_len = 0;
            int32_t cl = 0, cr = 0;
            for (int32_t i = 0; i < r.n_cigar; ++i) {
                const uint32_t c = strk_fe::rd_u32(r.cigar + 4 * (size_t)i), op = c & 15u;
                if (strk_fe::consumes_ref(op)) ref_len += c >> 4;
                if (op == 4 && i == 0) cl = (int32_t)(c >> 4);
                if (op == 4 && i == r.n_cigar - 1) cr = (int32_t)(c >> 4);
            }
            rec_off[n] = off; tid[n] = r.tid; pos[n] = r.pos; end[n] = (int32_t)(r.pos + ref_len); flag[n] = r.flag;
            l_seq[n] = r.l_seq; clip_l[n] = cl; clip_r[n] = cr;
        }
        ++n;
        off = next;
    }
    if (end_off) *end_off = off;
    return n;
}

int64_t strk_bam_scan(const uint8_t* buf, int64_t n_bytes, int64_t first_rec, int64_t cap, int64_t* rec_off, int32_t* tid,
                      int32_t* pos, int32_t* end, int32_t* flag, int32_t* l_seq, int32_t* clip_l, int32_t* clip_r) {
    return bam_scan_impl(buf, n_bytes, first_rec, cap, rec_off, tid, pos, end, flag, l_seq, clip_l, clip_r, nullptr);
}

int64_t strk_bam_scan_piece(const uint8_t* buf, int64_t n_bytes, int64_t first_rec, int64_t cap, int64_t* rec_off, int32_t* tid,
                            int32_t* pos, int32_t* end, int32_t* flag, int32_t* l_seq, int32_t* clip_l, int32_t* clip_r,
                            int64_t* end_off) {
    if (!end_off) return fail(STRK_E_INVALID, "end_off is NULL");
    return bam_scan_impl(buf, n_bytes, first_rec, cap, rec_off, tid, pos, end, flag, l_seq, clip_l, clip_r, end_off);
}

int64_t strk_bam_names(const uint8_t* buf, int64_t n_bytes, int64_t n, const int64_t* rec_off, uint8_t* out, int64_t out_cap,
                       int64_t* out_off) {
    if (!buf || n < 0 || (n > 0 && (!rec_off || !out_off))) return fail(STRK_E_INVALID, "bad argument");
    int64_t w = 0;
    if (out_off) out_off[0] = 0;
    for (int64_t i = 0; i < n; ++i) {
        strk_fe::Rec r;
        int64_t next = 0;
        if (!strk_fe::parse_rec(buf, n_bytes, rec_off[i], &r, &next)) return fail(STRK_E_INVALID, "malformed BAM record at byte %lld", (long long)rec_off[i]);
        const int64_t len = r.l_name > 0 ? r.l_name - 1 : 0;
        if (out) {
            if (w + len > out_cap) return fail(STRK_E_NOMEM, "name buffer too small");
            memcpy(out + w, r.name, (size_t)len);
        }
        w += len;
        out_off[i + 1] = w;
    }
    return w;
}

int strk_extract_reads(const uint8_t* buf, int64_t n_bytes, int32_t n_items, const int64_t* rec_off, const int64_t* coords,
                       const uint32_t* alt_cigar, const int64_t* alt_cigar_off, const int64_t* alt_start, int32_t flank_size,
                       int32_t min_avg_phred, int32_t wildcard_threshold, int32_t* status, int32_t* nfl, int32_t* ntr,
                       int32_t* nfr, uint8_t* seqs, int64_t seq_cap, int64_t* seq_off) {
    if (n_items < 0 || flank_size < 0) return fail(STRK_E_INVALID, "bad argument");
    if (n_items == 0) { if (seq_off) seq_off[0] = 0; return 0; }
    if (!buf || !rec_off || !coords || !status || !nfl || !ntr || !nfr || !seq_off) return fail(STRK_E_INVALID, "NULL argument");
    const strk_fe::AltCigars alt{alt_cigar, alt_cigar_off, alt_start};
    strk_groups::Message msg;
    if (strk_fe::check_alt(n_items, alt, &msg)) return fail(STRK_E_INVALID, "%s", msg.text);
    static const char kBases[] = "=ACMGRSVTWYHKDBN";
    // contiguous slices, one thread per thousand items (strk_threads.h)
    auto parallel = [&](auto&& body) { strk_threads::parallel_slices(n_items, 1024, 32, body); };
    // pass 1: where each read's flank | tract | flank lies (read positions a <= b <= c <= d), status, lengths
    std::vector<int64_t> cut((size_t)n_items * 2);   // a and b; c = b + ntr, d = c + nfr
    strk_threads::FirstBad bad;
    parallel([&](int32_t i0, int32_t i1) {
        strk_fe::Runs runs;
        for (int32_t it = i0; it < i1; ++it) {
            status[it] = 1; nfl[it] = ntr[it] = nfr[it] = 0;
            strk_fe::Rec r;
            int64_t next = 0;
            if (!strk_fe::parse_rec(buf, n_bytes, rec_off[it], &r, &next)) { bad.report(it); return; }
            const uint8_t* cig;
            int32_t n_cig;
            int64_t start;
            strk_fe::item_alignment(r, it, alt, &cig, &n_cig, &start);
            runs.build(cig, n_cig, start);
            int64_t q[4];
            if (!strk_fe::read_coords(runs, coords[4 * (size_t)it], coords[4 * (size_t)it + 1], coords[4 * (size_t)it + 2], coords[4 * (size_t)it + 3], q)) continue;
            const int64_t b = q[1], c = q[2];
            const int64_t a = std::max(q[0], b - flank_size), d = std::min(q[3], c + flank_size);
            if (a < 0 || d > r.l_seq || a > b || b > c || c > d) continue;   // coordinates outside the read: incomplete
            const bool has_qual = !(r.l_seq > 0 && r.qual[0] == 0xFF);
            if (has_qual && c > b) {   // LowMeanBaseQual on the tract bases (call_locus.py:1099-1115)
                int64_t sum = 0;
                for (int64_t i = b; i < c; ++i) sum += r.qual[i];
                if ((double)sum / (double)(c - b) < (double)min_avg_phred) { status[it] = 2; continue; }
            }
            status[it] = 0;
            nfl[it] = (int32_t)(b - a); ntr[it] = (int32_t)(c - b); nfr[it] = (int32_t)(d - c);
            cut[2 * (size_t)it] = a;
        }
    });
    if (bad.get() >= 0) return fail(STRK_E_INVALID, "item %d: malformed BAM record", (int)bad.get());
    int64_t w = 0;
    seq_off[0] = 0;
    for (int32_t it = 0; it < n_items; ++it) {
        w += (int64_t)nfl[it] + ntr[it] + nfr[it];
        seq_off[it + 1] = w;
    }
    if (!seqs) return 0;   // size query: seq_off[n_items] bytes are needed
    if (w > seq_cap) return fail(STRK_E_NOMEM, "sequence buffer too small (%lld < %lld)", (long long)seq_cap, (long long)w);
    // pass 2: bases (4 bit -> ASCII), low-quality bases -> 'X' (call_locus.py:79,1101-1106)
    parallel([&](int32_t i0, int32_t i1) {
        for (int32_t it = i0; it < i1; ++it) {
            if (status[it] != 0) continue;
            strk_fe::Rec r;
            int64_t next = 0;
            (void)strk_fe::parse_rec(buf, n_bytes, rec_off[it], &r, &next);
            const bool has_qual = !(r.l_seq > 0 && r.qual[0] == 0xFF);
            const int64_t a = cut[2 * (size_t)it], d = a + nfl[it] + ntr[it] + nfr[it];
            uint8_t* o = seqs + seq_off[it];
            for (int64_t i = a; i < d; ++i) {
                const uint8_t byte = r.seq[i >> 1];
                char ch = kBases[(i & 1) ? (byte & 15) : (byte >> 4)];
                if (has_qual && (int32_t)r.qual[i] <= wildcard_threshold) ch = 'X';
                *o++ = (uint8_t)ch;
            }
        }
    });
    return 0;
}

// Which of the records fetched for each locus are used (the rule, the check and the host twin: strk_select.h).  Every record is
// parsed before the rule runs; threads take runs of sixteen loci.
int strk_select_reads(const uint8_t* buf, int64_t n_bytes, int32_t n_loci, const int64_t* item_off, const int64_t* rec_off, int32_t rules,
                      int32_t max_reads, uint8_t* out_reason, uint8_t* out_status, int32_t* out_n_kept) {
    const strk_sel::Input in{n_bytes, n_loci, item_off, rec_off, rules, max_reads};
    strk_groups::Message msg;
    if (strk_sel::check_input(in, &msg)) return fail(STRK_E_INVALID, "strk_select_reads: %s", msg.text);
    if (n_loci == 0) return 0;
    const int64_t n_items = item_off[n_loci];
    if (!out_n_kept || (n_items > 0 && (!buf || !out_reason || !out_status))) return fail(STRK_E_INVALID, "strk_select_reads: NULL argument");
    const int nt = (int)std::min<int64_t>({(int64_t)host_cpus(), 32, n_items / 4096});
    strk_threads::FirstBad bad;
    strk_threads::parallel_chunks(n_items, 4096, nt, [&](int64_t i0, int64_t i1) {
        const int64_t b = strk_sel::host_first_bad(buf, in, i0, i1);
        if (b >= 0) bad.report(b);
    });
    if (bad.get() >= 0) return fail(STRK_E_INVALID, "strk_select_reads: item %lld: malformed BAM record", (long long)bad.get());
    strk_threads::parallel_chunks<strk_sel::HostTable>(n_loci, 16, nt, [&](int64_t l0, int64_t l1, strk_sel::HostTable& table) {
        for (int32_t l = (int32_t)l0; l < l1; ++l) strk_sel::host_locus(buf, in, l, table, out_reason, out_status, out_n_kept);
    });
    return 0;
}

// Inflates `blocks` of `comp` into `out` on up to n_threads threads (<= 0: the CPUs of this process; 32 at most) that take
// sixteen blocks at a time; false when a block is corrupt.  thread_per_16: at most one thread per sixteen blocks (a range of a
// few blocks is not worth starting threads for).
static bool bgzf_inflate_blocks(const uint8_t* comp, const std::vector<strk_fe::BgzfBlock>& blocks, uint8_t* out, int32_t n_threads,
                                bool thread_per_16) {
    int nt = std::max(1, std::min<int>(n_threads > 0 ? n_threads : host_cpus(), 32));
    if (thread_per_16) nt = (int)std::min<size_t>((size_t)nt, 1 + (blocks.size() + 15) / 16);
    std::atomic<int> bad{0};
    strk_threads::parallel_chunks((int64_t)blocks.size(), 16, nt, [&](int64_t k0, int64_t k1) {
        for (int64_t k = k0; k < k1; ++k)
            if (!strk_fe::bgzf_inflate_block(comp, blocks[(size_t)k], out)) bad.store(1);
    });
    return bad.load() == 0;
}

int64_t strk_bgzf_inflate_range(const uint8_t* comp, int64_t n_comp, int64_t coff, uint8_t* out, int64_t out_cap,
                                int64_t* next_coff, int32_t n_threads) {
    if (!comp || !out || !next_coff || n_comp < 0 || coff < 0 || coff > n_comp || out_cap < 0) return fail(STRK_E_INVALID, "bad argument");
    // walk the block headers from `coff` while the decompressed blocks still fit
    std::vector<strk_fe::BgzfBlock> blocks;
    int64_t off = coff, total = 0;
    while (off < n_comp) {
        std::vector<strk_fe::BgzfBlock> one;
        int64_t sz = 0;
        // the header of one block: reuse the indexer on a window that holds exactly this block
        if (off + 18 > n_comp) return fail(STRK_E_INVALID, "truncated BGZF block header at byte %lld", (long long)off);
        const uint8_t* p = comp + off;
        if (p[0] != 0x1f || p[1] != 0x8b || p[2] != 8 || !(p[3] & 4)) return fail(STRK_E_INVALID, "not a BGZF block at byte %lld", (long long)off);
        const int xlen = strk_fe::rd_u16(p + 10);
        int bsize = -1;
        for (int64_t x = 12; x + 4 <= 12 + xlen && off + x + 4 <= n_comp;) {
            const int slen = strk_fe::rd_u16(p + x + 2);
            if (p[x] == 'B' && p[x + 1] == 'C' && slen == 2 && x + 6 <= 12 + xlen && off + x + 6 <= n_comp) bsize = strk_fe::rd_u16(p + x + 4);
            x += 4 + slen;
        }
        if (bsize < 0 || off + bsize + 1 > n_comp) return fail(STRK_E_INVALID, "truncated BGZF block at byte %lld", (long long)off);
        if (strk_fe::bgzf_index(p, bsize + 1, &one, &sz) || one.size() != 1) return fail(STRK_E_INVALID, "bad BGZF block at byte %lld", (long long)off);
        if (total + one[0].out_len > out_cap) break;
        one[0].in_off += off;
        one[0].out_off = total;
        total += one[0].out_len;
        blocks.push_back(one[0]);
        off += bsize + 1;
    }
    *next_coff = off;
    return bgzf_inflate_blocks(comp, blocks, out, n_threads, true) ? total : fail(STRK_E_INVALID, "corrupt BGZF block (inflate or CRC failed)");
}

int64_t strk_bgzf_inflate(const uint8_t* comp, int64_t n_comp, uint8_t* out, int64_t out_cap, int32_t n_threads) {
    if (!comp || n_comp < 0) return fail(STRK_E_INVALID, "bad argument");
    std::vector<strk_fe::BgzfBlock> blocks;
    int64_t total = 0, bad = 0;
    if (strk_fe::bgzf_index(comp, n_comp, &blocks, &total, &bad))
        return fail(STRK_E_INVALID, "not a BGZF stream (or truncated): bad BGZF block at byte %lld", (long long)bad);
    if (!out) return total;   // size query
    if (out_cap < total) return fail(STRK_E_NOMEM, "output buffer too small (%lld < %lld)", (long long)out_cap, (long long)total);
    return bgzf_inflate_blocks(comp, blocks, out, n_threads, false) ? total : fail(STRK_E_INVALID, "corrupt BGZF block (inflate or CRC failed)");
}

