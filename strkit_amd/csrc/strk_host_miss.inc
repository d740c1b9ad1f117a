// Window-miss resolution on the host (strkit/call/call_locus.py:1129-1161 order kept): resolve_misses().
// Part of strk_api.hip: included inside its anonymous namespace (uses fail(), HIP_TRY, DevBuf, strk_ctx and the
// scoring helpers defined there); not a stand-alone header.
struct SeenVec {
    std::vector<uint8_t> v;
    bool test(int k) const { return v[(size_t)k] != 0; }
    void set(int k) { v[(size_t)k] = 1; }
};

// Host-driven rounds for loci whose search left the speculative window.  Everything here works on
// DEVICE batch pointers; host copies of the small metadata are fetched once.
// Host copy of one locus that needs window-miss rounds: only the slices of its own reads are fetched.
struct MissLocus {
    int l = 0, r0 = 0, r1 = 0, m = 1;
    int first = 0;                 // first read the host (re)plays
    double frac = 0.0;
    int32_t need_lo = 0, need_hi = 0;
    std::vector<int32_t> est, win_lo, win_n, rep, nfl, ntr, nfr, table, o_cn, o_score, o_n, o_start, ext_lo;
    std::vector<int64_t> tab_off;
    std::vector<uint8_t> exact;
    std::vector<std::vector<int32_t>> ext;   // exact, widened tables of re-scored reads
    std::vector<uint8_t> tries;              // widenings a read has had: its window grows geometrically
    int rounds = 0;                          // rounds this locus has been pending for
};

int resolve_misses(strk_ctx* c, const strk_batch* b, const strk_params& p, KArgs a, ReplayArgs rp, hipStream_t st,
                   strk_stats* stats, int err_bits) {
    const int nl = b->n_loci, ts = a.table_stride;
    std::vector<int32_t> read_off(nl + 1), motif_off(nl + 1), next_read(nl), need_lo(nl), need_hi(nl);
    std::vector<double> frac(nl);
    // Every copy of this function is stream-ordered on the CALL'S OWN stream.  (A blocking hipMemcpy runs on the null stream,
    // which waits for — and holds back — the work of every other blocking stream of the process: the dozens of small copies
    // of one miss round then serialised all the calls in flight, 216 -> 140 M reads/s once a call had six such loci.)
    auto d2h = [&](void* dst, const void* src, size_t bytes) { return hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, st); };
    HIP_TRY(d2h(read_off.data(), b->read_off, (size_t)(nl + 1) * 4));
    HIP_TRY(d2h(motif_off.data(), b->motif_off, (size_t)(nl + 1) * 4));
    HIP_TRY(d2h(next_read.data(), rp.next_read, (size_t)nl * 4));
    HIP_TRY(d2h(need_lo.data(), rp.need_lo, (size_t)nl * 4));
    HIP_TRY(d2h(need_hi.data(), rp.need_hi, (size_t)nl * 4));
    HIP_TRY(d2h(frac.data(), rp.frac, (size_t)nl * 8));
    HIP_TRY(hipStreamSynchronize(st));

    // Few loci with misses (the usual case): fetch only their slices.  Many (noisy reads whose banded tables cannot
    // be certified from a different start): one bulk copy per array is cheaper than thirteen small ones per locus.
    int n_pending = 0;
    for (int l = 0; l < nl; ++l) n_pending += next_read[l] < read_off[l + 1];
    const bool bulk = n_pending > std::max(24, nl / 64);   // (the bulk copy includes the whole score table: never for a handful of a big batch)
    const size_t nr = (size_t)b->n_reads;
    std::vector<int32_t> m_est, m_win_lo, m_win_n, m_rep, m_nfl, m_ntr, m_nfr, m_cn, m_score, m_n, m_start, m_table;
    std::vector<int64_t> m_tab_off;
    std::vector<uint8_t> m_exact;
    if (bulk) {
        auto all32 = [&](std::vector<int32_t>& v, const int32_t* src, size_t cnt) {
            v.resize(cnt);
            return d2h(v.data(), src, cnt * 4);
        };
        HIP_TRY(all32(m_est, b->est_cn, nr));
        HIP_TRY(all32(m_win_lo, a.win_lo, nr));
        HIP_TRY(all32(m_win_n, a.win_n, nr));
        HIP_TRY(all32(m_rep, a.rep, nr));
        HIP_TRY(all32(m_nfl, b->nfl, nr));
        HIP_TRY(all32(m_ntr, b->ntr, nr));
        HIP_TRY(all32(m_nfr, b->nfr, nr));
        HIP_TRY(all32(m_cn, rp.out_cn, nr));
        HIP_TRY(all32(m_score, rp.out_score, nr));
        HIP_TRY(all32(m_n, rp.out_n, nr));
        HIP_TRY(all32(m_start, rp.out_start, nr));
        HIP_TRY(all32(m_table, a.table, nr * ts));
        m_tab_off.resize(nr);
        HIP_TRY(d2h(m_tab_off.data(), a.tab_off, nr * 8));
        if (a.band_mode) {
            m_exact.resize(nr);
            HIP_TRY(d2h(m_exact.data(), a.exact, nr));
        }
        HIP_TRY(hipStreamSynchronize(st));
    }
    // an eighth of the call's loci pending: not stragglers but a sample whose windows are too small for it (noisy reads of long
    // short-motif tracts) — their loci take the reads behind the one that missed along from the first round on (see below)
    const bool many_pending = (size_t)n_pending * 8 > (size_t)nl;
    std::vector<MissLocus> loci;
    loci.reserve((size_t)n_pending);
    for (int l = 0; l < nl; ++l) {
        if (next_read[l] >= read_off[l + 1]) continue;
        MissLocus L;
        L.l = l; L.r0 = read_off[l]; L.r1 = read_off[l + 1]; L.m = motif_off[l + 1] - motif_off[l];
        L.first = next_read[l]; L.frac = frac[l]; L.need_lo = need_lo[l]; L.need_hi = need_hi[l];
        const size_t n = (size_t)(L.r1 - L.r0);
        auto get32 = [&](std::vector<int32_t>& v, const int32_t* src, const std::vector<int32_t>& mirror) {
            if (bulk) {
                v.assign(mirror.begin() + L.r0, mirror.begin() + L.r1);
                return hipSuccess;
            }
            v.resize(n);
            return d2h(v.data(), src + L.r0, n * 4);
        };
        HIP_TRY(get32(L.est, b->est_cn, m_est));
        HIP_TRY(get32(L.win_lo, a.win_lo, m_win_lo));
        HIP_TRY(get32(L.win_n, a.win_n, m_win_n));
        HIP_TRY(get32(L.rep, a.rep, m_rep));
        HIP_TRY(get32(L.nfl, b->nfl, m_nfl));
        HIP_TRY(get32(L.ntr, b->ntr, m_ntr));
        HIP_TRY(get32(L.nfr, b->nfr, m_nfr));
        HIP_TRY(get32(L.o_cn, rp.out_cn, m_cn));
        HIP_TRY(get32(L.o_score, rp.out_score, m_score));
        HIP_TRY(get32(L.o_n, rp.out_n, m_n));
        HIP_TRY(get32(L.o_start, rp.out_start, m_start));
        L.exact.assign(n, 1);
        // copies of a read share the table slot of their first occurrence, which lies in the same locus
        if (bulk) {
            L.tab_off.assign(m_tab_off.begin() + L.r0, m_tab_off.begin() + L.r1);
            if (a.band_mode) L.exact.assign(m_exact.begin() + L.r0, m_exact.begin() + L.r1);
            L.table.assign(m_table.begin() + (size_t)L.r0 * ts, m_table.begin() + (size_t)L.r1 * ts);
        } else {
            L.tab_off.resize(n);
            HIP_TRY(d2h(L.tab_off.data(), a.tab_off + L.r0, n * 8));
            if (a.band_mode) HIP_TRY(d2h(L.exact.data(), a.exact + L.r0, n));
            L.table.resize(n * ts);
            HIP_TRY(d2h(L.table.data(), a.table + (size_t)L.r0 * ts, n * ts * 4));
        }
        L.ext.resize(n);
        L.ext_lo.assign(n, 0);
        L.tries.assign(n, 0);
        L.rounds = many_pending ? 1 : 0;
        loci.push_back(std::move(L));   // (the vectors' buffers move with them: the copies in flight still land where they should)
    }
    HIP_TRY(hipStreamSynchronize(st));

    std::vector<MissLocus*> pending;
    for (auto& L : loci) pending.push_back(&L);
    int rounds = 0, miss_reads = 0, rc;
    if ((rc = c->win_lo2.ensure((size_t)b->n_reads * 4))) return rc;
    if ((rc = c->win_n2.ensure((size_t)b->n_reads * 4))) return rc;
    if ((rc = c->tab_off2.ensure((size_t)b->n_reads * 8))) return rc;
    while (!pending.empty()) {
        if (++rounds > 4096) return fail(STRK_E_DEVICE, "window-miss resolution did not converge");
        // 1. windows wanted this round: the read that missed of every pending locus — and, from a locus's second round on, the
        //    reads behind it too, widened as often as the one that missed has been.  The reads of a locus are searched in order
        //    (the start of each depends on the results before it), so a locus whose reads mostly leave their windows — long
        //    homopolymer or dinucleotide tracts of noisy reads: the estimate is off by dozens of copies — went through one round
        //    per read, each as long as the DP of one 12 kb window on one wave: 50 rounds, 0.35 s for 250 loci x 40 reads
        //    (tools/long_probe.py) while the chip idled.  One miss in a locus stays a single-read round (HiFi: the usual case).
        std::vector<int32_t> items, w_lo, w_n;
        std::vector<int64_t> w_off;
        std::vector<MissLocus*> it_L;
        std::vector<int> it_k;
        size_t tab2 = 0, n_chunks = 0;
        int bad_window = 0;
        auto want = [&](MissLocus* L, int k, int64_t need_lo, int64_t need_hi, int widenings) {
            const bool has_ext = !L->ext[k].empty();
            const int64_t cur_lo = has_ext ? L->ext_lo[k] : L->win_lo[k];
            const int64_t cur_hi = cur_lo + (has_ext ? (int64_t)L->ext[k].size() : L->win_n[k]) - 1;
            // the margin doubles with every widening of a read (a start far from the tract's size walks dozens of steps: one
            // round per one or two of them, each re-scoring the whole table so far, took minutes for a batch of wild estimates —
            // tools/fuzz_parity.py); a candidate more is one fork row and |motif| prefix rows
            int64_t margin = 0;
            for (int t = 0; t < widenings; ++t) {
                margin += (int64_t)p.window << std::min<int>(L->tries[k], 5);
                if (L->tries[k] < 255) ++L->tries[k];
            }
            const int64_t lo2 = std::min<int64_t>(cur_lo, std::max<int64_t>(0, need_lo - margin));
            const int64_t hi2 = std::max<int64_t>(cur_hi, need_hi + margin);
            if (hi2 - lo2 + 1 > (int64_t)1 << 20) { bad_window = 1; return; }
            items.push_back(L->r0 + k);
            w_lo.push_back((int32_t)lo2);
            w_n.push_back((int32_t)(hi2 - lo2 + 1));
            w_off.push_back((int64_t)tab2);
            it_L.push_back(L);
            it_k.push_back(k);
            tab2 += (size_t)(hi2 - lo2 + 1);
            n_chunks += ((size_t)(hi2 - lo2 + 1) + kTableMax - 1) / kTableMax;
        };
        for (MissLocus* L : pending) {
            const int k = L->first - L->r0;
            want(L, k, L->need_lo, L->need_hi, 1);
            ++miss_reads;
            if (L->rounds >= 1) {
                const int target = std::min<int>(L->tries[k], 6);   // (the margin stops doubling there: no more joint widenings)
                for (int k2 = k + 1; k2 < L->r1 - L->r0; ++k2) {
                    if (L->tries[k2] >= target) continue;
                    const bool has_ext = !L->ext[k2].empty();
                    const int64_t cur_lo = has_ext ? L->ext_lo[k2] : L->win_lo[k2];
                    const int64_t cur_hi = cur_lo + (has_ext ? (int64_t)L->ext[k2].size() : L->win_n[k2]) - 1;
                    want(L, k2, cur_lo, cur_hi, target - L->tries[k2]);
                }
            }
            ++L->rounds;
        }
        if (bad_window) return fail(STRK_E_INVALID, "candidate window grew past 2^20 sizes");
        // 2. score them exactly on the device (per-read window arrays are patched entry by entry)
        if ((rc = c->table2.ensure(tab2 * 4))) return rc;
        if ((rc = c->items.ensure(items.size() * 4))) return rc;
        if ((rc = c->cls_list.ensure((size_t)kNumLists * n_chunks * 2 * 4))) return rc;
        std::vector<int32_t> f_lo, f_n;   // full-size images when many reads are re-scored (must outlive the copies)
        std::vector<int64_t> f_off;
        if (items.size() > 48) {
            f_lo.assign(nr, 0);
            f_n.assign(nr, 0);
            f_off.assign(nr, 0);
            for (size_t i = 0; i < items.size(); ++i) {
                const size_t r = (size_t)items[i];
                f_lo[r] = w_lo[i];
                f_n[r] = w_n[i];
                f_off[r] = w_off[i];
            }
            HIP_TRY(hipMemcpyAsync(c->win_lo2.p, f_lo.data(), nr * 4, hipMemcpyHostToDevice, st));
            HIP_TRY(hipMemcpyAsync(c->win_n2.p, f_n.data(), nr * 4, hipMemcpyHostToDevice, st));
            HIP_TRY(hipMemcpyAsync(c->tab_off2.p, f_off.data(), nr * 8, hipMemcpyHostToDevice, st));
        } else {
            for (size_t i = 0; i < items.size(); ++i) {
                const size_t r = (size_t)items[i];
                HIP_TRY(hipMemcpyAsync(c->win_lo2.as<int32_t>() + r, &w_lo[i], 4, hipMemcpyHostToDevice, st));
                HIP_TRY(hipMemcpyAsync(c->win_n2.as<int32_t>() + r, &w_n[i], 4, hipMemcpyHostToDevice, st));
                HIP_TRY(hipMemcpyAsync(c->tab_off2.as<int64_t>() + r, &w_off[i], 8, hipMemcpyHostToDevice, st));
            }
        }
        HIP_TRY(hipMemcpyAsync(c->items.p, items.data(), items.size() * 4, hipMemcpyHostToDevice, st));
        KArgs a2 = a;
        a2.win_lo = c->win_lo2.as<int32_t>();
        a2.win_n = c->win_n2.as<int32_t>();
        a2.tab_off = c->tab_off2.as<int64_t>();
        a2.table = c->table2.as<int32_t>();
        a2.cls_list = c->cls_list.as<int32_t>();
        a2.list_stride = (int32_t)n_chunks;
        a2.spec = nullptr;
        a2.band_mode = 0;   // window-miss rounds always score exactly
        a2.exact = nullptr;
        std::vector<int32_t> t2(tab2);
        // (widened windows: hundreds of generic-kernel rows each, or a start far above the tract — the scratch may have to grow)
        if ((rc = score_until_scratch_fits(c, a2, c->items.as<int32_t>(), (int)items.size(), 0, st, false, &a, t2.data(), c->table2.p, tab2 * 4)))
            return rc;
        if ((rc = check_error_bits(c->h_counters.cnt(kCntError) & ~kErrEmpty))) return rc;
        if (stats) {
            stats->n_fallback += c->h_counters.cnt(kCntClass0 + kGenericClass);
            stats->dp_cells += (int64_t)c->h_counters.cells();
        }
        for (size_t i = 0; i < items.size(); ++i) {
            MissLocus* L = it_L[i];
            const int k = it_k[i];
            L->ext_lo[k] = w_lo[i];
            L->ext[k].assign(t2.begin() + w_off[i], t2.begin() + w_off[i] + w_n[i]);
        }
        // 3. replay the pending loci on the host until the next miss
        std::vector<MissLocus*> still;
        for (MissLocus* L : pending) {
            int r = L->first;
            double fr = L->frac;
            bool missed = false;
            for (; r < L->r1; ++r) {
                const int k = r - L->r0;
                int start = L->est[k];
                double fr_try = fr;
                if (p.feedback) start = feedback_start(L->est[k], &fr_try);
                const bool use_ext = !L->ext[k].empty();
                const int32_t* sc = use_ext ? L->ext[k].data() : L->table.data() + (L->tab_off[k] - (int64_t)L->r0 * ts);
                const int32_t lo = use_ext ? L->ext_lo[k] : L->win_lo[k];
                const int32_t n = use_ext ? (int32_t)L->ext[k].size() : L->win_n[k];
                SeenVec seen;
                seen.v.assign((size_t)std::max(n, 1), 0);
                SearchResult res;
                const int rpk = L->rep[k] - L->r0;   // first occurrence of this read's bytes (same locus)
                if (use_ext || !a.band_mode || L->exact[rpk]) {
                    res = search_replay(start, p.step_size, p.local_search_range, p.max_iters, p.tie_rule == STRK_TIE_LAST, sc,
                                        lo, n, seen, p.narrowing);
                } else {   // banded table of the device pass: same certified search as k_replay
                    const BandGeo geo = band_geometry(L->nfl[rpk], L->ntr[rpk], L->nfr[rpk], L->m, lo, n, a.band_tune);
                    auto ub = [&](int kk) { return band_ub(geo, L->nfl[rpk], L->ntr[rpk], L->nfr[rpk], L->m, lo + kk, p.end_flags); };
                    const CertResult cr = search_replay_cert(start, p.step_size, p.local_search_range, p.max_iters,
                                                             p.tie_rule == STRK_TIE_LAST, sc, lo, n, seen, ub, p.narrowing);
                    res = cr.res;
                    if (cr.uncertain) { res.miss = 1; res.need_lo = lo; res.need_hi = lo + n - 1; }
                }
                if (res.miss) {
                    L->need_lo = res.need_lo;
                    L->need_hi = res.need_hi;
                    missed = true;
                    break;
                }
                fr = fr_try;
                L->o_start[k] = start;
                L->o_n[k] = res.n_explored;
                if (res.empty) {
                    L->o_cn[k] = 0; L->o_score[k] = 0;
                    err_bits |= kErrEmpty;
                    continue;
                }
                L->o_cn[k] = res.cn;
                L->o_score[k] = res.score;
                if (p.feedback) feedback_update(&fr, res.cn, start);
            }
            L->first = r;
            L->frac = fr;
            if (missed) still.push_back(L);
        }
        pending.swap(still);
    }
    if (bulk) {   // write back through the full-size images
        for (auto& L : loci) {
            std::copy(L.o_cn.begin(), L.o_cn.end(), m_cn.begin() + L.r0);
            std::copy(L.o_score.begin(), L.o_score.end(), m_score.begin() + L.r0);
            std::copy(L.o_n.begin(), L.o_n.end(), m_n.begin() + L.r0);
            std::copy(L.o_start.begin(), L.o_start.end(), m_start.begin() + L.r0);
        }
        HIP_TRY(hipMemcpyAsync(rp.out_cn, m_cn.data(), nr * 4, hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(rp.out_score, m_score.data(), nr * 4, hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(rp.out_n, m_n.data(), nr * 4, hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(rp.out_start, m_start.data(), nr * 4, hipMemcpyHostToDevice, st));
    } else {
        for (auto& L : loci) {   // write back the reads the host finished
            const size_t n = (size_t)(L.r1 - L.r0);
            HIP_TRY(hipMemcpyAsync(rp.out_cn + L.r0, L.o_cn.data(), n * 4, hipMemcpyHostToDevice, st));
            HIP_TRY(hipMemcpyAsync(rp.out_score + L.r0, L.o_score.data(), n * 4, hipMemcpyHostToDevice, st));
            HIP_TRY(hipMemcpyAsync(rp.out_n + L.r0, L.o_n.data(), n * 4, hipMemcpyHostToDevice, st));
            HIP_TRY(hipMemcpyAsync(rp.out_start + L.r0, L.o_start.data(), n * 4, hipMemcpyHostToDevice, st));
        }
    }
    HIP_TRY(hipStreamSynchronize(st));
    if (stats) {
        stats->n_miss_reads = miss_reads;
        stats->n_miss_rounds = rounds;
    }
    return check_error_bits(err_bits);
}

