// Pipelined host-buffer entry point: count_loci_pipelined() behind strk_count_loci.
// Part of strk_api.hip: included inside its anonymous namespace (uses the owning types of strk_host.h, strk_ctx, check_batch_range,
// submit_device / finish_device defined there); not a stand-alone header.
//
// What it replaces: upload of the whole batch from pageable memory, compute, four blocking downloads — one after the other
// (65 M reads/s on the bench workload while the device-resident path ran at 216 M).  The reference's worker loop hands one
// block of loci after the other to the counter (strkit/call/call_sample.py:103-138; call_locus.py:1148-1155 per read), so a
// batch is cut into sub-batches of whole loci (loci are independent: the start-count feedback stays inside a locus) that
// travel through four upload slots and two compute contexts:
//
//   host threads   copy the sub-batch's slices of the caller's arrays into ONE pinned block (offsets rebased)   [CPU]
//   slot stream    one H2D copy of that block -> the batched call on the slot's own context -> one D2H copy    [PCIe / GPU]
//                  of the four result arrays into a pinned block
//   calling thread scatters the results into the caller's arrays, adds the statistics up                       [CPU]
//
// so that staging of sub-batch k + 2, the transfer of k + 1 and the kernels of k overlap.  The bases are addressed through
// the caller's own seq_off values: the device pointer handed to the kernels is (block + offset of the bases - seq_off[first
// read]), so the int64 offsets need no rebasing pass.

constexpr int kPipeDefaultMB = 24;   // sub-batch size of the host pipeline (STRKIT_AMD_PIPE_MB)

size_t pipe_sub_bytes() {
    const char* e = getenv("STRKIT_AMD_PIPE_MB");
    return (size_t)std::max(1, e ? atoi(e) : kPipeDefaultMB) << 20;
}

struct CopyPool {
    struct Piece { uint8_t* dst; const uint8_t* src; size_t n; };
    std::vector<std::thread> threads;
    std::mutex mu;
    std::condition_variable cv_go, cv_done;
    std::vector<Piece> pieces;
    std::atomic<size_t> next{0};
    uint64_t generation = 0;
    int busy = 0;
    bool stop = false;

    explicit CopyPool(int n_threads) {
        for (int i = 0; i < n_threads; ++i) threads.emplace_back([this] { worker(); });
    }
    ~CopyPool() {
        {
            std::lock_guard<std::mutex> lk(mu);
            stop = true;
        }
        cv_go.notify_all();
        for (auto& t : threads) t.join();
    }
    void drain() {
        for (;;) {
            const size_t i = next.fetch_add(1, std::memory_order_relaxed);
            if (i >= pieces.size()) return;
            memcpy(pieces[i].dst, pieces[i].src, pieces[i].n);
        }
    }
    void worker() {
        uint64_t seen = 0;
        for (;;) {
            {
                std::unique_lock<std::mutex> lk(mu);
                cv_go.wait(lk, [&] { return stop || generation != seen; });
                if (stop) return;
                seen = generation;
            }
            drain();
            {
                std::lock_guard<std::mutex> lk(mu);
                if (--busy == 0) cv_done.notify_all();
            }
        }
    }
    // copies every piece; the calling thread takes part; returns when all are done
    void run(std::vector<Piece>&& p) {
        if (threads.empty() || p.size() < 2) {
            for (const auto& q : p) memcpy(q.dst, q.src, q.n);
            return;
        }
        {
            std::lock_guard<std::mutex> lk(mu);
            pieces = std::move(p);
            next.store(0, std::memory_order_relaxed);
            busy = (int)threads.size();
            ++generation;
        }
        cv_go.notify_all();
        drain();
        std::unique_lock<std::mutex> lk(mu);
        cv_done.wait(lk, [&] { return busy == 0; });
    }
};

struct HostPipe {
    // Upload slots and compute contexts are separate: up to kSlots sub-batches are staged / on their way over PCIe while at most
    // kCtx batched calls run on the device.  (Three calls in flight form a convoy: the small LDS-heavy kernels behind one call's
    // band pass wait for the persistent band blocks of the other two — profiles/README.md round 3 — so two it is.)
    static constexpr int kSlots = 4, kCtx = 2;
    enum State { kFree = 0, kUploaded, kComputing };
    // (members are destroyed last to first: the compute contexts, the slots, the copy stream, the copy threads)
    size_t sub_bytes = 0;
    std::unique_ptr<CopyPool> pool;
    Stream copy_st;
    struct Slot {
        PinnedBuf h_in, h_out;   // the staged sub-batch; its four result arrays
        DevBuf d_in, d_out;
        Event ev_h2d;
        State state = kFree;
        int ctx = -1;            // compute context while kComputing
        int seq = 0;             // submission order
        int r0 = 0, nr = 0;
        strk_batch db;           // device view of the sub-batch
    } slot[kSlots];
    struct Ctx {
        strk_ctx* sub = nullptr;
        Stream st;
        bool busy = false;
        ~Ctx() { strk_destroy(sub); }
    } ctx[kCtx];
};

int pipe_get(strk_ctx* c, HostPipe** out) {
    if (c->pipe) { *out = c->pipe; return 0; }
    std::unique_ptr<HostPipe> p(new HostPipe());
    p->sub_bytes = pipe_sub_bytes();
    const char* t = getenv("STRKIT_AMD_COPY_THREADS");
    p->pool.reset(new CopyPool(std::max(0, std::min(15, t ? atoi(t) : std::min(7, host_cpus() - 1)))));
    bool ok = hipStreamCreateWithFlags(&p->copy_st.h, hipStreamNonBlocking) == hipSuccess;
    for (auto& x : p->ctx) {
        if (!ok) break;
        const int rc = strk_init(c->device, &x.sub);
        if (rc) return rc;
        ok = hipStreamCreateWithFlags(&x.st.h, hipStreamNonBlocking) == hipSuccess;
    }
    for (auto& s : p->slot)
        if (ok) ok = hipEventCreateWithFlags(&s.ev_h2d.h, hipEventDisableTiming) == hipSuccess;
    if (!ok) return fail(STRK_E_DEVICE, "host pipeline: stream / event creation failed");
    c->pipe = *out = p.release();
    return 0;
}

inline size_t up16(size_t x) { return (x + 15) & ~(size_t)15; }

// Is [ptr, ptr + bytes) page-locked host memory the DMA engines can read in place (hipHostMalloc / hipHostRegister,
// strk_host_register)?  Pageable memory answers with an error or "unregistered", depending on the runtime.
bool host_range_pinned(const void* ptr, size_t bytes) {
    if (!ptr || bytes == 0) return false;
    hipPointerAttribute_t at;
    for (const uint8_t* q : {static_cast<const uint8_t*>(ptr), static_cast<const uint8_t*>(ptr) + bytes - 1}) {
        if (hipPointerGetAttributes(&at, q) != hipSuccess) { (void)hipGetLastError(); return false; }
        if (at.type != hipMemoryTypeHost) return false;
    }
    return true;
}

// Validates loci [l0, l1) of the host batch (check_batch_range), stages them into the slot's pinned block and
// enqueues its upload on the copy stream.
int pipe_upload(HostPipe* p, HostPipe::Slot& s, const strk_batch* b, int l0, int l1, bool direct) {
    const int r0 = b->read_off[l0], r1 = b->read_off[l1];
    const size_t nr = (size_t)(r1 - r0), nl = (size_t)(l1 - l0);
    int rc;
    if ((rc = check_batch_range(b, (size_t)l0, (size_t)l1))) return rc;
    const int64_t s0 = b->seq_off[r0], s1 = b->seq_off[r1];
    const int32_t m0 = b->motif_off[l0], m1 = b->motif_off[l1];
    const size_t nbases = (size_t)(s1 - s0), nmot = (size_t)(m1 - m0);
    // block layout (every part on a 16-byte boundary)
    const size_t o_seq_off = 0;
    const size_t o_nfl = o_seq_off + up16((nr + 1) * 8);
    const size_t o_ntr = o_nfl + up16(nr * 4), o_nfr = o_ntr + up16(nr * 4), o_est = o_nfr + up16(nr * 4);
    const size_t o_read_off = o_est + up16(nr * 4);
    const size_t o_motif_off = o_read_off + up16((nl + 1) * 4);
    const size_t o_motifs = o_motif_off + up16((nl + 1) * 4);
    const size_t o_seqs = o_motifs + up16(nmot + 1);
    const size_t total = o_seqs + up16(nbases + 16);
    if ((rc = s.h_in.ensure(total))) return rc;
    if ((rc = s.d_in.ensure(total))) return rc;
    if ((rc = s.d_out.ensure(std::max<size_t>(nr, 1) * 16))) return rc;
    if ((rc = s.h_out.ensure(std::max<size_t>(nr, 1) * 16))) return rc;
    uint8_t* const h_in = s.h_in.as<uint8_t>();
    {
        std::vector<CopyPool::Piece> pieces;
        auto add = [&](size_t off, const void* src, size_t n) {
            const uint8_t* sp = static_cast<const uint8_t*>(src);
            constexpr size_t kPiece = (size_t)512 << 10;
            for (size_t k = 0; k < n; k += kPiece) pieces.push_back({h_in + off + k, sp + k, std::min(kPiece, n - k)});
        };
        add(o_seq_off, b->seq_off + r0, (nr + 1) * 8);
        add(o_nfl, b->nfl + r0, nr * 4);
        add(o_ntr, b->ntr + r0, nr * 4);
        add(o_nfr, b->nfr + r0, nr * 4);
        add(o_est, b->est_cn + r0, nr * 4);
        add(o_motifs, b->motifs + m0, nmot);
        if (!direct) add(o_seqs, b->seqs + s0, nbases);
        int32_t* ro = reinterpret_cast<int32_t*>(h_in + o_read_off);
        int32_t* mo = reinterpret_cast<int32_t*>(h_in + o_motif_off);
        for (size_t k = 0; k <= nl; ++k) {
            ro[k] = b->read_off[l0 + k] - r0;
            mo[k] = b->motif_off[l0 + k] - m0;
        }
        p->pool->run(std::move(pieces));
    }
    uint8_t* d = s.d_in.as<uint8_t>();
    if (direct) {
        // the caller's bases are page-locked: DMA from where they lie (93 % of the bytes); the per-read arrays and the rebased
        // offsets (24 bytes per read) travel in the slot's block as before — two copies per sub-batch, not seven
        HIP_TRY(hipMemcpyAsync(d, h_in, o_seqs, hipMemcpyHostToDevice, p->copy_st));
        if (nbases) HIP_TRY(hipMemcpyAsync(d + o_seqs, b->seqs + s0, nbases, hipMemcpyHostToDevice, p->copy_st));
    } else {
        HIP_TRY(hipMemcpyAsync(s.d_in.p, h_in, total, hipMemcpyHostToDevice, p->copy_st));
    }
    HIP_TRY(hipEventRecord(s.ev_h2d, p->copy_st));
    strk_batch& db = s.db;
    db.n_reads = (int32_t)nr;
    db.n_loci = (int32_t)nl;
    db.seq_off = reinterpret_cast<const int64_t*>(d + o_seq_off);
    db.nfl = reinterpret_cast<const int32_t*>(d + o_nfl);
    db.ntr = reinterpret_cast<const int32_t*>(d + o_ntr);
    db.nfr = reinterpret_cast<const int32_t*>(d + o_nfr);
    db.est_cn = reinterpret_cast<const int32_t*>(d + o_est);
    db.read_off = reinterpret_cast<const int32_t*>(d + o_read_off);
    db.motif_off = reinterpret_cast<const int32_t*>(d + o_motif_off);
    db.motifs = d + o_motifs;
    db.seqs = d + o_seqs - s0;   // the kernels add the caller's own seq_off values
    s.state = HostPipe::kUploaded;
    s.r0 = r0;
    s.nr = (int)nr;
    return 0;
}

// The batched call of an uploaded sub-batch on a free compute context (behind its upload).
int pipe_compute(HostPipe* p, HostPipe::Slot& s, int k, const strk_params* params) {
    HostPipe::Ctx& c = p->ctx[k];
    HIP_TRY(hipStreamWaitEvent(c.st, s.ev_h2d, 0));
    int32_t* o = s.d_out.as<int32_t>();
    const size_t st_ = std::max<size_t>((size_t)s.nr, 1);
    const int rc = submit_device(c.sub, &s.db, params, o, o + st_, o + 2 * st_, o + 3 * st_, c.st);
    if (rc) return rc;
    s.state = HostPipe::kComputing;
    s.ctx = k;
    c.busy = true;
    return 0;
}

// Waits for the slot's sub-batch, resolves its window misses, brings the results home.
int pipe_complete(HostPipe* p, HostPipe::Slot& s, int32_t* out_cn, int32_t* out_score, int32_t* out_n, int32_t* out_start, strk_stats* agg) {
    HostPipe::Ctx& c = p->ctx[s.ctx];
    s.state = HostPipe::kFree;
    c.busy = false;
    strk_stats st;
    int rc = finish_device(c.sub, &st);
    if (rc && rc != STRK_E_EMPTY) return rc;
    const size_t nr = (size_t)s.nr, stride = std::max<size_t>(nr, 1);
    if (nr) {
        const int32_t* h_out = s.h_out.as<int32_t>();
        HIP_TRY(hipMemcpyAsync(s.h_out.p, s.d_out.p, stride * 16, hipMemcpyDeviceToHost, c.st));
        HIP_TRY(hipStreamSynchronize(c.st));
        if (out_cn) memcpy(out_cn + s.r0, h_out, nr * 4);
        if (out_score) memcpy(out_score + s.r0, h_out + stride, nr * 4);
        if (out_n) memcpy(out_n + s.r0, h_out + 2 * stride, nr * 4);
        if (out_start) memcpy(out_start + s.r0, h_out + 3 * stride, nr * 4);
    }
    if (agg) {
        agg->dp_cells += st.dp_cells; agg->n_fallback += st.n_fallback; agg->n_miss_reads += st.n_miss_reads;
        agg->n_miss_rounds += st.n_miss_rounds; agg->kernel_ms += st.kernel_ms; agg->dp_kernel_ms += st.dp_kernel_ms;
        agg->n_dp_launches += st.n_dp_launches; agg->n_dedup_reads += st.n_dedup_reads; agg->n_band_reads += st.n_band_reads;
        agg->n_band_fallback += st.n_band_fallback; agg->band_kernel_ms += st.band_kernel_ms; agg->window_used = st.window_used;
        agg->band_bytes += st.band_bytes; agg->exact_bytes += st.exact_bytes; agg->band_wide_kernel_ms += st.band_wide_kernel_ms;
        agg->long_kernel_ms += st.long_kernel_ms; agg->generic_kernel_ms += st.generic_kernel_ms; agg->head_ms += st.head_ms;
        agg->replay_ms += st.replay_ms; agg->n_long_reads += st.n_long_reads; agg->wide_bytes += st.wide_bytes;
        agg->long_bytes += st.long_bytes;
        agg->band_cells += st.band_cells; agg->wide_cells += st.wide_cells; agg->exact_cells += st.exact_cells; agg->long_cells += st.long_cells;
        for (int k = 0; k < kWinBuckets; ++k)
            if (st.window_bucket[k]) agg->window_bucket[k] = st.window_bucket[k];
    }
    return rc;
}

// strk_count_loci on host buffers, pipelined.  *taken = false: the batch is too small to be worth cutting up (or malformed in a
// way the direct path reports) and the caller takes the direct path; else the call's return code (0 / STRK_E_EMPTY / an error).
int count_loci_pipelined(strk_ctx* c, const strk_batch* b, const strk_params* params, int32_t* out_cn, int32_t* out_score,
                         int32_t* out_n, int32_t* out_start, strk_stats* stats, bool* taken) {
    *taken = false;
    if (!b || b->n_reads <= 0 || b->n_loci <= 0 || !b->seq_off || !b->read_off || !b->nfl || !b->ntr || !b->nfr || !b->motifs ||
        !b->motif_off || !b->seqs || !b->est_cn)
        return 0;   // the direct path reports what is wrong with such a batch
    if (b->read_off[0] != 0 || b->read_off[b->n_loci] != b->n_reads) return 0;
    // the cutting loop below indexes seq_off / nfl / ... with read_off[l] of loci beyond the sub-batch being validated: one pass
    // over the offsets first (a violation: the direct path reports it as STRK_E_INVALID)
    // (non-decreasing from read_off[0] = 0 to read_off[n_loci] = n_reads: every one of them is a read of the batch)
    if (check_batch_loci(b, 0, (size_t)b->n_loci)) return 0;
    const int64_t total_bytes = b->seq_off[b->n_reads] - b->seq_off[0] + (int64_t)b->n_reads * 24;
    // (the decision needs the sub-batch size, which lives in the pipe: cheap to read before the pipe exists)
    if (total_bytes < (int64_t)(pipe_sub_bytes() / 2)) return 0;
    HostPipe* p = nullptr;
    int rc;
    if ((rc = pipe_get(c, &p))) { *taken = true; return rc; }
    *taken = true;
    HIP_TRY(hipSetDevice(c->device));
    if (stats) memset(stats, 0, sizeof *stats);
    const int nl = b->n_loci;
    // page-locked bases (strk_host_register / hipHostMalloc) are read by DMA where they lie
    const bool direct = host_range_pinned(b->seqs + b->seq_off[0], (size_t)(b->seq_off[b->n_reads] - b->seq_off[0]));
    int next_l = 0, n_sub = 0, rc_keep = 0, err = 0;
    std::string err_msg, empty_msg;
    auto note = [&](int r) {
        if (r == STRK_E_EMPTY) { rc_keep = r; empty_msg = g_err; }
        else if (r && !err) { err = r; err_msg = g_err; }
    };
    auto oldest = [&](HostPipe::State st) {
        int best = -1;
        for (int k = 0; k < HostPipe::kSlots; ++k)
            if (p->slot[k].state == st && (best < 0 || p->slot[k].seq < p->slot[best].seq)) best = k;
        return best;
    };
    for (;;) {
        int k_up = oldest(HostPipe::kUploaded), k_ctx = -1, k_free = oldest(HostPipe::kFree);
        for (int k = 0; k < HostPipe::kCtx && k_ctx < 0; ++k)
            if (!p->ctx[k].busy) k_ctx = k;
        // (At most two sub-batches computing on the device process-wide unless this pipeline has none of its own there: with
        // three or four calls in flight the device falls into the convoy of DESIGN.md section 3 — 190 M reads/s against 240 M —
        // which is what two callers with a pipeline each ran into, round 3: 88 M together against 112 M for one.)
        int own_computing = 0;
        for (int k = 0; k < HostPipe::kSlots; ++k) own_computing += p->slot[k].state == HostPipe::kComputing;
        const bool device_has_room = own_computing == 0 || g_calls_in_flight.load(std::memory_order_relaxed) < 2;
        if (k_up >= 0 && k_ctx >= 0 && !err && device_has_room) {   // 1. an uploaded sub-batch and a free context: compute
            rc = pipe_compute(p, p->slot[k_up], k_ctx, params);
            if (rc) { note(rc); p->slot[k_up].state = HostPipe::kFree; }
            continue;
        }
        if (next_l < nl && k_free >= 0 && !err) {                 // 2. a free slot: stage and upload the next sub-batch
            // whole loci up to ~sub_bytes; the first three are an eighth, a quarter and half of that, so that the device starts
            // early (a call's kernels are the more efficient the more reads it holds: few large sub-batches, not many small)
            // (Halving the last sub-batches too, so that little is left to compute behind the last upload, was measured: nine
            // sub-batches instead of six, and every sub-batch costs the calling thread ~0.13 ms of submission: 99 -> 89 M reads/s.)
            // (Also measured: the calling thread starting calls / fetching results between its pieces of a staging copy instead of
            // only copying — 81-90 against 92-100 M reads/s pageable: its share of the copy is worth more than the earlier starts.)
            // (Also measured: one small sub-batch first, full ones in the middle, two small ones last — the same count of six:
            // 99.7 against 109.6 M reads/s with page-locked bases, 88 against 84 M pageable; the ramp stays.)
            const size_t budget = p->sub_bytes >> (n_sub < 3 ? 3 - n_sub : 0);
            int l1 = next_l;
            const int64_t base_bytes = b->seq_off[b->read_off[next_l]];
            const int base_reads = b->read_off[next_l];
            while (l1 < nl) {
                ++l1;
                const int64_t bytes = b->seq_off[b->read_off[l1]] - base_bytes + (int64_t)(b->read_off[l1] - base_reads) * 24;
                if ((size_t)bytes >= budget) break;
            }
            rc = pipe_upload(p, p->slot[k_free], b, next_l, l1, direct);
            if (rc) { note(rc); continue; }
            p->slot[k_free].seq = n_sub++;
            next_l = l1;
            continue;
        }
        const int k_done = oldest(HostPipe::kComputing);           // 3. nothing to start: finish the oldest call in flight
        if (k_done >= 0) {
            note(pipe_complete(p, p->slot[k_done], out_cn, out_score, out_n, out_start, stats));
            continue;
        }
        if (err) {   // uploads that will not be computed any more
            (void)hipStreamSynchronize(p->copy_st);
            for (auto& s : p->slot) s.state = HostPipe::kFree;
        }
        break;
    }
    if (err) { g_err = err_msg; return err; }
    if (stats) stats->n_sub_batches = n_sub;   // (n_dp_launches keeps its meaning: DP launch rounds, summed over the sub-batches)
    if (rc_keep) g_err = empty_msg;
    return rc_keep;
}
