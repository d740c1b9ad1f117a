// strk_replay.h — k_replay: search replay per locus — a lane per read, the start-count feedback serial only at its events
// Part of strk_kernels.h: included at its end, after the shared definitions (KArgs, counters, k_hash, k_plan).
#pragma once

namespace strk {

// ---------------------------------------------------------------------------------------------
// Search replay: one wave per locus takes its reads in caller order (call_locus.py:1082) with the
// start-count feedback (call_locus.py:1129-1136,1161) and replays the hill climb on the table.
//
// Three steps per locus (strk_search.h, "The walk over the reads of a locus"):
//   1. Pass 1, band calls: every first occurrence with a band table runs the certificate search from its ESTIMATE in its own
//      lane, on (table, ub) as the band kernel left them, and stores the result to spec[r].  A read that does not certify is
//      listed for the exact kernels here (band_read_to_exact, exact[r] = 1), before the walk looks at any exact[] byte.
//      (Replaying from the starts the feedback can turn the estimate into — est +- 1, 2 — was tried so that the walk would never
//      meet an uncertain table: half of the HiFi reads then fail, because a search window that does not hold the best size has a
//      maximum 5 |motif| to 7 |motif| per size below it, under the 2 * len(diagonal) bound of its inexact entries.  Reads that
//      turn out uncertain from their real start are re-scored on the device instead: the append lists below.)
//   2. The walk, 64 reads per batch, lane i owning read base + i: under the current fraction every lane tests replay_quiet
//      for its read; one ballot finds the first lane that is not quiet, the quiet lanes in front of it commit their stored
//      results at once, and that one read — an EVENT — goes through the wave-uniform serial code (values fetched with
//      v_readlane): the search from the moved start, the fan-out to the exact lists, the stop for a pending exact table, the miss,
//      the empty result, feedback_update.  The walk goes on behind it with the new fraction: the same double, updated by the same
//      two functions in the same order as a walk read by read.
//   3. Hand-over: next_read, frac, stop, need_lo / need_hi and the per-bucket miss counters.
// ---------------------------------------------------------------------------------------------
struct ReplayArgs {
    int32_t max_iters, lsr, step, tie_last, feedback, narrow;
    int32_t* out_cn;
    int32_t* out_score;
    int32_t* out_n;
    int32_t* out_start;
    // per-locus resume state
    int32_t* next_read;   // [n_loci] first read not yet finished (== read_off[l+1] when done)
    double* frac;         // [n_loci]
    int32_t* need_lo;     // [n_loci] window wanted by the read that missed
    int32_t* need_hi;
    // Two passes when the banded kernel took part (strk_api.hip: ... k_dp_band -> k_replay pass 1 -> exact kernels -> k_replay
    // pass 2).  Pass 1 (pre_exact = 1) runs BEFORE the exact kernels: it searches the band tables (step 1 above) and walks every
    // locus as far as certified band tables carry it.  At a read whose table is still to be written by the exact kernels (a band
    // fall-back, a read the band never took) it notes where the locus stopped and leaves; at a read whose banded table cannot
    // certify the search from the start the feedback gave it (step 1 certified it from the estimate only) it first appends that
    // read and every later read of the locus that still has a banded table to the exact kernels' class lists — reads of a locus
    // look alike: what is uncertain for one usually is for the next.  Pass 2 (resume = 1) runs behind the exact kernels and takes
    // the stopped loci from there with exact tables, so that the only misses left for the host are searches that leave their
    // candidate window.  (Before: every uncertain read was a miss, and every call of the bench workload paid a host round.)
    int32_t pre_exact;     // 1: pass 1
    int32_t resume;        // 1: pass 2 — continue the loci with stop[l] == kStopRescore from next_read / frac
    int32_t* stop;         // [n_loci] kStopNone / kStopRescore / kStopMiss
};
constexpr int kStopNone = 0, kStopRescore = 1, kStopMiss = 2;

// One wave per locus: lane i holds the inputs of the i-th read of a batch (coalesced loads).
// (at most 88 VGPRs — it has 64: a wave of this kernel then fits next to the two resident waves of a band kernel on a SIMD, so that
// the replay of one call runs inside the band pass of the next one instead of waiting for a free CU slot)
#ifndef STRK_REPLAY_WAVES
#define STRK_REPLAY_WAVES 5   // waves per SIMD the register allocator aims at (tools/exp_build.sh variants)
#endif
__global__ void __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(STRK_REPLAY_WAVES, 8))) k_replay(KArgs a, ReplayArgs p) {
    const int l = blockIdx.x;
    const int lane = threadIdx.x;
    const int r_end = a.read_off[l + 1];
    double frac = 0.0;
    int r_next = a.read_off[l];   // first read not finished yet
    if (p.resume) {
        if (p.stop[l] != kStopRescore) return;
        r_next = p.next_read[l];
        frac = p.frac[l];
    }
    // ---- 1. the certificate search of the band tables from the estimate, a lane per read ----
    // The whole locus before the walk starts: which reads the exact kernels get does not depend on where the walk stops.
    if (p.pre_exact && a.band_mode && a.spec) {
        const int m = a.motif_off[l + 1] - a.motif_off[l];
        for (int base = r_next; base < r_end; base += 64) {
            const int r = base + lane;
            if (r >= r_end || a.rep[r] != r || a.exact[r]) continue;   // a copy takes its first occurrence's result from spec[]
            const int wlo = a.win_lo[r], wn = min(a.win_n[r], 64);
            const int32_t* const ubp = a.ub + a.tab_off[r];
            SeenMask64 seen;
            auto ub = [&](int k) { return ubp[k]; };
            const CertResult cr = search_replay_cert(a.est_cn[r], p.step, p.lsr, p.max_iters, p.tie_last, a.table + a.tab_off[r],
                                                     wlo, wn, seen, ub, p.narrow);
            if (!cr.uncertain) {
                a.spec[r] = make_int4(cr.res.cn, cr.res.score, cr.res.n_explored,
                                      (cr.res.miss ? kSpecMiss : 0) | (cr.res.empty ? kSpecEmpty : 0));
            } else {
                band_read_to_exact(a, r, a.nfl[r], a.ntr[r], a.nfr[r], m, wlo, wn);
                a.exact[r] = 1;
            }
        }
        // spec[] and exact[] as stored above are what the lanes of the walk load: other lanes of this same wave, so the stores only
        // have to be complete (work-group scope: one CU, one vector L1).  That holds because a block IS one wave
        // (__launch_bounds__(64), one locus per block): the wave that wrote is the wave that reads.  Several loci or waves per
        // block would keep it; a reader in ANOTHER block would need device scope.  A device-scope fence here writes the L2 back
        // and invalidates it once per locus: pass 1 of the bench workload took 339 us with it, 69 us without
        // (profiles/r21_replay_lanes.txt, "First build").
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
    }
    // ---- 2. the walk ----
    bool missed = false, rescore = false;
    for (int base = r_next; base < r_end && !missed && !rescore; base += 64) {
        const int cnt = min(64, r_end - base);
        const int rl = base + lane;
        const unsigned ro = (unsigned)rl;   // (unsigned: the four output stores share one 32-bit offset, base addresses in SGPRs)
        // what the lane keeps of its read: estimate, stored result, and the flags with the pending bit on top of them
        constexpr int kPendingBit = 4;
        int my_est = 0, my_flags = kSpecMiss;
        int4 my_spec = make_int4(0, 0, 0, 0);
        if (lane < cnt) {
            const int rp = a.rep[rl];
            my_est = a.est_cn[rl];
            if (a.spec) {
                my_spec = a.spec[rp];
                my_flags = my_spec.w;
            }
            if (p.pre_exact && (!a.band_mode || a.exact[rp])) my_flags |= kPendingBit;
        }
        int done = 0;
        while (done < cnt) {
            // the first read at or behind `done` that is not quiet under this fraction (lanes without a read count as such)
            const WalkRead rd = {my_est, my_spec.x, my_spec.y, my_spec.z, my_flags & (kSpecMiss | kSpecEmpty), my_flags & kPendingBit};
            const bool quiet = lane < cnt && replay_quiet(rd, p.feedback, frac);
            const unsigned long long loud = __builtin_amdgcn_ballot_w64(!quiet) & (~0ull << done);
            const int ev = min(loud ? (int)__builtin_ctzll(loud) : 64, cnt);
            if (lane >= done && lane < ev) {
                p.out_cn[ro] = my_spec.x;
                p.out_score[ro] = my_spec.y;
                p.out_n[ro] = my_spec.z;
                p.out_start[ro] = my_est;
            }
            done = ev;
            if (ev >= cnt) break;
            // the event: one read through the serial code, wave-uniform
            const int i = __builtin_amdgcn_readfirstlane(ev);
            const int est = __builtin_amdgcn_readlane(my_est, i);
            int start = est;
            double frac_try = frac;
            if (p.feedback) start = feedback_start(est, &frac_try);
            // (wave-uniform by construction; said so, or the search below is compiled as per-lane code: 96 VGPRs instead of 64)
            start = __builtin_amdgcn_readfirstlane(start);
            SearchResult res;
            const int spec_flags = __builtin_amdgcn_readlane(my_flags, i);
            if (start == est && !(spec_flags & kSpecMiss)) {
                // the search from the estimate is stored (step 1 above, or the exact kernels' own)
                res.cn = __builtin_amdgcn_readlane(my_spec.x, i);
                res.score = __builtin_amdgcn_readlane(my_spec.y, i);
                res.n_explored = __builtin_amdgcn_readlane(my_spec.z, i);
                res.miss = 0;
                res.empty = (spec_flags & kSpecEmpty) ? 1 : 0;
            } else {
                const int r = base + i;
                const int rp = a.rep[r];
                SeenMask64 seen;
                const bool is_exact = !a.band_mode || a.exact[rp];
                if (p.pre_exact && is_exact) {   // its table comes with the exact kernels: pass 2 continues here
                    rescore = true;
                    break;
                }
                if (is_exact) {
                    res = search_replay(start, p.step, p.lsr, p.max_iters, p.tie_last, a.table + a.tab_off[r], a.win_lo[r],
                                        min(a.win_n[r], 64), seen, p.narrow);
                } else {
                    // banded table: lower bounds + certificate (the bounds as the band kernel stored them); an ambiguous
                    // comparison asks for exact scores
                    const int m = a.motif_off[l + 1] - a.motif_off[l];
                    const int wlo = a.win_lo[r], wn = min(a.win_n[r], 64);
                    const int32_t* const ubp = a.ub + a.tab_off[r];
                    auto ub = [&](int k) { return ubp[k]; };
                    const CertResult cr = search_replay_cert(start, p.step, p.lsr, p.max_iters, p.tie_last,
                                                             a.table + a.tab_off[r], wlo, wn, seen, ub, p.narrow);
                    res = cr.res;
                    if (cr.uncertain && p.pre_exact) {
                        // this read and the rest of the locus go to the exact kernels (every read at most once: test-and-set of
                        // its flag byte), lane j taking read r + j, r + j + 64, ...
                        for (int q0 = r; q0 < r_end; q0 += 64) {
                            const int q = q0 + lane;
                            if (q >= r_end) continue;
                            const int rq = a.rep[q];
                            unsigned* const w = reinterpret_cast<unsigned*>(a.exact + (rq & ~3));
                            const unsigned bit = 1u << (8 * (rq & 3));
                            if (atomicOr(w, bit) & (0xffu << (8 * (rq & 3)))) continue;   // exact already, or listed by another lane
                            band_read_to_exact(a, rq, a.nfl[rq], a.ntr[rq], a.nfr[rq], m, a.win_lo[rq], min(a.win_n[rq], kTableMax));
                        }
                        rescore = true;
                        break;
                    }
                    if (cr.uncertain) { res.miss = 1; res.need_lo = wlo; res.need_hi = wlo + wn - 1; }
                }
            }
            if (res.miss) {
                if (lane == 0) {
                    p.need_lo[l] = res.need_lo;
                    p.need_hi[l] = res.need_hi;
                    atomicAdd(&a.counters[kCntMiss], 1);
                }
                missed = true;
                break;
            }
            frac = frac_try;
            if (res.empty) {
                if (lane == 0) atomicOr(&a.counters[kCntError], kErrEmpty);  // the reference would raise here
                res.cn = 0;
                res.score = 0;
            }
            if (lane == i) {
                p.out_cn[ro] = res.cn;
                p.out_score[ro] = res.score;
                p.out_n[ro] = res.n_explored;
                p.out_start[ro] = start;
            }
            if (p.feedback && !res.empty && res.cn != start) feedback_update(&frac, res.cn, start);  // += 0 otherwise
            done = i + 1;
        }
        r_next = base + done;
    }
    // ---- 3. hand-over ----
    if (lane == 0) {
        p.next_read[l] = r_next;
        p.frac[l] = frac;
        p.stop[l] = rescore ? kStopRescore : (missed ? kStopMiss : kStopNone);
        // loci whose search left its window, per motif-length bucket (the host adapts each bucket's default window; k_plan
        // counts the loci of a bucket)
        if (missed) atomicAdd(&a.counters[kCntMissB + win_bucket(a.motif_off[l + 1] - a.motif_off[l])], 1);
    }
}

}  // namespace strk
