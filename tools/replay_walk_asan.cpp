// k_replay's walk over the reads of a locus (strk_search.h: replay_quiet, replay_walk_serial, replay_walk_events) on random loci,
// for a host build under AddressSanitizer + UBSan (tools/replay_walk_asan.sh) and for tests/test_replay_walk_host.py.
//   replay_walk_asan [n_loci [seed]]
//   prints "<loci> <reads> <events> <resets> <errors> <loci without event> <events at lane 0> <at lane 63> <at lane 0 of a second batch>"
// Per locus the walk by events (batches of 64 lanes, the ballot a loop over the lanes) must end like the walk read by read: the
// same stop, the same first unfinished read, the same bits of the fraction, the same four outputs of every finished read.
// Loci: 1-200 reads; estimates from 0 up; stored results equal to the start or off by up to +-3; reads without a stored result,
// with an empty one, with a pending table; searches from a moved start that miss, do not certify or score nothing; feedback on
// and off; both passes.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "../strkit_amd/csrc/strk_search.h"

using namespace strk;

namespace {

struct Moved {   // what a search from a start other than the estimate (or without a stored result) gives for one read
    int32_t delta, miss, uncertain, empty;
};

}  // namespace

int main(int argc, char** argv) {
    const long n_loci = argc > 1 ? atol(argv[1]) : 1000000;
    std::mt19937 rng(argc > 2 ? (unsigned)atol(argv[2]) : 21u);
    long reads = 0, events = 0, resets = 0, errors = 0, no_event = 0, ev_lane0 = 0, ev_lane63 = 0, ev_batch2 = 0;
    std::vector<WalkRead> rd;
    std::vector<Moved> mv;
    std::vector<WalkOut> out_s, out_e;
    for (long it = 0; it < n_loci; ++it) {
        const int kind = (int)(it % 4);   // 0: nothing happens; 1: one event at a chosen read; 2: noisy; 3: small estimates, results below them
        int n = 1 + (int)(rng() % 200);
        if (kind == 1 && it % 8 == 1) n = 65 + (int)(rng() % 136);
        const int feedback = (it % 11 == 0) ? 0 : 1;
        const int pre_exact = (int)((it / 4) % 2);
        const int single = kind == 1 ? (it % 3 == 0 ? 0 : (it % 3 == 1 ? (n > 63 ? 63 : n - 1) : (n > 64 ? 64 : (int)(rng() % n)))) : -1;
        const int est0 = kind == 3 ? (int)(rng() % 4) : 2 + (int)(rng() % 60);
        rd.assign(n, WalkRead{0, 0, 0, 0, 0, 0});
        mv.assign(n, Moved{0, 0, 0, 0});
        for (int i = 0; i < n; ++i) {
            WalkRead& q = rd[i];
            q.est = est0 + (kind >= 2 ? (int)(rng() % 3) - 1 : 0);
            if (q.est < 0) q.est = 0;
            int d = 0;
            if (kind == 2 && rng() % 6 == 0) d = (int)(rng() % 7) - 3;
            if (kind == 3 && rng() % 3 == 0) d = -(int)(rng() % 4);
            if (i == single) d = 1 + (int)(rng() % 3);
            q.cn = q.est + d < 0 ? 0 : q.est + d;
            q.score = (int)(rng() % 1000);
            q.n_explored = 1 + (int)(rng() % 20);
            if (kind >= 2) {
                if (rng() % 40 == 0) q.flags |= kSpecMiss;
                if (rng() % 90 == 0) q.flags |= kSpecEmpty;
                if (pre_exact && rng() % 50 == 0) q.pending = 1;
                if (q.pending && rng() % 2) q.flags |= kSpecMiss;   // a read of the exact kernels has no result in pass 1
                mv[i].delta = (int)(rng() % 7) - 3;
                mv[i].miss = rng() % 60 == 0;
                mv[i].uncertain = rng() % 45 == 0;
                mv[i].empty = rng() % 120 == 0;
            }
        }
        auto search = [&](int32_t i, int32_t start, int32_t* uncertain) {
            SearchResult res = {0, 0, 0, 0, 0, 0, 0};
            const Moved& m = mv[i];
            *uncertain = m.uncertain;
            res.miss = m.miss;
            res.need_lo = start - 4;
            res.need_hi = start + 4;
            res.empty = m.empty;
            res.cn = start + m.delta < 0 ? 0 : start + m.delta;
            res.score = 7 * start + i;
            res.n_explored = 3 + (start & 7);
            return res;
        };
        out_s.assign(n, WalkOut{-1, -1, -1, -1});
        out_e.assign(n, WalkOut{-1, -1, -1, -1});
        double frac_s = 0.0, frac_e = 0.0;
        if (pre_exact == 0 && it % 5 == 0) frac_s = frac_e = ((int)(rng() % 9) - 4) / 16.0;   // pass 2 takes a locus up with a fraction
        int32_t next_s = -1, next_e = -1;
        const int32_t how_s = replay_walk_serial(rd.data(), n, feedback, pre_exact, &frac_s, out_s.data(), &next_s, search);
        long ev_here = 0;
        auto on_event = [&](int32_t lane, int32_t base) {
            ++ev_here;
            ev_lane0 += lane == 0 && base == 0;
            ev_lane63 += lane == 63;
            ev_batch2 += lane == 0 && base == 64;
            if (feedback) {
                double f = frac_e;
                (void)feedback_start(rd[base + lane].est, &f);
                resets += !same_double_bits(f, frac_e);
            }
        };
        const int32_t how_e = replay_walk_events(rd.data(), n, feedback, pre_exact, &frac_e, out_e.data(), &next_e, search, on_event);
        if (how_s != how_e || next_s != next_e || !same_double_bits(frac_s, frac_e)) ++errors;
        for (int i = 0; i < n && i < next_s && i < next_e; ++i) errors += memcmp(&out_s[i], &out_e[i], sizeof(WalkOut)) != 0;
        reads += n;
        events += ev_here;
        no_event += ev_here == 0;
    }
    printf("%ld %ld %ld %ld %ld %ld %ld %ld %ld\n", n_loci, reads, events, resets, errors, no_event, ev_lane0, ev_lane63, ev_batch2);
    return errors != 0;
}
