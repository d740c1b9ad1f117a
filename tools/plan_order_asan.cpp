// k_plan's counting sort of a block's band items (strk_plan_order.h: plan_bin, plan_order_host) on random key sets, for a host
// build under AddressSanitizer + UBSan (tools/plan_order_asan.sh) and for tests/test_band_scope_host.py.
//   plan_order_asan [n_sets [seed]]     prints "<sets> <items> <errors>"
// Checked per set: every band item gets a slot, the slots are exactly 0 .. count - 1, and along the slots the keys
// (class, bin of the rows, read index) never fall.
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "../strkit_amd/csrc/strk_plan_order.h"

int main(int argc, char** argv) {
    const long n_sets = argc > 1 ? atol(argv[1]) : 1000000;
    std::mt19937 rng(argc > 2 ? (unsigned)atol(argv[2]) : 19u);
    using namespace strk;
    std::vector<int> cls(kPlanScope), rows(kPlanScope), slot(kPlanScope), hist(kPlanBins), inv(kPlanScope);
    long items = 0, errors = 0;
    for (long it = 0; it < n_sets; ++it) {
        // how full the block is, how many classes it mixes, how wide the rows spread: from empty to full, from one bin to all
        const unsigned fill = (it % 7 == 0) ? 0xffffffffu : (rng() >> (rng() % 32));
        const int n_cls = 1 + rng() % kNumBandClasses, c0 = rng() % kNumBandClasses;
        const int spread = 1 << (rng() % 15);
        const int rpt = (it % 3 == 0) ? 1 : kPlanReadsPerThread;   // small calls: one read per thread
        const int N = kPlanThreads * rpt;
        const int n_valid = (it % 5 == 0) ? (int)(rng() % (N + 1)) : N;   // a last block: no reads behind n_valid
        int count = 0;
        for (int i = 0; i < N; ++i) {
            const bool item = i < n_valid && rng() <= fill;
            cls[i] = item ? (c0 + (int)(rng() % n_cls)) % kNumBandClasses : -1;
            rows[i] = (int)(rng() % spread) + (int)(rng() % 3) - 1;   // (-1 and rows beyond a class's limit: the clamp)
            count += item;
        }
        const int total = plan_order_host(cls.data(), rows.data(), slot.data(), hist.data(), rpt);
        if (total != count) ++errors;
        for (int k = 0; k < count; ++k) inv[k] = -1;
        for (int i = 0; i < N; ++i) {
            if (cls[i] < 0) { errors += slot[i] != -1; continue; }
            if (slot[i] < 0 || slot[i] >= count || inv[slot[i]] >= 0) { ++errors; continue; }
            inv[slot[i]] = i;
        }
        for (int k = 1; k < count; ++k) {
            const int a = inv[k - 1], b = inv[k];
            if (a < 0 || b < 0) { ++errors; continue; }
            const int ka = plan_bin(cls[a], rows[a]), kb = plan_bin(cls[b], rows[b]);   // bins are numbered class by class
            if (cls[a] > cls[b] || (cls[a] == cls[b] && ka > kb) || (ka == kb && a > b)) ++errors;
            if ((cls[a] < cls[b]) != (ka < kb) && cls[a] != cls[b]) ++errors;
        }
        items += count;
    }
    printf("%ld %ld %ld\n", n_sets, items, errors);
    return errors != 0;
}
