// The host side of strk_realign that runs before any launch (strk_realign_plan.h: the input check, the chunks by trace
// budget, the order inside a chunk, the layout of a chunk's workspaces).  Every input array is a heap block of exactly its
// length, so a read one element past any of them is reported under AddressSanitizer / UBSan (tools/realign_asan.sh);
// tests/test_host.py builds it plain and requires exit 0.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <memory>
#include <random>
#include <utility>
#include <vector>
#include "../strkit_amd/csrc/strk_realign_plan.h"

namespace {

namespace RP = strk_realign_plan;
using strk::RealignPair;

struct Call {   // n pairs: the three offset arrays, n + 1 long each
    int32_t n = 0;
    std::unique_ptr<int64_t[]> s1_off, s2_off, cigar_off;
    int32_t open = 7, ext = 0, gap_pref = 0;
    Call(const std::vector<int64_t>& n1, const std::vector<int64_t>& n2, const std::vector<int64_t>& cap, int64_t base = 0)
        : n((int32_t)n1.size()), s1_off(new int64_t[n1.size() + 1]), s2_off(new int64_t[n1.size() + 1]), cigar_off(new int64_t[n1.size() + 1]) {
        s1_off[0] = base; s2_off[0] = 3 * base; cigar_off[0] = base / 2;
        for (int32_t p = 0; p < n; ++p) {
            s1_off[p + 1] = s1_off[p] + n1[p];
            s2_off[p + 1] = s2_off[p] + n2[p];
            cigar_off[p + 1] = cigar_off[p] + cap[p];
        }
    }
    int plan(size_t budget, RP::Plan* out, strk_groups::Message* why) const {
        return RP::plan(n, s1_off.get(), s2_off.get(), cigar_off.get(), open, ext, gap_pref, budget, out, why);
    }
};

int g_failed = 0, g_refusals = 0;

void failed(const char* what, long a = 0, long b = 0) {
    fprintf(stderr, "FAILED %s (%ld, %ld)\n", what, a, b);
    ++g_failed;
}

void refused(int rc, const strk_groups::Message& why, int code, const char* text, const char* what) {
    ++g_refusals;
    if (rc != code || strcmp(why.text, text)) {
        fprintf(stderr, "FAILED refusal %s: rc %d, message '%s'\n", what, rc, why.text);
        ++g_failed;
    }
}

void expect_refusal(const Call& c, int code, const char* text, const char* what) {
    RP::Plan plan;
    strk_groups::Message why;
    refused(c.plan((size_t)1 << 30, &plan, &why), why, code, text, what);
}

// [off, off + len) of every item: disjoint and inside [0, sum)
bool ranges_fit(std::vector<std::pair<int64_t, int64_t>> r, size_t sum) {
    std::sort(r.begin(), r.end());
    int64_t end = 0;
    for (const auto& [off, len] : r) {
        if (off < end || len < 0) return false;
        end = off + len;
    }
    return (size_t)end <= sum;
}

void check_plan(const Call& c, size_t budget, const RP::Plan& plan, long* chunks) {
    const int n = c.n;
    if ((int)plan.pairs.size() != n || (int)plan.trace_bytes.size() != n) return failed("sizes");
    int next = 0;
    for (const RP::Chunk& ch : plan.chunks) {
        ++*chunks;
        if (ch.p0 != next || ch.p1 <= ch.p0 || ch.p1 > n) return failed("chunks are not consecutive", ch.p0, ch.p1);
        next = ch.p1;
        const int m = ch.p1 - ch.p0;
        size_t tsum = 0, esum = 0, csum = 0;
        double cells = 0;
        std::vector<char> seen((size_t)m, 0);
        std::vector<std::pair<int64_t, int64_t>> tr, ed, cg;
        for (int k = ch.p0; k < ch.p1; ++k) {
            const RealignPair& r = plan.pairs[(size_t)k];
            if (r.orig < 0 || r.orig >= m || seen[(size_t)r.orig]++) return failed("orig is no permutation", k, r.orig);
            const int p = ch.p0 + r.orig;   // the caller's pair
            const int64_t n1 = c.s1_off[p + 1] - c.s1_off[p], n2 = c.s2_off[p + 1] - c.s2_off[p], cap = c.cigar_off[p + 1] - c.cigar_off[p];
            const int cl = n1 <= 256 ? 4 : n1 <= 512 ? 8 : n1 <= 1024 ? 16 : 32;
            const int64_t ntiles = (n1 + 64 * cl - 1) / (64 * cl);
            if (r.n1 != n1 || r.n2 != n2 || r.s1_off != c.s1_off[p] - c.s1_off[0] || r.s2_off != c.s2_off[p] - c.s2_off[0] || r.reserved != 0)
                failed("the pair's sequences", p);
            if (r.cl != cl || r.ntiles != ntiles || r.pad != ntiles * 64 * cl - n1 || r.pad < 0 || r.pad >= 64 * cl) failed("cl / ntiles / pad", p);
            if (r.cig_cap != std::min<int64_t>(cap, 2 * n1 + 4)) failed("cig_cap", p);
            const size_t tb = plan.trace_bytes[(size_t)p];
            if (tb % 256 || tb < (size_t)(ntiles * (n2 + 63) * 64 * (cl / 2)) || tb >= (size_t)(ntiles * (n2 + 63) * 64 * (cl / 2)) + 256) failed("trace bytes", p);
            if (r.trace_off % 256) failed("trace_off is not 256-aligned", p);
            tr.push_back({r.trace_off, (int64_t)tb});
            if ((r.edge_off >= 0) != (ntiles > 1) || (ntiles <= 1 && r.edge_off != -1)) failed("edge_off", p);
            if (ntiles > 1) ed.push_back({r.edge_off, 4 * n2});
            cg.push_back({r.cig_off, r.cig_cap});
            tsum += tb;
            esum += ntiles > 1 ? (size_t)(4 * n2) : 0;
            csum += (size_t)r.cig_cap;
            cells += (double)ntiles * 64 * cl * (double)(n2 + 63);
            if (k > ch.p0) {   // widest class first, then most work first, stable
                const RealignPair& q = plan.pairs[(size_t)k - 1];
                const int64_t wq = (int64_t)q.ntiles * (q.n2 + 63), wr = (int64_t)r.ntiles * (r.n2 + 63);
                if (q.cl < r.cl || (q.cl == r.cl && (wq < wr || (wq == wr && q.orig > r.orig)))) failed("order inside the chunk", k);
            }
        }
        if (tsum != ch.tsum || esum != ch.esum || csum != ch.csum) failed("sums", ch.p0);
        if (cells != ch.cells) failed("cells", ch.p0);
        if (!ranges_fit(tr, ch.tsum)) failed("trace ranges", ch.p0);
        if (!ranges_fit(ed, ch.esum)) failed("edge ranges", ch.p0);
        if (!ranges_fit(cg, ch.csum)) failed("CIGAR ranges", ch.p0);
        if (ch.tsum > budget && m > 1) failed("a chunk of several pairs beyond the budget", ch.p0);
        // the cut is greedy: the pair behind the chunk did not fit
        if (ch.p1 < n && ch.tsum + plan.trace_bytes[(size_t)ch.p1] <= budget) failed("a chunk ends early", ch.p0);
    }
    if (next != n) failed("chunks do not cover the call", next, n);
}

}  // namespace

int main() {
    std::mt19937 rng(14);
    long calls = 0, chunks = 0;
    const int64_t edges[] = {1, 3, 255, 256, 257, 512, 513, 1024, 1025, 2048, 2049, 4096, 4097, 5000};
    const size_t budgets[] = {(size_t)1 << 20, (size_t)2 << 20, (size_t)8 << 20, (size_t)64 << 20, (size_t)16 << 30};
    for (int it = 0; it < 300; ++it) {
        const int n = 1 + (int)(rng() % 60);
        std::vector<int64_t> n1, n2, cap;
        for (int p = 0; p < n; ++p) {
            n1.push_back(rng() % 3 == 0 ? edges[rng() % (sizeof edges / sizeof *edges)] : 1 + (int64_t)(rng() % (it % 5 == 0 ? 6000 : 700)));
            n2.push_back(1 + (int64_t)(rng() % (it % 4 == 0 ? 4000 : 400)));
            cap.push_back(rng() % 4 == 0 ? (int64_t)(rng() % 8) : 2 * n1.back() + 4 + (int64_t)(rng() % 3));
        }
        Call c(n1, n2, cap, it % 3 == 0 ? 0 : (int64_t)(rng() % 100000));
        c.open = (int32_t)(rng() % 4097);
        c.ext = (int32_t)(rng() % (unsigned)(c.open + 1));
        for (int64_t len : n1)   // a valid call: every pair's gap costs inside the number format
            while (RP::gap_cost_reach(c.open, c.ext, len) >= RP::kGapCostLimit) c.ext /= 2;
        c.gap_pref = (int32_t)(rng() % 2);
        for (size_t budget : budgets) {
            RP::Plan plan;
            strk_groups::Message why;
            const int rc = c.plan(budget, &plan, &why);
            if (rc) failed("a valid call was refused", it, rc);
            else check_plan(c, budget, plan, &chunks);
            ++calls;
        }
    }
    {   // no pairs: valid whatever the arrays are, and nothing to run
        RP::Plan plan;
        strk_groups::Message why;
        if (RP::plan(0, nullptr, nullptr, nullptr, -1, -1, 7, 1, &plan, &why) != 0 || !plan.chunks.empty() || !plan.pairs.empty()) failed("no pairs");
        ++calls;
    }
    // every refusal by its code and its text, and which of two faults is found first
    const std::vector<int64_t> three{10, 20, 30}, caps{24, 44, 64};
    const Call good(three, three, caps);
    {
        RP::Plan plan;
        strk_groups::Message why;
        refused(RP::plan(-1, nullptr, nullptr, nullptr, 7, 0, 0, 1 << 20, &plan, &why), why, strk_groups::kInvalid, "n_pairs < 0", "n_pairs < 0");
        refused(RP::plan(3, nullptr, good.s2_off.get(), good.cigar_off.get(), 7, 0, 0, 1 << 20, &plan, &why), why, strk_groups::kInvalid, "NULL argument", "no s1_off");
        refused(RP::plan(3, good.s1_off.get(), nullptr, good.cigar_off.get(), 7, 0, 0, 1 << 20, &plan, &why), why, strk_groups::kInvalid, "NULL argument", "no s2_off");
        refused(RP::plan(3, good.s1_off.get(), good.s2_off.get(), nullptr, 9, 10, 5, 1 << 20, &plan, &why), why, strk_groups::kInvalid, "NULL argument", "no cigar_off, before the penalties");
    }
    for (auto [open, ext] : {std::pair{-1, 0}, std::pair{7, -1}, std::pair{4097, 0}, std::pair{3, 5}}) {
        Call c(three, three, caps);
        c.open = open; c.ext = ext; c.gap_pref = 2;   // (the penalties are looked at before gap_pref)
        expect_refusal(c, strk_groups::kInvalid, "need 0 <= extend <= open <= 4096", "penalties");
    }
    for (int pref : {-1, 2}) {
        Call c({0, 20, 30}, three, caps);   // (gap_pref is looked at before any pair)
        c.gap_pref = pref;
        expect_refusal(c, strk_groups::kInvalid, "bad gap_pref", "gap_pref");
    }
    expect_refusal(Call({10, 0, 30}, three, {24, -1, 64}), strk_groups::kInvalid, "pair 1: empty sequence", "empty s1, before its capacity");
    expect_refusal(Call(three, {10, 20, 0}, caps), strk_groups::kInvalid, "pair 2: empty sequence", "empty s2");
    expect_refusal(Call({10, -5, 30}, three, caps), strk_groups::kInvalid, "pair 1: empty sequence", "decreasing s1_off");
    expect_refusal(Call({10, (1 << 20) + 1, 0}, three, caps), strk_groups::kInvalid, "pair 1: sequence too long (1048577 x 20)", "long s1, before the pair behind it");
    expect_refusal(Call(three, {(1 << 24) + 1, 20, 30}, {-1, 44, 64}), strk_groups::kInvalid, "pair 0: sequence too long (10 x 16777217)", "long s2, before its capacity");
    expect_refusal(Call(three, three, {24, 44, -1}), strk_groups::kInvalid, "pair 2: negative CIGAR capacity", "negative capacity");
    expect_refusal(Call({10, 1 << 20}, {20, 1 << 24}, {24, 44}), RP::kNoMem, "pair 1: trace of 8796126052352 bytes", "a trace beyond 128 GiB");
    {   // the longest pair that is taken: 128 GiB is the limit, 2^20 x 2^17 stays below it
        RP::Plan plan;
        strk_groups::Message why;
        const Call c({1 << 20}, {1 << 17}, {0});
        if (c.plan((size_t)1 << 20, &plan, &why) != 0) failed("2^20 x 2^17 was refused");
        else check_plan(c, (size_t)1 << 20, plan, &chunks);
        ++calls;
    }
    {   // the gap-cost bound 2*open + (n1 - 2)*extend < 2^24: the last (open, extend, n1) taken and the first refused, along each
        // of the three; the n1 = 2^20 corner; the pair is named, and the bound is looked at before the capacity
        struct { int32_t open, ext; int64_t n1; bool ok; long long reach; } const cases[] = {
            {4096, 4096, 4095, true, 0}, {4096, 4096, 4096, false, 16777216}, {4096, 4096, 4097, false, 16781312},
            {4096, 4095, 4096, true, 0}, {4096, 4095, 4097, false, 16777217},
            {4096, 4000, 4194, true, 0}, {4096, 4001, 4194, false, 16780384},
            {3071, 2048, 8191, true, 0}, {3072, 2048, 8191, false, 16777216},
            {4096, 1, 16769026, false, 16777216},   // (n1 beyond 2^20 is refused as too long first)
            {4096, 15, 1 << 20, true, 0}, {16, 16, 1 << 20, false, 16777216}, {4096, 4096, 1 << 20, false, 4294967296ll},
            {4096, 4096, 1, true, 0}, {4096, 4096, 2, true, 0}, {7, 0, 1 << 20, true, 0},
        };
        for (const auto& k : cases) {
            Call c({10, k.n1}, {20, 1}, {24, -1});
            c.open = k.open; c.ext = k.ext;
            RP::Plan plan;
            strk_groups::Message why;
            const int rc = c.plan((size_t)1 << 20, &plan, &why);
            char text[256];
            if (k.n1 > (1 << 20)) snprintf(text, sizeof text, "pair 1: sequence too long (%lld x 1)", (long long)k.n1);
            else if (k.ok) snprintf(text, sizeof text, "pair 1: negative CIGAR capacity");
            else snprintf(text, sizeof text, "pair 1: gap costs beyond the number format (2*open + (n1 - 2)*extend = %lld, must be below 16777216)", k.reach);
            refused(rc, why, strk_groups::kInvalid, text, "gap-cost bound");
            if (k.ok != (RP::gap_cost_reach(k.open, k.ext, k.n1) < RP::kGapCostLimit)) failed("gap_cost_reach", k.open, k.ext);
            if (k.ok) {   // and with a capacity it is planned
                Call g({10, k.n1}, {20, 1}, {24, 0});
                g.open = k.open; g.ext = k.ext;
                if (g.plan((size_t)1 << 20, &plan, &why) != 0) failed("a pair inside the gap-cost bound was refused", k.open, k.ext);
                else check_plan(g, (size_t)1 << 20, plan, &chunks);
                ++calls;
            }
        }
    }
    printf("realign_asan: %ld valid calls, %ld chunks, %d refusals, %d failed\n", calls, chunks, g_refusals, g_failed);
    return g_failed ? 1 : 0;
}
