// mi_asan.cpp — host-only driver of strk_mi.h (the per-locus routine behind strk_mi_trio_host) and strk_mi_check.h, for the
// sanitizers:   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=undefined tools/mi_asan.cpp -o mi_asan && ./mi_asan
// (tests/test_mi_tool.py builds it without a sanitizer and runs it).  What it holds the header to, over a built-in corpus:
//   the special functions against the C library (exp, erfc), against closed forms (chi-square tails of 2 and 4 degrees) and, for
//   large statistics over many degrees (tails of 1e-200 to 1e-300), against scipy's values and a long double sum of the terms;
//   the exact Mann-Whitney tail against the enumeration of every arrangement, sides up to 6, and its symmetry on long sides;
//   host_locus on hand loci (statuses, the first of four equal p-values, a de novo step found in the father's allele) and on
//   random loci, where the table built by sorting must give what counting over the raw reads gives;
//   every refusal of the input check.
// The program counts its own failures and exits 0 without one.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <random>
#include <string>
#include <vector>

#include "../strkit_amd/csrc/strk_mi.h"
#include "../strkit_amd/csrc/strk_mi_check.h"

namespace {

int g_checks = 0, g_failed = 0;

void expect(bool ok, const char* what) {
    ++g_checks;
    if (!ok) { ++g_failed; std::printf("FAILED: %s\n", what); }
}
bool close_to(double a, double b, double rtol) { return a == b || std::fabs(a - b) <= rtol * std::fmax(std::fabs(a), std::fabs(b)); }

struct Loci {
    std::vector<int64_t> off{0};
    std::vector<int32_t> cn, gt, ci95;
    void add(const std::vector<std::vector<int32_t>>& groups) {
        for (const auto& g : groups) {
            cn.insert(cn.end(), g.begin(), g.end());
            off.push_back((int64_t)cn.size());
            const int32_t call = g.empty() ? 0 : g[0];
            gt.push_back(call);
            ci95.push_back(call - 1); ci95.push_back(call + 1);
        }
    }
    int32_t n() const { return (int32_t)(off.size() / 6); }
};

struct Result {
    std::vector<int8_t> respects;
    std::vector<double> p;
    std::vector<int32_t> config, from, status;
};

Result run(const Loci& L, int test, double sig) {
    Result r;
    const size_t n = (size_t)L.n();
    r.respects.assign(7 * n, 9); r.p.assign(n, -1.0); r.config.assign(n, -9); r.from.assign(n, -9); r.status.assign(n, -9);
    strk_mi::Args a{};
    a.grp_off = L.off.data(); a.cn = L.cn.data(); a.gt = L.gt.data(); a.ci95 = L.ci95.data();
    a.test = test; a.sig_level = sig; a.widen = 0.0;
    a.respects = r.respects.data(); a.p = r.p.data(); a.config = r.config.data(); a.from = r.from.data(); a.status = r.status.data();
    std::vector<uint64_t> keys;
    std::vector<int32_t> tval, tcnt;
    std::vector<strk_mi::U128> ws;
    for (size_t l = 0; l < n; ++l) strk_mi::host_locus(a, (int64_t)l, keys, tval, tcnt, ws);
    return r;
}

// P(U >= u) by enumerating every choice of n1 positions among n1 + n2
double brute_sf(int n1, int n2, int u) {
    const int n = n1 + n2;
    long long hit = 0, all = 0;
    for (unsigned mask = 0; mask < (1u << n); ++mask) {
        if (__builtin_popcount(mask) != n1) continue;
        int stat = 0, below = 0;   // U1 = sum over x of the y below it
        for (int i = 0; i < n; ++i) {
            if ((mask >> i) & 1u) stat += below;
            else ++below;
        }
        ++all;
        hit += stat >= u ? 1 : 0;
    }
    return (double)hit / (double)all;
}

void special_functions() {
    for (double x = -740.0; x < 705.0; x += 3.37) expect(close_to(strk_mi::exp_d(x), std::exp(x), 1e-14), "exp_d against exp");
    expect(strk_mi::exp_d(-800.0) == 0.0 && strk_mi::exp_d(0.0) == 1.0, "exp_d at the ends");
    for (double x = -3.0; x < 26.0; x += 0.0713) expect(close_to(strk_mi::erfc_d(x), std::erfc(x), 1e-12), "erfc_d against erfc");
    expect(strk_mi::erfc_d(0.0) == 1.0 && std::isnan(strk_mi::erfc_d(std::nan(""))), "erfc_d at 0 and of a NaN");
    for (double x = 0.01; x < 1400.0; x *= 1.31) {
        expect(close_to(strk_mi::chi2_sf(2, x), std::exp(-x / 2), 1e-12), "chi2_sf of 2 degrees = exp(-x / 2)");
        expect(close_to(strk_mi::chi2_sf(4, x), std::exp(-x / 2) * (1 + x / 2), 1e-12), "chi2_sf of 4 degrees");
        expect(close_to(strk_mi::chi2_sf(1, x), std::erfc(std::sqrt(x / 2)), 1e-12), "chi2_sf of 1 degree = erfc(sqrt(x / 2))");
        double prev = 0.0;
        for (int dof = 1; dof < 40; dof += 3) {   // more degrees, a heavier tail
            const double q = strk_mi::chi2_sf(5000 + dof, 5400.0 + x), far = strk_mi::chi2_sf(5000 + dof, x);
            expect(q > prev && q < 1.0 && far > 0.999999 && far <= 1.0, "chi2_sf of many degrees: inside [0, 1], growing with the degrees");
            prev = q;
        }
    }
    // a large statistic over many degrees: e^(-x / 2) alone is denormal or 0 there while the tail is far above 1e-300
    // (values of scipy.stats.chi2.sf, scipy 1.15)
    const struct { int dof; double x, want; } deep[] = {
        {110, 1600.0, 9.960127432295515e-263}, {1500, 4000.0, 3.5430288239906716e-226}, {110, 1480.0, 1.6987761840876897e-238},
        {99, 1600.0, 2.841212427476395e-269},  {111, 1700.0, 1.991823846465042e-282},   {60, 1500.0, 5.326945235582446e-274},
        {1000, 3300.0, 5.098001594312757e-243}, {2001, 5000.0, 4.185580099013133e-256}};
    for (const auto& d : deep) expect(close_to(strk_mi::chi2_sf(d.dof, d.x), d.want, 1e-10), "chi2_sf of a large statistic over many degrees against scipy");
    // the same tails from the terms' logarithms in long double: even degrees, Q(m, h) = sum_{j<m} e^(j ln h - lgamma(j + 1) - h)
    for (int m : {30, 55, 200, 750})
        for (double x : {1420.0, 1600.0, 2200.0, 4000.0}) {
            const long double h = x / 2;
            long double q = 0;
            for (int j = 0; j < m; ++j) q += expl(j * logl(h) - lgammal((long double)j + 1) - h);
            if (q > 1e-300L) expect(close_to(strk_mi::chi2_sf(2 * m, x), (double)q, 1e-10), "chi2_sf of a large statistic against the sum of its terms in long double");
        }
    expect(strk_mi::chi2_sf(0, 3.0) == 1.0 && strk_mi::chi2_sf(7, 0.0) == 1.0, "chi2_sf without degrees or without a statistic");
}

void exact_tail() {
    std::vector<strk_mi::U128> ws;
    for (int n1 = 1; n1 <= 6; ++n1)
        for (int n2 = 1; n2 <= 6; ++n2) {
            const int64_t cap = strk_mi::exact_entries_for(n1, n2);
            ws.assign((size_t)cap, strk_mi::U128{7, 7});
            for (int u = 0; u <= n1 * n2; ++u)
                expect(close_to(strk_mi::mwu_exact_sf(n1, n2, u, ws.data(), cap), brute_sf(n1, n2, u), 1e-13), "exact tail against the enumeration");
        }
    // long sides: P(U >= u) + P(U >= mn - u + 1) = 1, coefficients beyond 2^53 (8 against 300)
    for (int n2 : {64, 300, 5000}) {
        const int n1 = 8;
        const int64_t mn = (int64_t)n1 * n2, cap = strk_mi::exact_entries_for(n1, n2);
        ws.assign((size_t)cap, strk_mi::U128{0, 0});
        for (int64_t u : {(int64_t)1, mn / 4, mn / 2, mn / 2 + 1, mn - 3, mn}) {
            const double a = strk_mi::mwu_exact_sf(n1, n2, u, ws.data(), cap), b = strk_mi::mwu_exact_sf(n2, n1, mn - u + 1, ws.data(), cap);
            expect(close_to(a + b, 1.0, 1e-12) && a >= 0.0 && b >= 0.0, "exact tail: the two tails add up to 1");
        }
        expect(std::isnan(strk_mi::mwu_exact_sf(n1, n2, mn / 2, ws.data(), 3)), "exact tail: a workspace too small is a NaN, not a write");
    }
}

void hand_loci() {
    Loci L;
    L.add({{5, 5}, {5}, {5, 5}, {5}, {5}, {5, 5}});                 // 0: one value everywhere
    L.add({{5, 6}, {7}, {5, 5}, {}, {6}, {7}});                     // 1: an empty parent group
    L.add({{}, {}, {5, 5}, {6}, {6}, {7}});                         // 2: no child reads
    L.add({{7, 8, 9}, {8, 9, 10}, {3, 4}, {4, 3}, {5, 4}, {4, 5}});   // 3: four equal configurations
    L.add({{10, 10, 10, 11, 10, 10, 10, 10}, {17, 18, 18, 18, 18, 19, 18, 18}, {10, 10, 10, 10, 9, 10, 10, 10},
           {12, 12, 12, 12, 13, 12, 12, 12}, {15, 15, 15, 14, 15, 15, 15, 16}, {20, 20, 21, 20, 20, 20, 20, 20}});   // 4: de novo, father's allele
    const Result x2 = run(L, strk_mi::kTestX2, 0.05), wmw = run(L, strk_mi::kTestWmw, 0.05);
    expect(x2.status[0] == strk_mi::kTested && x2.p[0] == 1.0 && x2.config[0] == 0, "one bin: p = 1 exactly");
    expect(wmw.status[0] == strk_mi::kOverlap && std::isnan(wmw.p[0]) && wmw.config[0] == -1, "complete overlap is not tested under wmw");
    expect(x2.status[1] == strk_mi::kEmptyParent && wmw.status[1] == strk_mi::kEmptyParent, "empty parent group");
    expect(x2.status[2] == strk_mi::kEmptyChild && wmw.status[2] == strk_mi::kEmptyChild, "empty child");
    expect(x2.config[3] == 0 && wmw.config[3] == 0 && x2.from[3] == strk_mi::kFromNone, "of four equal p-values the first wins");
    expect(x2.p[4] < 0.05 && x2.config[4] == 0 && x2.from[4] == strk_mi::kFromPat, "a de novo step in the father's allele");
    expect(x2.respects[0] == 1 && x2.respects[3] == -1 && x2.respects[4] == -1, "respects: strict, and the kinds without input");
}

// U1 and the tie term by counting over the raw reads
void random_loci() {
    std::mt19937 rng(22);
    Loci L;
    for (int k = 0; k < 200; ++k) {
        std::vector<std::vector<int32_t>> g(6);
        const int spread = 1 + (int)(rng() % 40), depth = 1 + (int)(rng() % (k % 10 == 0 ? 400 : 30));
        for (auto& x : g)
            for (int i = 0, n = 1 + (int)(rng() % depth); i < n; ++i) x.push_back((int32_t)(rng() % spread) * (k % 7 == 0 ? 613 : 1));
        L.add(g);
    }
    const Result r = run(L, strk_mi::kTestWmw, 0.05), r2 = run(L, strk_mi::kTestX2, 0.05), r3 = run(L, strk_mi::kTestWmwGt, 0.05);
    for (int32_t l = 0; l < L.n(); ++l) {
        if (r.status[l] != strk_mi::kTested) continue;
        // the chosen configuration's two-sided p again, from U counted pair by pair (asymptotic branch only: sides above 8 or ties)
        const int c = r.config[l];
        std::vector<int32_t> x, y;
        for (int g : {2 + (c >> 1), 4 + (c & 1)}) x.insert(x.end(), L.cn.begin() + L.off[6 * l + g], L.cn.begin() + L.off[6 * l + g + 1]);
        y.assign(L.cn.begin() + L.off[6 * l], L.cn.begin() + L.off[6 * l + 2]);
        double u1 = 0;
        for (int32_t a : x)
            for (int32_t b : y) u1 += a > b ? 1.0 : (a == b ? 0.5 : 0.0);
        std::vector<int32_t> all(x);
        all.insert(all.end(), y.begin(), y.end());
        std::sort(all.begin(), all.end());
        double tie = 0;
        for (size_t i = 0, j; i < all.size(); i = j) {
            for (j = i; j < all.size() && all[j] == all[i]; ++j) {}
            const double t = (double)(j - i);
            tie += t * t * t - t;
        }
        const double n1 = (double)x.size(), n2 = (double)y.size(), n = n1 + n2;
        if ((n1 > 8 && n2 > 8) || tie > 0) {
            const double u = std::fmax(u1, n1 * n2 - u1), s = std::sqrt(n1 * n2 / 12.0 * ((n + 1.0) - tie / (n * (n - 1.0))));
            const double p = std::fmin(1.0, std::erfc((u - n1 * n2 / 2.0) / s / std::sqrt(2.0)));
            expect(std::isnan(p) ? std::isnan(r.p[l]) : close_to(r.p[l], p, 1e-10), "wmw p of the chosen configuration from pair counting");
        }
        expect(r2.p[l] >= 0.0 && r2.p[l] <= 1.0 && r3.p[l] >= 0.0 && r3.p[l] <= 1.0, "p inside [0, 1]");
    }
}

void refusals() {
    Loci L;
    L.add({{5, 6}, {7}, {5, 5}, {6}, {6}, {7}});
    L.add({{5, 6}, {7}, {5, 5}, {6}, {6}, {7}});
    strk_mi_params p{};
    p.test = STRK_MI_TEST_X2; p.sig_level = 0.05;
    const auto refused = [&](const strk_mi_check::Input& in, const char* part) {
        strk_groups::Message m;
        m.text[0] = 0;
        const int rc = strk_mi_check::check(in, strk_mi::kMaxGroup, &m);
        expect(rc == STRK_E_INVALID && std::strstr(m.text, part) != nullptr, part);
    };
    const strk_mi_check::Input good{L.n(), L.off.data(), L.cn.data(), (int64_t)L.cn.size(), L.gt.data(), L.ci95.data(), nullptr, nullptr, nullptr, &p};
    strk_groups::Message m;
    expect(strk_mi_check::check(good, strk_mi::kMaxGroup, &m) == 0, "a good input passes");
    strk_mi_check::Input in = good;
    in.n_loci = -1; refused(in, "n_loci < 0");
    in = good; in.p = nullptr; refused(in, "params is NULL");
    strk_mi_params q = p;
    in = good; in.p = &q;
    q.test = 4; refused(in, "test 4");
    q = p; q.sig_level = 1.0; refused(in, "sig_level");
    q = p; q.sig_level = std::nan(""); refused(in, "sig_level");
    q = p; q.widen = -1.0; refused(in, "widen");
    q = p; q.piece_loci = -1; refused(in, "piece_loci");
    in = good; in.gt = nullptr; refused(in, "NULL argument");
    in = good; in.grp_off = nullptr; refused(in, "NULL argument");
    in = good; in.seq_id = L.gt.data(); refused(in, "seq_id is given without seq_len");
    in = good; in.seq_len = L.gt.data(); refused(in, "seq_len is given without seq_id");
    std::vector<int64_t> off = L.off;
    off[8] = off[7] - 1; in = good; in.grp_off = off.data(); refused(in, "locus 1: grp_off is decreasing at group 1");
    off = L.off; off[12] += 1; in = good; in.grp_off = off.data(); refused(in, "locus 1: group 5 ends at read");
    off = L.off; off[0] = 1; in = good; in.grp_off = off.data(); refused(in, "grp_off[0] must be 0");
    std::vector<int32_t> cn = L.cn;
    cn[9] = -1; in = good; in.cn = cn.data(); refused(in, "has the copy number -1");
    std::vector<int32_t> ci = L.ci95;
    ci[14] = ci[15] + 1; in = good; in.ci95 = ci.data(); refused(in, "locus 1: ci95 of allele 1");
    in = good; in.ci99 = ci.data(); refused(in, "locus 1: ci99 of allele 1");
    std::vector<int64_t> big(7, 0);
    for (int g = 3; g <= 6; ++g) big[g] = strk_mi::kMaxGroup + 1;
    std::vector<int32_t> many((size_t)strk_mi::kMaxGroup + 1, 3);
    in = good; in.n_loci = 1; in.grp_off = big.data(); in.cn = many.data(); in.n_cn = (int64_t)many.size();
    refused(in, "locus 0: group 2 has 65536 reads (at most 65535)");
    q = p; q.test = STRK_MI_TEST_NONE; in = good; in.p = &q; in.grp_off = nullptr; in.cn = nullptr;
    expect(strk_mi_check::check(in, strk_mi::kMaxGroup, &m) == 0, "without a test the reads may be missing");
}

}  // namespace

int main() {
    special_functions();
    exact_tail();
    hand_loci();
    random_loci();
    refusals();
    std::printf("mi_asan: %d checks, %d failed\n", g_checks, g_failed);
    return g_failed ? 1 : 0;
}
