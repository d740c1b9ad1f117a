// The host side of strk_call_alleles and strk_call_alleles_phased that runs before any launch (strk_alleles_check.h and
// strk_phase_check.h: every input check; strk_groups.h: the piece cutter over per-locus costs shaped like the phased call's).
// Every array is a heap block of exactly its length, so a read one element past any of them is reported under
// AddressSanitizer / UBSan (tools/phase_asan.sh); tests/test_host.py builds it plain and requires exit 0.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <random>
#include <string>
#include <tuple>
#include <vector>
#include "../strkit_amd/csrc/strk_phase_check.h"

namespace {

struct Call {
    std::vector<int32_t> read_off, cn, n_alleles, hp, ps, snv_off;
    std::vector<double> w;
    std::vector<uint64_t> seed;
    std::vector<uint8_t> base, qual;
    strk_allele_params p{4, 2, 100, 3, 100, 3, 0, 0, 1e-3, 1e-6, 5.0};
    strk_phase_params pp{8, 20, 3, 0, 0.2, 0.1, 0};
    bool tags = true, snvs = true;
    strk_phase_check::Input input() const {
        return {{(int32_t)n_alleles.size(), read_off.data(), cn.data(), w.data(), n_alleles.data(), seed.data(), &p}, &pp,
                tags ? hp.data() : nullptr, tags ? ps.data() : nullptr, snvs ? snv_off.data() : nullptr, (int64_t)base.size(),
                snvs ? base.data() : nullptr, snvs ? qual.data() : nullptr};
    }
};

Call make(std::mt19937& rng, int n_loci, int max_n, int max_s) {
    Call c;
    c.read_off.push_back(0);
    c.snv_off.push_back(0);
    for (int l = 0; l < n_loci; ++l) {
        const int n = (int)(rng() % (unsigned)(max_n + 1)), s = (int)(rng() % (unsigned)(max_s + 1));
        c.read_off.push_back(c.read_off.back() + n);
        c.snv_off.push_back(c.snv_off.back() + s);
        c.n_alleles.push_back(1 + (int)(rng() % 2));
        c.seed.push_back(rng());
        for (int r = 0; r < n; ++r) {
            c.cn.push_back((int32_t)(rng() % 50));
            c.w.push_back(0.5 + (double)(rng() % 100) / 100.0);
            c.hp.push_back((int32_t)(rng() % 3) - 1);
            c.ps.push_back((int32_t)(rng() % 3) - 1);
        }
        c.base.resize(c.base.size() + (size_t)n * s, 'A');
        c.qual.resize(c.qual.size() + (size_t)n * s, 40);
    }
    return c;
}

int g_failed = 0, g_refusals = 0;

// strk_call_alleles' own check (the limits of strk_alleles.h)
void expect_plain(const Call& c, bool ok, const char* what, const char* needle = "") {
    strk_groups::Message m;
    m.text[0] = 0;
    const int rc = strk_alleles_check::check(c.input(), {65535, 1024, 15, 2}, &m);
    if (!(ok ? rc == 0 : (rc == strk_groups::kInvalid && strstr(m.text, needle)))) {
        fprintf(stderr, "FAILED plain %s: rc %d, message '%s'\n", what, rc, m.text);
        ++g_failed;
    }
    g_refusals += !ok;
}

// two loci of five reads, or one of n_reads
Call plain_call(int n_reads = 0) {
    Call c;
    c.tags = c.snvs = false;
    if (n_reads) c.read_off = {0, n_reads};
    else c.read_off = {0, 5, 10};
    for (int r = 0; r < c.read_off.back(); ++r) {
        c.cn.push_back(r);
        c.w.push_back(1.0);
    }
    c.n_alleles.assign(c.read_off.size() - 1, 2);
    c.seed.assign(c.read_off.size() - 1, 1);
    return c;
}

void expect(const Call& c, bool ok, const char* what, const char* needle = "") {
    const strk_phase_check::Limits lim{1024, 64, 1024, 15};
    std::vector<int64_t> cell_off;
    strk_groups::Message m;
    m.text[0] = 0;
    const int rc = strk_phase_check::check(c.input(), lim, cell_off, &m);
    const bool good = ok ? rc == 0 : (rc == strk_groups::kInvalid && strstr(m.text, needle));
    g_refusals += !ok;
    if (!good) {
        fprintf(stderr, "FAILED %s: rc %d, message '%s'\n", what, rc, m.text);
        ++g_failed;
    }
    if (ok && rc == 0 && c.snvs) {   // the cells in front of every locus
        int64_t cells = 0;
        for (size_t l = 0; l + 1 < c.read_off.size(); ++l) {
            if (cell_off[l] != cells) { fprintf(stderr, "FAILED %s: cell_off[%zu]\n", what, l); ++g_failed; }
            cells += (int64_t)(c.read_off[l + 1] - c.read_off[l]) * (c.snv_off[l + 1] - c.snv_off[l]);
        }
        if (cell_off.back() != cells || cells != (int64_t)c.base.size()) { fprintf(stderr, "FAILED %s: total cells\n", what); ++g_failed; }
    }
}

}  // namespace

int main() {
    std::mt19937 rng(12);
    long calls = 0, pieces = 0;
    for (int it = 0; it < 200; ++it) {
        Call c = make(rng, 1 + (int)(rng() % 40), it % 10 == 0 ? 1024 : 40, it % 7 == 0 ? 64 : 5);
        expect(c, true, "valid call");
        Call t = c;
        t.tags = false;
        expect(t, true, "no tags");
        t = c;
        t.snvs = false;
        expect(t, true, "no SNVs");
        // piece cutting over costs of the call's shape: masks, the matrix beyond the LDS cut, a fixed part per locus
        const size_t L = c.n_alleles.size();
        auto cost = [&](size_t l) {
            const int64_t n = c.read_off[l + 1] - c.read_off[l];
            return (int64_t)(8 * n + (n > 80 ? 8 * n * n : 0) + 4096);
        };
        for (int64_t budget : {(int64_t)1, (int64_t)10000, (int64_t)1 << 20, (int64_t)1 << 40})
            for (size_t max_items : {(size_t)1, (size_t)3, (size_t)32768}) {
                std::vector<int64_t> off;
                size_t p0 = 0;
                while (p0 < L) {
                    int64_t used = 0;
                    const size_t p1 = strk_groups::cut_piece(p0, L, cost, budget, max_items, off, &used);
                    int64_t sum = 0;
                    bool good = p1 > p0 && p1 <= L && p1 - p0 <= max_items && off.size() == p1 - p0;
                    for (size_t l = p0; good && l < p1; ++l) {
                        good = off[l - p0] == sum;
                        sum += cost(l);
                    }
                    good = good && used == sum && (p1 - p0 == 1 || used <= budget);
                    if (!good) { fprintf(stderr, "FAILED piece at %zu\n", p0); ++g_failed; }
                    p0 = p1;
                    ++pieces;
                }
            }
        calls += 3;
    }
    Call c = make(rng, 6, 12, 3);
    while (c.read_off.back() < 6 || c.base.empty()) c = make(rng, 6, 12, 3);
    Call t = c;
    t.snv_off[1] = t.snv_off[0] + 65;
    for (size_t l = 2; l < t.snv_off.size(); ++l) t.snv_off[l] = std::max(t.snv_off[l], t.snv_off[1]);
    t.base.assign((size_t)65 * 2000, 'A');
    t.qual.assign((size_t)65 * 2000, 40);
    expect(t, false, "65 SNVs", "SNVs (at most 64)");
    t = c;
    for (size_t l = 1; l < t.read_off.size(); ++l) t.read_off[l] += 1025;
    t.cn.resize((size_t)t.read_off.back(), 3);
    t.w.resize((size_t)t.read_off.back(), 1.0);
    t.hp.resize((size_t)t.read_off.back(), -1);
    t.ps.resize((size_t)t.read_off.back(), -1);
    expect(t, false, "1 025+ reads", "reads (at most 1024)");
    t = c;
    t.ps.clear();
    {
        const strk_phase_check::Limits lim{1024, 64, 1024, 15};
        std::vector<int64_t> cell_off;
        strk_groups::Message m;
        strk_phase_check::Input in = t.input();
        in.ps = nullptr;
        if (strk_phase_check::check(in, lim, cell_off, &m) != strk_groups::kInvalid || !strstr(m.text, "hp and ps")) {
            fprintf(stderr, "FAILED hp without ps\n");
            ++g_failed;
        }
        ++g_refusals;
    }
    t = c;
    t.base.pop_back();
    t.qual.pop_back();
    expect(t, false, "short cell buffer", "cells");
    t = c;
    t.w[t.w.size() / 2] = 0.0;
    expect(t, false, "zero weight", "weight");
    t = c;
    t.w[0] = std::numeric_limits<double>::quiet_NaN();
    expect(t, false, "NaN weight", "weight");
    t = c;
    t.w.back() = -1.0;
    expect(t, false, "negative weight", "weight");
    t = c;
    t.n_alleles[2] = 3;
    expect(t, false, "three alleles", "n_alleles");
    t = c;
    t.read_off[3] = t.read_off[2] - 1;
    expect(t, false, "decreasing read_off", "decreasing");
    t = c;
    t.p.min_allele_reads = 0;   // only a group's call needs it: the plain checker takes it
    expect(t, false, "min_allele_reads 0", "min_allele_reads");
    expect_plain(t, true, "min_allele_reads 0");
    t = c;
    t.p.num_bootstrap = 1025;
    expect(t, false, "1 025 bootstraps", "num_bootstrap");
    t = c;
    t.pp.snv_quality_threshold = 256;
    expect(t, false, "quality threshold 256", "snv_quality_threshold");
    t = c;
    t.pp.piece_loci = -1;
    expect(t, false, "negative piece", "piece_loci");
    // strk_call_alleles: the refusals of tests/test_gpu_alleles.py::test_invalid_input_is_rejected_before_any_launch
    const double nan = std::numeric_limits<double>::quiet_NaN();
    expect_plain(plain_call(), true, "valid call");
    expect_plain(plain_call(65535), true, "65 535 reads");
    expect_plain(plain_call(65536), false, "65 536 reads", "locus 0: 65536 reads (at most 65535)");
    for (auto [l, n_alleles, needle] : {std::tuple{1, 3, "locus 1: n_alleles 3"}, std::tuple{0, 0, "locus 0: n_alleles 0"}}) {
        t = plain_call();
        t.n_alleles[l] = n_alleles;
        expect_plain(t, false, "n_alleles", needle);
    }
    for (auto [r, weight, needle] : {std::tuple{7, 0.0, "locus 1: read 7"}, std::tuple{2, nan, "locus 0: read 2"}, std::tuple{6, -1.0, "locus 1: read 6"}}) {
        t = plain_call();
        t.w[r] = weight;
        expect_plain(t, false, "weight", needle);
    }
    for (int b : {1, 1025}) {
        t = plain_call();
        t.p.num_bootstrap = b;
        expect_plain(t, false, "num_bootstrap", "num_bootstrap");
    }
    for (int n : {0, 16}) {
        t = plain_call();
        t.p.n_init = n;
        expect_plain(t, false, "n_init", "n_init");
    }
    t = plain_call();
    t.p.reg_covar = 0.0;
    expect_plain(t, false, "reg_covar 0", "reg_covar");
    printf("phase_asan: %ld valid calls, %ld pieces, %d refusals, %d failed\n", calls, pieces, g_refusals, g_failed);
    return g_failed ? 1 : 0;
}
