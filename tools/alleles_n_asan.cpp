// Host-only driver of strk_alleles_check.h under the limits of strk_call_alleles_n: random valid calls of one to six alleles
// per locus and every refusal, on arrays of exactly their length, so that a sanitizer build sees any read beyond them.
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=all -o alleles_n_check tools/alleles_n_asan.cpp && ./alleles_n_check
// Counts its own failures; prints "<checks> checks, <n> failed" and exits 0 without one.
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

#include "../strkit_amd/csrc/strk_alleles_check.h"

namespace {

int g_checks = 0, g_failed = 0;

void expect(bool ok, const char* what) {
    ++g_checks;
    if (!ok) {
        ++g_failed;
        std::printf("FAILED: %s\n", what);
    }
}

struct Call {
    std::vector<int32_t> read_off, cn, n_alleles;
    std::vector<double> w;
    std::vector<uint64_t> seed;
    strk_allele_params p;
    strk_alleles_check::Input input() const {
        return {(int32_t)n_alleles.size(), read_off.data(), cn.data(), w.data(), n_alleles.data(), seed.data(), &p};
    }
};

strk_allele_params defaults() {
    strk_allele_params p{};
    p.min_reads = 4;
    p.min_allele_reads = 2;
    p.num_bootstrap = 100;
    p.n_init = 3;
    p.max_iter = 100;
    p.filter_factor = 3;
    p.tol = 1e-3;
    p.reg_covar = 1e-6;
    p.expansion_ratio = 5.0;
    return p;
}

Call random_call(std::mt19937& rng, int n_loci) {
    Call c;
    c.p = defaults();
    c.read_off.push_back(0);
    for (int l = 0; l < n_loci; ++l) {
        const int n = (int)(rng() % 40);
        for (int r = 0; r < n; ++r) {
            c.cn.push_back((int32_t)(rng() % 100));
            c.w.push_back(1e-9 + (double)(rng() % 1000));
        }
        c.read_off.push_back((int32_t)c.cn.size());
        c.n_alleles.push_back(1 + (int32_t)(rng() % 6));
        c.seed.push_back(rng());
    }
    if (c.cn.empty()) {   // (data() of an empty vector may be NULL, which the check refuses for a call with loci)
        c.cn.reserve(1);
        c.w.reserve(1);
    }
    return c;
}

const strk_alleles_check::Limits kLim{65535, 1024, 15, 6};

int check(const Call& c, strk_groups::Message* m, int max_alleles = 6) {
    return strk_alleles_check::check(c.input(), {kLim.max_reads, kLim.max_bootstrap, kLim.max_init, max_alleles}, m);
}

bool refused(const Call& c, const char* word) {
    strk_groups::Message m;
    m.text[0] = 0;
    const int rc = check(c, &m);
    const bool ok = rc == strk_groups::kInvalid && std::strstr(m.text, word) != nullptr;
    if (!ok) std::printf("  rc %d, message '%s', wanted '%s'\n", rc, m.text, word);
    return ok;
}

}  // namespace

int main() {
    std::mt19937 rng(20261019);
    strk_groups::Message m;
    for (int t = 0; t < 300; ++t) {
        const Call c = random_call(rng, 1 + (int)(rng() % 30));
        expect(check(c, &m) == 0, "a valid call is accepted");
    }
    {   // no loci: valid whatever the arrays are, but not without parameters
        Call c = random_call(rng, 3);
        strk_alleles_check::Input in = c.input();
        in.n_loci = 0;
        in.read_off = nullptr;
        in.cn = nullptr;
        expect(strk_alleles_check::check(in, kLim, &m) == 0, "a call of no loci is valid");
        in.p = nullptr;
        expect(strk_alleles_check::check(in, kLim, &m) == strk_groups::kInvalid && std::strstr(m.text, "params"), "params NULL");
        in = c.input();
        in.n_loci = -1;
        expect(strk_alleles_check::check(in, kLim, &m) == strk_groups::kInvalid, "n_loci < 0");
        in = c.input();
        in.seed = nullptr;
        expect(strk_alleles_check::check(in, kLim, &m) == strk_groups::kInvalid && std::strstr(m.text, "NULL"), "NULL argument");
    }
    for (int t = 0; t < 100; ++t) {
        const int n_loci = 2 + (int)(rng() % 20);
        const int l = (int)(rng() % n_loci);
        char word[64];
        {
            Call c = random_call(rng, n_loci);
            const int bad = (t % 2) ? 7 + (int)(rng() % 100) : -(int)(rng() % 5);
            c.n_alleles[l] = bad;
            std::snprintf(word, sizeof word, "locus %d: n_alleles %d is outside 1..6", l, bad);
            expect(refused(c, word), "a count outside 1..6 is refused by locus and value");
            c.n_alleles[l] = 3;
            expect(check(c, &m, 2) == strk_groups::kInvalid, "max_alleles is the limit");
        }
        {
            Call c = random_call(rng, n_loci);
            if (c.read_off[l + 1] > c.read_off[l]) {
                const int r = c.read_off[l] + (int)(rng() % (c.read_off[l + 1] - c.read_off[l]));
                const double bads[] = {0.0, -1.0, NAN, INFINITY};
                c.w[r] = bads[t % 4];
                std::snprintf(word, sizeof word, "locus %d: read %d has weight", l, r);
                expect(refused(c, word), "a weight that is not finite and > 0 is refused");
            }
        }
        {
            Call c = random_call(rng, n_loci);
            if (c.read_off[l + 1] > c.read_off[l] + 1 && l + 1 < n_loci) {
                std::swap(c.read_off[l], c.read_off[l + 1]);
                if (l == 0) {
                    expect(refused(c, "read_off[0] must be 0"), "read_off[0]");
                } else {
                    std::snprintf(word, sizeof word, "locus %d: read_off is decreasing", l);
                    // the locus in front grew: it is named only if it now exceeds nothing; accept either locus's refusal
                    strk_groups::Message mm;
                    expect(check(c, &mm) == strk_groups::kInvalid, "decreasing read_off is refused");
                }
            }
        }
    }
    {   // the parameters: the refusals of strk_alleles_check, in its words
        struct { const char* word; void (*edit)(strk_allele_params&); } cases[] = {
            {"num_bootstrap", [](strk_allele_params& p) { p.num_bootstrap = 1; }},
            {"num_bootstrap", [](strk_allele_params& p) { p.num_bootstrap = 1025; }},
            {"n_init", [](strk_allele_params& p) { p.n_init = 0; }},
            {"n_init", [](strk_allele_params& p) { p.n_init = 16; }},
            {"min_reads", [](strk_allele_params& p) { p.min_reads = 0; }},
            {"max_iter", [](strk_allele_params& p) { p.max_iter = 0; }},
            {"filter_factor", [](strk_allele_params& p) { p.filter_factor = 0; }},
            {"reg_covar", [](strk_allele_params& p) { p.reg_covar = 0.0; }},
            {"tol", [](strk_allele_params& p) { p.tol = -1.0; }},
            {"expansion_ratio", [](strk_allele_params& p) { p.expansion_ratio = NAN; }},
        };
        for (auto& k : cases) {
            Call c = random_call(rng, 4);
            k.edit(c.p);
            expect(refused(c, k.word), k.word);
        }
    }
    {   // too many reads in one locus
        Call c = random_call(rng, 2);
        c.read_off = {0, 3, 3 + 65536};
        c.cn.assign(3 + 65536, 7);
        c.w.assign(3 + 65536, 1.0);
        expect(refused(c, "locus 1: 65536 reads"), "more reads than the count rows hold");
    }
    std::printf("%d checks, %d failed\n", g_checks, g_failed);
    return g_failed ? 1 : 0;
}
