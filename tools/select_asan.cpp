// The host side of read selection (strk_select.h: the input checker, the record pre-pass and the host rule) over a seeded corpus
// of records and over truncated and hostile streams: offsets in mid-record, past the end and negative, a stream cut inside a
// record, a name length that runs past its record, a block size of garbage.  Every stream is a heap block of exactly its
// length, so a read one byte past it is reported under AddressSanitizer / UBSan (tools/select_asan.sh); tests/
// test_select_tool.py builds it plain and requires exit 0.  The rule's results are compared with a map-and-loop statement of it,
// written here.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <map>
#include <random>
#include <set>
#include <string>
#include <vector>
#include "../strkit_amd/csrc/strk_select.h"

namespace {

int g_failed = 0, g_checks = 0, g_refusals = 0;

void expect(bool ok, const char* what, long long detail = 0) {
    ++g_checks;
    if (!ok) {
        fprintf(stderr, "FAILED %s (%lld)\n", what, detail);
        ++g_failed;
    }
}

void put32(std::vector<uint8_t>& v, uint32_t x) { for (int k = 0; k < 4; ++k) v.push_back((uint8_t)(x >> (8 * k))); }
void put16(std::vector<uint8_t>& v, uint32_t x) { for (int k = 0; k < 2; ++k) v.push_back((uint8_t)(x >> (8 * k))); }

// one record with its block_size appended to `s`: `name` as raw bytes, a <l_seq>M CIGAR; returns its offset
int64_t add_record(std::vector<uint8_t>& s, const std::string& name, uint32_t flag, uint32_t l_seq, int l_name_override = -1) {
    const int64_t off = (int64_t)s.size();
    std::vector<uint8_t> b;
    put32(b, 0); put32(b, 100);
    b.push_back((uint8_t)(l_name_override >= 0 ? l_name_override : (int)name.size() + 1)); b.push_back(60); put16(b, 4681);
    put16(b, 1); put16(b, flag);
    put32(b, l_seq); put32(b, 0xffffffffu); put32(b, 0xffffffffu); put32(b, 0);
    b.insert(b.end(), name.begin(), name.end()); b.push_back(0);
    put32(b, l_seq << 4);
    for (uint32_t i = 0; i < (l_seq + 1) / 2; ++i) b.push_back(0x12);
    for (uint32_t i = 0; i < l_seq; ++i) b.push_back(30);
    put32(s, (uint32_t)b.size());
    s.insert(s.end(), b.begin(), b.end());
    return off;
}

struct Heap {   // the stream as a heap block of exactly its length
    uint8_t* p;
    int64_t n;
    explicit Heap(const std::vector<uint8_t>& v, int64_t cut = -1) : n(cut >= 0 ? cut : (int64_t)v.size()) { p = new uint8_t[(size_t)n + 1] + 1; memcpy(p, v.data(), (size_t)n); }
    ~Heap() { delete[] (p - 1); }   // (offset by one: the records then lie at odd addresses)
};

// 0, -1 (refused by the checker) or -2 - item (a record refused); fills the outputs when 0
int run(const Heap& h, const std::vector<int64_t>& item_off, const std::vector<int64_t>& rec_off, int rules, int max_reads,
        std::vector<uint8_t>* reason, std::vector<uint8_t>* status, std::vector<int32_t>* kept) {
    const strk_sel::Input in{h.n, (int32_t)item_off.size() - 1, item_off.data(), rec_off.data(), rules, max_reads};
    strk_groups::Message msg;
    if (strk_sel::check_input(in, &msg)) return -1;
    const int64_t n = item_off.back();
    const int64_t bad = strk_sel::host_first_bad(h.p, in, 0, n);
    if (bad >= 0) return (int)(-2 - bad);
    reason->assign((size_t)n + 1, 0xEE); status->assign((size_t)n + 1, 0xEE); kept->assign(item_off.size(), -7);
    strk_sel::HostTable t;
    for (int32_t l = 0; l < in.n_loci; ++l) strk_sel::host_locus(h.p, in, l, t, reason->data(), status->data(), kept->data());
    expect((*reason)[(size_t)n] == 0xEE && (*status)[(size_t)n] == 0xEE && kept->back() == -7, "nothing is written behind the outputs");
    return 0;
}

void corpus(std::mt19937& rng) {
    // names: random bytes of every length class around the compare step, twins, prefixes, one name for a whole locus
    std::vector<std::string> names = {"", "a", std::string(254, 'q')};
    for (int n = 1; n <= 2 * strk_sel::kCmpStep + 1; ++n) {
        std::string s((size_t)n, 'A');
        for (auto& ch : s) ch = (char)(1 + rng() % 255);
        names.push_back(s);
        std::string t = s; t.back() = (char)(t.back() == 1 ? 2 : 1); names.push_back(t);
        std::string u = s; u.front() = (char)(u.front() == 1 ? 2 : 1); names.push_back(u);
        names.push_back(s + "x");
    }
    const uint32_t flags[] = {0, 16, 0x100, 0x800, 0x900, 0x110};
    std::vector<uint8_t> s(13, 0);   // a header of odd length in front
    std::vector<int64_t> offs;
    std::vector<std::pair<std::string, uint32_t>> recs;
    for (int i = 0; i < 1500; ++i) {
        const std::string& nm = i % 5 == 4 ? names[0 + rng() % 3] : names[rng() % names.size()];
        const uint32_t f = flags[rng() % 6];
        offs.push_back(add_record(s, nm, f, 1 + rng() % 10));
        recs.push_back({nm, f});
    }
    const Heap h(s);
    for (int round = 0; round < 60; ++round) {
        std::vector<int64_t> item_off = {0}, rec_off;
        std::vector<int> which;
        const int n_loci = 1 + (int)(rng() % 5);
        for (int l = 0; l < n_loci; ++l) {
            const int sizes[] = {0, 1, 2, 63, 64, 65, 257, 700};
            int n = sizes[rng() % 8], i = (int)(rng() % 200);
            for (int k = 0; k < n && i < 1500; ++k, i += 1 + (int)(rng() % 2)) { rec_off.push_back(offs[(size_t)i]); which.push_back(i); }
            item_off.push_back((int64_t)rec_off.size());
        }
        for (int rules = 0; rules < 8; ++rules) {
            const int caps[] = {1, 3, 250, INT32_MAX};
            const int cap = caps[rng() % 4];
            std::vector<uint8_t> reason, status;
            std::vector<int32_t> kept;
            expect(run(h, item_off, rec_off, rules, cap, &reason, &status, &kept) == 0, "a good call", round);
            for (int l = 0; l < n_loci; ++l) {      // the rule, with a map and a set
                std::map<std::string, int> st;
                for (int64_t i = item_off[(size_t)l]; i < item_off[(size_t)l + 1]; ++i) st[recs[(size_t)which[(size_t)i]].first] |= recs[(size_t)which[(size_t)i]].second & 0x800 ? 2 : 1;
                std::set<std::string> seen;
                int64_t survivors = 0;
                for (int64_t i = item_off[(size_t)l]; i < item_off[(size_t)l + 1]; ++i) {
                    const auto& r = recs[(size_t)which[(size_t)i]];
                    int why = 0;
                    if ((rules & 1) && (r.second & 0x800)) why = 1;
                    else if ((rules & 2) && (r.second & 0x100)) why = 2;
                    else if ((rules & 4) && seen.count(r.first)) why = 3;
                    else if (survivors++ >= cap) why = 4;
                    if (why != 1 && why != 2) seen.insert(r.first);
                    expect(reason[(size_t)i] == why && status[(size_t)i] == st[r.first], "reason and status of an item", i);
                }
                expect(kept[(size_t)l] == (survivors < cap ? survivors : cap), "the number kept", l);
            }
        }
    }
}

void hostile(std::mt19937& rng) {
    std::vector<uint8_t> s;
    std::vector<int64_t> offs;
    for (int i = 0; i < 8; ++i) offs.push_back(add_record(s, "read" + std::to_string(i % 3), i % 2 ? 0x800 : 0, 5));
    const int64_t end = (int64_t)s.size();
    std::vector<uint8_t> reason, status;
    std::vector<int32_t> kept;
    const std::vector<int64_t> item_off = {0, 4, 8};
    {
        const Heap h(s);
        expect(run(h, item_off, offs, 7, 250, &reason, &status, &kept) == 0, "the good stream");
        auto refused = [&](int item, int64_t off, int want, const char* what) {
            ++g_refusals;
            std::vector<int64_t> o = offs;
            o[(size_t)item] = off;
            expect(run(h, item_off, o, 7, 250, &reason, &status, &kept) == want, what, off);
        };
        for (int64_t d = 1; d < 40; ++d) refused(5, offs[5] + d, d + offs[5] > end - strk_sel::kFixed ? -1 : -2 - 5, "an offset in mid-record");
        refused(2, -1, -1, "a negative offset");
        refused(2, INT64_MIN, -1, "the most negative offset");
        refused(2, end, -1, "the end of the stream");
        refused(2, end - 35, -1, "no room for the fixed part");
        refused(2, INT64_MAX, -1, "an offset that wraps");
        for (int round = 0; round < 2000; ++round) {     // any offset at all: refused or a record start, never a read outside
            const int64_t off = (int64_t)(rng() % (uint64_t)(end + 64)) - 32;
            std::vector<int64_t> o = offs;
            o[3] = off;
            const int rc = run(h, item_off, o, (int)(rng() % 8), 2, &reason, &status, &kept);
            bool start = false;
            for (int64_t x : offs) start = start || x == off;
            expect(start ? rc == 0 : rc < 0, "a random offset", off);
        }
        auto bad_args = [&](std::vector<int64_t> io, int rules, int cap, const char* what) {
            ++g_refusals;
            expect(run(h, io, offs, rules, cap, &reason, &status, &kept) == -1, what);
        };
        bad_args({0, 5, 4}, 7, 250, "item_off descends");
        bad_args({1, 4, 8}, 7, 250, "item_off does not start at 0");
        bad_args(item_off, 8, 250, "rules 8");
        bad_args(item_off, -1, 250, "rules -1");
        bad_args(item_off, 7, 0, "max_reads 0");
        bad_args(item_off, 7, -5, "max_reads < 0");
    }
    for (int64_t cut = 0; cut < end; ++cut) {            // the stream cut anywhere: the records that are whole still answer
        const Heap h(s, cut);
        int n_whole = 0;
        while (n_whole < 8 && (n_whole == 7 ? end : offs[(size_t)n_whole + 1]) <= cut) ++n_whole;
        const int rc = run(h, item_off, offs, 7, 250, &reason, &status, &kept);
        expect(rc != 0 && (rc == -1 || rc == -2 - n_whole), "a truncated stream", cut);
        ++g_refusals;
    }
    {   // a name length that runs past its record, a block size of garbage
        std::vector<uint8_t> t;
        const int64_t a = add_record(t, "ok", 0, 4), b = add_record(t, "x", 0, 0, 255), c = add_record(t, "tail", 0, 3);
        const Heap h(t);
        expect(run(h, {0, 2}, {a, c}, 4, 250, &reason, &status, &kept) == 0, "two good records around a bad one");
        expect(run(h, {0, 3}, {a, b, c}, 4, 250, &reason, &status, &kept) == -2 - 1, "a name longer than its record");
        std::vector<uint8_t> u = t;
        const uint32_t huge = 0x7fffffffu;
        memcpy(u.data() + c, &huge, 4);
        const Heap h2(u);
        expect(run(h2, {0, 2}, {a, c}, 4, 250, &reason, &status, &kept) == -2 - 1, "a block size past the stream");
        const uint32_t neg = 0xfffffff0u;
        memcpy(u.data() + c, &neg, 4);
        const Heap h3(u);
        expect(run(h3, {0, 2}, {a, c}, 4, 250, &reason, &status, &kept) == -2 - 1, "a negative block size");
        g_refusals += 3;
    }
}

}  // namespace

int main() {
    std::mt19937 rng(20261020);
    corpus(rng);
    hostile(rng);
    printf("select: %d checks, %d refusals, %d failed\n", g_checks, g_refusals, g_failed);
    return g_failed ? 1 : 0;
}
