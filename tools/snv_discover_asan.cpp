// The host side of the SNV discovery (strk_snv_discover.h: the per-base test, the window and tile geometry, the span of an
// alignment, the input checker, the nearest-1 024 rule and the host twin of the pileup) over built-in records, well-formed and
// hostile: a CIGAR longer than its bases, a record cut off inside its fixed part, an offset that is no record start.  Every
// buffer is a heap block of exactly its length, so a read one byte past a record or one element past an array is reported under
// AddressSanitizer / UBSan (g++ -fsanitize=address,undefined, as tools/phase_inputs_asan.sh does for its program);
// tests/test_snv_discover_tool.py builds it plain and requires exit 0.  The candidates are compared with a base-by-base
// pileup written here.
#include <cstdint>
#include <cstdio>
#include <array>
#include <cstring>
#include <map>
#include <random>
#include <vector>
#include "../strkit_amd/csrc/strk_snv_discover.h"

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

struct Read {
    int32_t pos;
    std::vector<uint32_t> cigar;
    std::vector<uint8_t> nib, qual;   // one code / quality per base
    bool has_qual;
};

std::vector<uint8_t> record(const Read& r) {
    std::vector<uint8_t> b;
    const uint32_t l_seq = (uint32_t)r.nib.size();
    put32(b, 0);
    put32(b, 0); put32(b, (uint32_t)r.pos);
    b.push_back(2); b.push_back(60); put16(b, 4680);
    put16(b, (uint32_t)r.cigar.size()); put16(b, 0);
    put32(b, l_seq); put32(b, 0xffffffffu); put32(b, 0xffffffffu); put32(b, 0);
    b.push_back('r'); b.push_back(0);
    for (uint32_t c : r.cigar) put32(b, c);
    for (uint32_t i = 0; i < l_seq; i += 2) b.push_back((uint8_t)((r.nib[i] << 4) | (i + 1 < l_seq ? r.nib[i + 1] : 0)));
    for (uint32_t i = 0; i < l_seq; ++i) b.push_back(r.has_qual ? r.qual[i] : 0xFF);
    const uint32_t block = (uint32_t)b.size() - 4;
    memcpy(b.data(), &block, 4);
    return b;
}

Read random_read(std::mt19937& rng, int32_t around) {
    Read r;
    r.pos = around - 400 + (int32_t)(rng() % 300);
    const int n_ops = 1 + (int)(rng() % 90);
    const uint32_t clips[] = {3, 99, 100, 300};
    for (int i = 0; i < n_ops; ++i) {
        uint32_t op = (i % 2 == 0) ? 0u : (uint32_t)(rng() % 9), len = rng() % 20 == 0 ? 0u : 1u + rng() % (n_ops < 8 ? 300 : 30);
        if ((i == 0 || i == n_ops - 1) && rng() % 2) { op = 4; len = clips[rng() % 4]; }
        else if (op == 4) op = 0;
        r.cigar.push_back((len << 4) | op);
    }
    uint32_t n_q = 0;
    for (uint32_t c : r.cigar)
        if (strk_fe::consumes_query(c & 15u)) n_q += c >> 4;
    if (rng() % 8 == 0 && n_q > 4) n_q -= 3;            // a CIGAR longer than its sequence
    r.has_qual = rng() % 6 != 0;
    const uint8_t acgt[] = {1, 2, 4, 8};
    for (uint32_t i = 0; i < n_q; ++i) {
        r.nib.push_back(rng() % 10 == 0 ? (uint8_t)(rng() % 16) : acgt[rng() % 2 + 2 * (i % 2)]);   // (two bases a position: sites everywhere)
        r.qual.push_back((uint8_t)(10 + rng() % 25));
    }
    return r;
}

// base by base: the counts of a read at every reference position it counts at
void pile(const Read& r, int32_t clip_threshold, int32_t take_in, int32_t mbq, std::map<int64_t, std::array<int, 4>>* counts) {
    int64_t ref = r.pos, q = 0, s = -1, e = -1;
    std::map<int64_t, int> slot_at;
    for (uint32_t c : r.cigar) {
        const uint32_t op = c & 15u, len = c >> 4;
        for (uint32_t k = 0; k < len; ++k) {
            if (strk_fe::is_aligned(op)) {
                if (s < 0) s = ref;
                e = ref + 1;
                if (q < (int64_t)r.nib.size()) {
                    const uint8_t code = r.nib[(size_t)q];
                    const int slot = code == 1 ? 0 : code == 2 ? 1 : code == 4 ? 2 : code == 8 ? 3 : -1;
                    if (slot >= 0 && (!r.has_qual || r.qual[(size_t)q] >= mbq)) slot_at[ref] = slot;
                }
            }
            if (strk_fe::consumes_ref(op)) ++ref;
            if (strk_fe::consumes_query(op)) ++q;
        }
    }
    if (s < 0) return;
    const size_t n = r.cigar.size();
    const int64_t cl = (r.cigar[0] & 15u) == 4 ? r.cigar[0] >> 4 : 0, cr = (r.cigar[n - 1] & 15u) == 4 ? r.cigar[n - 1] >> 4 : 0;
    const int64_t lo = s + (cl >= clip_threshold ? take_in : 0), hi = e - (cr >= clip_threshold ? take_in : 0);
    for (const auto& kv : slot_at)
        if (kv.first >= lo && kv.first < hi) ++(*counts)[kv.first][kv.second];
}

struct Call {
    std::vector<uint8_t> buf;
    std::vector<int64_t> rec_off, left, right;
    std::vector<int32_t> item_locus, kept_off, kept_item;
    strk_sd::DiscoverInput in(int32_t window, int32_t mbq, int32_t mar) const {
        return strk_sd::DiscoverInput{(int64_t)buf.size(), (int32_t)rec_off.size(), rec_off.data(), item_locus.data(), (int32_t)left.size(), left.data(),
                                      right.data(), kept_off.data(), kept_item.data(), {nullptr, nullptr, nullptr}, 100, 250, window, mbq, mar};
    }
};

Call one_locus(const std::vector<std::vector<uint8_t>>& recs, int64_t left, int64_t right) {
    Call c;
    std::vector<uint8_t> buf;
    for (const auto& r : recs) { c.rec_off.push_back((int64_t)buf.size()); buf.insert(buf.end(), r.begin(), r.end()); }
    c.buf.assign(buf.begin(), buf.end());
    c.buf.shrink_to_fit();
    c.left = {left}; c.right = {right};
    c.item_locus.assign(recs.size(), 0);
    c.kept_off = {0, (int32_t)recs.size()};
    for (size_t i = 0; i < recs.size(); ++i) c.kept_item.push_back((int32_t)i);
    return c;
}

void well_formed(std::mt19937& rng) {
    for (int round = 0; round < 200; ++round) {
        const int64_t left = 1000 + (int64_t)(rng() % 50), right = left + 20;
        const int32_t window = round % 3 == 0 ? 5000 : (round % 3 == 1 ? 300 : 4096), mbq = (int32_t)(rng() % 30), mar = 1 + (int32_t)(rng() % 3);
        std::vector<Read> reads;
        std::vector<std::vector<uint8_t>> recs;
        for (unsigned k = 2 + rng() % 12; k > 0; --k) { reads.push_back(random_read(rng, (int32_t)left)); recs.push_back(record(reads.back())); }
        const Call c = one_locus(recs, left, right);
        const strk_sd::DiscoverInput in = c.in(window, mbq, mar);
        strk_groups::Message m;
        expect(strk_sd::check_discover(in, &m) == 0, "a valid call is accepted", round);
        expect(strk_sd::host_first_bad(c.buf.data(), in, 0, in.n_items) == -1, "well-formed records parse", round);
        std::vector<uint32_t> scratch;
        std::vector<int64_t> got, want;
        strk_sd::host_discover_locus(c.buf.data(), in, 0, scratch, got);
        std::map<int64_t, std::array<int, 4>> counts;
        for (const Read& r : reads) pile(r, 100, 250, mbq, &counts);
        int32_t a_thr, t_thr;
        strk_pi::thresholds((int32_t)reads.size(), mar, &a_thr, &t_thr);
        for (const auto& kv : counts) {
            const int64_t p = kv.first;
            if (p < 0 || !((p >= left - window && p < left) || (p >= right && p < right + window))) continue;
            int n = 0;
            for (int k = 0; k < 4; ++k) n += kv.second[k] >= a_thr;
            if (n >= 2) want.push_back(p);
        }
        strk_sd::keep_nearest(want, left, right, (size_t)strk_pi::kMaxCand);
        expect(got == want, "candidates of random reads", round);
        // the span of every alignment against the same expansion
        for (size_t i = 0; i < reads.size(); ++i) {
            int64_t lo = 0, hi = 0;
            std::vector<uint8_t> cig;
            for (uint32_t x : reads[i].cigar) put32(cig, x);
            std::vector<uint8_t> exact(cig);
            const bool found = strk_sd::alignment_span(exact.data(), (int32_t)reads[i].cigar.size(), reads[i].pos, 100, 250, &lo, &hi);
            int64_t ref = reads[i].pos, s = -1, e = -1;
            for (uint32_t x : reads[i].cigar) {
                if (strk_fe::is_aligned(x & 15u) && (x >> 4) > 0) { if (s < 0) s = ref; e = ref + (x >> 4); }
                if (strk_fe::consumes_ref(x & 15u)) ref += x >> 4;
            }
            expect(found == (s >= 0), "span found", round);
            if (found) {
                const size_t n = reads[i].cigar.size();
                const int64_t cl = (reads[i].cigar[0] & 15u) == 4 ? reads[i].cigar[0] >> 4 : 0, cr = (reads[i].cigar[n - 1] & 15u) == 4 ? reads[i].cigar[n - 1] >> 4 : 0;
                expect(lo == s + (cl >= 100 ? 250 : 0) && hi == e - (cr >= 100 ? 250 : 0), "span", round);
            }
        }
    }
}

void geometry_and_nearest() {
    int64_t t0, c0, t1;
    strk_sd::tile_range(10000, 10060, 5000, 0, 0, &t0, &c0, &t1); expect(t0 == 5000 && c0 == 5000 && t1 == 9096, "left tile 0 of 5000");
    strk_sd::tile_range(10000, 10060, 5000, 0, 1, &t0, &c0, &t1); expect(t0 == 9096 && t1 == 10000, "left tile 1 of 5000: 904 positions");
    strk_sd::tile_range(10000, 10060, 8192, 1, 1, &t0, &c0, &t1); expect(t0 == 10060 + 4096 && t1 == 10060 + 8192, "right tile 1 of 8192");
    strk_sd::tile_range(3000, 3060, 8192, 0, 0, &t0, &c0, &t1); expect(t0 == -5192 && c0 == 0 && t1 == -1096, "a tile in front of the contig counts nothing");
    strk_sd::tile_range(3000, 3060, 8192, 0, 1, &t0, &c0, &t1); expect(t0 == -1096 && c0 == 0 && t1 == 3000, "a window cut at 0");
    expect(strk_sd::tiles_per_side(1) == 1 && strk_sd::tiles_per_side(4096) == 1 && strk_sd::tiles_per_side(4097) == 2 && strk_sd::tiles_per_side(65536) == 16, "tiles per side");
    expect(strk_sd::is_candidate(0x0000000200000002ull, 2) && !strk_sd::is_candidate(0x0000000100000002ull, 2) && strk_sd::is_candidate(0xffff000000000005ull, 5) &&
           !strk_sd::is_candidate(0xffffull, 1), "two of four counts");
    // 1 101 positions: distance 1 on the left, every even distance up to 1 100 on both sides; the last place goes to the left one of a pair
    std::vector<int64_t> c;
    const int64_t left = 50000, right = 50060;
    for (int64_t d = 1100; d >= 2; d -= 2) c.push_back(left - d);
    c.push_back(left - 1);
    for (int64_t d = 2; d <= 1100; d += 2) c.push_back(right - 1 + d);
    strk_sd::keep_nearest(c, left, right, 1024);
    expect(c.size() == 1024 && c.front() == left - 1024 && c.back() == right - 1 + 1022, "nearest 1 024, the tie to the left", (long long)c.size());
    std::vector<int64_t> few = {1, 2, 90000};
    strk_sd::keep_nearest(few, left, right, 1024);
    expect(few.size() == 3, "fewer than the limit stay");
    std::vector<int64_t> only_right;
    for (int64_t d = 0; d < 2000; ++d) only_right.push_back(right + d);
    strk_sd::keep_nearest(only_right, left, right, 1024);
    expect(only_right.size() == 1024 && only_right.front() == right && only_right.back() == right + 1023, "one side alone");
}

void hostile() {
    Read good;
    good.pos = 100; good.cigar = {40u << 4}; good.nib.assign(40, 1); good.qual.assign(40, 30); good.has_qual = true;
    Read other = good;
    other.nib[5] = 2;
    {   // a CIGAR longer than its bases: the pairs without a base count nothing and nothing behind the record is read
        Read lng = good, lng2 = other;
        lng.cigar = {60u << 4}; lng2.cigar = {60u << 4};
        const Call c = one_locus({record(lng), record(lng2), record(lng), record(lng2)}, 200, 220);
        const strk_sd::DiscoverInput in = c.in(300, 20, 2);
        std::vector<uint32_t> scratch;
        std::vector<int64_t> got;
        strk_sd::host_discover_locus(c.buf.data(), in, 0, scratch, got);
        expect(got == std::vector<int64_t>{105}, "a CIGAR longer than its sequence", (long long)got.size());
    }
    {   // a record cut off inside its fixed part, as the last of the buffer
        std::vector<uint8_t> cut = record(good);
        cut.resize(20);
        const Call c = one_locus({record(good), cut}, 200, 220);
        expect(strk_sd::host_first_bad(c.buf.data(), c.in(300, 20, 2), 0, 2) == 1, "cut record refused");
        ++g_refusals;
    }
    {   // an offset that is no record start, and one whose four bytes end at the buffer's last byte
        Call c = one_locus({record(good), record(other), record(good)}, 200, 220);
        c.rec_off[1] += 2;
        expect(strk_sd::host_first_bad(c.buf.data(), c.in(300, 20, 2), 0, 3) == 1, "an offset inside a record refused");
        c.rec_off[1] = (int64_t)c.buf.size() - 4;
        strk_groups::Message m;
        expect(strk_sd::check_discover(c.in(300, 20, 2), &m) == 0 && strk_sd::host_first_bad(c.buf.data(), c.in(300, 20, 2), 0, 3) == 1, "the last four bytes are no record");
        g_refusals += 2;
    }
    {   // a block_size that claims more than the buffer holds
        std::vector<uint8_t> lie = record(good);
        const uint32_t big = 1u << 20;
        memcpy(lie.data(), &big, 4);
        const Call c = one_locus({lie}, 200, 220);
        expect(strk_sd::host_first_bad(c.buf.data(), c.in(300, 20, 2), 0, 1) == 0, "a block longer than the buffer refused");
        ++g_refusals;
    }
}

void checker() {
    Read good;
    good.pos = 100; good.cigar = {40u << 4}; good.nib.assign(40, 1); good.qual.assign(40, 30); good.has_qual = true;
    const Call ok = one_locus({record(good), record(good), record(good)}, 200, 220);
    auto refuse = [&](const strk_sd::DiscoverInput& in, const char* needle) {
        strk_groups::Message m;
        m.text[0] = 0;
        expect(strk_sd::check_discover(in, &m) == strk_groups::kInvalid && strstr(m.text, needle), needle);
        ++g_refusals;
    };
    const strk_sd::DiscoverInput base = ok.in(8192, 20, 2);
    { auto in = base; in.n_items = -1; refuse(in, "< 0"); }
    { auto in = base; in.n_bytes = -1; refuse(in, "< 0"); }
    { auto in = base; in.take_in = -1; refuse(in, ">= 0"); }
    { auto in = base; in.window = 0; refuse(in, "window"); }
    { auto in = base; in.window = strk_sd::kMaxWindow + 1; refuse(in, "window"); }
    { auto in = base; in.min_base_qual = 256; refuse(in, "min_base_qual"); }
    { auto in = base; in.min_base_qual = -1; refuse(in, "min_base_qual"); }
    { auto in = base; in.min_allele_reads = 0; refuse(in, "min_allele_reads"); }
    { auto in = base; in.left_coord = nullptr; refuse(in, "NULL"); }
    { auto in = base; in.rec_off = nullptr; refuse(in, "NULL"); }
    { auto in = base; std::vector<int64_t> l = {221}; in.left_coord = l.data(); refuse(in, "left_coord > right_coord"); }
    { auto in = base; std::vector<int64_t> r = {(int64_t)1 << 41}; in.right_coord = r.data(); refuse(in, "coordinate"); }
    { auto in = base; std::vector<int64_t> ro = {0, -1, 0}; in.rec_off = ro.data(); refuse(in, "item 1: rec_off"); }
    { auto in = base; std::vector<int64_t> ro = {0, 0, in.n_bytes - 3}; in.rec_off = ro.data(); refuse(in, "item 2: rec_off"); }
    { auto in = base; std::vector<int32_t> lc = {0, 1, 0}; in.item_locus = lc.data(); refuse(in, "item 1: item_locus"); }
    { auto in = base; std::vector<int32_t> ki = {0, 3, 1}; in.kept_item = ki.data(); refuse(in, "out of range"); }
    { auto in = base; std::vector<int32_t> ko = {1, 3}; in.kept_off = ko.data(); refuse(in, "start at 0"); }
    { auto in = base; std::vector<int32_t> ko = {0, -1}; in.kept_off = ko.data(); refuse(in, "decreasing"); }
    { auto in = base; in.kept_off = nullptr; refuse(in, "kept_off"); }
    { auto in = base; std::vector<uint32_t> ops = {16}; in.alt.ops = ops.data(); refuse(in, "both"); }
    {   // two loci: a kept read of the other locus; and 65 536 kept reads of one record
        auto in = base;
        std::vector<int64_t> l = {200, 900}, r = {220, 920};
        std::vector<int32_t> lc = {0, 0, 1}, ko = {0, 3, 3};
        in.n_loci = 2; in.left_coord = l.data(); in.right_coord = r.data(); in.item_locus = lc.data(); in.kept_off = ko.data();
        refuse(in, "belongs to locus");
    }
    {
        auto in = base;
        std::vector<int32_t> many((size_t)strk_sd::kMaxKept + 1, 0), ko = {0, strk_sd::kMaxKept + 1};
        in.kept_off = ko.data(); in.kept_item = many.data();
        refuse(in, "at most 65535");
        ko[1] = strk_sd::kMaxKept;
        strk_groups::Message m;
        expect(strk_sd::check_discover(in, &m) == 0, "65 535 kept reads are accepted");
    }
}

}  // namespace

int main() {
    std::mt19937 rng(20250117);
    well_formed(rng);
    geometry_and_nearest();
    hostile();
    checker();
    printf("snv discovery: %d checks, %d refusals, %d failed\n", g_checks, g_refusals, g_failed);
    return g_failed ? 1 : 0;
}
