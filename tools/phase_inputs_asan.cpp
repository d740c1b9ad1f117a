// The host side of the phased call's file inputs (strk_phase_inputs.h: the auxiliary-field walk, the cell walk, the choice of the
// useful SNVs and the two input checkers) over well-formed records and over hostile ones: a truncated auxiliary chain, a Z field
// without its NUL, a B count that overflows, a CG placeholder whose array is longer than the record.  Every buffer is a heap
// block of exactly its length, so a read one byte past a record or one element past an array is reported under
// AddressSanitizer / UBSan (tools/phase_inputs_asan.sh); tests/test_phase_inputs_tool.py builds it plain and requires exit 0.
// The cells are compared with a base-by-base expansion of the alignment written here, the tags with what was generated.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <map>
#include <random>
#include <string>
#include <vector>
#include "../strkit_amd/csrc/strk_phase_inputs.h"

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
void puts_(std::vector<uint8_t>& v, const char* s, size_t n) { v.insert(v.end(), s, s + n); }

struct Read {
    int32_t pos;
    std::vector<uint32_t> cigar;
    std::vector<uint8_t> nib, qual;   // one code / quality per base
    bool has_qual;
    std::vector<uint8_t> tags;
};

// the record with its block_size, nothing behind it
std::vector<uint8_t> record(const Read& r, bool placeholder = false) {
    std::vector<uint8_t> b;
    const uint32_t l_seq = (uint32_t)r.nib.size();
    std::vector<uint32_t> cig = r.cigar;
    std::vector<uint8_t> tags = r.tags;
    if (placeholder) {   // SAM 4.2.2: <l_seq>S<ref_len>N in the fixed field, the real CIGAR in CG:B,I
        uint32_t ref_len = 0;
        for (uint32_t c : r.cigar)
            if (strk_fe::consumes_ref(c & 15u)) ref_len += c >> 4;
        cig = {(l_seq << 4) | 4u, (ref_len << 4) | 3u};
        puts_(tags, "CGBI", 4);
        put32(tags, (uint32_t)r.cigar.size());
        for (uint32_t c : r.cigar) put32(tags, c);
    }
    put32(b, 0);                       // block_size, filled below
    put32(b, 0); put32(b, (uint32_t)r.pos);
    b.push_back(2); b.push_back(60); put16(b, 4680);
    put16(b, (uint32_t)cig.size()); put16(b, 0);
    put32(b, l_seq); put32(b, 0xffffffffu); put32(b, 0xffffffffu); put32(b, 0);
    b.push_back('r'); b.push_back(0);
    for (uint32_t c : cig) put32(b, c);
    for (uint32_t i = 0; i < l_seq; i += 2) b.push_back((uint8_t)((r.nib[i] << 4) | (i + 1 < l_seq ? r.nib[i + 1] : 0)));
    for (uint32_t i = 0; i < l_seq; ++i) b.push_back(r.has_qual ? r.qual[i] : 0xFF);
    b.insert(b.end(), tags.begin(), tags.end());
    const uint32_t block = (uint32_t)b.size() - 4;
    memcpy(b.data(), &block, 4);
    return b;
}

void int_tag(std::vector<uint8_t>& t, const char* name, char ty, int64_t v) {
    puts_(t, name, 2);
    t.push_back((uint8_t)ty);
    const int n = (ty == 'c' || ty == 'C') ? 1 : ((ty == 's' || ty == 'S') ? 2 : 4);
    for (int k = 0; k < n; ++k) t.push_back((uint8_t)((uint64_t)v >> (8 * k)));
}

void noise_tag(std::mt19937& rng, std::vector<uint8_t>& t) {
    switch (rng() % 4) {
        case 0: puts_(t, "RGZgroup", 8); t.push_back(0); break;
        case 1: { puts_(t, "ZBBs", 4); const uint32_t n = rng() % 5; put32(t, n); for (uint32_t k = 0; k < 2 * n; ++k) t.push_back((uint8_t)rng()); break; }
        case 2: puts_(t, "XAAq", 4); break;
        default: puts_(t, "XFf", 3); put32(t, 0x3fc00000u); break;
    }
}

Read random_read(std::mt19937& rng, int32_t* want_hp, int32_t* want_ps) {
    Read r;
    r.pos = 1000 + (int32_t)(rng() % 100);
    const int n_ops = (int)(rng() % 140);
    const uint32_t clips[] = {3, 99, 100, 300};
    for (int i = 0; i < n_ops; ++i) {
        uint32_t op = (i % 2 == 0) ? 0u : (uint32_t)(rng() % 9), len = rng() % 20 == 0 ? 0u : 1u + rng() % (n_ops < 8 ? 300 : 12);
        if ((i == 0 || i == n_ops - 1) && rng() % 2) { op = 4; len = clips[rng() % 4]; }
        else if (op == 4) op = 0;
        r.cigar.push_back((len << 4) | op);
    }
    uint32_t n_q = 0;
    for (uint32_t c : r.cigar)
        if (strk_fe::consumes_query(c & 15u)) n_q += c >> 4;
    if (rng() % 16 == 0 && n_q > 4) n_q -= 3;            // a CIGAR longer than its sequence
    r.has_qual = rng() % 8 != 0;
    for (uint32_t i = 0; i < n_q; ++i) {
        r.nib.push_back((uint8_t)(rng() % 16));
        r.qual.push_back((uint8_t)(rng() % 60));
    }
    *want_hp = *want_ps = -1;
    const char types[] = "cCsSiI";
    const int mode = (int)(rng() % 4);   // 0 none, 1 HP only, 2-3 both
    for (unsigned k = rng() % 3; k > 0; --k) noise_tag(rng, r.tags);
    int32_t hp = 1 + (int32_t)(rng() % 2), ps = (int32_t)(rng() % 100);
    if (mode >= 1) int_tag(r.tags, "HP", types[rng() % 6], hp);
    for (unsigned k = rng() % 2; k > 0; --k) noise_tag(rng, r.tags);
    if (mode >= 2) int_tag(r.tags, "PS", types[rng() % 6], ps);
    for (unsigned k = rng() % 2; k > 0; --k) noise_tag(rng, r.tags);
    if (mode >= 2) { *want_hp = hp; *want_ps = ps; }
    return r;
}

// base by base: reference coordinate -> (byte, quality) of the alignment, and [lo, hi)
void expand(const Read& r, int32_t clip_threshold, int32_t take_in, std::map<int64_t, std::pair<uint8_t, uint8_t>>* cells, int64_t* lo, int64_t* hi) {
    int64_t ref = r.pos, q = 0, s = -1, e = -1;
    for (uint32_t c : r.cigar) {
        const uint32_t op = c & 15u, len = c >> 4;
        for (uint32_t k = 0; k < len; ++k) {
            if (strk_fe::is_aligned(op)) {
                if (s < 0) s = ref;
                e = ref + 1;
                if (q < (int64_t)r.nib.size()) (*cells)[ref] = {(uint8_t)"=ACMGRSVTWYHKDBN"[r.nib[(size_t)q]], r.has_qual ? r.qual[(size_t)q] : (uint8_t)0};
            } else if (op == 2) {
                (*cells)[ref] = {(uint8_t)'_', 0};
            }
            if (strk_fe::consumes_ref(op)) ++ref;
            if (strk_fe::consumes_query(op)) ++q;
        }
    }
    const size_t n = r.cigar.size();
    const int64_t cl = n && (r.cigar[0] & 15u) == 4 ? r.cigar[0] >> 4 : 0, cr = n && (r.cigar[n - 1] & 15u) == 4 ? r.cigar[n - 1] >> 4 : 0;
    *lo = s + (cl >= clip_threshold ? take_in : 0);
    *hi = s < 0 ? s : e - (cr >= clip_threshold ? take_in : 0);
}

// one call of host_cells over records laid back to back in one exact block; returns what host_cells returns
int32_t run_cells(const std::vector<std::vector<uint8_t>>& recs, const std::vector<int64_t>& cand, std::vector<int32_t>* hp, std::vector<int32_t>* ps,
                  std::vector<uint8_t>* base, std::vector<uint8_t>* qual) {
    std::vector<uint8_t> buf;
    std::vector<int64_t> rec_off;
    for (const auto& r : recs) { rec_off.push_back((int64_t)buf.size()); buf.insert(buf.end(), r.begin(), r.end()); }
    std::vector<uint8_t> exact(buf);   // capacity == size is not promised for a grown vector; a fresh copy is exactly sized
    exact.shrink_to_fit();
    const int32_t n = (int32_t)recs.size();
    std::vector<int32_t> loc((size_t)n, 0), cand_off = {0, (int32_t)cand.size()};
    const strk_pi::CellsInput in{(int64_t)exact.size(), n, rec_off.data(), loc.data(), 1, cand_off.data(), cand.data(), nullptr, nullptr, nullptr, 100, 250};
    strk_groups::Message m;
    std::vector<int64_t> cell_off;
    if (strk_pi::check_cells(in, cell_off, &m)) { expect(false, m.text); return -2; }
    hp->assign((size_t)n, 0); ps->assign((size_t)n, 0);
    base->assign((size_t)cell_off.back(), 0); qual->assign((size_t)cell_off.back(), 0);
    return strk_pi::host_cells(exact.data(), in, cell_off.data(), 0, n, hp->data(), ps->data(), base->data(), qual->data());
}

void well_formed(std::mt19937& rng) {
    for (int round = 0; round < 300; ++round) {
        std::vector<Read> reads;
        std::vector<std::vector<uint8_t>> recs;
        std::vector<int32_t> whp, wps;
        for (unsigned k = 1 + rng() % 5; k > 0; --k) {
            int32_t a, b;
            reads.push_back(random_read(rng, &a, &b));
            recs.push_back(record(reads.back(), rng() % 5 == 0 && !reads.back().nib.empty()));   // (no placeholder without bases: l_seq 0 is none)
            whp.push_back(a); wps.push_back(b);
        }
        std::vector<int64_t> cand;
        for (int64_t c = 980; c < 980 + 1024 && cand.size() < (size_t)strk_pi::kMaxCand; c += 1 + (int64_t)(rng() % (1 + round % 4))) cand.push_back(c);
        std::vector<int32_t> hp, ps;
        std::vector<uint8_t> base, qual;
        expect(run_cells(recs, cand, &hp, &ps, &base, &qual) == -1, "well-formed records accepted", round);
        for (size_t i = 0; i < reads.size(); ++i) {
            expect(hp[i] == whp[i] && ps[i] == wps[i], "tags", hp[i]);
            std::map<int64_t, std::pair<uint8_t, uint8_t>> cells;
            int64_t lo, hi;
            expand(reads[i], 100, 250, &cells, &lo, &hi);
            bool same = true;
            for (size_t k = 0; k < cand.size(); ++k) {
                std::pair<uint8_t, uint8_t> want = {(uint8_t)'-', 0};
                const auto it = cells.find(cand[k]);
                if (it != cells.end() && cand[k] >= lo && cand[k] < hi) want = it->second;
                same = same && base[i * cand.size() + k] == want.first && qual[i * cand.size() + k] == want.second;
            }
            expect(same, "cells", round);
        }
    }
}

void hostile() {
    Read good;
    good.pos = 100; good.cigar = {10u << 4}; good.nib.assign(10, 1); good.qual.assign(10, 30); good.has_qual = true;
    int_tag(good.tags, "HP", 'C', 2); int_tag(good.tags, "PS", 's', 7);
    std::vector<std::vector<uint8_t>> bad_tags;
    auto bytes = [](const char* s, size_t n) { return std::vector<uint8_t>(s, s + n); };
    bad_tags.push_back(bytes("HPC\1PS", 6));                                   // a truncated chain
    bad_tags.push_back(bytes("HPC\1PSi\1\0", 9));                              // a value past the end
    bad_tags.push_back(bytes("HPC\1RGZgroup", 12));                            // Z without its NUL
    bad_tags.push_back(bytes("ZBBI\1\0\0\x40\0\0\0\0HPC\1", 16));              // a B count that overflows 32 bits when multiplied
    bad_tags.push_back(bytes("ZBBi\xff\xff\xff\xff", 8));                      // the largest B count
    bad_tags.push_back(bytes("ZBBi\1\0", 6));                                  // a B header cut off
    bad_tags.push_back(bytes("ZBBq\0\0\0\0", 8));                              // a B of an unknown type
    bad_tags.push_back(bytes("XXq\0", 4));                                     // an unknown type
    bad_tags.push_back(bytes("H", 1));
    const std::vector<int64_t> cand = {99, 100, 105, 109, 110};
    for (size_t k = 0; k < bad_tags.size(); ++k) {
        Read bad = good;
        bad.tags = bad_tags[k];
        std::vector<int32_t> hp, ps;
        std::vector<uint8_t> base, qual;
        expect(run_cells({record(good), record(bad), record(good)}, cand, &hp, &ps, &base, &qual) == 1, "hostile auxiliary fields refused", (long long)k);
        ++g_refusals;
        int32_t h, p;   // and the walk alone, on the exact bytes
        std::vector<uint8_t> exact(bad_tags[k]);
        expect(!strk_pi::aux_tags(exact.data(), (int64_t)exact.size(), &h, &p) && h == -1 && p == -1, "aux_tags refuses", (long long)k);
    }
    {   // the CG placeholder: its array read where it lies; one that claims more operations than the record holds is refused
        Read r = good;
        r.cigar = {6u << 4, (2u << 4) | 2u, 4u << 4};
        std::vector<int32_t> hp, ps;
        std::vector<uint8_t> base, qual;
        expect(run_cells({record(r, true)}, {99, 100, 105, 106, 107, 108, 111, 112}, &hp, &ps, &base, &qual) == -1, "CG placeholder accepted");
        expect(base.size() == 8 && memcmp(base.data(), "-AA__AA-", 8) == 0 && hp[0] == 2 && ps[0] == 7, "CG placeholder cells");
        std::vector<uint8_t> lie = record(r, true);
        const uint32_t many = 1000;
        memcpy(lie.data() + lie.size() - 12 - 4, &many, 4);
        expect(run_cells({lie}, cand, &hp, &ps, &base, &qual) == 0, "CG array longer than the record refused");
        ++g_refusals;
        r.tags.clear();
        std::vector<uint8_t> bare = record(r, true);
        bare.resize(bare.size() - 8 - 12);                          // the placeholder without its CG tag: all clip and skip
        const uint32_t block = (uint32_t)bare.size() - 4;
        memcpy(bare.data(), &block, 4);
        expect(run_cells({bare}, cand, &hp, &ps, &base, &qual) == -1 && memcmp(base.data(), "-----", 5) == 0, "bare placeholder: no cell");
    }
    {   // a record cut off inside its fixed part, and an offset that is no record start
        std::vector<uint8_t> cut = record(good);
        cut.resize(20);
        std::vector<int32_t> hp, ps;
        std::vector<uint8_t> base, qual;
        expect(run_cells({cut}, cand, &hp, &ps, &base, &qual) == 0, "cut record refused");
        ++g_refusals;
    }
}

void checkers(std::mt19937& rng) {
    auto refuse_cells = [&](const strk_pi::CellsInput& in, const char* needle) {
        strk_groups::Message m;
        m.text[0] = 0;
        std::vector<int64_t> off;
        expect(strk_pi::check_cells(in, off, &m) == strk_groups::kInvalid && strstr(m.text, needle), needle);
        ++g_refusals;
    };
    std::vector<int64_t> rec_off = {0, 40}, cand = {5, 9, 20}, alt_off = {0, 1, 1};
    std::vector<int32_t> loc = {0, 1}, cand_off = {0, 2, 3};
    std::vector<uint32_t> alt = {16};
    const strk_pi::CellsInput ok{100, 2, rec_off.data(), loc.data(), 2, cand_off.data(), cand.data(), alt.data(), alt_off.data(), nullptr, 100, 250};
    strk_groups::Message m;
    std::vector<int64_t> off;
    expect(strk_pi::check_cells(ok, off, &m) == 0 && off.size() == 3 && off[1] == 2 && off[2] == 3, "valid call accepted");
    { auto in = ok; in.n_items = -1; refuse_cells(in, "< 0"); }
    { auto in = ok; in.take_in = -1; refuse_cells(in, ">= 0"); }
    { auto in = ok; std::vector<int32_t> co = {1, 2, 3}; in.cand_off = co.data(); refuse_cells(in, "start at 0"); }
    { auto in = ok; std::vector<int32_t> co = {0, 2, 1}; in.cand_off = co.data(); refuse_cells(in, "decreasing"); }
    { auto in = ok; std::vector<int64_t> cp = {9, 5, 20}; in.cand_pos = cp.data(); refuse_cells(in, "ascending"); }
    { auto in = ok; std::vector<int64_t> cp = {5, 5, 20}; in.cand_pos = cp.data(); refuse_cells(in, "ascending"); }
    { auto in = ok; std::vector<int32_t> co = {0, 1025, 1026}; std::vector<int64_t> cp(1026); for (size_t k = 0; k < cp.size(); ++k) cp[k] = (int64_t)k;
      in.cand_off = co.data(); in.cand_pos = cp.data(); refuse_cells(in, "at most 1024"); }
    { auto in = ok; std::vector<int64_t> ro = {0, 97}; in.rec_off = ro.data(); refuse_cells(in, "rec_off"); }
    { auto in = ok; std::vector<int64_t> ro = {-1, 40}; in.rec_off = ro.data(); refuse_cells(in, "rec_off"); }
    { auto in = ok; std::vector<int32_t> lc = {0, 2}; in.item_locus = lc.data(); refuse_cells(in, "item_locus"); }
    { auto in = ok; std::vector<int32_t> lc = {-1, 0}; in.item_locus = lc.data(); refuse_cells(in, "item_locus"); }
    { auto in = ok; in.alt.ops = nullptr; refuse_cells(in, "both"); }
    { auto in = ok; std::vector<int64_t> ao = {1, 1, 1}; in.alt.off = ao.data(); refuse_cells(in, "alt_cigar_off[0]"); }
    { auto in = ok; std::vector<int64_t> ao = {0, 1, 0}; in.alt.off = ao.data(); refuse_cells(in, "decreasing"); }

    auto refuse_useful = [&](const strk_pi::UsefulInput& in, const char* needle) {
        strk_groups::Message mm;
        mm.text[0] = 0;
        expect(strk_pi::check_useful(in, &mm) == strk_groups::kInvalid && strstr(mm.text, needle), needle);
        ++g_refusals;
    };
    std::vector<int32_t> item_locus = {0, 0, 1}, kept_off = {0, 2, 3}, kept_item = {0, 1, 2};
    const strk_pi::UsefulInput uok{3, item_locus.data(), 2, kept_off.data(), kept_item.data(), 2};
    expect(strk_pi::check_useful(uok, &m) == 0, "valid useful call accepted");
    { auto in = uok; in.min_allele_reads = 0; refuse_useful(in, "min_allele_reads"); }
    { auto in = uok; std::vector<int32_t> ko = {1, 2, 3}; in.kept_off = ko.data(); refuse_useful(in, "start at 0"); }
    { auto in = uok; std::vector<int32_t> ko = {0, 2, 1}; in.kept_off = ko.data(); refuse_useful(in, "decreasing"); }
    { auto in = uok; std::vector<int32_t> ki = {0, 3, 2}; in.kept_item = ki.data(); refuse_useful(in, "out of range"); }
    { auto in = uok; std::vector<int32_t> ki = {0, -1, 2}; in.kept_item = ki.data(); refuse_useful(in, "out of range"); }
    { auto in = uok; std::vector<int32_t> ki = {0, 2, 2}; in.kept_item = ki.data(); refuse_useful(in, "belongs to locus"); }

    // the choice of the useful SNVs against a count written here
    for (int round = 0; round < 200; ++round) {
        const int32_t n = (int32_t)(rng() % 40), nc = (int32_t)(rng() % 200), mar = 1 + (int32_t)(rng() % 3);
        std::vector<uint8_t> cells((size_t)n * nc);
        const char alphabet[] = "AACCGT-_N";
        for (auto& b : cells) b = (uint8_t)alphabet[rng() % 9];
        std::vector<int32_t> il((size_t)n, 0), co = {0, nc}, ko = {0, n}, ki((size_t)n), sel((size_t)strk_pi::kMaxSnvs);
        std::vector<int64_t> cell_off((size_t)n + 1);
        for (int32_t i = 0; i <= n; ++i) { cell_off[(size_t)i] = (int64_t)i * nc; if (i < n) ki[(size_t)i] = i; }
        const strk_pi::UsefulInput in{n, il.data(), 1, ko.data(), ki.data(), mar};
        const int32_t s = strk_pi::host_useful_locus(in, co.data(), cell_off.data(), cells.data(), 0, sel.data());
        int32_t a_thr, t_thr, w = 0;
        strk_pi::thresholds(n, mar, &a_thr, &t_thr);
        bool same = true;
        for (int32_t c = 0; c < nc && w < strk_pi::kMaxSnvs; ++c) {
            std::map<uint8_t, int> cnt;
            int total = 0;
            for (int32_t r = 0; r < n; ++r) {
                const uint8_t b = cells[(size_t)r * nc + c];
                if (b != '-' && b != '_') { ++cnt[b]; ++total; }
            }
            int distinct = 0;
            for (const auto& kv : cnt) distinct += kv.second >= a_thr;
            if (distinct >= 2 && total >= t_thr) { same = same && w < s && sel[(size_t)w] == c; ++w; }
        }
        expect(same && w == s, "useful SNVs", round);
    }
    int32_t a, t;
    strk_pi::thresholds(10, 2, &a, &t); expect(a == 2 && t == 6, "thresholds of 10 reads", t);
    strk_pi::thresholds(30, 2, &a, &t); expect(a == 6 && t == 16, "thresholds of 30 reads", t);
    strk_pi::thresholds(0, 2, &a, &t); expect(a == 2 && t == 5, "thresholds of no read", t);
}

}  // namespace

int main() {
    std::mt19937 rng(20240611);
    well_formed(rng);
    hostile();
    checkers(rng);
    printf("phase inputs: %d checks, %d refusals, %d failed\n", g_checks, g_refusals, g_failed);
    return g_failed ? 1 : 0;
}
