// The host side of the annotation reader (strk_gff.h: the rule of one line, the id of a feature, the host walk with its join, the
// closing pass with its capacities) over the corpus of tests/annot_cases.py and over truncations of every corpus text.  Every text
// is a heap block of exactly its length, so a read one byte past a line, a field or the text is reported under AddressSanitizer /
// UBSan (tools/gff_asan.sh); tests/test_annotations.py builds it plain and requires exit 0.
//   gff_asan <directory written by annot_cases.dump()>
// Per case <name>.q: "gtf <0|1>", then either "refuse <offset> <contig>" or, per contig, "query <contig> <n> s e ..." followed per
// locus by the number of its ids and the ids ('=' in front of each).  The whole text must give exactly those ids, through arrays of
// exactly the sizes the size query names; a truncation, read as a piece and as a file that ends there, must end on a line start
// and, as a piece of a text that is not refused, give per locus a prefix of the whole text's ids.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>
#include <dirent.h>
#include "../strkit_amd/csrc/strk_gff.h"

namespace {

int g_failed = 0;
long long g_checks = 0, g_refusals = 0;

void expect(bool ok, const char* what, const std::string& where, long long detail = 0) {
    ++g_checks;
    if (!ok) {
        fprintf(stderr, "FAILED %s: %s (%lld)\n", where.c_str(), what, detail);
        ++g_failed;
    }
}

struct Run { bool refused = false; long long bad_off = -1; int64_t end_off = 0; std::vector<std::vector<std::string>> ids; };

// strk_gff_overlaps on one thread: overlaps_host, then emit twice (the size query, then arrays of exactly those sizes)
Run run(const uint8_t* t, int64_t n, const std::string& contig, int gtf, bool final, const std::vector<int64_t>& ls, const std::vector<int64_t>& le) {
    Run out;
    strk_gff::Result r;
    strk_gff::Message msg;
    const int32_t n_loci = (int32_t)ls.size();
    if (strk_gff::overlaps_host(t, n, 0, contig.c_str(), gtf, final ? 1 : 0, -1, n_loci, ls.data(), le.data(), &r, &msg,
                                [](int32_t m, auto&& body) { body(0, m); })) {
        out.refused = true;
        sscanf(msg.text, "line at byte %lld", &out.bad_off);
        return out;
    }
    out.end_off = r.end_off;
    int64_t sizes[4];
    strk_gff::emit(r, n_loci, 0, nullptr, nullptr, 0, nullptr, nullptr, nullptr, nullptr, 0, nullptr, sizes);
    std::vector<int32_t> pl((size_t)sizes[0]), pf((size_t)sizes[0]), fk((size_t)sizes[1]);
    std::vector<int64_t> fb((size_t)sizes[1]), fe((size_t)sizes[1]), fo((size_t)(2 * sizes[1] + 1));
    std::vector<uint8_t> text((size_t)sizes[2]);
    const int64_t k = strk_gff::emit(r, n_loci, sizes[0], pl.data(), pf.data(), sizes[1], fb.data(), fe.data(), fk.data(), fo.data(), sizes[2], text.data(), sizes);
    out.ids.resize((size_t)n_loci);
    for (int64_t i = 0; i < k; ++i) {
        const int32_t j = pf[(size_t)i];
        const std::string type((const char*)text.data() + fo[(size_t)(2 * j)], (size_t)(fo[(size_t)(2 * j + 1)] - fo[(size_t)(2 * j)]));
        const std::string val((const char*)text.data() + fo[(size_t)(2 * j + 1)], (size_t)(fo[(size_t)(2 * j + 2)] - fo[(size_t)(2 * j + 1)]));
        std::string id = val;
        if (fk[(size_t)j] == strk_gff::kIdExon) id = type + ":" + val;
        if (fk[(size_t)j] == strk_gff::kIdPosition) id = type + ":" + contig + "-" + std::to_string(fb[(size_t)j]) + "-" + std::to_string(fe[(size_t)j]);
        out.ids[(size_t)pl[(size_t)i]].push_back(id);
    }
    return out;
}

std::vector<uint8_t> slurp(const std::string& path) {
    std::ifstream f(path, std::ios::binary);
    return std::vector<uint8_t>((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
}

Run run_copy(const std::vector<uint8_t>& text, size_t len, const std::string& contig, int gtf, bool final, const std::vector<int64_t>& ls,
             const std::vector<int64_t>& le) {
    uint8_t* block = (uint8_t*)malloc(len ? len : 1);   // exactly `len` bytes
    memcpy(block, text.data(), len);
    const Run r = run(block, (int64_t)len, contig, gtf, final, ls, le);
    free(block);
    return r;
}

void truncations(const std::vector<uint8_t>& text, const std::string& where, const std::string& contig, int gtf, const std::vector<int64_t>& ls,
                 const std::vector<int64_t>& le, const Run* full) {
    // every length for short texts, a stride (and every length near the end) for long ones
    const size_t stride = text.size() > 100000 ? 997 : (text.size() > 6000 ? 97 : 1);
    for (size_t len = 0; len < text.size(); len += (len + 300 > text.size() ? 1 : stride))
        for (int final = 0; final < 2; ++final) {
            const Run r = run_copy(text, len, contig, gtf, final != 0, ls, le);
            if (r.refused) { ++g_refusals; continue; }
            const bool ok = r.end_off >= 0 && r.end_off <= (int64_t)len && (final ? r.end_off == (int64_t)len : (r.end_off == 0 || text[(size_t)r.end_off - 1] == '\n'));
            expect(ok, "end_off of a truncation", where, (long long)len);
            if (!final && full)
                for (size_t l = 0; l < ls.size(); ++l) {
                    const auto &a = r.ids[l], &b = full->ids[l];
                    expect(a.size() <= b.size() && std::equal(a.begin(), a.end(), b.begin()), "a piece gives a prefix of the whole", where, (long long)len);
                }
        }
}

}  // namespace

int main(int argc, char** argv) {
    if (argc != 2) { fprintf(stderr, "usage: %s <corpus directory>\n", argv[0]); return 2; }
    const std::string dir = argv[1];
    DIR* d = opendir(dir.c_str());
    if (!d) { fprintf(stderr, "cannot open %s\n", dir.c_str()); return 2; }
    std::vector<std::string> names;
    while (dirent* e = readdir(d)) {
        const std::string f = e->d_name;
        if (f.size() > 4 && f.substr(f.size() - 4) == ".txt") names.push_back(f.substr(0, f.size() - 4));
    }
    closedir(d);
    int n_cases = 0;
    for (const std::string& name : names) {
        const std::vector<uint8_t> text = slurp(dir + "/" + name + ".txt");
        std::ifstream q(dir + "/" + name + ".q");
        std::string row, word;
        int gtf = 0;
        ++n_cases;
        while (std::getline(q, row)) {
            std::istringstream in(row);
            in >> word;
            if (word == "gtf") { in >> gtf; continue; }
            if (word == "refuse") {
                long long off;
                std::string contig;
                in >> off >> contig;
                const std::vector<int64_t> ls{0}, le{100};
                const Run r = run_copy(text, text.size(), contig, gtf, true, ls, le);
                expect(r.refused && r.bad_off == off, "refusal names the line", name, r.bad_off);
                g_refusals += r.refused;
                truncations(text, name, contig, gtf, ls, le, nullptr);
                continue;
            }
            if (word != "query") continue;
            std::string contig;
            size_t n_loci;
            in >> contig >> n_loci;
            std::vector<int64_t> ls(n_loci), le(n_loci);
            for (size_t l = 0; l < n_loci; ++l) in >> ls[l] >> le[l];
            std::vector<std::vector<std::string>> want(n_loci);
            for (size_t l = 0; l < n_loci; ++l) {
                std::getline(q, row);
                const int n_ids = atoi(row.c_str());
                for (int i = 0; i < n_ids; ++i) {
                    std::getline(q, row);
                    want[l].push_back(row.substr(1));
                }
            }
            const Run full = run_copy(text, text.size(), contig, gtf, true, ls, le);
            expect(!full.refused, "the whole text is read", name + " " + contig);
            if (full.refused) continue;
            expect(full.ids == want, "ids of the whole text", name + " " + contig);
            expect(full.end_off == (int64_t)text.size(), "end_off of the whole text", name + " " + contig, full.end_off);
            truncations(text, name + " " + contig, contig, gtf, ls, le, &full);
        }
    }
    printf("%d cases, %lld checks, %lld refusals, %d failed\n", n_cases, g_checks, g_refusals, g_failed);
    return (g_failed || n_cases == 0) ? 1 : 0;
}
