// The host side of the candidate-SNV reader (strk_vcf.h: the rule of one line, the host walk with its slice merge, the closing pass
// with its capacities; strk_lines.h: the lines) over the corpus
// of tests/vcf_cases.py and over every truncation of every corpus text at every byte length.  Every text is a heap block of
// exactly its length, so a read one byte past a line, a field or the text is reported under AddressSanitizer / UBSan
// (tools/vcf_snvs_asan.sh); tests/test_vcf_snvs_host.py builds it plain and requires exit 0.
//   vcf_snvs_asan <directory written by vcf_cases.dump()>
// Per window of a case (<name>.q: contig beg end start, then the expected positions or "refuse"): the whole text must give the
// expected positions; a truncation, read as a piece (not final), must give a prefix of them and an end_off on a line start.  Every
// text is walked twice, as one slice and in slices of three lines, which must agree in everything.
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
#include "../strkit_amd/csrc/strk_vcf.h"

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

struct Result {
    int64_t n = 0, end_off = 0;
    int32_t past = 0;
    bool refused = false;
    std::vector<int64_t> pos;
    std::vector<uint8_t> ref, ids;
    std::vector<int64_t> id_off;
    bool operator==(const Result& o) const {
        return n == o.n && end_off == o.end_off && past == o.past && refused == o.refused && pos == o.pos && ref == o.ref && ids == o.ids && id_off == o.id_off;
    }
};

// strk_vcf_snvs with `par` for its threads: snvs_host, then finish twice (the size query, then arrays of exactly those sizes)
template <class Par>
Result run_par(const uint8_t* t, int64_t n_bytes, int64_t start, const std::string& contig, int64_t beg, int64_t end, bool final, Par&& par) {
    Result r;
    strk_vcf::Walk w;
    strk_vcf::snvs_host(t, n_bytes, start, contig.c_str(), beg, end, final ? 1 : 0, 0, &w, par);
    r.end_off = w.end_off; r.past = w.past;
    strk_vcf::Message msg;
    int64_t id_bytes = 0, none[1];
    const int64_t n = strk_vcf::finish(w.kept, w.bad_off, -1, 0, nullptr, nullptr, none, nullptr, 0, &id_bytes, &msg);   // the size query
    if (n < 0) { r.refused = true; return r; }
    r.pos.resize((size_t)n); r.ref.resize((size_t)n); r.id_off.resize((size_t)n + 1); r.ids.resize((size_t)id_bytes);
    r.n = strk_vcf::finish(w.kept, w.bad_off, -1, n, r.pos.data(), r.ref.data(), r.id_off.data(), r.ids.data(), id_bytes, &id_bytes, &msg);
    return r;
}

// one slice, then slices of three lines handed over last to first (the merge has to order them): both must give the same
Result run(const uint8_t* t, int64_t n_bytes, int64_t start, const std::string& contig, int64_t beg, int64_t end, bool final, const std::string& where) {
    const Result one = run_par(t, n_bytes, start, contig, beg, end, final, [](int32_t m, auto&& body) { body(0, m); });
    const Result sliced = run_par(t, n_bytes, start, contig, beg, end, final, [](int32_t m, auto&& body) {
        for (int32_t i0 = (m - 1) / 3 * 3; m > 0 && i0 >= 0; i0 -= 3) body(i0, std::min(m, i0 + 3));
    });
    expect(one == sliced, "slices of three lines give what one slice gives", where, (long long)n_bytes);
    return one;
}

std::vector<uint8_t> slurp(const std::string& path) {
    std::ifstream f(path, std::ios::binary);
    return std::vector<uint8_t>((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
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
        if (f.size() > 4 && f.substr(f.size() - 4) == ".vcf") names.push_back(f.substr(0, f.size() - 4));
    }
    closedir(d);
    int n_cases = 0;
    for (const std::string& name : names) {
        const std::vector<uint8_t> text = slurp(dir + "/" + name + ".vcf");
        std::ifstream q(dir + "/" + name + ".q");
        std::string row;
        ++n_cases;
        while (std::getline(q, row)) {
            std::istringstream in(row);
            std::string contig, tok;
            long long beg, end, start;
            in >> contig >> beg >> end >> start;
            std::vector<int64_t> want;
            bool refuse = false;
            while (in >> tok) {
                if (tok == "refuse") refuse = true;
                else want.push_back(atoll(tok.c_str()));
            }
            // the whole text, in a block of exactly its length
            uint8_t* whole = (uint8_t*)malloc(text.size() ? text.size() : 1);
            memcpy(whole, text.data(), text.size());
            const Result full = run(whole, (int64_t)text.size(), start, contig, beg, end, true, name + " " + row);
            free(whole);
            expect(full.refused == refuse, "refusal", name + " " + row);
            g_refusals += full.refused;
            if (!refuse) {
                expect(full.pos == want, "positions of the whole text", name + " " + row, (long long)full.pos.size());
                expect(full.end_off == (int64_t)text.size(), "end_off of the whole text", name + " " + row, full.end_off);
            }
            // every truncation, as a piece and as a file that ends there
            for (size_t len = (size_t)start; len < text.size(); ++len) {
                uint8_t* cut = (uint8_t*)malloc(len ? len : 1);
                memcpy(cut, text.data(), len);
                for (int final = 0; final < 2; ++final) {
                    const Result r = run(cut, (int64_t)len, start, contig, beg, end, final != 0, name + " " + row);
                    if (r.refused) { ++g_refusals; continue; }
                    bool ok = r.end_off >= start && r.end_off <= (int64_t)len && (final ? r.end_off == (int64_t)len : (r.end_off == start || cut[r.end_off - 1] == '\n'));
                    expect(ok, "end_off of a truncation", name + " " + row, (long long)len);
                    if (!final && !refuse) {
                        ok = r.pos.size() <= full.pos.size() && std::equal(r.pos.begin(), r.pos.end(), full.pos.begin());
                        expect(ok, "a piece gives a prefix of the whole", name + " " + row, (long long)len);
                    }
                    expect(r.id_off.size() == r.pos.size() + 1 && r.id_off.back() == (int64_t)r.ids.size(), "ID offsets", name + " " + row, (long long)len);
                }
                free(cut);
            }
        }
    }
    printf("%d cases, %lld checks, %lld refusals, %d failed\n", n_cases, g_checks, g_refusals, g_failed);
    return (g_failed || n_cases == 0) ? 1 : 0;
}
