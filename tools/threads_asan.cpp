// The host scaffolding that the stages on items of an alignment file share (strk_threads.h: the two thread fans, the first
// malformed item, the piece loop) and the check of the substitute alignments (strk_bamrec.h: check_alt): every fan covers
// [0, n) exactly once for sizes around its thresholds on 1 to 32 threads, FirstBad keeps the minimum under 32 reporting
// threads, the piece loop covers its items in ascending pieces up to INT32_MAX without forming a sum in 32 bits (arithmetic
// only: the function it calls counts), and check_alt gives every refusal by its message over heap blocks of exactly their
// length.  The copy plan of a staged buffer (strk_stage_plan.h): over parts around the alignment and around kDirectBytes, zeros,
// empty parts, rooms between and behind parts and direct neighbours, every byte of a part that goes up is covered by exactly
// one copy or memset, no stretch of the image runs over more than the alignment padding between two parts, nothing leaves the
// buffer, and small neighbours take one copy.  tools/threads_asan.sh runs it under AddressSanitizer + UBSan and under ThreadSanitizer; tests/test_threads_tool.py
// builds it plain and requires exit 0.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <memory>
#include <vector>
#include "../strkit_amd/csrc/strk_bamrec.h"
#include "../strkit_amd/csrc/strk_stage_plan.h"
#include "../strkit_amd/csrc/strk_threads.h"

namespace {

int g_failed = 0, g_checks = 0;

void expect(bool ok, const char* what, long long a = 0, long long b = 0) {
    ++g_checks;
    if (!ok) {
        fprintf(stderr, "FAILED %s (%lld, %lld)\n", what, a, b);
        ++g_failed;
    }
}

bool all_once(const std::vector<uint8_t>& seen) {
    for (const uint8_t s : seen)
        if (s != 1) return false;
    return true;
}

void fans() {
    const int64_t sizes[] = {0, 1, 1023, 1024, 1025, 2047, 2048, 32 * 1024 + 1};
    for (const int64_t n : sizes) {
        for (int nt = 1; nt <= 32; ++nt) {
            std::vector<uint8_t> seen((size_t)n, 0);
            std::atomic<int> calls{0}, out_of_range{0};
            const auto mark = [&](int64_t i0, int64_t i1) {
                ++calls;
                if (i0 < 0 || i1 > n || i0 > i1) { ++out_of_range; return; }
                for (int64_t i = i0; i < i1; ++i) ++seen[(size_t)i];   // (slices that overlapped would race here as well)
            };
            strk_threads::slices_on(n, nt, mark);
            expect(all_once(seen) && !out_of_range && calls >= 1 && calls <= nt, "slices cover [0, n) once", n, nt);
            for (const int64_t chunk : {(int64_t)1, (int64_t)16, (int64_t)4096}) {
                if (chunk == 1 && n > 4096) continue;
                std::fill(seen.begin(), seen.end(), 0);
                calls = 0;
                strk_threads::parallel_chunks(n, chunk, nt, mark);
                expect(all_once(seen) && !out_of_range && calls == (n + chunk - 1) / chunk, "chunks cover [0, n) once", n, nt);
            }
            // a thread's scratch is its own, made once
            struct Scratch { int64_t items = 0; int made = 1; };
            std::atomic<int64_t> total{0};
            strk_threads::parallel_chunks<Scratch>(n, 16, nt, [&](int64_t i0, int64_t i1, Scratch& s) {
                s.items += i1 - i0;
                total += (i1 - i0) * s.made;
            });
            expect(total == n, "chunks with scratch cover [0, n)", n, nt);
        }
        // the thresholds of the entries: one thread per 1 024 items, at most 32 and the CPUs there are
        std::vector<uint8_t> seen((size_t)n, 0);
        std::atomic<int> calls{0};
        strk_threads::parallel_slices(n, 1024, 32, [&](int64_t i0, int64_t i1) {
            ++calls;
            for (int64_t i = i0; i < i1; ++i) ++seen[(size_t)i];
        });
        const int64_t most = std::max<int64_t>(1, std::min<int64_t>({(int64_t)strk_threads::host_cpus(), 32, n / 1024}));
        expect(all_once(seen) && calls >= 1 && calls <= most, "parallel_slices: one thread per 1 024 items", n, calls);
    }
}

void first_bad() {
    strk_threads::FirstBad none;
    expect(none.get() == -1, "FirstBad without a report");
    for (int round = 0; round < 8; ++round) {
        strk_threads::FirstBad bad;
        // thread t reports items t + 32 k, descending or ascending by round: the minimum is `round`
        strk_threads::fan(32, [&](int t) {
            for (int k = 0; k < 200; ++k) {
                const int64_t i = (int64_t)t + 32 * ((round & 1) ? k : 199 - k);
                if (i >= round) bad.report(i);
            }
        });
        expect(bad.get() == round, "FirstBad under 32 threads", bad.get(), round);
    }
    expect(strk_threads::first_bad_of_word(0, INT32_MAX) == -1 && strk_threads::first_bad_of_word(INT32_MAX, INT32_MAX) == 0 &&
               strk_threads::first_bad_of_word(1, INT32_MAX) == INT32_MAX - 1 && strk_threads::first_bad_of_word(7, 9) == 2,
           "a kernel's word decodes to its item");
}

void pieces() {
    for (const int32_t n : {1, 9, INT32_MAX}) {
        for (const int64_t want : {(int64_t)0, (int64_t)1, (int64_t)n - 1, (int64_t)n, ((int64_t)1 << 30) + 1, (int64_t)INT32_MAX}) {
            const int32_t piece = (int32_t)want;
            const int64_t limit = piece > 0 ? piece : n;
            int64_t next = 0, n_pieces = 0;
            bool ok = true;
            const int rc = strk_threads::for_pieces(n, piece, [&](int32_t i0, int32_t i1) {
                ok = ok && i0 == next && i1 > i0 && i1 <= n && (int64_t)i1 - i0 <= limit;
                next = i1;
                ++n_pieces;
                return 0;
            });
            expect(rc == 0 && ok && next == n && n_pieces == ((int64_t)n + limit - 1) / limit, "pieces cover [0, n) in order", n, piece);
        }
    }
    int calls = 0;
    expect(strk_threads::for_pieces(9, 2, [&](int32_t, int32_t i1) { ++calls; return i1 >= 4 ? -5 : 0; }) == -5 && calls == 2,
           "the piece loop stops at the first error");
    expect(strk_threads::for_pieces(0, 4, [&](int32_t, int32_t) { return -1; }) == 0, "no items, no piece");
}

// arrays on the heap, of exactly their length
template <class T>
std::unique_ptr<T[]> block(std::initializer_list<T> v) {
    std::unique_ptr<T[]> p(new T[v.size()]);
    std::copy(v.begin(), v.end(), p.get());
    return p;
}

void alt_check() {
    strk_groups::Message msg;
    const auto ops = block<uint32_t>({16, 32, 48});
    const auto off = block<int64_t>({0, 2, 2, 3});
    const auto start = block<int64_t>({5, 0, 7});
    const auto refuse = [&](const strk_fe::AltCigars& alt, int32_t n, const char* part) {
        msg.text[0] = 0;
        expect(strk_fe::check_alt(n, alt, &msg) == strk_groups::kInvalid && strstr(msg.text, part), part);
    };
    expect(strk_fe::check_alt(3, {ops.get(), off.get(), start.get()}, &msg) == 0, "a good triple");
    expect(strk_fe::check_alt(3, {ops.get(), off.get(), nullptr}, &msg) == 0, "no starts");
    expect(strk_fe::check_alt(3, {nullptr, nullptr, nullptr}, &msg) == 0, "no triple");
    expect(strk_fe::check_alt(3, {nullptr, nullptr, start.get()}, &msg) == 0, "starts alone are not read");
    const auto empty = block<int64_t>({0, 0, 0, 0});
    expect(strk_fe::check_alt(3, {ops.get(), empty.get(), nullptr}, &msg) == 0, "a triple without operations");
    refuse({nullptr, off.get(), start.get()}, 3, "alt_cigar and alt_cigar_off must both be given or both be NULL");
    refuse({ops.get(), nullptr, start.get()}, 3, "alt_cigar and alt_cigar_off must both be given or both be NULL");
    const auto from1 = block<int64_t>({1, 2, 2, 3});
    refuse({ops.get(), from1.get(), nullptr}, 3, "alt_cigar_off[0] must be 0");
    const auto down = block<int64_t>({0, 2, 1, 3});
    refuse({ops.get(), down.get(), nullptr}, 3, "item 1: alt_cigar_off is decreasing (or a CIGAR too long)");
    const auto huge = block<int64_t>({0, 1, (int64_t)INT32_MAX + 2});   // (the offsets alone are read: no such array of operations)
    refuse({ops.get(), huge.get(), nullptr}, 2, "item 1: alt_cigar_off is decreasing (or a CIGAR too long)");

    // the alignment an item walks: the record's own, or its substitute
    const uint8_t rec_cigar[4] = {0x40, 0, 0, 0};
    strk_fe::Rec r{};
    r.cigar = rec_cigar; r.n_cigar = 1; r.pos = 100;
    const uint8_t* cig;
    int32_t n_cig;
    int64_t at;
    const strk_fe::AltCigars alt{ops.get(), off.get(), start.get()};
    strk_fe::item_alignment(r, 0, alt, &cig, &n_cig, &at);
    expect(cig == reinterpret_cast<const uint8_t*>(ops.get()) && n_cig == 2 && at == 5, "item 0 walks its substitute");
    strk_fe::item_alignment(r, 1, alt, &cig, &n_cig, &at);
    expect(cig == rec_cigar && n_cig == 1 && at == 100, "item 1 walks its record's CIGAR");
    strk_fe::item_alignment(r, 2, {ops.get(), off.get(), nullptr}, &cig, &n_cig, &at);
    expect(cig == reinterpret_cast<const uint8_t*>(ops.get() + 2) && n_cig == 1 && at == 0, "item 2 without starts begins at 0");
    strk_fe::item_alignment(r, 2, {nullptr, nullptr, nullptr}, &cig, &n_cig, &at);
    expect(cig == rec_cigar && n_cig == 1 && at == 100, "no triple: the record's CIGAR");
}

// The plan of `l` against its parts, byte by byte; n_copies >= 0: the plan has that many steps.
void check_plan(const strk_stage::Layout& l, const char* what, int n_copies = -1) {
    using strk_stage::Copy;
    const size_t n = l.cv.bytes;
    const std::vector<Copy> plan = strk_stage::plan(l.up());
    std::vector<uint8_t> in_part(n, 0), covered(n, 0);
    for (const strk_stage::Part& p : l.up()) {
        expect(p.at % 256 == 0 && p.at + p.bytes <= n, what, (long long)p.at, (long long)p.bytes);
        for (size_t b = 0; b < p.bytes; ++b) in_part[p.at + b] = 1;
    }
    bool inside = true, once = true, short_gaps = true, exact = true;
    for (const Copy& k : plan) {
        if (k.bytes == 0 || k.at + k.bytes > n) { inside = false; continue; }
        size_t gap = 0;
        for (size_t b = k.at; b < k.at + k.bytes; ++b) {
            ++covered[b];
            gap = in_part[b] ? 0 : gap + 1;
            if (gap > 255 || (gap && k.kind != Copy::kImage)) short_gaps = false;   // (a direct copy or a memset is one part, whole)
        }
        if (k.kind == Copy::kImage) continue;
        bool found = false;   // the part it is: zeros for a memset, the caller's memory for a direct copy
        for (const strk_stage::Part& p : l.up())
            found = found || (p.at == k.at && p.bytes == k.bytes && p.mem == k.mem && (p.mem != nullptr) == (k.kind == Copy::kDirect));
        exact = exact && found && k.bytes >= strk_stage::kDirectBytes;
    }
    for (size_t b = 0; b < n; ++b)
        if (in_part[b] ? covered[b] != 1 : covered[b] > 1) once = false;
    expect(inside, "plan: copies lie inside the buffer", (long long)n);
    expect(once, what);
    expect(short_gaps, "plan: no stretch runs over more than the padding between two parts");
    expect(exact, "plan: a direct copy or a memset is one large part");
    if (n_copies >= 0) expect((int)plan.size() == n_copies, what, (long long)plan.size(), n_copies);
}

void stage_plan() {
    using strk_stage::Layout;
    constexpr size_t kD = strk_stage::kDirectBytes;
    static_assert(kD == 262144, "the threshold tests/test_gpu_context_staging.py is written for");
    static const std::vector<char> mem(kD + 4, 'x');   // (the plan keeps addresses and reads nothing)
    for (const size_t bytes : {(size_t)1, (size_t)255, (size_t)256, (size_t)257, kD - 4, kD, kD + 4}) {
        for (const bool zeros : {false, true}) {
            Layout one;
            one.put(zeros ? nullptr : mem.data(), bytes);
            check_plan(one, "plan: one part", 1);
            Layout mid;   // between two small parts: one stretch below the threshold, three steps from it on
            mid.put(mem.data(), 40);
            zeros ? mid.zero(bytes) : mid.put(mem.data(), bytes);
            mid.put(mem.data(), 8);
            check_plan(mid, "plan: a part between two small ones", bytes < kD ? 1 : 3);
        }
    }
    Layout small;   // n small neighbours: one copy
    for (int k = 1; k <= 12; ++k) k % 4 ? small.put(mem.data(), (size_t)k * 100) : small.zero((size_t)k * 100);
    check_plan(small, "plan: small neighbours take one copy", 1);
    Layout empty;   // empty parts, also first and last, and nothing else
    empty.put(mem.data(), 0);
    check_plan(empty, "plan: nothing to send", 0);
    empty.put(mem.data(), 100);
    empty.zero(0);
    empty.put(nullptr, 0);
    empty.put(mem.data(), 300);
    empty.put(mem.data(), 0);
    check_plan(empty, "plan: empty parts are skipped", 1);
    Layout gap;   // a room between two small parts is not sent
    gap.put(mem.data(), 100);
    gap.room((size_t)1 << 20);
    gap.put(mem.data(), 100);
    check_plan(gap, "plan: a stretch ends at a room", 2);
    Layout results;   // a result between two parts is a room of the way up
    results.put(mem.data(), 100);
    results.get(nullptr, 4096);
    results.zero(100);
    check_plan(results, "plan: a stretch ends at a result", 2);
    Layout last;   // a room last
    last.put(mem.data(), 1000);
    last.zero(24);
    last.room(kD);
    check_plan(last, "plan: a room last", 1);
    Layout direct;   // direct neighbours, a memset among them, small parts around
    direct.put(mem.data(), 16);
    direct.put(mem.data(), kD);
    direct.put(mem.data(), kD + 4);
    direct.zero(kD);
    direct.put(mem.data(), 16);
    direct.put(mem.data(), 16);
    check_plan(direct, "plan: direct neighbours", 5);
}

}  // namespace

int main() {
    fans();
    first_bad();
    pieces();
    alt_check();
    stage_plan();
    std::printf("threads_asan: %d checks, %d failed\n", g_checks, g_failed);
    return g_failed ? 1 : 0;
}
