// strk_threads.h — what the host entries that walk the items of a file share: the CPUs of the process, the two thread fans
// (contiguous slices, chunks taken from a counter), the first malformed item of a call, and the cut of a call's items into
// pieces.  Host only and nothing of HIP in here: the header compiles with the host compiler alone (tools/threads_asan.cpp runs
// it under the sanitizers).
#pragma once
#include <sched.h>
#include <stdint.h>

#include <algorithm>
#include <atomic>
#include <thread>
#include <type_traits>
#include <vector>

namespace strk_threads {

// CPUs this process may run on (a container's share, not the machine's core count)
inline int host_cpus() {
    cpu_set_t set;
    CPU_ZERO(&set);
    if (sched_getaffinity(0, sizeof set, &set) == 0 && CPU_COUNT(&set) > 0) return CPU_COUNT(&set);
    return (int)std::max(1u, std::thread::hardware_concurrency());
}

// work(t) for t in [0, n_threads): t = 0 on the calling thread, the others on threads of their own, all joined on return
template <class Work>
void fan(int n_threads, Work&& work) {
    std::vector<std::thread> th;
    for (int t = 1; t < n_threads; ++t) th.emplace_back([&work, t] { work(t); });
    work(0);
    for (auto& x : th) x.join();
}

// body(i0, i1) over [0, n) cut into n_threads contiguous slices (fewer where the slices run out)
template <class Body>
void slices_on(int64_t n, int n_threads, Body&& body) {
    const int64_t nt = std::max(n_threads, 1), per = (n + nt - 1) / nt;
    fan((int)std::min<int64_t>(nt, per > 0 ? (n + per - 1) / per : 1), [&](int t) { body(t * per, std::min(n, (t + 1) * per)); });
}

// The same on one thread per min_per_thread items, at most max_threads and the CPUs of the process.  Starting threads costs
// more than a few hundred items do, and a caller that loads the next block's records meanwhile needs the other cores.
template <class Body>
void parallel_slices(int64_t n, int64_t min_per_thread, int max_threads, Body&& body) {
    slices_on(n, (int)std::min<int64_t>({(int64_t)host_cpus(), (int64_t)max_threads, n / min_per_thread}), body);
}

struct NoScratch {};

// n_threads threads take [0, n) in chunks of `chunk` from a counter.  body(i0, i1), or body(i0, i1, scratch) with a Scratch
// that every thread constructs once for itself (tables and vectors that a chunk would otherwise allocate anew).
template <class Scratch = NoScratch, class Body>
void parallel_chunks(int64_t n, int64_t chunk, int n_threads, Body&& body) {
    std::atomic<int64_t> next{0};
    fan(std::max(n_threads, 1), [&](int) {
        Scratch scratch;
        for (int64_t i0; (i0 = next.fetch_add(chunk)) < n;) {
            if constexpr (std::is_same_v<Scratch, NoScratch>) body(i0, std::min(n, i0 + chunk));
            else body(i0, std::min(n, i0 + chunk), scratch);
        }
    });
}

// The first malformed item of a call, whichever threads meet how many of them.
class FirstBad {
    std::atomic<int64_t> first_{INT64_MAX};

  public:
    void report(int64_t i) {
        int64_t cur = first_.load();
        while (i < cur && !first_.compare_exchange_weak(cur, i)) {}
    }
    int64_t get() const { return first_.load() == INT64_MAX ? -1 : first_.load(); }
};

// The same from a kernel's word: the lanes write atomicMax(bad, base - item) with a base above every item (the larger value is
// the earlier item), 0 stands for none.  -1 when none was written.
inline int64_t first_bad_of_word(int32_t word, int64_t base) { return word ? base - word : -1; }

// fn(i0, i1) over [0, n_items) in ascending pieces of at most piece_items items (0: all of them in one); stops at the first
// piece for which fn returns non-zero and returns that.  i0 + piece is formed in 64 bits: it may pass INT32_MAX.
template <class Fn>
int for_pieces(int32_t n_items, int32_t piece_items, Fn&& fn) {
    const int64_t n = n_items, piece = piece_items > 0 ? piece_items : n;
    for (int64_t i0 = 0; i0 < n; i0 += piece)
        if (const int rc = fn((int32_t)i0, (int32_t)std::min(n, i0 + piece))) return rc;
    return 0;
}

}  // namespace strk_threads
