// strk_stage_plan.h — the layout of a staged device buffer and the list of copies that fills it: what Staging (strk_host.h)
// executes.  No HIP in it: tools/threads_asan.cpp checks the plan on the CPU.
#pragma once

#include <cstddef>
#include <vector>

namespace strk_stage {

// A part of this size or more goes up from, or comes down to, the caller's memory where it lies; a smaller one passes through
// the page-locked image with its neighbours.  tests/test_gpu_context_staging.py crosses this size with the arrays of an allele
// call (it names the figure: 262 144).
constexpr size_t kDirectBytes = (size_t)256 << 10;
constexpr size_t kAlign = 256;

// Sub-buffers of one device buffer, each 256-aligned: take() every part, ensure(bytes) the DevBuf, add the offsets to its p.
struct Carve {
    size_t bytes = 0;
    size_t take(size_t n) {
        const size_t at = bytes;
        bytes += (n + kAlign - 1) & ~(kAlign - 1);
        return at;
    }
};

struct Part { size_t at; const void* mem; size_t bytes; };   // (mem == nullptr on the way up: zeros)

// One step of a transfer: a stretch [at, at + bytes) of the image and the buffer alike, a part between the buffer and `mem`,
// or zeros set on the device.
struct Copy {
    enum Kind { kImage, kDirect, kClear } kind;
    size_t at, bytes;
    const void* mem;
};

// The copies for `parts` (ascending offsets, as put() makes them).  Parts below kDirectBytes that lie side by side share one
// stretch; a stretch ends at a larger part and at any gap wider than the alignment padding (a room() between two parts is not
// sent).  Empty parts are skipped.
inline std::vector<Copy> plan(const std::vector<Part>& parts) {
    std::vector<Copy> out;
    bool open = false;   // out.back() is a stretch that the next small part may extend
    for (const Part& p : parts) {
        if (!p.bytes) continue;
        if (p.bytes >= kDirectBytes) {
            out.push_back(Copy{p.mem ? Copy::kDirect : Copy::kClear, p.at, p.bytes, p.mem});
            open = false;
        } else if (open && p.at - (out.back().at + out.back().bytes) < kAlign) {
            out.back().bytes = p.at + p.bytes - out.back().at;
        } else {
            out.push_back(Copy{Copy::kImage, p.at, p.bytes, nullptr});
            open = true;
        }
    }
    return out;
}

// What one call sends up (put, zero), what only the kernels write (room) and what comes back (get), each named once.
struct Layout {
    Carve cv;
    size_t room(size_t bytes) { return cv.take(bytes); }
    size_t zero(size_t bytes) { return put(nullptr, bytes); }
    size_t put(const void* src, size_t bytes) {
        const size_t at = cv.take(bytes);
        up_.push_back(Part{at, src, bytes});
        return at;
    }
    // a result: into `dst`, or (dst == nullptr) into the image, where at() reads it
    size_t get(void* dst, size_t bytes) {
        const size_t at = cv.take(bytes);
        down_.push_back(Part{at, dst, bytes});
        return at;
    }
    const std::vector<Part>& up() const { return up_; }

  protected:
    std::vector<Part> up_, down_;
};

}  // namespace strk_stage
