// strk_host.h — what every part of the host side (strk_api.hip and the fragments spliced into it) stands on: the error
// message of the calling thread (fail, HIP_TRY) and the types that own a HIP resource and give it back when they go out of
// scope.  Host code only; no kernel sees any of this.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/strkit_amd.h"
#include "strk_bamrec.h"

namespace {

thread_local std::string g_err;

int fail(int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_err = buf;
    return code;
}

#define HIP_TRY(expr)                                                                          \
    do {                                                                                       \
        hipError_t e_ = (expr);                                                                \
        if (e_ != hipSuccess)                                                                  \
            return fail(e_ == hipErrorOutOfMemory ? STRK_E_NOMEM : STRK_E_DEVICE, "%s: %s", #expr, hipGetErrorString(e_)); \
    } while (0)

// Memory of the runtime (p, cap bytes), given back by Free.  Move-only: the one object that holds the pointer frees it.
template <hipError_t (*Free)(void*)>
struct OwnedMem {
    void* p = nullptr;
    size_t cap = 0;
    OwnedMem() = default;
    OwnedMem(const OwnedMem&) = delete;
    OwnedMem& operator=(const OwnedMem&) = delete;
    OwnedMem(OwnedMem&& o) noexcept : p(o.p), cap(o.cap) {
        o.p = nullptr;
        o.cap = 0;
    }
    OwnedMem& operator=(OwnedMem&& o) noexcept {
        if (this != &o) {
            release();
            p = o.p;
            cap = o.cap;
            o.p = nullptr;
            o.cap = 0;
        }
        return *this;
    }
    ~OwnedMem() { release(); }
    template <class T> T* as() const { return static_cast<T*>(p); }
    template <class T> T* at(size_t byte_off) const { return reinterpret_cast<T*>(static_cast<char*>(p) + byte_off); }
    void release() {
        if (p) (void)Free(p);
        p = nullptr;
        cap = 0;
    }
};

// Device memory.
struct DevBuf : OwnedMem<hipFree> {
    // head_room: a quarter more than asked for, so that a buffer that grows call by call is not re-allocated every time;
    // the two multi-gigabyte buffers of an alignment file (strk_dbam.inc) take exactly what they need
    int ensure(size_t bytes, bool head_room = true) {
        if (bytes <= cap) return 0;
        release();
        size_t want = head_room ? bytes + bytes / 4 + 256 : bytes + 256;
        hipError_t e = hipMalloc(&p, want);
        if (e != hipSuccess) {
            p = nullptr;
            (void)hipGetLastError();   // the failed hipMalloc's error is sticky per thread: a retry with less memory must not meet it
            return fail(STRK_E_NOMEM, "hipMalloc(%zu): %s", want, hipGetErrorString(e));
        }
        cap = want;
        return 0;
    }
};

// Sub-buffers of one device buffer, each 256-aligned: take() every part, ensure(bytes) the DevBuf, add the offsets to its p.
struct Carve {
    size_t bytes = 0;
    size_t take(size_t n) {
        const size_t at = bytes;
        bytes += (n + 255) & ~(size_t)255;
        return at;
    }
};

// Page-locked host memory.
struct PinnedBuf : OwnedMem<hipHostFree> {
    // exactly `bytes` (blocks of a fixed size); what the buffer held is gone
    hipError_t alloc(size_t bytes) {
        release();
        const hipError_t e = hipHostMalloc(&p, bytes, hipHostMallocDefault);
        if (e == hipSuccess) cap = bytes;
        else p = nullptr;
        return e;
    }
    // at least `bytes`, with a quarter of head-room (blocks that grow call by call)
    int ensure(size_t bytes) {
        if (bytes <= cap) return 0;
        const size_t want = bytes + bytes / 4 + 4096;
        if (alloc(want) != hipSuccess) return fail(STRK_E_NOMEM, "hipHostMalloc(%zu) failed", want);
        return 0;
    }
};

// What one call sends to a device buffer and takes back from it, as one image in page-locked memory of its owner: every part
// has its 256-aligned offset in the image and in the buffer alike.  put() and zero() name what goes up (the bytes are read by
// upload(): they must still be there), room() reserves what only the kernels write.  upload() gathers the parts into the image
// and sends every stretch of neighbouring parts with one hipMemcpy; a part of kDirectBytes or more goes up from where it lies
// instead (the runtime locks its pages and copies at the same rate; gathering 12 MB first cost a call of 300 000 items more
// than half a millisecond, profiles/r30_item_stages.txt).  download() brings one range of the buffer back into the image in
// one copy, and at() reads a part of it there.
struct Staging {
    static constexpr size_t kDirectBytes = (size_t)256 << 10;
    explicit Staging(PinnedBuf& image) : image_(image) {}
    Carve cv;
    size_t room(size_t bytes) { return cv.take(bytes); }
    size_t zero(size_t bytes) { return put(nullptr, bytes); }
    size_t put(const void* src, size_t bytes) {
        const size_t at = cv.take(bytes);
        parts_.push_back(Part{at, src, bytes});
        return at;
    }
    int upload(DevBuf& b) {
        int rc;
        if ((rc = b.ensure(cv.bytes)) || (rc = image_.ensure(cv.bytes))) return rc;
        size_t from = 0, to = 0;   // the stretch of the image that has been gathered and not sent
        for (const Part& p : parts_) {
            const bool direct = p.src && p.bytes >= kDirectBytes;
            if (direct || to == from) {
                if (to > from) HIP_TRY(hipMemcpy(b.at<char>(from), image_.at<char>(from), to - from, hipMemcpyHostToDevice));
                from = to = p.at;
            }
            if (direct) {
                HIP_TRY(hipMemcpy(b.at<char>(p.at), p.src, p.bytes, hipMemcpyHostToDevice));
                continue;
            }
            if (p.src) memcpy(image_.at<char>(p.at), p.src, p.bytes);
            else memset(image_.at<char>(p.at), 0, p.bytes);
            to = p.at + p.bytes;
        }
        if (to > from) HIP_TRY(hipMemcpy(b.at<char>(from), image_.at<char>(from), to - from, hipMemcpyHostToDevice));
        return 0;
    }
    int download(const DevBuf& b, size_t from, size_t to) {   // (after upload(): the image has room for every part)
        if (to > from) HIP_TRY(hipMemcpy(image_.at<char>(from), b.at<char>(from), to - from, hipMemcpyDeviceToHost));
        return 0;
    }
    template <class T> const T* at(size_t byte_off) const { return image_.at<T>(byte_off); }

  private:
    struct Part { size_t at; const void* src; size_t bytes; };
    PinnedBuf& image_;
    std::vector<Part> parts_;
};

// The substitute alignments of a call of n items (strk_bamrec.h, checked by check_alt) into its staging: ops | offsets | starts
// (zeros for start == NULL).  A triple that holds no operation at all is absent: on() then gives three NULLs.
struct StagedAlt {
    bool present = false;
    size_t ops = 0, off = 0, start = 0;
    strk_fe::AltCigars on(const DevBuf& b) const {
        if (!present) return strk_fe::AltCigars{nullptr, nullptr, nullptr};
        return strk_fe::AltCigars{b.at<uint32_t>(ops), b.at<int64_t>(off), b.at<int64_t>(start)};
    }
};
inline StagedAlt stage_alt(Staging& st, size_t n, const strk_fe::AltCigars& alt) {
    StagedAlt s;
    if (!alt.off || alt.off[n] <= 0) return s;
    s.present = true;
    s.ops = st.put(alt.ops, (size_t)alt.off[n] * 4);
    s.off = st.put(alt.off, (n + 1) * 8);
    s.start = alt.start ? st.put(alt.start, n * 8) : st.zero(n * 8);
    return s;
}

// A stream or an event, destroyed with its owner.  Empty until the owner creates it (hipStreamCreate...(&s.h)); converts to the
// plain handle wherever the runtime wants one.
template <class H, hipError_t (*Destroy)(H)>
struct Handle {
    H h = nullptr;
    Handle() = default;
    Handle(const Handle&) = delete;
    Handle& operator=(const Handle&) = delete;
    ~Handle() { if (h) (void)Destroy(h); }
    operator H() const { return h; }
};
using Stream = Handle<hipStream_t, hipStreamDestroy>;
using Event = Handle<hipEvent_t, hipEventDestroy>;

}  // namespace
