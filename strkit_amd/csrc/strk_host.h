// strk_host.h — what every part of the host side (strk_api.hip and the fragments spliced into it) stands on: the error
// message of the calling thread (fail, HIP_TRY) and the types that own a HIP resource and give it back when they go out of
// scope.  Host code only; no kernel sees any of this.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdio>
#include <string>

#include "../../include/strkit_amd.h"

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
