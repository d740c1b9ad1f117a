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
#include "strk_stage_plan.h"

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

using strk_stage::Carve;   // (strk_stage_plan.h)

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
// has its 256-aligned offset in the image and in the buffer alike (the layout and the plan of copies: strk_stage_plan.h).
// put() and zero() name what goes up (the bytes are read by upload(): they must still be there), room() reserves what only the
// kernels write, get() what comes back.  upload() gathers the parts into the image and sends every stretch of neighbouring
// parts with one copy; a part of kDirectBytes or more goes up from where it lies instead (the runtime locks its pages and
// copies at the same rate; gathering 12 MB first cost a call of 300 000 items more than half a millisecond,
// profiles/r30_item_stages.txt), and zeros of that size are set on the device.  download() brings the get() parts back the
// same way (small neighbours in one copy into the image, large ones straight to where they go) or one range of the buffer
// into the image; scatter() hands the small results to their arrays, and at() reads a part in the image.
// Without a stream the copies are synchronous (the item stages of an alignment file).  With one they are enqueued on it (the
// context calls, strk_ctx::side), and the image belongs to the stream until the caller has waited on it: after an upload
// nothing gathers into the same image before that wait, and after a download the image is read, and scatter() called, only
// after it.
struct Staging : strk_stage::Layout {
    static constexpr size_t kDirectBytes = strk_stage::kDirectBytes;
    explicit Staging(PinnedBuf& image) : image_(image) {}
    int upload(DevBuf& b) { return upload_by(b, Sync{}); }
    int upload(DevBuf& b, hipStream_t st) { return upload_by(b, OnStream{st}); }
    int download(const DevBuf& b, size_t from, size_t to) {   // (after upload(): the image has room for every part)
        if (to > from) HIP_TRY(Sync{}.copy(image_.at<char>(from), b.at<char>(from), to - from, hipMemcpyDeviceToHost));
        return 0;
    }
    int download(const DevBuf& b, size_t from, size_t to, hipStream_t st) {
        if (to > from) HIP_TRY(OnStream{st}.copy(image_.at<char>(from), b.at<char>(from), to - from, hipMemcpyDeviceToHost));
        return 0;
    }
    int download(const DevBuf& b, hipStream_t st) {   // every get() part
        std::vector<strk_stage::Part> parts = down_;
        for (strk_stage::Part& p : parts)
            if (!p.mem) p.mem = image_.at<char>(p.at);
        for (const strk_stage::Copy& k : strk_stage::plan(parts)) {
            void* dst = k.kind == strk_stage::Copy::kImage ? image_.at<char>(k.at) : const_cast<void*>(k.mem);
            HIP_TRY(OnStream{st}.copy(dst, b.at<char>(k.at), k.bytes, hipMemcpyDeviceToHost));
        }
        return 0;
    }
    void scatter() const {
        for (const strk_stage::Part& p : down_)
            if (p.mem && p.bytes < kDirectBytes) memcpy(const_cast<void*>(p.mem), image_.at<char>(p.at), p.bytes);
    }
    template <class T> const T* at(size_t byte_off) const { return image_.at<T>(byte_off); }
    template <class T> T* mut(size_t byte_off) { return image_.at<T>(byte_off); }   // (a result that the caller completes in place)

  private:
    struct Sync {
        hipError_t copy(void* d, const void* s, size_t n, hipMemcpyKind k) const { return hipMemcpy(d, s, n, k); }
        hipError_t clear(void* d, size_t n) const { return hipMemset(d, 0, n); }
    };
    struct OnStream {
        hipStream_t st;
        hipError_t copy(void* d, const void* s, size_t n, hipMemcpyKind k) const { return hipMemcpyAsync(d, s, n, k, st); }
        hipError_t clear(void* d, size_t n) const { return hipMemsetAsync(d, 0, n, st); }
    };
    template <class How>
    int upload_by(DevBuf& b, const How& how) {
        int rc;
        if ((rc = b.ensure(cv.bytes)) || (rc = image_.ensure(cv.bytes))) return rc;
        for (const strk_stage::Part& p : up_) {
            if (p.bytes >= kDirectBytes) continue;
            if (p.mem) memcpy(image_.at<char>(p.at), p.mem, p.bytes);
            else memset(image_.at<char>(p.at), 0, p.bytes);
        }
        for (const strk_stage::Copy& k : strk_stage::plan(up_)) {
            if (k.kind == strk_stage::Copy::kClear) HIP_TRY(how.clear(b.at<char>(k.at), k.bytes));
            else HIP_TRY(how.copy(b.at<char>(k.at), k.kind == strk_stage::Copy::kDirect ? k.mem : image_.at<char>(k.at), k.bytes, hipMemcpyHostToDevice));
        }
        return 0;
    }
    PinnedBuf& image_;
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

// A checked view of groups (strk_groups.h) into a call's staging: offsets | starts | lengths | bases.  With d_seqs the bases are
// on the device already: none are staged, and on() gives the caller's pointer.  Nor are they when no sequence has a byte.
struct StagedGroups {
    size_t off = 0, start = 0, len = 0, seqs = 0;
    const uint8_t* d_seqs = nullptr;
    struct Ptrs { const int32_t* off; const int64_t* start; const int32_t* len; const uint8_t* seqs; };
    Ptrs on(const DevBuf& b) const {
        return Ptrs{b.at<int32_t>(off), b.at<int64_t>(start), b.at<int32_t>(len), d_seqs ? d_seqs : b.at<uint8_t>(seqs)};
    }
};
inline StagedGroups stage_groups(Staging& st, const strk_groups::View& v, const strk_groups::Totals& t, const uint8_t* h_seqs, const uint8_t* d_seqs) {
    StagedGroups s;
    const size_t ns = (size_t)t.n_seqs;
    s.d_seqs = d_seqs;
    s.off = st.put(v.group_off, ((size_t)v.n_groups + 1) * 4);
    s.start = st.put(v.seq_start, ns * 8);
    s.len = st.put(v.seq_len, ns * 4);
    if (!d_seqs) s.seqs = t.total_len > 0 ? st.put(h_seqs, (size_t)v.n_seq_bytes) : st.room(1);
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
