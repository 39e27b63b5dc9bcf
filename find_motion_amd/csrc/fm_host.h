// fm_host.h — the host toolkit every device object builds on: one fail function and one try macro, owning
// device / page-locked buffers, stream and event holders.  Only the HIP runtime API and the standard
// library: a plain host compiler builds it (tests/host/fm_host_selftest.cpp).  New objects take it from here.
#pragma once

#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <cstdarg>
#include <cstddef>
#include <cstdio>
#include <string>
#include <utility>

namespace fm {

// The message into *err (may be null); returns code, so that `return failf(...)` reports and leaves.
inline int vfailf(std::string* err, int code, const char* fmt, va_list ap) {
    char buf[512];
    vsnprintf(buf, sizeof buf, fmt, ap);
    if (err) *err = buf;
    return code;
}
inline int failf(std::string* err, int code, const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vfailf(err, code, fmt, ap);
    va_end(ap);
    return code;
}

// Leaves the calling function with FM_EHIP and "<expr>: <hip error string>" in *errp when expr fails.
#define FM_HIP_TRY(errp, expr)                                                                                \
    do {                                                                                                      \
        hipError_t fm_e_ = (expr);                                                                            \
        if (fm_e_ != hipSuccess) return fm::failf(errp, FM_EHIP, "%s: %s", #expr, hipGetErrorString(fm_e_)); \
    } while (0)

struct DevMem {
    static hipError_t alloc(void** p, size_t bytes) { return hipMalloc(p, bytes); }
    static void release(void* p) { (void)hipFree(p); }
};
struct PinMem {
    static hipError_t alloc(void** p, size_t bytes) { return hipHostMalloc(p, bytes, hipHostMallocDefault); }
    static void release(void* p) { (void)hipHostFree(p); }
};

// An owning pointer with its capacity in elements: move-only, freed by the destructor.  Empty (null,
// capacity 0) or holding one live block; never dangling, never a capacity without its block.
template <class T, class Mem>
class Buf {
public:
    Buf() = default;
    Buf(const Buf&) = delete;
    Buf& operator=(const Buf&) = delete;
    Buf(Buf&& o) noexcept : p_(o.p_), cap_(o.cap_) { o.p_ = nullptr, o.cap_ = 0; }
    Buf& operator=(Buf&& o) noexcept {
        if (this != &o) {
            reset();
            std::swap(p_, o.p_);
            std::swap(cap_, o.cap_);
        }
        return *this;
    }
    ~Buf() { reset(); }

    T* get() const { return p_; }
    operator T*() const { return p_; }  // (kernel arguments, copies, subscripts)
    size_t capacity() const { return cap_; }
    void reset() {
        if (p_) Mem::release((void*)p_);
        p_ = nullptr;
        cap_ = 0;
    }
    // At least `want` elements: nothing happens when the buffer holds them already.  Otherwise the block is
    // replaced by one of `count` elements (the caller's growth policy, >= want; contents are not kept), and
    // the buffer is left empty when that allocation fails.
    hipError_t reserve(size_t want, size_t count) {
        if (p_ && want <= cap_) return hipSuccess;
        reset();
        count = std::max(count, want);
        void* p = nullptr;
        const hipError_t e = Mem::alloc(&p, std::max<size_t>(count, 1) * sizeof(T));
        if (e != hipSuccess) return e;
        p_ = (T*)p;
        cap_ = count;
        return hipSuccess;
    }
    hipError_t reserve(size_t count) { return reserve(count, count); }

private:
    T* p_ = nullptr;
    size_t cap_ = 0;
};
template <class T> using DevBuf = Buf<T, DevMem>;
template <class T> using PinBuf = Buf<T, PinMem>;

// Buffers that grow together (a device array and its page-locked copy): if any is short of `want` all are
// replaced, and a failure empties all of them, so that no two can disagree about their capacity.
template <class... B>
hipError_t reserve_all(size_t want, size_t count, B&... b) {
    if (((b.get() && want <= b.capacity()) && ...)) return hipSuccess;
    (b.reset(), ...);
    hipError_t e = hipSuccess;
    ((e = e == hipSuccess ? b.reserve(want, count) : e), ...);
    if (e != hipSuccess) (b.reset(), ...);
    return e;
}

// A stream / an event and its destruction; put() is the address a create call fills.
struct Stream {
    Stream() = default;
    Stream(const Stream&) = delete;
    Stream& operator=(const Stream&) = delete;
    ~Stream() {
        if (s) (void)hipStreamDestroy(s);
    }
    hipStream_t* put() { return &s; }
    operator hipStream_t() const { return s; }
    hipStream_t s = nullptr;
};
struct Event {
    Event() = default;
    Event(const Event&) = delete;
    Event& operator=(const Event&) = delete;
    ~Event() {
        if (e) (void)hipEventDestroy(e);
    }
    hipEvent_t* put() { return &e; }
    operator hipEvent_t() const { return e; }
    hipEvent_t e = nullptr;
};

}  // namespace fm
