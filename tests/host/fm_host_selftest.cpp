// fm_host_selftest.cpp — fm_host.h's buffers and holders against a malloc-backed stand-in for the HIP runtime
// that counts live allocations and can fail the k-th one.  A stand-alone host program (no libamdhip64), built
// with AddressSanitizer and UBSan by tests/test_fm_host_selftest.py.  One script of reserves, group reserves
// and moves runs with every allocation failing in turn and once with none: whatever fails, a buffer (or its
// whole group) is empty afterwards, and nothing is left allocated at the end.
#include <cstdio>
#include <cstdlib>
#include <utility>

#include "../../find_motion_amd/csrc/fm_host.h"
#include "../../include/find_motion_amd.h"

static int g_live = 0;      // allocations, streams and events not yet released
static int g_allocs = 0;    // allocations asked for in this run
static int g_fail_at = 0;   // the allocation (1-based) that fails; 0: none

static hipError_t fake_alloc(void** p, size_t bytes) {
    if (++g_allocs == g_fail_at) {
        *p = nullptr;
        return hipErrorOutOfMemory;
    }
    *p = std::malloc(bytes ? bytes : 1);
    g_live++;
    return hipSuccess;
}
template <class H>
static hipError_t fake_handle(H* h) {
    *h = (H)std::malloc(1);
    g_live++;
    return hipSuccess;
}
static hipError_t fake_release(void* p) {
    if (p) g_live--;
    std::free(p);
    return hipSuccess;
}

hipError_t hipMalloc(void** p, size_t bytes) { return fake_alloc(p, bytes); }
hipError_t hipHostMalloc(void** p, size_t bytes, unsigned int) { return fake_alloc(p, bytes); }
hipError_t hipFree(void* p) { return fake_release(p); }
hipError_t hipHostFree(void* p) { return fake_release(p); }
hipError_t hipStreamCreate(hipStream_t* s) { return fake_handle(s); }
hipError_t hipStreamCreateWithFlags(hipStream_t* s, unsigned int) { return fake_handle(s); }
hipError_t hipStreamDestroy(hipStream_t s) { return fake_release(s); }
hipError_t hipEventCreate(hipEvent_t* e) { return fake_handle(e); }
hipError_t hipEventCreateWithFlags(hipEvent_t* e, unsigned) { return fake_handle(e); }
hipError_t hipEventDestroy(hipEvent_t e) { return fake_release(e); }
const char* hipGetErrorString(hipError_t e) { return e == hipErrorOutOfMemory ? "out of memory" : "error"; }

static int g_bad = 0;
#define CHECK(cond)                                                                              \
    do {                                                                                         \
        if (!(cond)) {                                                                           \
            std::fprintf(stderr, "line %d (failing allocation %d): %s\n", __LINE__, g_fail_at, #cond); \
            g_bad++;                                                                             \
        }                                                                                        \
    } while (0)

template <class B>
static bool empty(const B& b) {
    return b.get() == nullptr && b.capacity() == 0;
}

// a reserve that ended as e: the buffer holds what was asked for, or nothing
template <class B>
static void check_reserved(const B& b, hipError_t e, size_t want, size_t count) {
    if (e == hipSuccess) {
        CHECK(b.get() != nullptr && b.capacity() >= want && b.capacity() <= count);
        for (size_t i = 0; i < b.capacity(); i++) b.get()[i] = {};  // (the block really has capacity() elements)
    } else {
        CHECK(empty(b));
    }
}

static int try_reserve(std::string* err, fm::DevBuf<int>& b, size_t n) {
    FM_HIP_TRY(err, b.reserve(n));
    return FM_OK;
}

static void script() {
    fm::Stream st;
    fm::Event ev;
    CHECK(hipStreamCreateWithFlags(st.put(), 0) == hipSuccess && (hipStream_t)st != nullptr);
    CHECK(hipEventCreate(ev.put()) == hipSuccess && (hipEvent_t)ev != nullptr);

    fm::DevBuf<int> a;
    CHECK(empty(a));
    hipError_t e = a.reserve(10);
    check_reserved(a, e, 10, 10);
    int* first = a.get();
    e = a.reserve(5);  // smaller: nothing happens to a buffer that holds its block
    if (first) CHECK(e == hipSuccess && a.get() == first && a.capacity() == 10);
    else check_reserved(a, e, 5, 5);
    e = a.reserve(20, 30);  // larger: replaced by the policy's count
    check_reserved(a, e, 20, 30);
    if (e == hipSuccess) CHECK(a.capacity() == 30);

    fm::DevBuf<double> d0;
    fm::DevBuf<char> d1;
    fm::PinBuf<double> h0;
    fm::PinBuf<char> h1;
    for (size_t want : {(size_t)8, (size_t)200}) {
        e = fm::reserve_all(want, want + want / 4 + 64, d0, d1, h0, h1);
        if (e == hipSuccess) {
            check_reserved(d0, e, want, want + want / 4 + 64);
            check_reserved(d1, e, want, want + want / 4 + 64);
            check_reserved(h0, e, want, want + want / 4 + 64);
            check_reserved(h1, e, want, want + want / 4 + 64);
            CHECK(d0.capacity() == d1.capacity() && d1.capacity() == h0.capacity() && h0.capacity() == h1.capacity());
        } else {
            CHECK(empty(d0) && empty(d1) && empty(h0) && empty(h1));
        }
    }

    int* held = a.get();
    const size_t cap = a.capacity();
    fm::DevBuf<int> m(std::move(a));  // the block moves, the source is empty
    CHECK(empty(a) && m.get() == held && m.capacity() == cap);
    fm::DevBuf<int> m2;
    e = m2.reserve(3);
    check_reserved(m2, e, 3, 3);
    m2 = std::move(m);  // releases m2's own block
    CHECK(empty(m) && m2.get() == held && m2.capacity() == cap);

    std::string msg;
    fm::DevBuf<int> t;
    const int rc = try_reserve(&msg, t, 7);  // FM_HIP_TRY: FM_EHIP and "<expr>: <error string>"
    if (rc == FM_OK) CHECK(t.capacity() == 7 && msg.empty());
    else CHECK(rc == FM_EHIP && empty(t) && msg == "b.reserve(n): out of memory");
    CHECK(fm::failf(nullptr, FM_EINVAL, "%d", 1) == FM_EINVAL);
    m2.reset();
    CHECK(empty(m2));
}

int main() {
    script();
    CHECK(g_live == 0);
    const int total = g_allocs;
    CHECK(total == 12);  // two reserves that allocate, two groups of four, two more
    for (int k = 1; k <= total; k++) {
        g_allocs = 0;
        g_fail_at = k;
        script();
        CHECK(g_live == 0);
        CHECK(g_allocs >= k);  // the failing allocation was reached
    }
    std::printf("fm_host selftest: %d failing positions, %d errors\n", total, g_bad);
    return g_bad ? 1 : 0;
}
