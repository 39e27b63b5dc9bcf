// fm_timer.cpp — KernelTimer (fm_internal.h): per-kernel timing by events or in-kernel stamps.
#include <algorithm>
#include <cstdio>
#include <cstring>

#include "fm_internal.h"

namespace fm {
int KernelTimer::id_of(const char* name) {
    for (size_t i = 0; i < names.size(); i++)
        if (names[i] == name || std::strcmp(names[i], name) == 0) return (int)i;
    names.push_back(name);
    ms.push_back(0);
    ms_sq.push_back(0);
    stamped.push_back(0);
    stamped_ms.push_back(0);
    busy.push_back(Busy{});
    launches.push_back(0);
    calls.push_back(0);
    return (int)names.size() - 1;
}
int KernelTimer::begin(const char* name, hipStream_t st) {
    if (!enabled) return -1;
    if (!st) st = stream;
    if (pixel_only && st != stream && st != stream2) return -1;
    const int id = id_of(name);
    // events on every launch cost the pipeline ~7% (each record is a barrier packet):
    // the pixel-only mode times a sample of the launches of the kernels it cannot stamp
    if (pixel_only && calls[id]++ % kSample != 0) return -1;
    hipEvent_t a, b;
    if (pool.size() >= 2) {
        a = pool.back(); pool.pop_back();
        b = pool.back(); pool.pop_back();
    } else {
        if (hipEventCreate(&a) != hipSuccess || hipEventCreate(&b) != hipSuccess) return -1;
    }
    (void)hipEventRecord(a, st);
    pending.push_back({id, a, b, st});
    return (int)pending.size() - 1;
}
void KernelTimer::end(int token) {
    if (token < 0 || token >= (int)pending.size()) return;
    (void)hipEventRecord(pending[token].b, pending[token].st);
}
void KernelTimer::collect() {
    std::vector<Rec> keep;
    for (auto& r : pending) {
        if (hipEventQuery(r.b) == hipErrorNotReady) {  // a later batch still running
            keep.push_back(r);
            continue;
        }
        float t = 0;
        if (hipEventElapsedTime(&t, r.a, r.b) == hipSuccess) {
            ms[r.id] += t;
            launches[r.id] += 1;
        }
        pool.push_back(r.a);
        pool.push_back(r.b);
    }
    pending.swap(keep);
}
// Stamped launches (pixel-only mode): the round-4 sampled events opened their window at the marker
// ahead of the kernel, so it took in the queue's waits, and one launch in four was a biased sample
// (a sampled mean of 709 us against a 655.5 us step).  Stamps time every launch from its first
// workgroup's start to its last wave's end.
uint64_t* KernelTimer::stamp(const char* name) {
    if (!enabled || !pixel_only) return nullptr;
    if (!d_stamps) {
        if (hipMalloc(&d_stamps, sizeof(uint64_t) * 2 * kStampRing) != hipSuccess) {
            d_stamps = nullptr;
            enabled = false;
            return nullptr;
        }
        std::vector<uint64_t> init(2 * kStampRing);
        for (int i = 0; i < kStampRing; i++) init[2 * i] = ~0ull, init[2 * i + 1] = 0;
        if (hipMemcpy(d_stamps, init.data(), init.size() * sizeof(uint64_t), hipMemcpyHostToDevice) != hipSuccess) {
            enabled = false;
            return nullptr;
        }
    }
    const int id = id_of(name);
    if ((int)stamp_ids.size() >= kStampRing) {
        unstamped++;
        return nullptr;
    }
    stamp_ids.push_back(id);
    return d_stamps + 2 * (stamp_ids.size() - 1);
}
int KernelTimer::fold_stamps() {
    if (stamp_ids.empty()) return 0;
    if (stream) (void)hipStreamSynchronize(stream);
    if (stream2) (void)hipStreamSynchronize(stream2);
    if (stream3) (void)hipStreamSynchronize(stream3);
    for (hipStream_t st : extra) (void)hipStreamSynchronize(st);  // (an entry read while its kernel runs is lost)
    const size_t n = stamp_ids.size();
    std::vector<uint64_t> v(2 * n);
    if (hipMemcpy(v.data(), d_stamps, v.size() * sizeof(uint64_t), hipMemcpyDeviceToHost) != hipSuccess) return -1;
    const bool dump = dev_env("FM_STAMP_DUMP") != nullptr;  // dev build: every launch's window to stderr
    for (size_t i = 0; i < n; i++) {
        if (dump) std::fprintf(stderr, "kstamp %s %llu %llu\n", names[stamp_ids[i]], (unsigned long long)v[2 * i],
                               (unsigned long long)v[2 * i + 1]);
        if (v[2 * i] == ~0ull || v[2 * i + 1] <= v[2 * i]) continue;  // (a kernel that does not stamp)
        const double t = (double)(v[2 * i + 1] - v[2 * i]) * 1e-5;  // 100 MHz ticks -> ms
        ms[stamp_ids[i]] += t;
        ms_sq[stamp_ids[i]] += t * t;
        stamped[stamp_ids[i]] += 1;
        stamped_ms[stamp_ids[i]] += t;
        launches[stamp_ids[i]] += 1;
    }
    // the union of each kernel's launch windows (launches of one kernel may overlap: two input streams)
    std::vector<std::pair<uint64_t, uint64_t>> iv;
    for (size_t id = 0; id < names.size(); id++) {
        iv.clear();
        for (size_t i = 0; i < n; i++)
            if (stamp_ids[i] == (int)id && v[2 * i] != ~0ull && v[2 * i + 1] > v[2 * i]) iv.emplace_back(v[2 * i], v[2 * i + 1]);
        std::sort(iv.begin(), iv.end());
        Busy& b = busy[id];
        for (const auto& [s0, e0] : iv) {
            if (b.open && s0 <= b.e) {
                b.e = std::max(b.e, e0);
                continue;
            }
            if (b.open) b.ms += (double)(b.e - b.s) * 1e-5;
            b.s = s0, b.e = e0, b.open = true;
        }
    }
    for (size_t i = 0; i < n; i++) v[2 * i] = ~0ull, v[2 * i + 1] = 0;
    stamp_ids.clear();
    return hipMemcpy(d_stamps, v.data(), v.size() * sizeof(uint64_t), hipMemcpyHostToDevice) == hipSuccess ? 0 : -1;
}
void KernelTimer::reset() {
    fold_stamps();  // (launches stamped before the reset are dropped with the sums below)
    std::fill(ms.begin(), ms.end(), 0.0);
    std::fill(ms_sq.begin(), ms_sq.end(), 0.0);
    std::fill(stamped.begin(), stamped.end(), 0);
    std::fill(stamped_ms.begin(), stamped_ms.end(), 0.0);
    std::fill(busy.begin(), busy.end(), Busy{});
    std::fill(launches.begin(), launches.end(), 0);
    std::fill(calls.begin(), calls.end(), 0);
    unstamped = 0;
}
KernelTimer::~KernelTimer() {
    if (d_stamps) (void)hipFree(d_stamps);
    for (auto& r : pending) {
        (void)hipEventDestroy(r.a);
        (void)hipEventDestroy(r.b);
    }
    for (auto e : pool) (void)hipEventDestroy(e);
}
}  // namespace fm
