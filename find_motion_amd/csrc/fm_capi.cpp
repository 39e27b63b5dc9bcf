// fm_capi.cpp — C ABI of the MI355X motion-detection hot path (include/find_motion_amd.h).
//
// Owns the per-context device state (background models, masks, batch
// buffers), has the host-side tables OpenCV builds per call (fm_tables.cpp)
// built once at fm_create, and sequences the kernels of the fm_*.hip files
// on the context's streams (submit: one short function, one stage each).
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <unordered_map>
#include <vector>

#include "fm_scan.h"
#include "fm_roi.h"

namespace fm {
hipError_t launch_pixel_pp(hipStream_t st, const PixelArgs& a, const double* bg_in, double* bg_out);
int pixel_lds_bytes(int ksize);
}  // namespace fm

using namespace fm;

namespace {

thread_local std::string g_last_error;

using ResizeMode = AreaMode::Kind;
constexpr fm_ctx* kNoCtx = nullptr;  // a failure before a context exists: fm_last_error(nullptr) has it

}  // namespace

// The pixel stage of a context, and what follows from it.
enum class PixelPath { PerFrame, Fused, Pix, Small, Wide, Rgb, Mog2 };
using ScanLaunch = hipError_t (*)(hipStream_t, const FusedArgs&, uint8_t*, uint64_t*, uint64_t*);
struct PathTraits {
    const char* name;  // fm_plan's pixel_path
    bool tiles;        // the tile machinery sits behind it: batch slots, tile CCL (else one launch per frame, pixel CCL)
    bool bits;         // it writes threshold bits for the dilating contour pass (else k_fused dilates itself)
    bool scan;         // a blur + scan path (fm_scan.h): it writes its own tile flags, 8 words per tile-frame, and
                       // k_tile_flags is not run for it
    int bg_ch;         // doubles per work pixel of the background: [h][w][3] on a colour context, none for a mixture
    int blur_ch;       // channels of a slot's blur scratch
    ScanLaunch launch;           // a scan path's blur + scan pair (Mog2 launches its two kernels itself)
    const char* timer[2][3];     // and its timer names, steady / init launch: blur, scan, the pair under events
};
constexpr PathTraits kPathTraits[] = {
    {"pixel", false, false, false, 1, 0, nullptr, {}},
    {"fused", true, false, false, 1, 0, nullptr, {}},
    {"pix", true, true, false, 1, 0, nullptr, {}},
    {"small", true, true, true, 1, 1, launch_small,
     {{"small_blur", "small_scan", "small"}, {"small_blur_init", "small_scan_init", "small_init"}}},
    {"wide", true, true, true, 1, 1, launch_wide,
     {{"wide_blur", "wide_scan", "wide"}, {"wide_blur_init", "wide_scan_init", "wide_init"}}},
    {"rgb", true, true, true, 3, 3, launch_rgb,
     {{"rgb_blur", "rgb_scan", "rgb"}, {"rgb_blur_init", "rgb_scan_init", "rgb_init"}}},
    {"mog2", true, true, true, 0, 1, nullptr, {}},
};

// One batch's device results.  The fused paths keep kSlots slots: the pixel
// kernels run in submission order on the pixel stream (the background
// recurrence), each slot's contour pass on its own stream, so the latency-bound
// contour passes of consecutive batches overlap each other and the next
// batches' pixel kernels.
#ifndef FM_SLOTS
// with the labelling gate a chain finishes later, and 4 slots left the pixel stream idle while the host waited
// to reuse one: 6 slots 406.4 vs 396.4 k frames/s (4 alternating rounds, round 3).  Round 5, 6 / 8 / 10 slots
// (profiles/r05q_slots_ab.txt): the driver's command 374-409 / 401-403 / 393-413 k, mode D (60 steps)
// 762-767 / 775-792 / 801-805 k; a slot is ~0.41 GB of device memory at the headline shape
#define FM_SLOTS 10
#endif
constexpr int kSlots = FM_SLOTS;
constexpr int kWideSlots = 4;  // batch slots of the wide-Gaussian path (its slots carry the blur scratch)
constexpr size_t kRgbSlotBytes = size_t(256) << 20;  // colour motion: blur scratch of a slot above which kWideSlots
struct BatchSlot {
    uint8_t* d_in = nullptr;        // host-fed staging [T][S][H][W][3]
    uint8_t* d_yuv = nullptr;       // host-fed YUV staging of fm_submit_yuv (first use; grown on demand)
    size_t yuv_cap = 0;             // its bytes
    const uint8_t** d_ytab = nullptr;  // fm_submit_yuv_list: the batch's frame addresses [max_batch * S] on the device
    const uint8_t** h_ytab = nullptr;  // and their page-locked staging
    uint8_t* d_work = nullptr;      // resized BGR [T][S][h][w][3] (mode D)
    uint8_t* d_planes = nullptr;    // [3][T][S][h*w] gray, blur, frame_delta (FM_FLAG_KEEP_PLANES)
    uint64_t* d_bits = nullptr;     // threshold bit rows (k_pix output)
    uint8_t* d_blur = nullptr;      // blur + scan paths: blur bytes [T*S][channels][w][nty * 64] between the two kernels
    float* d_alpha = nullptr;       // Gaussian mixture: the learning rate of each frame [T][S]
    float* h_alpha = nullptr;       // and its page-locked staging
    uint64_t* d_dbits = nullptr;    // dilated bit rows = VideoFrame.thresh
    TileRec* d_tiles = nullptr;
    NodeRec* d_nodes = nullptr;
    uint32_t* d_tflag = nullptr;    // [F][ntiles] where tiles have threshold bits
    uint8_t* d_candf = nullptr;     // [F][ntiles] tiles the contour pass labelled
    int32_t* d_clist = nullptr;     // [F][ntiles] candidate lists
    int32_t* d_rlist = nullptr;     // [F][ntiles] empty-region representatives
    int32_t* d_regrep = nullptr;    // [F][ntiles] empty tile -> region representative
    int32_t* d_ncr = nullptr;       // [F][2]
    int32_t* d_heavy = nullptr;     // [F * ntiles] heavy-tile list
    int32_t* d_count = nullptr;     // [3F+3]: counts, overflow flags, pool / heavy words, frame quotas, frames done
    int32_t* h_count = nullptr;     // pinned [F]
    int32_t* h_overflow = nullptr;  // pinned [F]
    int32_t* dh_count = nullptr;     // device aliases of the two (mapped): the fused path's k_counts writes them
    int32_t* dh_overflow = nullptr;
    int32_t* h_stats = nullptr;     // mapped [2]: shared-pool nodes, heavy tiles (k_counts)
    int32_t* dh_stats = nullptr;
    int32_t* h_rec = nullptr;       // mapped pinned [F][cap][5], written by the kernels
    int32_t* d_rec = nullptr;       // device alias of h_rec
    uint8_t* h_init = nullptr;      // pinned [S]
    hipEvent_t ev_pix = nullptr, ev_done = nullptr, ev_rs = nullptr, ev_lab = nullptr;  // (ev_lab: labelling done)
    hipEvent_t ev_in = nullptr;     // caller's stream (fm_set_hip_stream): its work queued before the submit
    hipStream_t ccl_stream = nullptr;  // this slot's contour pass (slots' passes run concurrently)
    int n = 0;                      // frames in flight in this slot (0 = none)
    FusedArgs fa{};                 // the contour pass's arguments (fm_wait re-emits frames past the cap)
    uint64_t gen = 0;               // submits into this slot
    size_t ccl_F = 0;               // frames (T*S) of the slot's last k_frame_contours batch (its re-armed words)
    const uint8_t* src = nullptr;   // the batch's source frames [T][S][H][W][3] on the device (fm_read_frame)
};

struct fm_ctx {
    fm_params p{};
    int h = 0, w = 0;
    size_t src_frame_bytes = 0, work_plane = 0;
    ResizeMode rmode = ResizeMode::Identity;
    int fast_sx = 1, fast_sy = 1;
    AreaAxis ax, ay;
    AreaUpAxis upx, upy;  // FM_FLAG_AREA_UPSCALE: the enlarging resize's taps and its kernel's tiling
    AreaUpPlan up_plan{};
    std::vector<int32_t> coef;

    // streams: pixel work (caller-replaceable), contour pass, synchronous reads
    hipStream_t own_stream = nullptr, stream = nullptr, aux_stream = nullptr;
    hipStream_t rs_stream = nullptr;  // input stream: host copies + resize, ahead of the pixel stream
    hipStream_t rs_stream2 = nullptr; // second input stream (odd slots' resizes), created with the first resize
    hipStream_t ccl_streams[kSlots] = {};
    int lab_prev = -1;  // slot of the last batch whose labelling was enqueued (the labelling gate)
    int nccl = 1;
    KernelTimer timer;

    // device state shared by all batches
    double* d_bg[2] = {nullptr, nullptr};
    int bg_cur = 0;
    uint8_t* d_keep = nullptr;    // [S][h*w]
    uint8_t* d_has_keep = nullptr;
    uint8_t* d_init = nullptr;
    uint8_t* d_mask = nullptr;    // fused: one plane (fm_read_mask expansion, pixel-CCL fallback); v1: [T][S][h*w]
    int32_t* d_label = nullptr;   // pixel-level CCL (v1 path, fused-path overflow fallback)
    int32_t* d_cid = nullptr;
    uint8_t* d_outer = nullptr;
    int32_t* d_rec_dev = nullptr;  // per-frame path: the batch's pixel-level CCL records [frames][max_contours][5]
    int32_t* d_rec_one = nullptr;  // relabel_frame: one frame's records [rec_one_cap][5] (grown on demand)
    size_t rec_one_cap = 0;
    int32_t* d_area = nullptr;     // FM_FLAG_CONTOUR_AREA: jobs [area_cap][3] + areas [area_cap]
    size_t area_cap = 0;
    // FM_FLAG_CONTOUR_POINTS (contour_points): all grown on demand, from counts known beforehand
    int32_t* d_trace = nullptr;    // jobs [trace_cap][8] + path lists [trace_cap] + results [trace_cap][3] + error word
    size_t trace_cap = 0;
    int32_t* d_cpts = nullptr;     // the batch's points [cpts_cap][2]
    size_t cpts_cap = 0;
    int32_t* h_pts = nullptr;      // page-locked copy of them: one device-to-host copy per batch
    size_t h_pts_cap = 0;
    std::vector<size_t> pts_off;   // [ready * S + 1] first point of each (t*S+s); empty before the first traced batch
    int32_t trace_n[2] = {0, 0};   // contours of the last waited batch traced staged (registers, LDS) / unstaged
    int64_t trace_steps = 0;       // border steps their count pass walked
    int32_t* d_rec_all = nullptr;  // k_emit_all records of one frame [rec_all_cap][5] + counter
    size_t rec_all_cap = 0;
    int rec_cap = 0;          // records per frame in each slot's mapped buffer (the first fetch; more -> k_emit_all)
    size_t dev_bytes = 0;     // device bytes the context holds now (fm_footprint)
    size_t pinned_bytes = 0;  // and its page-locked host allocations
    std::unordered_map<const void*, size_t> dev_sizes, pin_sizes;  // every buffer of either kind it owns -> its bytes
    PixelPath path = PixelPath::PerFrame;  // decided once by plan_context; everything else reads its traits
    const PathTraits& traits() const { return kPathTraits[(int)path]; }
    bool small_blur = false;       // Mog2: k_small_blur in front of the scan (small_supported), else k_wide_blur
    fm_mog2_params mog2{};         // its parameters
    float* d_mog_state = nullptr;  // [S][15][w][nty * 64] weight, mean, var of the five modes (fm_mog2.hip)
    uint8_t* d_mog_nm = nullptr;   // [S][w][nty * 64] modes in use
    uint8_t* d_mog_bg = nullptr;   // [h*w] fm_mog2_background's image
    std::vector<int64_t> mog_nframes;  // [S] frames each stream's model has seen (advanced at submit)
    bool frame_ccl = false;        // the contour pass as one workgroup per frame (ntiles <= kFrameCclTiles)
    int ntx = 0, nty = 0, ntiles = 0, nnodes = 0;  // nnodes: per batch slot
    int nquota = 0;                                             // nodes of each frame's quota
    int32_t *d_xofs = nullptr, *d_xcnt = nullptr, *d_yofs = nullptr, *d_ycnt = nullptr;
    float *d_xwt = nullptr, *d_ywt = nullptr;
    uint32_t *d_upx = nullptr, *d_upy = nullptr;

    // batches
    BatchSlot slots[kSlots];
    int nslots = 1;
    int next_slot = 0;
    std::vector<int> inflight;     // FIFO of submitted, not yet waited slots
    int ready_slot = -1;           // slot of the last waited batch
    uint64_t ready_gen = 0;
    int ready = 0;                 // frames of the last waited batch
    int fallbacks = 0;             // its frames relabelled by the pixel-level CCL (node pool exhausted)
    int32_t stats[2] = {0, 0};     // its contour pass: nodes from the shared pool, heavy tiles
    std::vector<int32_t> ready_counts;                    // [ready * S]
    std::vector<std::vector<fm_contour>> contours;        // per (t*S+s), sorted

    // retained source frames (fm_retain_reserve): ret_used.size() entries of ret_stride bytes each, outside the slots
    uint8_t* d_ret = nullptr;
    size_t ret_stride = 0;          // src_frame_bytes rounded up to 256
    std::vector<uint8_t> ret_used;  // per entry: handed out by fm_retain_frames, not yet released
    int ret_in_use = 0;
    RetainPair* d_rtab = nullptr;   // the copies of one fm_retain_frames call, [entries] on the device
    RetainPair* h_rtab = nullptr;   // and their page-locked staging

    std::vector<uint8_t> bg_init, has_keep;
    std::string err;
    uint64_t* d_ts = nullptr;     // FM_TS: contour-pass phase stamps (profiling)
    uint64_t* d_pts = nullptr;    // FM_PTS=<file>: k_pix workgroup stamps of the last launch (profiling)
    int pts_ring = 1;             // FM_PTS_RING=<n>: stamps of the last n launches, oldest first (profiling)
    long long pts_launches = 0;
    int32_t* h_err = nullptr;     // mapped: FM_OOB violation bits (checked build), 0 otherwise
    int32_t* dh_err = nullptr;
    std::vector<double> ts_sum;   // summed phase deltas (cycles)
    std::vector<int64_t> ts_n;
    bool serial = false;  // FM_SERIAL: contour pass on the pixel stream (profiling: no overlap)
    int dbg_skip = 0;  // FM_DEBUG_SKIP: profiling-only stage ablation of k_fused (results invalid)

    // Releases everything the context took, also when fm_create gave up half way (nothing was enqueued
    // on its streams then; fm_destroy synchronises them first).
    ~fm_ctx() {
        for (hipStream_t st : ccl_streams)
            if (st) (void)hipStreamDestroy(st);
        for (hipStream_t st : {own_stream, aux_stream, rs_stream, rs_stream2})
            if (st) (void)hipStreamDestroy(st);
        for (BatchSlot& b : slots)
            for (hipEvent_t ev : {b.ev_pix, b.ev_done, b.ev_rs, b.ev_lab, b.ev_in})
                if (ev) (void)hipEventDestroy(ev);
        for (const auto& kv : dev_sizes) (void)hipFree(const_cast<void*>(kv.first));
        for (const auto& kv : pin_sizes) (void)hipHostFree(const_cast<void*>(kv.first));
    }
};

namespace fm {
// fm_host.h's failf for a context (FM_HIP_TRY(c, ...) too): the message is also the thread's last error
int failf(fm_ctx* c, int code, const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vfailf(&g_last_error, code, fmt, ap);
    va_end(ap);
    if (c) c->err = g_last_error;
    return code;
}
}  // namespace fm

namespace {

// Device and page-locked memory of the context: every allocation is entered in c->dev_sizes /
// c->pin_sizes (fm_footprint's totals), and ~fm_ctx frees whatever the two still hold.
template <class T>
int dalloc(fm_ctx* c, T** p, size_t count) {
    if (count == 0) count = 1;
    hipError_t e = hipMalloc((void**)p, count * sizeof(T));
    if (e != hipSuccess) return failf(c, FM_ENOMEM, "hipMalloc(%zu bytes): %s", count * sizeof(T), hipGetErrorString(e));
    c->dev_bytes += count * sizeof(T);
    c->dev_sizes[*p] = count * sizeof(T);
    return FM_OK;
}

template <class T>
hipError_t halloc(fm_ctx* c, T** p, size_t bytes, unsigned flags) {
    hipError_t e = hipHostMalloc((void**)p, bytes, flags);
    if (e == hipSuccess) {
        c->pinned_bytes += bytes;
        c->pin_sizes[*p] = bytes;
    }
    return e;
}

// At least `want` units in *p, whose capacity *cap counts the same units: a smaller buffer is replaced
// by one of `count` elements (contents not preserved) and leaves the footprint.
template <class T>
int grow(fm_ctx* c, T** p, size_t* cap, size_t want, size_t count) {
    if (want <= *cap) return FM_OK;
    if (auto it = c->dev_sizes.find(*p); it != c->dev_sizes.end()) {
        (void)hipFree(*p);
        c->dev_bytes -= it->second;
        c->dev_sizes.erase(it);
    }
    *p = nullptr;
    *cap = 0;
    if (int rc = dalloc(c, p, count)) return rc;
    *cap = want;
    return FM_OK;
}

// the page-locked counterpart
template <class T>
int grow_pinned(fm_ctx* c, T** p, size_t* cap, size_t want, size_t count) {
    if (want <= *cap) return FM_OK;
    if (auto it = c->pin_sizes.find(*p); it != c->pin_sizes.end()) {
        (void)hipHostFree(*p);
        c->pinned_bytes -= it->second;
        c->pin_sizes.erase(it);
    }
    *p = nullptr;
    *cap = 0;
    hipError_t e = halloc(c, p, count * sizeof(T), hipHostMallocDefault);
    if (e != hipSuccess) return failf(c, FM_ENOMEM, "hipHostMalloc(%zu bytes): %s", count * sizeof(T), hipGetErrorString(e));
    *cap = want;
    return FM_OK;
}

int check_idle(fm_ctx* c) {
    if (!c->inflight.empty()) return failf(c, FM_ESTATE, "a submit is in flight: call fm_wait first");
    return FM_OK;
}

int check_stream(fm_ctx* c, int stream) {
    if (stream < 0 || stream >= c->p.n_streams) return failf(c, FM_EINVAL, "stream %d out of range", stream);
    return FM_OK;
}

// results of the last waited batch (device-side ones live until its slot is resubmitted)
int check_frame(fm_ctx* c, int frame, int stream, bool device_data) {
    if (int rc = check_stream(c, stream)) return rc;
    if (frame < 0 || frame >= c->ready) return failf(c, FM_EINVAL, "frame %d not in the last batch (%d frames)", frame, c->ready);
    if (device_data && (c->ready_slot < 0 || c->slots[c->ready_slot].gen != c->ready_gen))
        return failf(c, FM_ESTATE, "the batch's device results were overwritten by a later submit");
    return FM_OK;
}

// every record of frame f of a finished fused-path batch (count known from k_emit)
int emit_all(fm_ctx* c, BatchSlot& B, size_t f, int count, std::vector<int32_t>& out) {
    if (int rc = grow(c, &c->d_rec_all, &c->rec_all_cap, (size_t)count, (size_t)count * 5 + 1)) return rc;
    hipStream_t st = c->aux_stream;
    int32_t* cnt = c->d_rec_all + (size_t)count * 5;
    FM_HIP_TRY(c, hipMemsetAsync(cnt, 0, sizeof(int32_t), st));
    FM_HIP_TRY(c, launch_emit_all(st, B.fa, (int)f, c->d_rec_all, cnt, count));
    out.resize((size_t)count * 5 + 1);
    FM_HIP_TRY(c, hipMemcpyAsync(out.data(), c->d_rec_all, out.size() * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    FM_HIP_TRY(c, hipStreamSynchronize(st));
    if (out.back() != count) return failf(c, FM_EHIP, "re-emit of frame %zu found %d contours, not %d", f, out.back(), count);
    out.pop_back();
    return FM_OK;
}

// frame f of a fused-path batch through the pixel-level CCL (from its dilated bit rows):
// all records into out, the count into count
int relabel_frame(fm_ctx* c, BatchSlot& B, size_t f, std::vector<int32_t>& out, int& count) {
    hipStream_t st = c->aux_stream;
    int32_t* dcnt = B.d_count + f;  // this frame's contour counter (the batch is finished)
    const uint8_t* mask = c->d_mask + f * c->work_plane;  // per-frame path: the batch's dilated masks
    if (c->traits().tiles) {
        FM_HIP_TRY(c, launch_expand_bits(st, B.d_dbits + f * c->ntiles * 64, B.d_candf + f * c->ntiles, c->d_mask, c->h,
                                      c->w, c->ntx));
        mask = c->d_mask;
    }
    for (int pass = 0; pass < 2; pass++) {
        FM_HIP_TRY(c, hipMemsetAsync(dcnt, 0, sizeof(int32_t), st));
        FM_HIP_TRY(c, hipMemsetAsync(c->d_outer, 0, c->work_plane, st));
        // its own record buffer: the per-frame path's d_rec_dev holds [frames][max_contours] records
        // for every submit and must keep that size
        CclArgs ca{mask, c->d_label, c->d_outer, c->d_cid, dcnt, c->d_rec_one, 1, c->h, c->w, (int)c->rec_one_cap};
        FM_HIP_TRY(c, launch_ccl(st, ca, nullptr));
        int32_t n = 0;
        FM_HIP_TRY(c, hipMemcpyAsync(&n, dcnt, sizeof(int32_t), hipMemcpyDeviceToHost, st));
        FM_HIP_TRY(c, hipStreamSynchronize(st));
        if ((size_t)n <= c->rec_one_cap) {
            count = n;
            out.resize((size_t)n * 5);
            FM_HIP_TRY(c, hipMemcpyAsync(out.data(), c->d_rec_one, out.size() * sizeof(int32_t), hipMemcpyDeviceToHost, st));
            FM_HIP_TRY(c, hipStreamSynchronize(st));
            return FM_OK;
        }
        if (int rc = grow(c, &c->d_rec_one, &c->rec_one_cap, (size_t)n, (size_t)n * 5)) return rc;
    }
    return failf(c, FM_EHIP, "pixel-level relabel of frame %zu did not converge", f);
}

// FM_FLAG_CONTOUR_AREA: 2 x contourArea of every contour of the finished batch in slot B, traced
// on the GPU from its start pixel on the batch's dilated masks (fm.py:679)
int contour_areas(fm_ctx* c, BatchSlot& B, size_t F) {
    std::vector<int32_t> jobs;
    for (size_t f = 0; f < F; f++)
        for (const fm_contour& o : c->contours[f]) {
            jobs.push_back((int32_t)f);
            jobs.push_back(o.origin_x);
            jobs.push_back(o.origin_y);
        }
    const size_t n = jobs.size() / 3;
    if (n == 0) return FM_OK;
    if (int rc = grow(c, &c->d_area, &c->area_cap, n, n * 4)) return rc;
    hipStream_t st = c->aux_stream;
    std::vector<int32_t> a2(n);
    FM_HIP_TRY(c, hipMemcpyAsync(c->d_area, jobs.data(), n * 3 * sizeof(int32_t), hipMemcpyHostToDevice, st));
    FM_HIP_TRY(c, launch_contour_area(st, c->traits().tiles ? B.d_dbits : nullptr, c->traits().tiles ? B.d_candf : nullptr,
                                   c->traits().tiles ? nullptr : c->d_mask, c->ntiles, c->ntx, c->h, c->w, c->d_area, (int)n,
                                   c->d_area + n * 3));
    FM_HIP_TRY(c, hipMemcpyAsync(a2.data(), c->d_area + n * 3, n * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    FM_HIP_TRY(c, hipStreamSynchronize(st));
    size_t k = 0;
    for (size_t f = 0; f < F; f++)
        for (fm_contour& o : c->contours[f]) {
            if (a2[k] < 0) return failf(c, FM_EHIP, "contour of frame %zu at (%d, %d) has no closed border", f, o.origin_x,
                                       o.origin_y);
            o.area2 = a2[k++];
        }
    return FM_OK;
}

// FM_FLAG_CONTOUR_POINTS: the CHAIN_APPROX_SIMPLE points of every contour of the finished batch in slot B
// (fm.py:269-272), traced on the GPU on the same masks as contour_areas: a count pass (npts, area2), the
// exclusive scan here, the buffers grown from the known total, an emit pass, one copy to the host.
int contour_points(fm_ctx* c, BatchSlot& B, size_t F) {
    c->trace_n[0] = c->trace_n[1] = 0;
    c->trace_steps = 0;
    c->pts_off.assign(F + 1, 0);
    size_t n = 0;
    for (size_t f = 0; f < F; f++) n += c->contours[f].size();
    if (n == 0) return FM_OK;
    if (n > 0x7fffffffull / 12) return failf(c, FM_ENOMEM, "%zu contours in one batch: too many to trace", n);
    std::vector<int32_t> up(n * 9);  // jobs, then the three paths' lists
    std::vector<int32_t> path[kTracePaths];
    size_t k = 0;
    for (size_t f = 0; f < F; f++)
        for (const fm_contour& o : c->contours[f]) {
            int32_t* j = &up[k * 8];
            j[0] = (int32_t)f, j[1] = o.origin_x, j[2] = o.origin_y, j[3] = o.x, j[4] = o.y, j[5] = o.w, j[6] = o.h, j[7] = 0;
            path[trace_box_path(o.w, o.h)].push_back((int32_t)k);
            k++;
        }
    int32_t* lists = &up[n * 8];
    for (auto& v : path) lists = std::copy(v.begin(), v.end(), lists);
    if (int rc = grow(c, &c->d_trace, &c->trace_cap, n, n * 12 + 1)) return rc;
    int32_t* d_jobs = c->d_trace;
    int32_t* d_res = c->d_trace + n * 9;
    int32_t* d_err = c->d_trace + n * 12;
    hipStream_t st = c->aux_stream;
    TraceArgs ta{c->traits().tiles ? B.d_dbits : nullptr, c->traits().tiles ? B.d_candf : nullptr, c->traits().tiles ? nullptr : c->d_mask,
                 c->ntiles, c->ntx, c->h, c->w, d_jobs, d_jobs + n * 8,
                 {(int)path[0].size(), (int)path[1].size(), (int)path[2].size(), (int)path[3].size()}, d_res, nullptr, d_err};
    std::vector<int32_t> res(n * 3);
    FM_HIP_TRY(c, hipMemcpyAsync(d_jobs, up.data(), up.size() * sizeof(int32_t), hipMemcpyHostToDevice, st));
    FM_HIP_TRY(c, hipMemsetAsync(d_err, 0, sizeof(int32_t), st));
    FM_HIP_TRY(c, launch_trace(st, ta, false, &c->timer));
    FM_HIP_TRY(c, hipMemcpyAsync(res.data(), d_res, res.size() * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    FM_HIP_TRY(c, hipStreamSynchronize(st));
    size_t total = 0;
    k = 0;
    for (size_t f = 0; f < F; f++) {
        c->pts_off[f] = total;
        for (fm_contour& o : c->contours[f]) {
            const int32_t* r = &res[k * 3];
            if (r[0] < 1) return failf(c, FM_EHIP, "contour of frame %zu at (%d, %d) has no closed border", f, o.origin_x,
                                      o.origin_y);
            o.npts = r[0];
            o.area2 = r[1];
            c->trace_steps += r[2];
            up[k * 8 + 7] = (int32_t)total;
            total += (size_t)r[0];
            if (total > 0x7fffffffull) return failf(c, FM_ENOMEM, "more than 2^31 contour points in one batch");
            k++;
        }
    }
    c->pts_off[F] = total;
    c->trace_n[0] = (int32_t)(path[0].size() + path[1].size() + path[2].size());
    c->trace_n[1] = (int32_t)path[3].size();
    // the total is known: size both point buffers before the emit pass touches them
    const size_t host_pts = std::max(total, (size_t)4096);
    if (int rc = grow(c, &c->d_cpts, &c->cpts_cap, total, total * 2)) return rc;
    if (int rc = grow_pinned(c, &c->h_pts, &c->h_pts_cap, host_pts, host_pts * 2)) return rc;
    ta.pts = c->d_cpts;
    int32_t err = 0;
    FM_HIP_TRY(c, hipMemcpyAsync(d_jobs, up.data(), n * 8 * sizeof(int32_t), hipMemcpyHostToDevice, st));
    FM_HIP_TRY(c, launch_trace(st, ta, true, &c->timer));
    FM_HIP_TRY(c, hipMemcpyAsync(c->h_pts, c->d_cpts, total * 2 * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    FM_HIP_TRY(c, hipMemcpyAsync(&err, d_err, sizeof(int32_t), hipMemcpyDeviceToHost, st));
    FM_HIP_TRY(c, hipStreamSynchronize(st));
    c->timer.collect();
    if (err) return failf(c, FM_EHIP, "the emit pass of the contour trace disagreed with its count pass (code %d)", err);
    return FM_OK;
}

}  // namespace

// ---------------------------------------------------------------------------
extern "C" {

int fm_abi_version(void) { return FM_ABI_VERSION; }

const char* fm_last_error(const fm_ctx* ctx) { return ctx ? ctx->err.c_str() : g_last_error.c_str(); }

// The context's host-side plan: validation, the work size, the resize mode and its tables, the taps and the
// choice of pixel path and slot count.  No device is touched; fm_create builds on it and fm_plan reports it,
// so the two cannot disagree.
static int plan_context(fm_ctx* c, const fm_params& p) {
    if (p.n_streams < 1 || p.src_w < 1 || p.src_h < 1 || p.box_size < 1 || p.max_batch < 1 || p.max_contours < 1)
        return failf(kNoCtx, FM_EINVAL, "invalid geometry (streams %d, src %dx%d, box %d, batch %d, contours %d)",
                    p.n_streams, p.src_w, p.src_h, p.box_size, p.max_batch, p.max_contours);
    if (p.ksize < 1 || (p.ksize & 1) == 0 || p.ksize > kMaxK)
        return failf(kNoCtx, FM_EINVAL, "ksize %d must be odd and in [1, %d]", p.ksize, kMaxK);
    if (!(p.avg == p.avg)) return failf(kNoCtx, FM_EINVAL, "avg is NaN");

    c->p = p;
    c->w = p.box_size;
    c->h = (int)(p.src_h * ((double)p.box_size / (double)p.src_w));  // imutils.resize
    if (c->h < 1) return failf(kNoCtx, FM_EINVAL, "work height is 0 (box %d, src %dx%d)", p.box_size, p.src_w, p.src_h);
    if ((int64_t)c->h * c->w >= (1ll << 31) / 2) return failf(kNoCtx, FM_ENOTSUP, "work image too large");

    // resize mode (cv::resize: copy if same size; INTER_AREA needs scale >= 1)
    const AreaMode m = area_resize_mode(p.src_w, p.src_h, c->w, c->h);
    if (m.kind == AreaMode::Upscale && !(p.flags & FM_FLAG_AREA_UPSCALE))
        return failf(kNoCtx, FM_ENOTSUP, "box_size %d > frame width %d: INTER_AREA upscaling is bilinear in OpenCV, not supported",
                     p.box_size, p.src_w);
    c->rmode = m.kind;
    if (m.kind == AreaMode::Upscale) {
        if (!build_area_up_axis(p.src_w, c->w, c->upx) || !build_area_up_axis(p.src_h, c->h, c->upy))
            return failf(kNoCtx, FM_ENOTSUP, "frame %dx%d too large for the INTER_AREA upscaling tables", p.src_w, p.src_h);
        c->up_plan = plan_area_up(c->upy, c->w);
    }
    if (m.kind == AreaMode::Fast) c->fast_sx = m.isx, c->fast_sy = m.isy;
    if (m.kind == AreaMode::General &&
        (!build_area_axis(p.src_w, c->w, m.sx, c->ax) || !build_area_axis(p.src_h, c->h, m.sy, c->ay)))
        return failf(kNoCtx, FM_ENOTSUP, "INTER_AREA table with non-consecutive taps");
    if (!gaussian_taps(p.ksize, c->coef)) return failf(kNoCtx, FM_EINVAL, "bad ksize %d", p.ksize);
    if (pixel_lds_bytes(p.ksize) > 160 * 1024) return failf(kNoCtx, FM_ENOTSUP, "ksize %d too large for the LDS tile", p.ksize);

    const int tiles = ((c->w + 63) / 64) * ((c->h + 63) / 64);
    const bool planes = (p.flags & FM_FLAG_KEEP_PLANES) != 0, px16 = (size_t)c->h * c->w >= 16;
    const bool fused = p.ksize <= fused_max_ksize() && fused_lds_bytes(p.ksize) <= 160 * 1024 &&
                       tiles <= 8192;  // region labelling holds the tile grid in LDS
    // small work images (mode D: 1080p -> 100 x 56), k <= 49 (k > 49 goes to the per-frame k_pixel, or to the wide
    // path, which no image this small reaches): frame-parallel blur + per-pixel scan (fm_small.hip; mode D
    // 634 -> 746 k frames/s, round 5), unless the caller keeps the gray / blur / delta planes (k_pix writes them).
    bool small = fused && px16 && !planes && small_supported(c->h, c->w, p.ksize) && dev_env("FM_NO_PIX") == nullptr;
    if (const char* e = dev_env("FM_SMALL")) small = small && std::atoi(e) != 0;
    const bool pix = fused && pix_supported(p.ksize) && px16 && pix_lds_bytes(p.ksize) <= 160 * 1024 &&
                     dev_env("FM_NO_PIX") == nullptr;
    // Gaussian sizes above k_fused's on more than kFrameCclTiles tiles (the reference's default blur scale with
    // a raised box: -B 1920 gives k = 97): frame-parallel strip blur + the same scan (fm_wide.hip), with the
    // tile machinery of the fused paths behind it.  Kept planes stay with the per-frame kernel, as above.
    bool wide = p.ksize > fused_max_ksize() && !planes && tiles > kFrameCclTiles && tiles <= 8192 &&
                wide_supported(p.ksize, c->coef.data());
    if (const char* e = dev_env("FM_WIDE")) wide = wide && std::atoi(e) != 0;
    // FM_FLAG_COLOUR_MOTION: the chain on the three channels (fm_rgb.hip) at any work size of at most 8,192 tiles
    // and any ksize up to 49, with the tile machinery of the fused paths behind it.  The gray, blur and delta
    // planes have no 3-channel form.
    const bool colour = (p.flags & FM_FLAG_COLOUR_MOTION) != 0, mog2 = (p.flags & FM_FLAG_MOG2) != 0;
    if (colour) {
        if (planes)
            return failf(kNoCtx, FM_ENOTSUP, "colour motion keeps no gray / blur / delta planes (FM_FLAG_KEEP_PLANES)");
        if (!rgb_supported(c->h, c->w, p.ksize))
            return failf(kNoCtx, FM_ENOTSUP, "colour motion takes ksize up to 49 and at most 8192 tiles (ksize %d, %d tiles)",
                         p.ksize, tiles);
    }
    // FM_FLAG_MOG2: the Gaussian-mixture model (fm_mog2.hip) behind k_small_blur where it takes the image, else
    // behind k_wide_blur (any odd ksize from 3: its taps are bytes, and ksize 1's single tap is 256), with the tile
    // machinery of the fused paths behind it.
    if (mog2) {
        if (colour)
            return failf(kNoCtx, FM_ENOTSUP, "the Gaussian-mixture model runs on the gray image (FM_FLAG_COLOUR_MOTION)");
        if (planes)
            return failf(kNoCtx, FM_ENOTSUP, "the Gaussian-mixture path keeps no gray / blur / delta planes (FM_FLAG_KEEP_PLANES)");
        if (tiles > 8192) return failf(kNoCtx, FM_ENOTSUP, "the Gaussian-mixture path takes at most 8192 tiles (%d)", tiles);
        c->small_blur = small_supported(c->h, c->w, p.ksize);
        if (!c->small_blur && !(p.ksize >= 3 && wide_supported(p.ksize, c->coef.data())))
            return failf(kNoCtx, FM_ENOTSUP, "ksize %d on %d x %d: neither k_small_blur nor k_wide_blur takes it", p.ksize,
                         c->w, c->h);
    }
    c->path = mog2 ? PixelPath::Mog2 : colour ? PixelPath::Rgb : wide ? PixelPath::Wide : small ? PixelPath::Small
              : pix ? PixelPath::Pix : fused ? PixelPath::Fused : PixelPath::PerFrame;
    // A slot of a scan path also holds its blur bytes, 1 B per pixel-frame (0.53 GB at 1080p x 256 frames, 2.1 GB at
    // 2160p) on the wide and mixture paths: kWideSlots of them.  A colour slot holds 3 B per pixel-frame: kWideSlots
    // where that is more than kRgbSlotBytes (1080p from 43 frames a batch on).  The small path's are small.
    const bool few = c->path == PixelPath::Wide || c->path == PixelPath::Mog2 ||
                     (c->path == PixelPath::Rgb &&
                      scan_scratch_bytes(c->w, (c->h + 63) / 64, (size_t)p.n_streams * p.max_batch, 3) > kRgbSlotBytes);
    c->nslots = !c->traits().tiles ? 1 : few ? std::min(kSlots, kWideSlots) : kSlots;
    return FM_OK;
}

int fm_plan(const fm_params* prm, struct fm_plan* out) {
    if (!prm || !out) return failf(kNoCtx, FM_EINVAL, "null argument");
    std::memset(out, 0, sizeof *out);
    fm_ctx c;  // host fields only: nothing to release
    if (int rc = plan_context(&c, *prm)) return rc;
    out->work_h = c.h;
    out->work_w = c.w;
    out->tiles = ((c.w + 63) / 64) * ((c.h + 63) / 64);
    out->max_inflight = c.nslots;
    std::snprintf(out->pixel_path, sizeof out->pixel_path, "%s", c.traits().name);
    return FM_OK;
}

int fm_resize_kind(const fm_params* prm, int* kind) {
    if (!prm || !kind) return failf(kNoCtx, FM_EINVAL, "null argument");
    fm_ctx c;  // host fields only: nothing to release
    if (int rc = plan_context(&c, *prm)) return rc;
    *kind = c.rmode == ResizeMode::Identity ? FM_RESIZE_IDENTITY : c.rmode == ResizeMode::Fast ? FM_RESIZE_FAST
            : c.rmode == ResizeMode::General ? FM_RESIZE_GENERAL : FM_RESIZE_UP;
    return FM_OK;
}

int fm_area_up_taps(int ssize, int dsize, int32_t* s0, int32_t* s1, int32_t* a0, int32_t* a1) {
    AreaUpAxis A;
    if (!s0 || !s1 || !a0 || !a1) return failf(kNoCtx, FM_EINVAL, "null argument");
    if (ssize < 1 || dsize < ssize) return failf(kNoCtx, FM_EINVAL, "not an enlarging axis (%d -> %d)", ssize, dsize);
    if (!build_area_up_axis(ssize, dsize, A)) return failf(kNoCtx, FM_ENOTSUP, "axis of %d too large for the tables", ssize);
    std::copy(A.s0.begin(), A.s0.end(), s0);
    std::copy(A.s1.begin(), A.s1.end(), s1);
    std::copy(A.a0.begin(), A.a0.end(), a0);
    std::copy(A.a1.begin(), A.a1.end(), a1);
    return FM_OK;
}

int fm_gaussian_taps(int ksize, int32_t* out) {
    std::vector<int32_t> taps;
    if (!out) return failf(kNoCtx, FM_EINVAL, "null argument");
    if (!gaussian_taps(ksize, taps)) return failf(kNoCtx, FM_EINVAL, "ksize %d must be odd and in [1, %d]", ksize, kMaxK);
    std::copy(taps.begin(), taps.end(), out);
    return FM_OK;
}

int fm_mog2_defaults(fm_mog2_params* out) {
    if (!out) return failf(kNoCtx, FM_EINVAL, "null argument");
    *out = fm_mog2_params{500, 16.f, 9.f, 0.9f, 15.f, 4.f, 75.f, 0.05f, 0.5f, 1, -1.0};
    return FM_OK;
}

// fm_create_mog2's parameter rules (no device is touched)
static int check_mog2(const fm_mog2_params& m) {
    if (m.history < 1) return failf(kNoCtx, FM_EINVAL, "mog2 history %d must be at least 1", m.history);
    for (float f : {m.var_threshold, m.var_threshold_gen, m.background_ratio, m.var_init, m.var_min, m.var_max,
                    m.complexity_reduction, m.shadow_tau})
        if (!std::isfinite(f) || f < 0.f) return failf(kNoCtx, FM_EINVAL, "mog2 parameter %g must be finite and not negative", (double)f);
    if (m.var_min > m.var_max) return failf(kNoCtx, FM_EINVAL, "mog2 var_min %g above var_max %g", (double)m.var_min, (double)m.var_max);
    if (!(m.background_ratio > 0.f && m.background_ratio <= 1.f))
        return failf(kNoCtx, FM_EINVAL, "mog2 background_ratio %g outside (0, 1]", (double)m.background_ratio);
    if (!(m.learning_rate <= 1.0)) return failf(kNoCtx, FM_EINVAL, "mog2 learning_rate %g above 1", m.learning_rate);
    return FM_OK;
}

static int create_context(fm_ctx** out, const fm_params* prm, const fm_mog2_params* mog2);

int fm_create(fm_ctx** out, const fm_params* prm) { return create_context(out, prm, nullptr); }

int fm_create_mog2(fm_ctx** out, const fm_params* prm, const fm_mog2_params* mog2) {
    if (!out || !prm) return failf(kNoCtx, FM_EINVAL, "null argument");
    *out = nullptr;
    if (mog2)
        if (int rc = check_mog2(*mog2)) return rc;
    fm_params p = *prm;
    p.flags |= FM_FLAG_MOG2;
    return create_context(out, &p, mog2);
}

static int create_context(fm_ctx** out, const fm_params* prm, const fm_mog2_params* mog2) {
    if (!out || !prm) return failf(kNoCtx, FM_EINVAL, "null argument");
    *out = nullptr;
    const fm_params& p = *prm;
    std::unique_ptr<fm_ctx> c(new fm_ctx());
    if (int rc = plan_context(c.get(), p)) return rc;
    if (c->path == PixelPath::Mog2) {
        if (mog2) c->mog2 = *mog2;
        else (void)fm_mog2_defaults(&c->mog2);
    }

    fm_ctx* cp = c.get();
    FM_HIP_TRY(cp, hipSetDevice(p.device));
    // The pixel stream at high priority: it gets a hardware queue of its own instead of sharing one (in
    // order) with a contour-pass stream.  (Round 4 gave small work images' pixel stream 8 CUs of its own
    // -- k_pix5's chain / producer waves on two tiles were a latency chain the next resize starved; the
    // small-image path of round 5 runs a batch's frames in parallel over every CU instead.)
    {
        int lo = 0, hi = 0;
        FM_HIP_TRY(cp, hipDeviceGetStreamPriorityRange(&lo, &hi));
        if (dev_env("FM_PIX_PRIO_OFF")) hi = lo;
        FM_HIP_TRY(cp, hipStreamCreateWithPriority(&c->own_stream, hipStreamNonBlocking, hi));
    }
#ifndef FM_CCL_QMODE_DEFAULT
#define FM_CCL_QMODE_DEFAULT 2  // contour streams take their own hardware queues (A/B: +3 %)
#endif
#ifndef FM_NCCL_DEFAULT
// three contour streams.  Round 5, 3 alternating rounds each: the driver's command 1 stream 363-367 k (chains in
// a row fall behind), 2 streams 400-403 k, 3 streams 388-403 k (pixel launch std 14-22 us either way but for
// one 58 us run); mode D (60 steps) 2 streams 679-697 k, 3 streams 803-810 k (profiles/r05m_ccl_streams_ab.txt,
// r05o_ccl_streams_ab.txt)
#define FM_NCCL_DEFAULT 3
#endif
    int ccl_qmode = FM_CCL_QMODE_DEFAULT;
    if (const char* e = dev_env("FM_CCL_QMODE")) ccl_qmode = std::atoi(e);
    c->nccl = FM_NCCL_DEFAULT;
    if (const char* e = dev_env("FM_CCL_STREAMS")) c->nccl = std::max(1, std::min(kSlots, std::atoi(e)));
    if (ccl_qmode == 2)  // contour streams take hardware queues before the rarely used aux / input streams
        for (int i = 0; i < c->nccl; i++) FM_HIP_TRY(cp, hipStreamCreateWithFlags(&c->ccl_streams[i], hipStreamNonBlocking));
    FM_HIP_TRY(cp, hipStreamCreateWithFlags(&c->aux_stream, hipStreamNonBlocking));
    // input stream: host-to-device copies and the resize run here, ahead of the pixel stream
    if (!dev_env("FM_RESIZE_INLINE")) FM_HIP_TRY(cp, hipStreamCreateWithFlags(&c->rs_stream, hipStreamNonBlocking));
    c->stream = c->own_stream;
    c->timer.enabled = (p.flags & (FM_FLAG_PROFILE | FM_FLAG_PROFILE_PIX)) != 0;
    c->timer.pixel_only = !(p.flags & FM_FLAG_PROFILE);
    c->timer.stream = c->stream;
    c->timer.stream2 = c->rs_stream;

    const size_t S = p.n_streams, T = p.max_batch;
    c->work_plane = (size_t)c->h * c->w;
    c->src_frame_bytes = (size_t)p.src_h * p.src_w * 3;
    const size_t frames = S * T, px = frames * c->work_plane;
    int rc;
    // contour-pass streams shared round-robin by the slots: few streams, because the
    // runtime multiplexes streams onto GPU_MAX_HW_QUEUES (4) hardware queues in order,
    // and a contour kernel queued ahead of a pixel kernel on a shared queue stalls it
    for (int i = 0; i < 2; i++)
        if ((rc = dalloc(cp, &c->d_bg[i], S * c->work_plane * c->traits().bg_ch))) return rc;
    if ((rc = dalloc(cp, &c->d_keep, S * c->work_plane)) || (rc = dalloc(cp, &c->d_has_keep, S)) ||
        (rc = dalloc(cp, &c->d_init, S)) || (rc = dalloc(cp, &c->d_mask, c->traits().tiles ? c->work_plane : px)))
        return rc;
    if (c->traits().tiles) {
        c->ntx = (c->w + 63) / 64;
        c->nty = (c->h + 63) / 64;
        c->ntiles = c->ntx * c->nty;
        c->frame_ccl = c->ntiles <= kFrameCclTiles;
        // (dev: 0 = never, 2 = at any size)
        if (const char* e = dev_env("FM_FRAME_CCL")) c->frame_ccl = std::atoi(e) == 2 || (c->frame_ccl && std::atoi(e) != 0);
        // union-find nodes: one per empty-tile region slot, each frame's quota, and a shared
        // overflow pool that holds at least one worst-case frame (frames past it take the
        // pixel-level fallback)
        const size_t tf = frames * (size_t)c->ntiles;
        c->nquota = c->ntiles * kNodesPerTileFrame;
        const size_t nn = tf + tf * kNodesPerTileFrame + std::max(tf * kNodesShared, (size_t)c->ntiles * kTileMaxRuns);
        if (nn >= (size_t)INT32_MAX) return failf(kNoCtx, FM_ENOTSUP, "batch too large for 32-bit node ids (%zu)", nn);
        c->nnodes = (int)nn;
    }
    // Contour records: the fused path's mapped buffer holds the first rec_cap records of each frame (a
    // frame with more is re-emitted whole at fm_wait, so max_contours never changes the results): about
    // 32 MB per slot however many frames a batch has -- [frames][max_contours] records of 20 B were 671 MB
    // per slot at 8 streams x 256 frames and max_contours 1 << 14 (4 GB pinned per rank).  The per-frame
    // path copies [frames][max_contours] records from the device and keeps that size.
    c->rec_cap = p.max_contours;
    if (c->traits().tiles)
        c->rec_cap = (int)std::min<size_t>((size_t)p.max_contours,
                                           std::max<size_t>(64, (size_t(32) << 20) / (frames * 5 * sizeof(int32_t))));
    for (int i = 0; i < c->nslots; i++) {
        BatchSlot& b = c->slots[i];
        if (c->rmode != ResizeMode::Identity && (rc = dalloc(cp, &b.d_work, px * 3))) return rc;
        if ((rc = dalloc(cp, &b.d_count, 3 * frames + 3))) return rc;
        // (k_frame_contours re-arms its slot-wide words at the end of each batch: they start at zero)
        if (hipMemset(b.d_count, 0, (3 * frames + 3) * sizeof(int32_t)) != hipSuccess)
            return failf(cp, FM_EHIP, "hipMemset of the batch counters failed");
        if ((p.flags & FM_FLAG_KEEP_PLANES) && (rc = dalloc(cp, &b.d_planes, px * 3))) return rc;
        if (c->traits().tiles) {
            if ((rc = dalloc(cp, &b.d_heavy, frames * c->ntiles)) ||
                (rc = dalloc(cp, &b.d_tiles, frames * c->ntiles)) ||
                (rc = dalloc(cp, &b.d_tflag, frames * c->ntiles * 8)) || (rc = dalloc(cp, &b.d_candf, frames * c->ntiles)) ||
                (rc = dalloc(cp, &b.d_clist, frames * c->ntiles)) || (rc = dalloc(cp, &b.d_rlist, frames * c->ntiles)) ||
                (rc = dalloc(cp, &b.d_regrep, frames * c->ntiles)) || (rc = dalloc(cp, &b.d_ncr, frames * 2)) ||
                (rc = dalloc(cp, &b.d_dbits, frames * c->ntiles * 64)) ||
                (c->traits().bits && (rc = dalloc(cp, &b.d_bits, frames * c->ntiles * 64))) ||
                (c->traits().blur_ch &&
                 (rc = dalloc(cp, &b.d_blur, scan_scratch_bytes(c->w, c->nty, frames, c->traits().blur_ch)))) ||
                (c->path == PixelPath::Mog2 && (rc = dalloc(cp, &b.d_alpha, frames))) ||
                (rc = dalloc(cp, &b.d_nodes, (size_t)c->nnodes)))
                return rc;
        }
        // contour records: mapped pinned host memory written directly by the kernels
        // (only the records that exist cross PCIe)
        FM_HIP_TRY(cp, halloc(cp, &b.h_rec, frames * (size_t)c->rec_cap * 5 * sizeof(int32_t), hipHostMallocMapped));
        FM_HIP_TRY(cp, hipHostGetDevicePointer((void**)&b.d_rec, b.h_rec, 0));
        FM_HIP_TRY(cp, halloc(cp, &b.h_count, frames * sizeof(int32_t), hipHostMallocMapped));
        FM_HIP_TRY(cp, hipHostGetDevicePointer((void**)&b.dh_count, b.h_count, 0));
        FM_HIP_TRY(cp, halloc(cp, &b.h_overflow, frames * sizeof(int32_t), hipHostMallocMapped));
        FM_HIP_TRY(cp, halloc(cp, &b.h_stats, 2 * sizeof(int32_t), hipHostMallocMapped));
        FM_HIP_TRY(cp, hipHostGetDevicePointer((void**)&b.dh_stats, b.h_stats, 0));
        FM_HIP_TRY(cp, hipHostGetDevicePointer((void**)&b.dh_overflow, b.h_overflow, 0));
        if (b.d_tflag) FM_HIP_TRY(cp, hipMemset(b.d_tflag, 0, frames * c->ntiles * 8 * sizeof(uint32_t)));
        FM_HIP_TRY(cp, halloc(cp, &b.h_init, S, 0));
        if (c->path == PixelPath::Mog2) FM_HIP_TRY(cp, halloc(cp, &b.h_alpha, frames * sizeof(float), 0));
        if (i < c->nccl && ccl_qmode != 2) {
            if (ccl_qmode == 1) {
                int lo = 0, hi = 0;
                FM_HIP_TRY(cp, hipDeviceGetStreamPriorityRange(&lo, &hi));
                FM_HIP_TRY(cp, hipStreamCreateWithPriority(&c->ccl_streams[i], hipStreamNonBlocking, hi));
            } else {
                FM_HIP_TRY(cp, hipStreamCreateWithFlags(&c->ccl_streams[i], hipStreamNonBlocking));
            }
        }
        b.ccl_stream = c->ccl_streams[i % c->nccl];
        if (i < c->nccl) c->timer.extra.push_back(b.ccl_stream);  // fold_stamps waits for it too
        for (hipEvent_t* ev : {&b.ev_pix, &b.ev_done, &b.ev_rs, &b.ev_lab, &b.ev_in})
            FM_HIP_TRY(cp, hipEventCreateWithFlags(ev, hipEventDisableTiming));
    }
    // pixel-level CCL: the whole batch on the v1 path, one frame for the fused path's overflow fallback
    const size_t ccl_px = c->traits().tiles ? c->work_plane : px;
    if ((rc = dalloc(cp, &c->d_label, ccl_px)) || (rc = dalloc(cp, &c->d_cid, ccl_px)) ||
        (rc = dalloc(cp, &c->d_outer, ccl_px)) ||
        (!c->traits().tiles && (rc = dalloc(cp, &c->d_rec_dev, frames * (size_t)p.max_contours * 5))) ||
        (rc = dalloc(cp, &c->d_rec_one, (size_t)p.max_contours * 5)))
        return rc;
    c->rec_one_cap = (size_t)p.max_contours;
    FM_HIP_TRY(cp, halloc(cp, &c->h_err, sizeof(int32_t), hipHostMallocMapped));
    FM_HIP_TRY(cp, hipHostGetDevicePointer((void**)&c->dh_err, c->h_err, 0));
    *c->h_err = 0;
    FM_HIP_TRY(cp, hipMemset(c->d_has_keep, 0, S));
    if (c->traits().bg_ch) {
        FM_HIP_TRY(cp, hipMemset(c->d_bg[0], 0, S * c->work_plane * c->traits().bg_ch * sizeof(double)));
        FM_HIP_TRY(cp, hipMemset(c->d_bg[1], 0, S * c->work_plane * c->traits().bg_ch * sizeof(double)));
    }
    auto up = [&](auto** d, const auto& v) -> int {
        int r = dalloc(cp, d, v.size());
        if (r) return r;
        hipError_t e = hipMemcpy(*d, v.data(), v.size() * sizeof(v[0]), hipMemcpyHostToDevice);
        return e == hipSuccess ? 0 : failf(cp, FM_EHIP, "hipMemcpy tables: %s", hipGetErrorString(e));
    };
    if (c->rmode == ResizeMode::Upscale && ((rc = up(&c->d_upx, c->upx.tab)) || (rc = up(&c->d_upy, c->upy.tab)))) return rc;
    if (c->rmode == ResizeMode::General) {
        if ((rc = up(&c->d_xofs, c->ax.ofs)) || (rc = up(&c->d_xcnt, c->ax.cnt)) || (rc = up(&c->d_xwt, c->ax.wt)) ||
            (rc = up(&c->d_yofs, c->ay.ofs)) || (rc = up(&c->d_ycnt, c->ay.cnt)) || (rc = up(&c->d_ywt, c->ay.wt)))
            return rc;
    }
    c->bg_init.assign(S, 0);
    c->has_keep.assign(S, 0);
    if (c->path == PixelPath::Mog2) {  // no pixel has a mode yet; modes at or above nmodes are never read
        if ((rc = dalloc(cp, &c->d_mog_state, mog2_state_floats((int)S, c->w, c->nty))) ||
            (rc = dalloc(cp, &c->d_mog_nm, mog2_nmodes_bytes((int)S, c->w, c->nty))) ||
            (rc = dalloc(cp, &c->d_mog_bg, c->work_plane)))
            return rc;
        FM_HIP_TRY(cp, hipMemset(c->d_mog_nm, 0, mog2_nmodes_bytes((int)S, c->w, c->nty)));
        c->mog_nframes.assign(S, 0);
    }
    if (const char* e = dev_env("FM_DEBUG_SKIP")) c->dbg_skip = std::atoi(e);
    c->serial = dev_env("FM_SERIAL") != nullptr;
    if (dev_env("FM_PTS") && c->traits().bits) {
        // per launch: [S][ntiles][4] workgroup stamps, then [S][ntiles][8 waves][4] k_pix5 phase cycles
        if (const char* e = dev_env("FM_PTS_RING")) c->pts_ring = std::max(1, std::min(256, std::atoi(e)));
        const size_t n = (size_t)S * c->ntiles * 36 * c->pts_ring;
        if ((rc = dalloc(cp, &c->d_pts, n))) return rc;
        FM_HIP_TRY(cp, hipMemset(c->d_pts, 0, n * sizeof(uint64_t)));
    }
    if (dev_env("FM_TS") && c->traits().tiles) {
        if ((rc = dalloc(cp, &c->d_ts, frames * c->ntiles * 16))) return rc;
        c->ts_sum.assign(16, 0.0);
        c->ts_n.assign(16, 0);
    }
    // the initialising hipMemset calls run on the null stream, which does not order the
    // context's non-blocking streams: finish them before the first submit can read the buffers
    FM_HIP_TRY(cp, hipDeviceSynchronize());
    *out = c.release();
    return FM_OK;
}

void fm_destroy(fm_ctx* c) {
    if (!c) return;
    if (c->d_pts) {  // profiling: per-workgroup (hw_id, xcc_id, realtime start/end, memtime start/end) of the last k_pix
        const size_t rec = (size_t)c->p.n_streams * c->ntiles * 36, n = rec * c->pts_ring;
        std::vector<uint64_t> v(n);
        if (hipDeviceSynchronize() == hipSuccess &&
            hipMemcpy(v.data(), c->d_pts, n * sizeof(uint64_t), hipMemcpyDeviceToHost) == hipSuccess) {
            if (FILE* fh = std::fopen(dev_env("FM_PTS"), "wb")) {  // dev build only (d_pts); oldest launch first
                const size_t r0 = (size_t)(c->pts_launches % c->pts_ring);
                for (int k = 0; k < c->pts_ring; k++)
                    std::fwrite(v.data() + ((r0 + k) % c->pts_ring) * rec, sizeof(uint64_t), rec, fh);
                std::fclose(fh);
            }
        }
    }
    if (c->d_ts) {
        std::fprintf(stderr, "[fm] contour-pass phase cycles (mean per labelled tile):");
        for (int k = 2; k < 16; k++)
            if (c->ts_n[k]) std::fprintf(stderr, " %d:%.0f(n=%lld)", k, c->ts_sum[k] / c->ts_n[k], (long long)c->ts_n[k]);
        std::fprintf(stderr, "\n");
    }
    (void)hipSetDevice(c->p.device);
    for (hipStream_t st : {c->own_stream, c->stream, c->aux_stream, c->rs_stream, c->rs_stream2})
        if (st) (void)hipStreamSynchronize(st);
    for (hipStream_t st : c->ccl_streams)
        if (st) (void)hipStreamSynchronize(st);
    delete c;
}

int fm_host_alloc(fm_ctx* c, size_t bytes, void** out) {
    if (!c || !out) return failf(c, FM_EINVAL, "null argument");
    *out = nullptr;
    FM_HIP_TRY(c, hipSetDevice(c->p.device));
    FM_HIP_TRY(c, hipHostMalloc(out, bytes, hipHostMallocPortable));
    return FM_OK;
}

int fm_host_free(fm_ctx* c, void* ptr) {
    if (!c) return failf(kNoCtx, FM_EINVAL, "null context");
    if (ptr) FM_HIP_TRY(c, hipHostFree(ptr));
    return FM_OK;
}

int fm_max_inflight(const fm_ctx* c) { return c ? c->nslots : failf(kNoCtx, FM_EINVAL, "null context"); }

int fm_work_size(const fm_ctx* c, int* h, int* w) {
    if (!c) return failf(kNoCtx, FM_EINVAL, "null context");
    if (h) *h = c->h;
    if (w) *w = c->w;
    return FM_OK;
}

int fm_set_mask(fm_ctx* c, int stream, const uint8_t* keep) {
    if (!c) return failf(kNoCtx, FM_EINVAL, "null context");
    if (int rc = check_idle(c)) return rc;
    if (int rc = check_stream(c, stream)) return rc;
    FM_HIP_TRY(c, hipSetDevice(c->p.device));
    const uint8_t flag = keep ? 1 : 0;
    if (keep)
        FM_HIP_TRY(c, hipMemcpyAsync(c->d_keep + (size_t)stream * c->work_plane, keep, c->work_plane,
                                  hipMemcpyHostToDevice, c->stream));
    FM_HIP_TRY(c, hipMemcpyAsync(c->d_has_keep + stream, &flag, 1, hipMemcpyHostToDevice, c->stream));
    FM_HIP_TRY(c, hipStreamSynchronize(c->stream));
    c->has_keep[stream] = flag;
    return FM_OK;
}

int fm_reset_stream(fm_ctx* c, int stream) {
    if (!c) return failf(kNoCtx, FM_EINVAL, "null context");
    if (int rc = check_idle(c)) return rc;
    if (int rc = check_stream(c, stream)) return rc;
    c->bg_init[stream] = 0;
    if (c->path == PixelPath::Mog2) {
        const size_t n = mog2_nmodes_bytes(1, c->w, c->nty);
        FM_HIP_TRY(c, hipSetDevice(c->p.device));
        FM_HIP_TRY(c, hipMemsetAsync(c->d_mog_nm + (size_t)stream * n, 0, n, c->stream));
        FM_HIP_TRY(c, hipStreamSynchronize(c->stream));
        c->mog_nframes[stream] = 0;
    }
    return FM_OK;
}

int fm_set_hip_stream(fm_ctx* c, void* s) {
    if (!c) return failf(kNoCtx, FM_EINVAL, "null context");
    if (int rc = check_idle(c)) return rc;
    c->stream = s ? (hipStream_t)s : c->own_stream;
    c->timer.stream = c->stream;
    return FM_OK;
}

// One batch's input as the five fm_submit* entry points describe it after their own validation.
namespace {
struct YuvSrc {
    int format, pitch;
    size_t chroma_offset, extent, stride;  // stride: bytes between frames (contiguous source)
};
enum class InputKind { Bgr, BgrStreams, Jpeg, Yuv, YuvList };
struct BatchInput {
    InputKind kind;
    int n;                       // frames per stream
    bool on_device;              // Bgr, BgrStreams, Yuv: the addresses are device memory (else host memory, copied)
    const uint8_t* frames;       // Bgr, Yuv: the batch's frames [n][S], contiguous
    const uint8_t* const* ptrs;  // BgrStreams: S streams' frames; Jpeg: n * S JPEGs; YuvList: n * S device addresses
    fm_mjpeg* dec;               // Jpeg: the decoder
    const size_t* sizes;         // and each JPEG's bytes
    YuvSrc yuv;                  // Yuv, YuvList: the resolved layout
};

// The stream the batch's input copies, conversion and resize run on: their own stream when there is
// a resize, so batch i+1's resize (many workgroups, HBM-bound) overlaps batch i's pixel kernel (few,
// when the work image is small); the pixel stream waits for it (submit).
int pick_input_stream(fm_ctx* c, const BatchInput& in, int si, hipStream_t* rs) {
    *rs = c->rs_stream ? c->rs_stream : c->stream;
#ifndef FM_RS_TWO
#define FM_RS_TWO 1
#endif
    // Consecutive batches' resizes on two input streams (odd slots on the second): in one in-order stream each
    // waited for the previous one's last wave and then its own dispatch (6-19 us a batch in mode D), on two the
    // next one's workgroups fill the previous one's tail.  Each batch's resize writes its own slot's buffer, and
    // the pixel stream waits for its batch's event, so the order of the batches is unchanged.
    if (FM_RS_TWO && c->rs_stream && in.kind != InputKind::Jpeg && c->rmode != ResizeMode::Identity && (si & 1)) {
        if (!c->rs_stream2) {
            FM_HIP_TRY(c, hipStreamCreateWithFlags(&c->rs_stream2, hipStreamNonBlocking));
            c->timer.stream3 = c->rs_stream2;
        }
        *rs = c->rs_stream2;
    }
    return FM_OK;
}

// the slot's BGR input buffer [max_batch][S][H][W][3], allocated by the first batch that is staged into it
int ensure_input_buffer(fm_ctx* c, BatchSlot& B) {
    if (B.d_in) return FM_OK;
    return dalloc(c, &B.d_in, (size_t)c->p.max_batch * c->p.n_streams * c->src_frame_bytes);
}

// YUV frames -> BGR frames in B.d_in, on the input stream
int stage_yuv(fm_ctx* c, BatchSlot& B, const BatchInput& in, hipStream_t rs, size_t F) {
    const YuvSrc& y = in.yuv;
    const size_t cap = (size_t)c->p.max_batch * c->p.n_streams;
    YuvArgs ya{};
    ya.src = in.frames;
    if (in.kind == InputKind::YuvList) {
        if (!B.d_ytab)
            if (int rc = dalloc(c, &B.d_ytab, cap)) return rc;
        if (!B.h_ytab) FM_HIP_TRY(c, halloc(c, &B.h_ytab, cap * sizeof(uint8_t*), hipHostMallocDefault));
        std::copy(in.ptrs, in.ptrs + F, B.h_ytab);  // (the slot is idle: its last batch was waited for)
        FM_HIP_TRY(c, hipMemcpyAsync(B.d_ytab, B.h_ytab, F * sizeof(uint8_t*), hipMemcpyHostToDevice, rs));
        ya.srcs = B.d_ytab;
    } else if (!in.on_device) {
        const size_t bytes = (F - 1) * y.stride + y.extent;
        if (bytes > B.yuv_cap) {  // first use, or a larger layout than the slot has seen: room for a full batch of it
            const size_t want = std::max(bytes, (cap - 1) * y.stride + y.extent);
            if (int rc = grow(c, &B.d_yuv, &B.yuv_cap, want, want)) return rc;
        }
        FM_HIP_TRY(c, hipMemcpyAsync(B.d_yuv, in.frames, bytes, hipMemcpyHostToDevice, rs));
        ya.src = B.d_yuv;
    }
    ya.frame_stride = y.stride;
    ya.chroma_offset = y.chroma_offset;
    ya.dst = B.d_in;
    ya.format = y.format;
    ya.pitch = y.pitch;
    ya.W = c->p.src_w;
    ya.H = c->p.src_h;
    ya.F = (int)F;
    FM_HIP_TRY(c, c->timer.timed(rs, "yuv2bgr", [&](uint64_t* ks, uint64_t*) {
        ya.kstamp = ks;
        return launch_yuv2bgr(rs, ya);
    }));
    return FM_OK;
}

// The batch's BGR frames [n][S][H][W][3] on the device: *src is the caller's device memory, read in
// place (*staged false: nothing was enqueued), or B.d_in, filled on the input stream rs (*staged true).
int stage_input(fm_ctx* c, BatchSlot& B, const BatchInput& in, hipStream_t rs, const uint8_t** src, bool* staged) {
    *staged = !(in.kind == InputKind::Bgr && in.on_device);
    *src = in.frames;
    if (!*staged) return FM_OK;
    if (int rc = ensure_input_buffer(c, B)) return rc;
    *src = B.d_in;
    const int S = c->p.n_streams;
    const size_t F = (size_t)in.n * S, fb = c->src_frame_bytes;
    switch (in.kind) {
        case InputKind::Bgr:
            FM_HIP_TRY(c, hipMemcpyAsync(B.d_in, in.frames, F * fb, hipMemcpyHostToDevice, rs));
            break;
        case InputKind::BgrStreams:  // stream s's frames -> rows s, S + s, 2S + s, ... of the [t][s] batch layout
            for (int s = 0; s < S; s++)
                FM_HIP_TRY(c, hipMemcpy2DAsync(B.d_in + (size_t)s * fb, (size_t)S * fb, in.ptrs[s], fb, fb, (size_t)in.n,
                                            in.on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, rs));
            break;
        case InputKind::Jpeg: {  // the decode side (§8(f)-3): JPEGs -> BGR frames in the batch's device buffer
            const int rc = fm_mjpeg_enqueue(in.dec, in.ptrs, in.sizes, (int)F, B.d_in, rs);
            FM_HIP_TRY(c, hipSetDevice(c->p.device));
            if (rc) return failf(c, rc, "JPEG decode: %s", fm_mjpeg_last_error(in.dec));
            break;
        }
        case InputKind::Yuv:
        case InputKind::YuvList:
            return stage_yuv(c, B, in, rs, F);
    }
    return FM_OK;
}

// INTER_AREA on the input stream: *work is the work-size batch [n][S][h][w][3] (src itself without a resize)
int resize_input(fm_ctx* c, BatchSlot& B, hipStream_t rs, const uint8_t* src, size_t F, const uint8_t** work) {
    *work = c->rmode == ResizeMode::Identity ? src : B.d_work;
    if (c->rmode == ResizeMode::General)
        FM_HIP_TRY(c, c->timer.timed(rs, "resize_area", [&](uint64_t* ks, uint64_t*) {
            return launch_resize_area(rs, src, B.d_work, (int)F, c->p.src_h, c->p.src_w, c->h, c->w, c->d_xofs, c->d_xcnt,
                                      c->d_xwt, c->ax.max_taps, c->d_yofs, c->d_ycnt, c->d_ywt, c->ay.max_taps, nullptr, ks);
        }));
    else if (c->rmode == ResizeMode::Fast)
        FM_HIP_TRY(c, c->timer.timed(rs, "resize_area_fast", [&](uint64_t* ks, uint64_t*) {
            return launch_resize_area_fast(rs, src, B.d_work, (int)F, c->p.src_h, c->p.src_w, c->h, c->w, c->fast_sx,
                                           c->fast_sy, ks);
        }));
    else if (c->rmode == ResizeMode::Upscale)
        FM_HIP_TRY(c, c->timer.timed(rs, "resize_area_up", [&](uint64_t* ks, uint64_t*) {
            return launch_resize_area_up(rs, src, B.d_work, (int)F, c->p.src_h, c->p.src_w, c->h, c->w, c->d_upx, c->d_upy,
                                         c->up_plan, nullptr, ks);
        }));
    return FM_OK;
}

// the fused paths' arguments for n frames per stream of the work-size batch `work` in slot B
FusedArgs fused_args(fm_ctx* c, BatchSlot& B, const uint8_t* work, int n, bool any_init) {
    const int S = c->p.n_streams;
    const long long npx = (long long)c->work_plane;
    FusedArgs fa{};
    fa.src = work;
    fa.bg_in = c->d_bg[c->bg_cur];
    fa.bg_out = c->d_bg[c->bg_cur ^ 1];
    fa.keep = c->d_keep;
    fa.has_keep = c->d_has_keep;
    fa.init = any_init ? c->d_init : nullptr;
    fa.mask_out = nullptr;
    fa.planes = B.d_planes;
    fa.bits = B.d_bits;
    fa.dbits = B.d_dbits;
    fa.tiles = B.d_tiles;
    fa.tflag = B.d_tflag;
    fa.tflag_waves = c->traits().scan ? 8 : 1;
    fa.candf = B.d_candf;
    fa.clist = B.d_clist;
    fa.rlist = B.d_rlist;
    fa.regrep = B.d_regrep;
    fa.ncr = B.d_ncr;
    fa.nodes = B.d_nodes;
    fa.count = B.d_count;
    fa.heavy = B.d_heavy;
    fa.rec = B.d_rec;
    fa.h_count = B.dh_count;
    fa.h_overflow = B.dh_overflow;
    fa.T = n;
    fa.S = S;
    fa.h = c->h;
    fa.w = c->w;
    fa.ksize = c->p.ksize;
    fa.thresh = c->p.threshold;
    fa.ntx = c->ntx;
    fa.nty = c->nty;
    fa.ntiles = c->ntiles;
    fa.nnodes = c->nnodes;
    fa.nquota = c->nquota;
    fa.h_stats = B.dh_stats;
    fa.cap = c->rec_cap;
    fa.cvt_simd = npx >= 16;
    fa.alpha = c->p.avg;
    fa.beta = 1.0 - c->p.avg;
    fa.acc_vec_end = npx - npx % 16;
    fa.any_keep = std::any_of(c->has_keep.begin(), c->has_keep.end(), [](uint8_t k) { return k != 0; }) ? 1 : 0;
    fa.dbg_skip = c->dbg_skip;
    fa.dbg_ts = c->d_ts;
    fa.dbg_pts = c->d_pts ? c->d_pts + (size_t)(c->pts_launches++ % c->pts_ring) * S * c->ntiles * 36 : nullptr;
    fa.dbg_err = c->dh_err;
    for (int i = 0; i < c->p.ksize; i++) fa.coef[i] = c->coef[i];
    fa.t_begin = 0;
    fa.t_end = n;
    return fa;
}

// The batch's pixel kernels on the pixel stream (the background recurrence is ordered here).  The counters
// are zeroed by k_pix (k_regions on the k_fused path); the tile flags of the 64 x 64 tile kernels' batches are
// written on the contour stream (k_tile_flags, run_contours), k_fused's are cleared by k_counts.
int run_pixel(fm_ctx* c, BatchSlot& B, const FusedArgs& fa, bool any_init) {
    hipStream_t ps = c->stream;
    const int n = fa.T;
    if (c->d_ts) FM_HIP_TRY(c, hipMemsetAsync(c->d_ts, 0, (size_t)n * fa.S * c->ntiles * 16 * sizeof(uint64_t), ps));
    if (!c->traits().bits) {
        FM_HIP_TRY(c, launch_fused(ps, fa, &c->timer));
        c->bg_cur ^= 1;
        return FM_OK;
    }
    if (c->path == PixelPath::Mog2) {
        // The whole batch in one launch pair (a stream's first frame is a frame like any other: no mode fits).
        // Each frame's learning rate from the stream's frame count, in double as OpenCV computes it; the counts
        // advance here, so batches in flight chain as the model itself does on the pixel stream.
        const int S = fa.S;
        for (int t = 0; t < n; t++)
            for (int s = 0; s < S; s++) {
                const int64_t nf = c->mog_nframes[s] + t + 1;
                const double lr = (c->mog2.learning_rate >= 0 && nf > 1)
                                      ? c->mog2.learning_rate
                                      : 1.0 / (double)std::min<int64_t>(2 * nf, (int64_t)c->mog2.history);
                B.h_alpha[(size_t)t * S + s] = (float)lr;
            }
        for (int s = 0; s < S; s++) c->mog_nframes[s] += n;
        FM_HIP_TRY(c, hipMemcpyAsync(B.d_alpha, B.h_alpha, (size_t)n * S * sizeof(float), hipMemcpyHostToDevice, ps));
        const Mog2Dev md{c->d_mog_state, c->d_mog_nm, B.d_alpha, c->mog2};
        FusedArgs fp = fa;
        fp.init = nullptr;
        // (each kernel timed on its own, so that the scan appears as mog2_scan under either profile flag)
        FM_HIP_TRY(c, c->timer.timed(ps, c->small_blur ? "small_blur" : "wide_blur", [&](uint64_t* ks, uint64_t*) {
            return c->small_blur ? launch_small_blur(ps, fp, B.d_blur, ks) : launch_wide_blur(ps, fp, B.d_blur, ks);
        }));
        FM_HIP_TRY(c, c->timer.timed(ps, "mog2_scan", [&](uint64_t* ks, uint64_t*) {
            return launch_mog2_scan(ps, fp, md, B.d_blur, ks);
        }));
        return FM_OK;
    }
    const bool planes = B.d_planes != nullptr;
    // each launch reads d_bg[cur] and writes d_bg[cur ^ 1]
    auto run = [&](int t0, int t1, bool init, const char* name) -> int {
        FusedArgs fp = fa;
        fp.t_begin = t0;
        fp.t_end = t1;
        fp.bg_in = c->d_bg[c->bg_cur];
        fp.bg_out = c->d_bg[c->bg_cur ^ 1];
        if (!init) fp.init = nullptr;
        const PathTraits& tr = c->traits();
        if (tr.launch) {  // not stamping (FM_FLAG_PROFILE, or the stamp ring full): the pair timed by events
            const char* const* nm = tr.timer[init];
            FM_HIP_TRY(c, c->timer.timed(ps, nm[0], [&](uint64_t* k1, uint64_t* k2) {
                return tr.launch(ps, fp, B.d_blur, k1, k2);
            }, true, nm[1], nm[2]));
        } else
            FM_HIP_TRY(c, c->timer.timed(ps, name, [&](uint64_t* ks, uint64_t*) {
                fp.kstamp = ks;
                return launch_pix(ps, fp, planes, init);
            }));
        c->bg_cur ^= 1;
        return FM_OK;
    };
    if (any_init) {  // first frames in their own launch: the steady-state kernel has no init select
        if (int rc = run(0, 1, true, "pix_init")) return rc;
        return n > 1 ? run(1, n, false, "pix") : FM_OK;
    }
    return run(0, n, false, "pix");
}

// The batch's contour pass on its slot's stream, after its pixel kernels; counts land in the mapped
// h_count / h_overflow.
// Consecutive batches on different contour streams: with 4 slots on 3 streams a fixed
// slot -> stream map put every fourth pair of consecutive chains on one stream, one after
// the other (the last batch's chain waited ≈130 µs for its predecessor's)
// (Batches taking the contour streams in turn instead of the fixed slot map: +2 % on one box,
// equal on another with 8 % longer pixel launches, round 3.)
int run_contours(fm_ctx* c, BatchSlot& B, int si, const FusedArgs& fa) {
    hipStream_t ps = c->stream, cs = c->serial ? ps : B.ccl_stream;
    const size_t F = (size_t)fa.T * fa.S;
    FM_HIP_TRY(c, hipEventRecord(B.ev_pix, ps));
    FM_HIP_TRY(c, hipStreamWaitEvent(cs, B.ev_pix, 0));
    // The 64 x 64 tile pixel kernels (launch_pix) store threshold bits only: every frame's tile flags, the init
    // frame's launch included, come from those bits here, at the head of the chain and ahead of the labelling gate.
    // (The small-image, wide-Gaussian and colour scans and k_fused write their own.)  Timed by events, like k_regions
    // (FM_FLAG_PROFILE; never in the pixel-only mode on a contour stream).
    if (c->traits().bits && !c->traits().scan)
        FM_HIP_TRY(c, c->timer.timed(cs, "tile_flags", [&](uint64_t*, uint64_t*) { return launch_tile_flags(cs, fa); }, false));
    if (c->frame_ccl) {  // small work images: the whole pass of a frame in one workgroup (no gate needed)
        FusedArgs fc = fa;
        // stamped by the dev build only; FM_FLAG_PROFILE: events around it (a contour stream: never in the pixel-only mode)
        FM_HIP_TRY(c, c->timer.timed(cs, "frame_contours", [&](uint64_t* ks, uint64_t*) {
            fc.kstamp = ks;
            // the slot-wide words (shared pool, heavy tally, frames done) sit at indices that depend on the batch's
            // frame count; the last workgroup re-arms them for a batch of the same size, so a slot whose batch size
            // changed (a stream's last, partial batch) zeroes them at the new indices first
            if (B.ccl_F != F) {
                hipError_t e = hipMemsetAsync(B.d_count + 2 * F, 0, 2 * sizeof(int32_t), cs);
                if (e == hipSuccess) e = hipMemsetAsync(B.d_count + 3 * F + 2, 0, sizeof(int32_t), cs);
                if (e != hipSuccess) return e;
                B.ccl_F = F;
            }
            return launch_frame_contours(cs, fc, c->traits().bits);
        }, kDevSwitches));
    } else {
        // the labelling gate: one batch's labelling kernel at a time (the previous batch's, on another contour
        // stream, is waited for), so the labelling of consecutive chains never bunches beside a pixel launch
        // (+1.5 %, 388.1 vs 382.3 k, 4 alternating rounds, round 3)
        hipEvent_t gate_wait = nullptr;
        if (!c->serial && c->lab_prev >= 0 && c->lab_prev != si) gate_wait = c->slots[c->lab_prev].ev_lab;
        FM_HIP_TRY(c, launch_tile_ccl(cs, fa, c->traits().bits, &c->timer, gate_wait, B.ev_lab));
        c->lab_prev = si;
    }
    B.fa = fa;
    FM_HIP_TRY(c, hipEventRecord(B.ev_done, cs));
    return FM_OK;
}

// the per-frame (v1) path: one pixel launch per batch step and the pixel-level CCL, all on the pixel stream
int run_per_frame(fm_ctx* c, BatchSlot& B, const uint8_t* work, int n, bool any_init) {
    hipStream_t ps = c->stream;
    const int S = c->p.n_streams;
    const size_t F = (size_t)n * S;
    const long long npx = (long long)c->work_plane;
    FM_HIP_TRY(c, hipMemsetAsync(B.d_count, 0, (2 * F + 1) * sizeof(int32_t), ps));
    PixelArgs a{};
    a.bg = nullptr;
    a.keep = c->d_keep;
    a.has_keep = c->d_has_keep;
    a.S = S;
    a.h = c->h;
    a.w = c->w;
    a.ksize = c->p.ksize;
    a.thresh = c->p.threshold;
    a.alpha = c->p.avg;
    a.beta = 1.0 - c->p.avg;
    a.acc_vec_end = npx - npx % 16;
    a.cvt_simd = npx >= 16;
    for (int i = 0; i < c->p.ksize; i++) a.coef[i] = c->coef[i];
    const size_t step_px = (size_t)S * c->work_plane;
    for (int t = 0; t < n; t++) {
        a.src = work + (size_t)t * step_px * 3;  // work image is [T][S][h][w][3] in every resize mode
        a.init = (t == 0 && any_init) ? c->d_init : nullptr;
        a.mask_out = c->d_mask + (size_t)t * step_px;
        if (B.d_planes) {
            a.gray_out = B.d_planes + (size_t)t * step_px;
            a.blur_out = B.d_planes + F * c->work_plane + (size_t)t * step_px;
            a.delta_out = B.d_planes + 2 * F * c->work_plane + (size_t)t * step_px;
        }
        FM_HIP_TRY(c, c->timer.timed(ps, "pixel", [&](uint64_t*, uint64_t*) {
            return launch_pixel_pp(ps, a, c->d_bg[c->bg_cur], c->d_bg[c->bg_cur ^ 1]);
        }, false));
        c->bg_cur ^= 1;
    }
    FM_HIP_TRY(c, hipMemsetAsync(c->d_outer, 0, F * c->work_plane, ps));
    CclArgs ca{c->d_mask, c->d_label, c->d_outer, c->d_cid, B.d_count, c->d_rec_dev, (int)F, c->h, c->w, c->p.max_contours};
    FM_HIP_TRY(c, launch_ccl(ps, ca, &c->timer));
    FM_HIP_TRY(c, hipMemcpyAsync(B.h_rec, c->d_rec_dev, F * c->p.max_contours * 5 * sizeof(int32_t), hipMemcpyDeviceToHost,
                              ps));
    FM_HIP_TRY(c, hipMemsetAsync(B.d_count + F, 0, F * sizeof(int32_t), ps));
    FM_HIP_TRY(c, hipMemcpyAsync(B.h_overflow, B.d_count + F, F * sizeof(int32_t), hipMemcpyDeviceToHost, ps));
    FM_HIP_TRY(c, hipMemcpyAsync(B.h_count, B.d_count, F * sizeof(int32_t), hipMemcpyDeviceToHost, ps));
    FM_HIP_TRY(c, hipEventRecord(B.ev_done, ps));
    return FM_OK;
}

// One batch into the next slot: its input staged and resized on an input stream, the pixel kernels on the
// pixel stream, the contour pass on the slot's stream.  fm_wait takes the slots in submission order.
int submit(fm_ctx* c, BatchInput in) {
    if (!c) return failf(kNoCtx, FM_EINVAL, "null context");
    if ((int)c->inflight.size() >= c->nslots)
        return failf(c, FM_ESTATE, "%d batch(es) already in flight: call fm_wait first", (int)c->inflight.size());
    const int S = c->p.n_streams, n = in.n;
    if (in.kind == InputKind::BgrStreams) {
        for (int s = 0; s < S; s++)
            if (!in.ptrs[s]) return failf(c, FM_EINVAL, "null frames for stream %d", s);
        if (in.on_device && S == 1) {  // one stream: [n][1] is the contiguous layout, read in place
            in.kind = InputKind::Bgr;
            in.frames = in.ptrs[0];
        }
    }
    if ((in.kind == InputKind::Bgr && !in.frames) || n < 1 || n > c->p.max_batch)
        return failf(c, FM_EINVAL, "n_frames %d outside [1, max_batch=%d] or null frames", n, c->p.max_batch);
    FM_HIP_TRY(c, hipSetDevice(c->p.device));
    const int si = c->next_slot;
    BatchSlot& B = c->slots[si];
    hipStream_t ps = c->stream, rs = nullptr;
    const uint8_t *src = nullptr, *work = nullptr;
    bool staged = false;
    int rc;
    if ((rc = pick_input_stream(c, in, si, &rs))) return rc;
    // On a caller's stream (fm_set_hip_stream) the batch is ordered after the work the caller queued there
    // before this call, such as the decode or copy that fills device input: the input stream waits for it
    // before it touches the input.  (The context's own stream only ever carries this context's work, which
    // the input stream runs ahead of: no wait there.)
    if (rs != ps && ps != c->own_stream) {
        FM_HIP_TRY(c, hipEventRecord(B.ev_in, ps));
        FM_HIP_TRY(c, hipStreamWaitEvent(rs, B.ev_in, 0));
    }
    if ((rc = stage_input(c, B, in, rs, &src, &staged)) ||
        (rc = resize_input(c, B, rs, src, (size_t)n * S, &work)))
        return rc;
    if (rs != ps && (staged || c->rmode != ResizeMode::Identity)) {  // something ran on the input stream
        FM_HIP_TRY(c, hipEventRecord(B.ev_rs, rs));
        FM_HIP_TRY(c, hipStreamWaitEvent(ps, B.ev_rs, 0));
    }
    bool any_init = false;
    for (int s = 0; s < S; s++) {
        B.h_init[s] = c->bg_init[s] ? 0 : 1;
        any_init |= B.h_init[s] != 0;
    }
    if (any_init) FM_HIP_TRY(c, hipMemcpyAsync(c->d_init, B.h_init, S, hipMemcpyHostToDevice, ps));
    if (c->traits().tiles) {
        const FusedArgs fa = fused_args(c, B, work, n, any_init);
        if ((rc = run_pixel(c, B, fa, any_init)) || (rc = run_contours(c, B, si, fa))) return rc;
    } else if ((rc = run_per_frame(c, B, work, n, any_init))) {
        return rc;
    }
    for (int s = 0; s < S; s++) c->bg_init[s] = 1;
    B.n = n;
    B.src = src;
    B.gen++;
    c->inflight.push_back(si);
    c->next_slot = (si + 1) % c->nslots;
    return FM_OK;
}
}  // namespace

int fm_submit(fm_ctx* c, const uint8_t* frames, int n, int on_device) {
    return submit(c, {InputKind::Bgr, n, on_device != 0, frames});
}

int fm_submit_streams(fm_ctx* c, const uint8_t* const* bgr, int n, int on_device) {
    if (!c) return failf(kNoCtx, FM_EINVAL, "null context");
    if (!bgr) return failf(c, FM_EINVAL, "null stream pointer array");
    return submit(c, {InputKind::BgrStreams, n, on_device != 0, nullptr, bgr});
}

int fm_submit_jpeg(fm_ctx* c, fm_mjpeg* dec, const uint8_t* const* jpegs, const size_t* sizes, int n) {
    if (!c) return failf(kNoCtx, FM_EINVAL, "null context");
    if (!dec || !jpegs || !sizes) return failf(c, FM_EINVAL, "null decoder or JPEG arrays");
    // the decoder writes n * S frames of its own size into the batch's input buffer (sized for this
    // context's frames): refuse any mismatch before anything is enqueued
    int dw = 0, dh = 0, ddev = -1, dmax = 0;
    if (fm_mjpeg_geometry(dec, &dw, &dh, &ddev, &dmax)) return failf(c, FM_EINVAL, "bad decoder");
    if (dw != c->p.src_w || dh != c->p.src_h || ddev != c->p.device)
        return failf(c, FM_EINVAL, "decoder for %dx%d frames on device %d, context for %dx%d on device %d", dw, dh, ddev,
                    c->p.src_w, c->p.src_h, c->p.device);
    if (n >= 1 && (long long)n * c->p.n_streams > dmax)
        return failf(c, FM_EINVAL, "decoder takes %d frames per call, the batch has %lld", dmax,
                    (long long)n * c->p.n_streams);
    return submit(c, {InputKind::Jpeg, n, false, nullptr, jpegs, dec, sizes});
}

// fm_yuv_layout resolved for width x height frames (pitch, chroma offset, extent, frame stride), or why not
static const char* yuv_resolve(int W, int H, const fm_yuv_layout* L, YuvSrc& y) {
    if (!L) return "null layout";
    if (L->format < FM_YUV_NV12 || L->format > FM_YUV_UYVY) return "unknown YUV format";
    const bool planar = L->format == FM_YUV_NV12 || L->format == FM_YUV_I420;
    if (W < 1 || H < 1) return "frame size below 1";
    if (W & 1) return "YUV frames need an even width";
    if (planar && (H & 1)) return "NV12 / I420 frames need an even height";
    const long long tight = planar ? (long long)W : 2ll * W;
    if (tight > INT32_MAX) return "frame too wide";
    if (L->pitch < 0 || (L->pitch != 0 && L->pitch < tight)) return "pitch below the tight row";
    const size_t pitch = L->pitch ? (size_t)L->pitch : (size_t)tight;
    if (L->format == FM_YUV_I420 && (pitch & 1)) return "I420 needs an even pitch (chroma rows are pitch / 2 bytes)";
    size_t coff = 0, extent = pitch * (size_t)H;
    if (planar) {
        if (L->chroma_offset < 0 || (L->chroma_offset != 0 && (size_t)L->chroma_offset < pitch * (size_t)H))
            return "chroma_offset inside the luma plane";
        coff = L->chroma_offset ? (size_t)L->chroma_offset : pitch * (size_t)H;
        // NV12: H/2 rows of pitch bytes; I420: two planes of H/2 rows of pitch/2 bytes
        extent = coff + (L->format == FM_YUV_NV12 ? pitch * (size_t)(H / 2) : (pitch / 2) * (size_t)H);
    }
    if (L->frame_stride != 0 && L->frame_stride < extent) return "frame_stride below the frame's extent";
    y.format = L->format;
    y.pitch = (int)pitch;
    y.chroma_offset = coff;
    y.extent = extent;
    y.stride = L->frame_stride ? L->frame_stride : extent;
    return nullptr;
}

int fm_yuv_frame_bytes(int width, int height, const fm_yuv_layout* layout, size_t* bytes) {
    if (bytes) *bytes = 0;
    if (!bytes) return failf(kNoCtx, FM_EINVAL, "null argument");
    YuvSrc y{};
    if (const char* why = yuv_resolve(width, height, layout, y)) return failf(kNoCtx, FM_EINVAL, "%s", why);
    *bytes = y.extent;
    return FM_OK;
}

int fm_submit_yuv(fm_ctx* c, const uint8_t* frames, int n, const fm_yuv_layout* layout, int on_device) {
    if (!c) return failf(kNoCtx, FM_EINVAL, "null context");
    if (!frames) return failf(c, FM_EINVAL, "null frames");
    YuvSrc y{};
    if (const char* why = yuv_resolve(c->p.src_w, c->p.src_h, layout, y)) return failf(c, FM_EINVAL, "%s", why);
    return submit(c, {InputKind::Yuv, n, on_device != 0, frames, nullptr, nullptr, nullptr, y});
}

int fm_submit_yuv_list(fm_ctx* c, const uint8_t* const* frames, int n, const fm_yuv_layout* layout) {
    if (!c) return failf(kNoCtx, FM_EINVAL, "null context");
    if (!frames) return failf(c, FM_EINVAL, "null frame address array");
    YuvSrc y{};
    if (const char* why = yuv_resolve(c->p.src_w, c->p.src_h, layout, y)) return failf(c, FM_EINVAL, "%s", why);
    if (n < 1 || n > c->p.max_batch) return failf(c, FM_EINVAL, "n_frames %d outside [1, max_batch=%d]", n, c->p.max_batch);
    for (size_t i = 0; i < (size_t)n * c->p.n_streams; i++)
        if (!frames[i]) return failf(c, FM_EINVAL, "null address for frame %zu", i);
    return submit(c, {InputKind::YuvList, n, true, nullptr, frames, nullptr, nullptr, y});
}

namespace {
using WholeFrames = std::vector<std::pair<size_t, std::vector<int32_t>>>;  // (frame, all its records), ascending

// Frames whose records do not fit the cap are fetched whole, so len(frame.contours)
// and the records kept never depend on max_contours (fm.py:674-694 counts them all).
int fetch_whole_frames(fm_ctx* c, BatchSlot& B, size_t F, WholeFrames& whole) {
    c->fallbacks = 0;
    for (size_t f = 0; f < F; f++) {
        const bool ovf = c->traits().tiles && B.h_overflow[f];
        if (!ovf && B.h_count[f] <= c->rec_cap) continue;
        std::vector<int32_t> v;
        if (c->traits().tiles && !ovf) {
            if (int rc = emit_all(c, B, f, B.h_count[f], v)) return rc;
        } else {
            // the contour pass ran out of nodes for this frame (fused path), or the per-frame
            // path kept only cap records: relabel it with the pixel-level CCL, every record
            int cnt = 0;
            if (int rc = relabel_frame(c, B, f, v, cnt)) return rc;
            B.h_count[f] = cnt;
            c->fallbacks += ovf;
        }
        whole.emplace_back(f, std::move(v));
    }
    return FM_OK;
}

// FM_TS (profiling): mean cycles between consecutive stamps of each labelled tile
int fold_phase_stamps(fm_ctx* c, size_t F) {
    std::vector<uint64_t> ts(F * c->ntiles * 16);
    FM_HIP_TRY(c, hipMemcpy(ts.data(), c->d_ts, ts.size() * sizeof(uint64_t), hipMemcpyDeviceToHost));
    for (size_t i = 0; i < F * c->ntiles; i++) {
        const uint64_t* t = &ts[i * 16];
        if (!t[1]) continue;
        uint64_t prev = t[1];
        for (int k = 2; k < 16; k++) {
            if (!t[k]) continue;
            c->ts_sum[k] += (double)(t[k] - prev);
            c->ts_n[k]++;
            prev = t[k];
        }
    }
    return FM_OK;
}

// the batch's records -> c->contours: each frame's fm_contour list sorted by start pixel (raster order)
void records_to_contours(fm_ctx* c, const BatchSlot& B, size_t F, const WholeFrames& whole) {
    const int cap = c->rec_cap;
    c->ready_counts.assign(B.h_count, B.h_count + F);
    c->contours.assign(F, {});
    size_t wi = 0;
    for (size_t f = 0; f < F; f++) {
        const int32_t* r = B.h_rec + f * cap * 5;
        int cnt = std::min(B.h_count[f], cap);
        if (wi < whole.size() && whole[wi].first == f) {
            r = whole[wi].second.data();
            cnt = (int)(whole[wi].second.size() / 5);
            wi++;
        }
        auto& v = c->contours[f];
        v.resize(cnt);
        std::vector<std::pair<int32_t, int>> order(cnt);
        for (int i = 0; i < cnt; i++) order[i] = {r[i * 5], i};
        std::sort(order.begin(), order.end());
        for (int i = 0; i < cnt; i++) {
            const int32_t* q = r + order[i].second * 5;
            fm_contour& o = v[i];
            o.x = q[1];
            o.y = q[2];
            o.w = q[3] - q[1] + 1;
            o.h = q[4] - q[2] + 1;
            o.origin_x = q[0] % c->w;
            o.origin_y = q[0] / c->w;
            o.area2 = -1;
            o.npts = 0;
        }
    }
}
}  // namespace

int fm_wait(fm_ctx* c) {
    if (!c) return failf(kNoCtx, FM_EINVAL, "null context");
    if (c->inflight.empty()) return FM_OK;
    FM_HIP_TRY(c, hipSetDevice(c->p.device));
    const int si = c->inflight.front();
    c->inflight.erase(c->inflight.begin());
    BatchSlot& B = c->slots[si];
#ifdef FM_DEV_SWITCHES  // host time in fm_wait (dev build): blocked on the batch vs the post-pass after it
    const auto hw0 = std::chrono::steady_clock::now();
#endif
    hipError_t e = hipEventSynchronize(B.ev_done);
    if (e != hipSuccess) {
        B.n = 0;
        return failf(c, FM_EHIP, "hipEventSynchronize: %s", hipGetErrorString(e));
    }
#ifdef FM_DEV_SWITCHES
    const auto hw1 = std::chrono::steady_clock::now();
#endif
    const int n = B.n;
    const size_t F = (size_t)n * c->p.n_streams;
#ifdef FM_BOUNDS_CHECK
    if (*c->h_err) return failf(c, FM_EHIP, "contour-pass bounds check failed: codes 0x%x", *c->h_err);
#endif
    if (c->traits().tiles) {
        c->stats[0] = B.h_stats[0];
        c->stats[1] = B.h_stats[1];
    }
    WholeFrames whole;
    if (int rc = fetch_whole_frames(c, B, F, whole)) return rc;
    c->timer.collect();
    if (c->d_ts)
        if (int rc = fold_phase_stamps(c, F)) return rc;
#ifdef FM_DEV_SWITCHES
    const auto hw2 = std::chrono::steady_clock::now();
#endif
    records_to_contours(c, B, F, whole);
#ifdef FM_DEV_SWITCHES
    if (c->timer.enabled) {
        const auto hw3 = std::chrono::steady_clock::now();
        auto add = [&](const char* name, std::chrono::steady_clock::duration d) {
            const int id = c->timer.id_of(name);
            c->timer.ms[id] += std::chrono::duration<double, std::milli>(d).count();
            c->timer.launches[id] += 1;
        };
        add("host:wait_sync", hw1 - hw0);
        add("host:wait_scan", hw2 - hw1);
        add("host:wait_records", hw3 - hw2);
    }
#endif
    if (c->p.flags & FM_FLAG_CONTOUR_POINTS) {  // (area2 comes with the points: no second trace)
        c->pts_off.clear();
        if (int rc = contour_points(c, B, F)) {
            c->pts_off.clear();
            return rc;
        }
    } else if (c->p.flags & FM_FLAG_CONTOUR_AREA) {
        if (int rc = contour_areas(c, B, F)) return rc;
    }
    c->ready = n;
    c->ready_slot = si;
    c->ready_gen = B.gen;
    B.n = 0;
    return FM_OK;
}

int fm_last_fallbacks(const fm_ctx* c) { return c ? c->fallbacks : failf(kNoCtx, FM_EINVAL, "null context"); }

int fm_last_ccl_stats(const fm_ctx* c, int32_t* shared_nodes, int32_t* heavy_tiles) {
    if (!c) return failf(kNoCtx, FM_EINVAL, "null context");
    if (shared_nodes) *shared_nodes = c->stats[0];
    if (heavy_tiles) *heavy_tiles = c->stats[1];
    return FM_OK;
}

int fm_last_trace_stats(const fm_ctx* c, int32_t* staged, int32_t* unstaged, int64_t* steps) {
    if (!c) return failf(kNoCtx, FM_EINVAL, "null context");
    if (staged) *staged = c->trace_n[0];
    if (unstaged) *unstaged = c->trace_n[1];
    if (steps) *steps = c->trace_steps;
    return FM_OK;
}

int fm_get_contour_points(fm_ctx* c, int frame, int stream, int32_t* xy, size_t cap, size_t* total) {
    if (total) *total = 0;
    if (!c || !total) return failf(c, FM_EINVAL, "null argument");
    if (!(c->p.flags & FM_FLAG_CONTOUR_POINTS))
        return failf(c, FM_ESTATE, "points not traced: create with FM_FLAG_CONTOUR_POINTS");
    if (c->pts_off.empty()) return failf(c, FM_ESTATE, "no traced batch: call fm_wait first");
    if (int rc = check_frame(c, frame, stream, false)) return rc;
    const size_t f = (size_t)frame * c->p.n_streams + stream;
    const size_t first = c->pts_off[f], n = c->pts_off[f + 1] - first;
    *total = n;
    if (cap < n) return failf(c, FM_EINVAL, "%zu points, room for %zu: call again with *total", n, cap);
    if (n && !xy) return failf(c, FM_EINVAL, "null point buffer");
    if (n) std::memcpy(xy, c->h_pts + first * 2, n * 2 * sizeof(int32_t));
    return FM_OK;
}

int fm_get_counts(fm_ctx* c, int32_t* counts) {
    if (!c || !counts) return failf(c, FM_EINVAL, "null argument");
    std::memcpy(counts, c->ready_counts.data(), c->ready_counts.size() * sizeof(int32_t));
    return FM_OK;
}

int fm_get_contours(fm_ctx* c, int frame, int stream, fm_contour* out, int cap) {
    if (!c) return failf(kNoCtx, FM_EINVAL, "null context");
    if (int rc = check_frame(c, frame, stream, false)) return rc;
    const size_t f = (size_t)frame * c->p.n_streams + stream;
    const auto& v = c->contours[f];
    const int m = out ? std::min<int>(cap, (int)v.size()) : 0;
    for (int i = 0; i < m; i++) out[i] = v[i];
    return c->ready_counts[f];
}

int fm_read_mask(fm_ctx* c, int frame, int stream, uint8_t* out) {
    if (!c || !out) return failf(c, FM_EINVAL, "null argument");
    if (int rc = check_frame(c, frame, stream, true)) return rc;
    FM_HIP_TRY(c, hipSetDevice(c->p.device));
    const size_t f = (size_t)frame * c->p.n_streams + stream;
    hipStream_t st = c->aux_stream;
    if (c->traits().tiles) {
        const BatchSlot& B = c->slots[c->ready_slot];
        FM_HIP_TRY(c, launch_expand_bits(st, B.d_dbits + f * c->ntiles * 64, B.d_candf + f * c->ntiles, c->d_mask, c->h, c->w,
                                      c->ntx));
        FM_HIP_TRY(c, hipMemcpyAsync(out, c->d_mask, c->work_plane, hipMemcpyDeviceToHost, st));
    } else {
        FM_HIP_TRY(c, hipMemcpyAsync(out, c->d_mask + f * c->work_plane, c->work_plane, hipMemcpyDeviceToHost, st));
    }
    FM_HIP_TRY(c, hipStreamSynchronize(st));
    return FM_OK;
}

int fm_read_threshold_bits(fm_ctx* c, int frame, int stream, uint64_t* out) {
    if (!c || !out) return failf(c, FM_EINVAL, "null argument");
    if (!c->traits().bits) return failf(c, FM_ESTATE, "this pixel path keeps no threshold bits");
    if (int rc = check_frame(c, frame, stream, true)) return rc;
    FM_HIP_TRY(c, hipSetDevice(c->p.device));
    const BatchSlot& B = c->slots[c->ready_slot];
    const size_t f = (size_t)frame * c->p.n_streams + stream;
    const size_t words = (size_t)c->ntiles * 64;
    FM_HIP_TRY(c, hipMemcpyAsync(out, B.d_bits + f * words, words * sizeof(uint64_t), hipMemcpyDeviceToHost, c->aux_stream));
    FM_HIP_TRY(c, hipStreamSynchronize(c->aux_stream));
    return FM_OK;
}

int fm_read_plane(fm_ctx* c, int plane, int frame, int stream, uint8_t* out) {
    if (!c || !out) return failf(c, FM_EINVAL, "null argument");
    if (plane < 0 || plane > FM_PLANE_SMALL) return failf(c, FM_EINVAL, "plane %d", plane);
    if (plane == FM_PLANE_SMALL && c->rmode == ResizeMode::Identity)
        return failf(c, FM_ESTATE, "no resize (box_size = frame width): the frame is the work image");
    if (plane != FM_PLANE_SMALL && !(c->p.flags & FM_FLAG_KEEP_PLANES))
        return failf(c, FM_ESTATE, "planes not kept: create with FM_FLAG_KEEP_PLANES");
    if (int rc = check_frame(c, frame, stream, true)) return rc;
    FM_HIP_TRY(c, hipSetDevice(c->p.device));
    const BatchSlot& B = c->slots[c->ready_slot];
    const size_t f = (size_t)frame * c->p.n_streams + stream;
    if (plane == FM_PLANE_SMALL) {  // the INTER_AREA output, [T][S][h][w][3]
        FM_HIP_TRY(c, hipMemcpyAsync(out, B.d_work + f * c->work_plane * 3, c->work_plane * 3, hipMemcpyDeviceToHost,
                                  c->aux_stream));
        FM_HIP_TRY(c, hipStreamSynchronize(c->aux_stream));
        return FM_OK;
    }
    const size_t Fcur = (size_t)c->ready * c->p.n_streams;
    FM_HIP_TRY(c, hipMemcpyAsync(out, B.d_planes + ((size_t)plane * Fcur + f) * c->work_plane, c->work_plane,
                              hipMemcpyDeviceToHost, c->aux_stream));
    FM_HIP_TRY(c, hipStreamSynchronize(c->aux_stream));
    return FM_OK;
}

int fm_read_frame(fm_ctx* c, int frame, int stream, uint8_t* out) {
    if (!c || !out) return failf(c, FM_EINVAL, "null argument");
    if (int rc = check_frame(c, frame, stream, true)) return rc;
    const BatchSlot& B = c->slots[c->ready_slot];
    if (!B.src) return failf(c, FM_ESTATE, "no source frames for the last waited batch");
    FM_HIP_TRY(c, hipSetDevice(c->p.device));
    FM_HIP_TRY(c, hipMemcpyAsync(out, B.src + ((size_t)frame * c->p.n_streams + stream) * c->src_frame_bytes,
                              c->src_frame_bytes, hipMemcpyDeviceToHost, c->aux_stream));
    FM_HIP_TRY(c, hipStreamSynchronize(c->aux_stream));
    return FM_OK;
}

int fm_frame_device(fm_ctx* c, int frame, int stream, const uint8_t** out) {
    if (!c || !out) return failf(c, FM_EINVAL, "null argument");
    if (int rc = check_frame(c, frame, stream, true)) return rc;
    const BatchSlot& B = c->slots[c->ready_slot];
    if (!B.src) return failf(c, FM_ESTATE, "no source frames for the last waited batch");
    *out = B.src + ((size_t)frame * c->p.n_streams + stream) * c->src_frame_bytes;
    return FM_OK;
}

}  // extern "C"

namespace {
// a device / page-locked buffer of the context leaves it and its footprint (nullptr: nothing)
void dfree(fm_ctx* c, const void* p) {
    auto it = c->dev_sizes.find(p);
    if (it == c->dev_sizes.end()) return;
    (void)hipFree(const_cast<void*>(p));
    c->dev_bytes -= it->second;
    c->dev_sizes.erase(it);
}

void pfree(fm_ctx* c, const void* p) {
    auto it = c->pin_sizes.find(p);
    if (it == c->pin_sizes.end()) return;
    (void)hipHostFree(const_cast<void*>(p));
    c->pinned_bytes -= it->second;
    c->pin_sizes.erase(it);
}

// the pool entry that starts at p and is handed out, or -1
long retained_entry(const fm_ctx* c, const uint8_t* p) {
    if (!c->d_ret || p < c->d_ret) return -1;
    const size_t off = (size_t)(p - c->d_ret);
    if (off % c->ret_stride || off / c->ret_stride >= c->ret_used.size()) return -1;
    return c->ret_used[off / c->ret_stride] ? (long)(off / c->ret_stride) : -1;
}
}  // namespace

extern "C" {

int fm_retain_reserve(fm_ctx* c, int frames) {
    if (!c) return failf(kNoCtx, FM_EINVAL, "null context");
    if (frames < 0) return failf(c, FM_EINVAL, "a pool of %d retained frames", frames);
    if (c->ret_in_use)
        return failf(c, FM_ESTATE, "%d retained frames are in use: release them before resizing the pool", c->ret_in_use);
    if ((size_t)frames == c->ret_used.size()) return FM_OK;
    FM_HIP_TRY(c, hipSetDevice(c->p.device));
    const size_t stride = (c->src_frame_bytes + 255) & ~(size_t)255;  // hipMalloc's base is 256-byte aligned too
    uint8_t* pool = nullptr;
    RetainPair *dtab = nullptr, *htab = nullptr;
    if (frames > 0) {  // the new pool first: a failure leaves the old one as it was
        int rc = dalloc(c, &pool, stride * (size_t)frames);
        if (!rc) rc = dalloc(c, &dtab, (size_t)frames);
        if (!rc && halloc(c, &htab, (size_t)frames * sizeof(RetainPair), hipHostMallocDefault) != hipSuccess)
            rc = failf(c, FM_ENOMEM, "hipHostMalloc(%zu bytes) for the retain table", (size_t)frames * sizeof(RetainPair));
        if (rc) {
            dfree(c, pool);
            dfree(c, dtab);
            return rc;
        }
    }
    dfree(c, c->d_ret);
    dfree(c, c->d_rtab);
    pfree(c, c->h_rtab);
    c->d_ret = pool;
    c->d_rtab = dtab;
    c->h_rtab = htab;
    c->ret_stride = stride;
    c->ret_used.assign((size_t)frames, 0);
    return FM_OK;
}

int fm_retain_frames(fm_ctx* c, const int32_t* frame_stream, int n, const uint8_t** dev_out) {
    if (!c) return failf(kNoCtx, FM_EINVAL, "null context");
    if (n < 0) return failf(c, FM_EINVAL, "%d frames to retain", n);
    if (n == 0) return FM_OK;
    if (!frame_stream || !dev_out) return failf(c, FM_EINVAL, "null argument");
    if (c->ready_slot < 0 || c->ready < 1) return failf(c, FM_ESTATE, "no batch has been waited for");
    const BatchSlot& B = c->slots[c->ready_slot];
    if (B.gen != c->ready_gen) return failf(c, FM_ESTATE, "the batch's device results were overwritten by a later submit");
    if (!B.src) return failf(c, FM_ESTATE, "no source frames for the last waited batch");
    const int S = c->p.n_streams;
    for (int i = 0; i < n; i++) {
        const int t = frame_stream[2 * i], s = frame_stream[2 * i + 1];
        if (t < 0 || t >= c->ready || s < 0 || s >= S)
            return failf(c, FM_EINVAL, "pair %d: (frame %d, stream %d) not in the last batch (%d frames of %d streams)", i,
                         t, s, c->ready, S);
    }
    const size_t cap = c->ret_used.size();
    if ((size_t)n > cap - (size_t)c->ret_in_use)
        return failf(c, FM_ENOMEM, "%d frames to retain, %zu of the pool's %zu entries free (fm_retain_reserve)", n,
                     cap - (size_t)c->ret_in_use, cap);
    size_t e = 0;
    for (int i = 0; i < n; i++, e++) {  // (the table is idle: the last call synchronised)
        while (c->ret_used[e]) e++;
        c->h_rtab[i] = {B.src + ((size_t)frame_stream[2 * i] * S + frame_stream[2 * i + 1]) * c->src_frame_bytes,
                        c->d_ret + e * c->ret_stride};
    }
    hipStream_t st = c->aux_stream;
    FM_HIP_TRY(c, hipSetDevice(c->p.device));
    FM_HIP_TRY(c, hipMemcpyAsync(c->d_rtab, c->h_rtab, (size_t)n * sizeof(RetainPair), hipMemcpyHostToDevice, st));
    FM_HIP_TRY(c, launch_retain_frames(st, c->d_rtab, n, c->src_frame_bytes));
    FM_HIP_TRY(c, hipStreamSynchronize(st));
    for (int i = 0; i < n; i++) {
        c->ret_used[(size_t)(c->h_rtab[i].dst - c->d_ret) / c->ret_stride] = 1;
        dev_out[i] = c->h_rtab[i].dst;
    }
    c->ret_in_use += n;
    return FM_OK;
}

int fm_release_frames(fm_ctx* c, const uint8_t* const* dev, int n) {
    if (!c) return failf(kNoCtx, FM_EINVAL, "null context");
    if (n < 0) return failf(c, FM_EINVAL, "%d frames to release", n);
    if (n == 0) return FM_OK;
    if (!dev) return failf(c, FM_EINVAL, "null argument");
    std::vector<long> idx((size_t)n);
    std::vector<uint8_t> seen(c->ret_used.size(), 0);
    for (int i = 0; i < n; i++) {
        idx[i] = retained_entry(c, dev[i]);
        if (idx[i] < 0 || seen[idx[i]])
            return failf(c, FM_EINVAL, "address %d (%p) is not a retained frame of this context, or was released", i,
                         (const void*)dev[i]);
        seen[idx[i]] = 1;
    }
    for (long k : idx) c->ret_used[k] = 0;
    c->ret_in_use -= n;
    return FM_OK;
}

int fm_read_retained(fm_ctx* c, const uint8_t* dev, uint8_t* host_out) {
    if (!c || !dev || !host_out) return failf(c, FM_EINVAL, "null argument");
    if (retained_entry(c, dev) < 0)
        return failf(c, FM_EINVAL, "%p is not a retained frame of this context, or was released", (const void*)dev);
    FM_HIP_TRY(c, hipSetDevice(c->p.device));
    FM_HIP_TRY(c, hipMemcpyAsync(host_out, dev, c->src_frame_bytes, hipMemcpyDeviceToHost, c->aux_stream));
    FM_HIP_TRY(c, hipStreamSynchronize(c->aux_stream));
    return FM_OK;
}

int fm_retained_count(const fm_ctx* c, int* in_use, int* capacity) {
    if (!c) return failf(kNoCtx, FM_EINVAL, "null context");
    if (in_use) *in_use = c->ret_in_use;
    if (capacity) *capacity = (int)c->ret_used.size();
    return FM_OK;
}

int fm_read_background(fm_ctx* c, int stream, double* out) {
    if (!c || !out) return failf(c, FM_EINVAL, "null argument");
    if (c->path == PixelPath::Mog2) return failf(c, FM_ESTATE, "a Gaussian-mixture context has no average: fm_mog2_background / fm_mog2_read_model");
    if (int rc = check_idle(c)) return rc;
    if (int rc = check_stream(c, stream)) return rc;
    if (!c->bg_init[stream]) return failf(c, FM_ESTATE, "stream %d has no background yet", stream);
    FM_HIP_TRY(c, hipSetDevice(c->p.device));
    FM_HIP_TRY(c, hipStreamSynchronize(c->stream));
    const size_t n = c->work_plane * c->traits().bg_ch;  // a colour context: [h][w][3]
    FM_HIP_TRY(c, hipMemcpyAsync(out, c->d_bg[c->bg_cur] + (size_t)stream * n, n * sizeof(double), hipMemcpyDeviceToHost,
                              c->stream));
    FM_HIP_TRY(c, hipStreamSynchronize(c->stream));
    return FM_OK;
}

int fm_write_background(fm_ctx* c, int stream, const double* in) {
    if (!c || !in) return failf(c, FM_EINVAL, "null argument");
    if (c->path == PixelPath::Mog2) return failf(c, FM_ESTATE, "a Gaussian-mixture context has no average: fm_mog2_write_model");
    if (int rc = check_idle(c)) return rc;
    if (int rc = check_stream(c, stream)) return rc;
    FM_HIP_TRY(c, hipSetDevice(c->p.device));
    const size_t n = c->work_plane * c->traits().bg_ch;
    FM_HIP_TRY(c, hipMemcpyAsync(c->d_bg[c->bg_cur] + (size_t)stream * n, in, n * sizeof(double), hipMemcpyHostToDevice,
                              c->stream));
    FM_HIP_TRY(c, hipStreamSynchronize(c->stream));
    c->bg_init[stream] = 1;
    return FM_OK;
}

int fm_background_channels(const fm_ctx* c, int* channels) {
    if (!c || !channels) return failf(kNoCtx, FM_EINVAL, "null argument");
    if (c->path == PixelPath::Mog2) return failf(kNoCtx, FM_ESTATE, "a Gaussian-mixture context has no average: fm_mog2_background");
    *channels = c->traits().bg_ch;
    return FM_OK;
}

// The Gaussian-mixture model of one stream between the device's column-major planes ([15][x][CS] floats and
// [x][CS] bytes) and the ABI's row-major [5][h][w] arrays: whole planes are copied and transposed on the host.
namespace {
int check_mog2_ctx(fm_ctx* c, int stream) {
    if (c->path != PixelPath::Mog2) return failf(c, FM_ESTATE, "not a Gaussian-mixture context (FM_FLAG_MOG2)");
    if (int rc = check_idle(c)) return rc;
    return check_stream(c, stream);
}
}  // namespace

int fm_mog2_read_model(fm_ctx* c, int stream, float* weight, float* mean, float* var, uint8_t* nmodes, int64_t* nframes) {
    if (!c) return failf(kNoCtx, FM_EINVAL, "null context");
    if (int rc = check_mog2_ctx(c, stream)) return rc;
    const int h = c->h, w = c->w, CS = c->nty * 64;
    const size_t PS = (size_t)w * CS;
    std::vector<uint8_t> nm(PS);
    std::vector<float> st(weight || mean || var ? 15 * PS : 0);
    FM_HIP_TRY(c, hipSetDevice(c->p.device));
    FM_HIP_TRY(c, hipStreamSynchronize(c->stream));
    FM_HIP_TRY(c, hipMemcpy(nm.data(), c->d_mog_nm + (size_t)stream * PS, PS, hipMemcpyDeviceToHost));
    if (!st.empty())
        FM_HIP_TRY(c, hipMemcpy(st.data(), c->d_mog_state + (size_t)stream * 15 * PS, 15 * PS * sizeof(float), hipMemcpyDeviceToHost));
    float* const dst[3] = {weight, mean, var};
    for (int y = 0; y < h; y++)
        for (int x = 0; x < w; x++) {
            const size_t pix = (size_t)x * CS + y, o = (size_t)y * w + x;
            const int n = nm[pix];
            if (nmodes) nmodes[o] = (uint8_t)n;
            for (int k = 0; k < 3; k++)
                if (dst[k])
                    for (int m = 0; m < 5; m++) dst[k][(size_t)m * h * w + o] = m < n ? st[(size_t)(k * 5 + m) * PS + pix] : 0.f;
        }
    if (nframes) *nframes = c->mog_nframes[stream];
    return FM_OK;
}

int fm_mog2_write_model(fm_ctx* c, int stream, const float* weight, const float* mean, const float* var,
                        const uint8_t* nmodes, const int64_t* nframes) {
    if (!c) return failf(kNoCtx, FM_EINVAL, "null context");
    if (!weight || !mean || !var || !nmodes || !nframes) return failf(c, FM_EINVAL, "null argument");
    if (int rc = check_mog2_ctx(c, stream)) return rc;
    if (*nframes < 0) return failf(c, FM_EINVAL, "nframes %lld is negative", (long long)*nframes);
    const int h = c->h, w = c->w, CS = c->nty * 64;
    const size_t PS = (size_t)w * CS;
    for (size_t i = 0; i < (size_t)h * w; i++)
        if (nmodes[i] > 5) return failf(c, FM_EINVAL, "nmodes %d above 5 at pixel %zu", (int)nmodes[i], i);
    std::vector<uint8_t> nm(PS, 0);
    std::vector<float> st(15 * PS, 0.f);
    const float* const src[3] = {weight, mean, var};
    for (int y = 0; y < h; y++)
        for (int x = 0; x < w; x++) {
            const size_t pix = (size_t)x * CS + y, o = (size_t)y * w + x;
            nm[pix] = nmodes[o];
            for (int k = 0; k < 3; k++)
                for (int m = 0; m < nmodes[o]; m++) st[(size_t)(k * 5 + m) * PS + pix] = src[k][(size_t)m * h * w + o];
        }
    FM_HIP_TRY(c, hipSetDevice(c->p.device));
    FM_HIP_TRY(c, hipStreamSynchronize(c->stream));
    FM_HIP_TRY(c, hipMemcpy(c->d_mog_nm + (size_t)stream * PS, nm.data(), PS, hipMemcpyHostToDevice));
    FM_HIP_TRY(c, hipMemcpy(c->d_mog_state + (size_t)stream * 15 * PS, st.data(), 15 * PS * sizeof(float), hipMemcpyHostToDevice));
    c->mog_nframes[stream] = *nframes;
    c->bg_init[stream] = 1;
    return FM_OK;
}

int fm_mog2_background(fm_ctx* c, int stream, uint8_t* out) {
    if (!c) return failf(kNoCtx, FM_EINVAL, "null context");
    if (!out) return failf(c, FM_EINVAL, "null argument");
    if (int rc = check_mog2_ctx(c, stream)) return rc;
    FM_HIP_TRY(c, hipSetDevice(c->p.device));
    const Mog2Dev md{c->d_mog_state, c->d_mog_nm, nullptr, c->mog2};
    FM_HIP_TRY(c, launch_mog2_background(c->stream, md, stream, c->h, c->w, c->nty, c->d_mog_bg));
    FM_HIP_TRY(c, hipMemcpyAsync(out, c->d_mog_bg, c->work_plane, hipMemcpyDeviceToHost, c->stream));
    FM_HIP_TRY(c, hipStreamSynchronize(c->stream));
    return FM_OK;
}

int fm_kernel_time_stats(fm_ctx* c, const char** names, double* ms, int64_t* launches, double* stamped_ms,
                         int64_t* stamped, double* ms_sq, double* busy_ms, int64_t* unstamped, int cap) {
    if (!c) return failf(kNoCtx, FM_EINVAL, "null context");
    FM_HIP_TRY(c, hipSetDevice(c->p.device));
    if (c->timer.fold_stamps() != 0) return failf(c, FM_EHIP, "reading the launch stamps failed");
    const auto& T = c->timer;
    const int n = (int)T.names.size();
    for (int i = 0; i < std::min(n, cap); i++) {
        if (names) names[i] = T.names[i];
        if (ms) ms[i] = T.ms[i];
        if (launches) launches[i] = T.launches[i];
        if (ms_sq) ms_sq[i] = T.ms_sq[i];
        if (stamped) stamped[i] = T.stamped[i];
        if (stamped_ms) stamped_ms[i] = T.stamped_ms[i];
        if (busy_ms) busy_ms[i] = T.busy[i].ms + (T.busy[i].open ? (double)(T.busy[i].e - T.busy[i].s) * 1e-5 : 0.0);
    }
    if (unstamped) *unstamped = T.unstamped;
    return n;
}

int fm_kernel_times(fm_ctx* c, const char** names, double* ms, int64_t* launches, int cap) {
    return fm_kernel_time_stats(c, names, ms, launches, nullptr, nullptr, nullptr, nullptr, nullptr, cap);
}

int fm_kernel_time_spread(fm_ctx* c, double* ms_sq, int cap) {
    if (!c || !ms_sq) return failf(c, FM_EINVAL, "null argument");
    return fm_kernel_time_stats(c, nullptr, nullptr, nullptr, nullptr, nullptr, ms_sq, nullptr, nullptr, cap);
}

int fm_kernel_time_busy(fm_ctx* c, double* busy_ms, int cap) {
    if (!c || !busy_ms) return failf(c, FM_EINVAL, "null argument");
    return fm_kernel_time_stats(c, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, busy_ms, nullptr, cap);
}

int fm_reset_kernel_times(fm_ctx* c) {
    if (!c) return failf(kNoCtx, FM_EINVAL, "null context");
    FM_HIP_TRY(c, hipSetDevice(c->p.device));
    c->timer.reset();
    return FM_OK;
}

int fm_footprint(const fm_ctx* c, size_t* device_bytes, size_t* pinned_bytes) {
    if (!c) return failf(kNoCtx, FM_EINVAL, "null context");
    if (device_bytes) *device_bytes = c->dev_bytes;
    if (pinned_bytes) *pinned_bytes = c->pinned_bytes;
    return FM_OK;
}

}  // extern "C"
