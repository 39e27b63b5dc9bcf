// fm_internal.h — shared declarations between the C ABI (fm_capi.cpp), its host helpers
// (fm_tables.cpp, fm_timer.cpp) and the gfx950 kernels (fm_*.hip).  Not part of the public boundary.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdlib>
#include <string>
#include <vector>

#include "../../include/find_motion_amd.h"

namespace fm {

template <int I> struct IntC { static constexpr int value = I; };
// compile-time unrolled loop: fn(IntC<0>{}), ..., fn(IntC<N-1>{})
template <int N, int I = 0, typename Fn>
__device__ __forceinline__ void static_for(Fn&& fn) {
    if constexpr (I < N) {
        fn(IntC<I>{});
        static_for<N, I + 1>(fn);
    }
}

// Developer switches (A/B experiments, profiling stamps) are read from the environment
// only by the dev build (make VARIANT=dev -> libfm_hip_dev.so); the product library
// ignores the environment.
#ifdef FM_DEV_SWITCHES
constexpr bool kDevSwitches = true;
#else
constexpr bool kDevSwitches = false;
#endif
inline const char* dev_env(const char* name) { return kDevSwitches ? std::getenv(name) : nullptr; }

// Bounds checks on every data-dependent index of the contour pass (make VARIANT=checked ->
// libfm_hip_checked.so): a violation sets bit `code` of the mapped error word, the access is
// skipped, and fm_wait fails with the codes.  Compiled out of the product library.
#ifdef FM_BOUNDS_CHECK
#define FM_OOB(a, cond, code) (!(cond) ? (atomicOr((a).dbg_err, 1 << (code)), true) : false)
#else
#define FM_OOB(a, cond, code) false
#endif

constexpr int kMaxK = 255;        // largest Gaussian size handled by the tiled kernel
constexpr int kCclBlock = 32;     // CCL block edge (pixels)
constexpr int kTileMaxRuns = 1600; // runs per 64x64 tile of a dilated mask (<= 24 per row => 1536)
constexpr int kHeavyWaves = 64;       // k_tile_heavy persistent waves (fm_ccl.hip)
constexpr int kNodesPerTileFrame = 32; // union-find nodes each frame owns per tile (its quota)
constexpr int kFrameCclTiles = 16;     // work images of at most this many tiles: one contour workgroup per frame
constexpr int kNodesShared = 16;       // + a shared overflow pool of this many per tile-frame (at least one
                                       //   worst-case frame), taken from only by frames past their quota

// Host-built INTER_AREA tables (computeResizeAreaTab restated in fm_tables.cpp).
// Per destination index d: taps start at src index ofs[d], cnt[d] taps, weights
// wt[d * max_taps + j] (float32 exactly as OpenCV stores DecimateAlpha::alpha).
struct AreaAxis {
    int n_dst = 0, max_taps = 0;
    std::vector<int32_t> ofs, cnt;
    std::vector<float> wt;
};

// Everything the per-frame pixel kernel needs for one batch step.
struct PixelArgs {
    const uint8_t* src;          // work-size BGR for this batch frame t: [S][h][w][3]
    double* bg;                  // [S][h*w]
    const uint8_t* keep;         // [S][h*w] (only read where has_keep[s])
    const uint8_t* has_keep;     // [S]
    const uint8_t* init;         // [S] 1 => bg := blur before the diff (first frame), or nullptr
    uint8_t* mask_out;           // dilated threshold [S][h*w]
    uint8_t* gray_out;           // optional planes [S][h*w] (nullptr when not kept)
    uint8_t* blur_out;
    uint8_t* delta_out;
    int S, h, w;
    int ksize;
    int thresh;
    double alpha, beta;          // beta = 1 - alpha
    long long acc_vec_end;       // h*w - (h*w % 16): AVX2 fma body vs scalar tail
    int cvt_simd;                // h*w >= 16: f64->f32->rne path of convertScaleAbs
    int32_t coef[kMaxK];         // fixed-point Gaussian taps (sum 256)
};

struct CclArgs {
    const uint8_t* mask;         // [F][h*w]
    int32_t* label;              // [F][h*w]
    uint8_t* outer;              // [F][h*w]
    int32_t* cid;                // [F][h*w]
    int32_t* count;              // [F]
    int32_t* rec;                // [F][cap][5]: first, minx, miny, maxx, maxy
    int F, h, w, cap;
};

// Temporally blocked fused kernel + tile-summary CCL (fm_fused.hip, fm_ccl.hip).
// Global CCL nodes of one batch slot: ids [0, F*ntiles) are the empty-tile regions
// (node f*ntiles + representative tile); a labelled candidate tile takes nroots
// consecutive ids (TileRec::nbase) from its frame's quota [F*ntiles + f*nquota, +nquota),
// or past that from the slot's shared overflow pool (ids from F*ntiles + F*nquota).
struct NodeRec {
    uint64_t key;     // foreground: (raster-first pixel << 32) | left-background reference
    int32_t parent;   // global union-find
    uint32_t flags;   // bit0 foreground, bit1 background touching the image border (outer)
    int32_t minx, maxx, maxy, pad;
};
struct TileRec {
    int32_t nroots;                   // components of the tile (ordinals 0..nroots-1, raster order)
    int32_t nbase;                    // node id of ordinal 0 (nodes of a candidate tile are consecutive)
    int32_t pad[2];
    uint16_t edges[256];              // 0..63 left col, 64.. right col, 128.. top row, 192.. bottom row:
                                      // component ordinal | fg << 15
};

// per-tile threshold-bit flags written by the pixel stage or by k_tile_flags (decide which tiles the
// 5x5 dilation can make non-empty: the tile itself or a neighbour's 2-px margin)
enum : uint32_t {
    FLAG_ANY = 1u, FLAG_L = 2u, FLAG_R = 4u, FLAG_T = 8u, FLAG_B = 16u,
    FLAG_TL = 32u, FLAG_TR = 64u, FLAG_BL = 128u, FLAG_BR = 256u,
};

struct FusedArgs {
    const uint8_t* src;          // work-size BGR frames [T][S][h][w][3]
    const double* bg_in;         // [S][h*w] background before the batch
    double* bg_out;              // [S][h*w] background after the batch
    const uint8_t* keep;         // [S][h*w]
    const uint8_t* has_keep;     // [S]
    const uint8_t* init;         // [S] or nullptr: 1 => bg := blur at the batch's first frame
    uint8_t* mask_out;           // [T][S][h*w] dilated threshold
    uint8_t* planes;             // optional [3][T][S][h*w] gray, blur, frame_delta
    uint64_t* bits;              // [F][ntiles][64] threshold rows as bit masks (k_pix output, k_dilate_ccl input)
    uint64_t* dbits;             // [F][ntiles][64] dilated rows (VideoFrame.thresh as bits; == bits when the
                                 // pixel kernel dilates itself, i.e. the generic-k k_fused path)
    TileRec* tiles;              // [F][ntiles]
    uint32_t* tflag;             // [F][ntiles][tflag_waves] FLAG_* bits: where the tile has threshold bits (dilated
                                 // bits on the k_fused path, which sets FLAG_ANY only).  Written by k_fused,
                                 // by the small-image / wide-Gaussian scans, or, for the 64 x 64 tile pixel
                                 // kernels, by k_tile_flags on the contour stream from `bits`
    uint8_t* candf;              // [F][ntiles] 1: the tile's dilated mask may be non-empty (labelled)
    int32_t* clist;              // [F][ntiles] candidate tiles of each frame
    int32_t* rlist;              // [F][ntiles] representative tile of each empty-tile region
    int32_t* regrep;             // [F][ntiles] empty tile -> its region's representative tile
    int32_t* ncr;                // [F][2] candidates, regions
    NodeRec* nodes;              // [nnodes]: F*ntiles region nodes, then the pool of candidate-tile nodes
    int32_t* count;              // [3F+3]: [f] external contours, [F+f] overflow flag, [2F] shared node-pool
                                 // fill, [2F+1] heavy tiles listed, [2F+2+f] frame f's node-quota fill, [3F+2]
                                 // frames done (k_frame_contours; its last workgroup re-arms [2F], [2F+1], [3F+2])
    int32_t* h_stats;            // mapped host [2]: nodes taken from the shared pool, heavy tiles (written by
                                 // k_counts, or by the last k_frame_contours workgroup; diagnostics)
    int32_t* heavy;              // [F * ntiles] tiles with more runs than the light CCL pass holds
    int32_t* rec;                // [F][cap][5]
    int32_t* h_count;            // mapped host [F]: external contours per frame (written by k_fold_emit)
    int32_t* h_overflow;         // mapped host [F]: frame needs the pixel-level fallback
    int T, S, h, w, ksize, thresh;
    int t_begin, t_end;          // k_pix: frames of the batch this launch processes
    int ntx, nty, ntiles, nnodes, cap, cvt_simd;
    int nquota;                  // nodes per frame quota
    int tflag_waves;             // words per tile-frame in tflag: 1 (k_fused's atomicOr, k_tile_flags) or 8 (the
                                 // small-image and wide-Gaussian scans)
    int dbg_skip;                // profiling-only stage ablation (FM_DEBUG_SKIP); 0 in normal use
    uint64_t* dbg_ts;            // profiling-only s_memtime stamps [F][ntiles][16] (FM_TS); nullptr in normal use
    uint64_t* dbg_pts;           // profiling-only k_pix workgroup stamps [S][ntiles][4] (FM_PTS); nullptr in normal use
    int32_t* dbg_err;            // mapped host word: FM_OOB violation bits (checked build only)
    double alpha, beta;
    long long acc_vec_end;
    int any_keep;                // some stream of the context has a keep-mask (k_pix5 variant choice)
    uint64_t* kstamp;            // this launch's [first start, last end] stamp pair (KernelTimer::stamp) or nullptr
    int32_t coef[kMaxK];
};

// In-kernel launch stamps (KernelTimer::stamp): thread 0 of every workgroup takes the 100 MHz
// s_memrealtime counter at its start into ks[0] (atomic min), lane 0 of every wave at its end into
// ks[1] (atomic max), so ks[1] - ks[0] is the launch from its first workgroup's start to its last
// wave's end.  Plain (vector) global atomics that return nothing.
__device__ __forceinline__ void kstamp_begin(uint64_t* ks) {
    if (ks && threadIdx.x == 0)
        atomicMin(reinterpret_cast<unsigned long long*>(ks), (unsigned long long)__builtin_amdgcn_s_memrealtime());
}
__device__ __forceinline__ void kstamp_end(uint64_t* ks) {
    if (ks && (threadIdx.x & 63) == 0)
        atomicMax(reinterpret_cast<unsigned long long*>(ks) + 1, (unsigned long long)__builtin_amdgcn_s_memrealtime());
}
// Kernels of thousands of short workgroups (the INTER_AREA resize): the start from the first 8
// workgroups dispatched, the end from wave 0 of every workgroup (one atomic per workgroup).
__device__ __forceinline__ void kstamp_begin_grid(uint64_t* ks) {
    if (blockIdx.x + blockIdx.y * gridDim.x < 8) kstamp_begin(ks);
}
__device__ __forceinline__ void kstamp_end_wg(uint64_t* ks) {
    if (threadIdx.x < 64) kstamp_end(ks);
}

// computeResizeAreaTab restated (fm_tables.cpp); false if a destination's taps are not consecutive
bool build_area_axis(int ssize, int dsize, double scale, AreaAxis& A);
// GaussianBlur's 8-bit fixed-point taps for CV_8U, sigma = 0 (fm_tables.cpp); false for an n it does not take
bool gaussian_taps(int n, std::vector<int32_t>& out);

// Kernel launchers (fm_kernels.hip, fm_fused.hip).  All asynchronous on `st`.
hipError_t launch_resize_area(hipStream_t st, const uint8_t* src, uint8_t* dst, int F, int H, int W,
                              int h, int w, const int32_t* xofs, const int32_t* xcnt, const float* xwt,
                              int xtaps, const int32_t* yofs, const int32_t* ycnt, const float* ywt,
                              int ytaps, const uint8_t* const* srcs = nullptr, uint64_t* kstamp = nullptr);
hipError_t launch_resize_area_fast(hipStream_t st, const uint8_t* src, uint8_t* dst, int F, int H, int W,
                                   int h, int w, int sx, int sy, uint64_t* kstamp = nullptr);
// INTER_AREA towards a larger image (cv::resize's bilinear resizer with area-mode taps; fm_roi.h builds xtab / ytab
// and the plan).  A workgroup takes `rows` destination rows of a span of `cols` destination columns (nspans spans
// per row) and holds the source bytes and the horizontal results of at most `nsrc` source rows in `lds` bytes of LDS.
struct AreaUpPlan {
    int rows, cols, nspans, nsrc, lds;
};
// 16-bit elements between two rows of horizontal results in LDS: the span's 3 * cols, two more that a lane's
// third dword may reach into, rows dword-aligned
__host__ __device__ constexpr int area_up_hstride(int cols) { return (3 * cols + 3) & ~1; }
// bytes between two rows of staged source bytes: up to cols + 1 source pixels from up to 3 bytes into the first
// dword, and the 12 bytes a lane reads from the dword of its first tap on
__host__ __device__ constexpr int area_up_rawstride(int cols) { return (3 * (cols + 1) + 15) & ~3; }
hipError_t launch_resize_area_up(hipStream_t st, const uint8_t* src, uint8_t* dst, int F, int H, int W, int h, int w,
                                 const uint32_t* xtab, const uint32_t* ytab, const AreaUpPlan& plan,
                                 const uint8_t* const* srcs = nullptr, uint64_t* kstamp = nullptr);
hipError_t launch_pixel(hipStream_t st, const PixelArgs& a);
// YUV frames -> packed BGR [F][H][W][3] (fm_yuv.hip).  Frame f is at srcs[f] (a device table of F
// addresses) when srcs is set, at src + f * frame_stride otherwise; pitch / chroma_offset as resolved
// from fm_yuv_layout (never 0).  runs, groups and total are filled in by the launcher.
struct YuvArgs {
    const uint8_t* src;
    const uint8_t* const* srcs;
    size_t frame_stride, chroma_offset;
    uint8_t* dst;
    int format, pitch, W, H, F;
    int runs, groups;     // lane runs per row, row groups (row pairs for 4:2:0) per frame
    long long total;      // F * groups * runs
    uint64_t* kstamp;
};
hipError_t launch_yuv2bgr(hipStream_t st, const YuvArgs& a);
// n copies of `bytes` bytes each in one launch (fm_kernels.hip, k_retain_frames): copy i from pairs[i].src (any
// alignment) to pairs[i].dst (16-byte aligned); pairs is a device table of n entries
struct RetainPair {
    const uint8_t* src;
    uint8_t* dst;
};
hipError_t launch_retain_frames(hipStream_t st, const RetainPair* pairs, int n, size_t bytes);
struct KernelTimer;
hipError_t launch_ccl(hipStream_t st, const CclArgs& a, KernelTimer* timer);
hipError_t launch_fused(hipStream_t st, const FusedArgs& a, KernelTimer* timer);
int fused_lds_bytes(int ksize);
int fused_max_ksize();
// k_pix (fm_pix.hip): chain once per pixel, threshold bits out; dilation in the CCL kernel
// frames [a.t_begin, a.t_end) of the batch; init: a.init may mark first frames (only at t_begin)
hipError_t launch_pix(hipStream_t st, const FusedArgs& a, bool planes, bool init);
int pix_lds_bytes(int ksize);
bool pix_supported(int ksize);
// The blur + scan paths: a frame-parallel blur into a scratch of blur bytes (scan_scratch_bytes, fm_scan.h), then
// fm_scan.h's scan of the frames in order around a per-pixel model.
// small work images (fm_small.hip): k_small_blur (one workgroup per frame) + k_small_scan (the running average)
bool small_supported(int h, int w, int ksize);
hipError_t launch_small(hipStream_t st, const FusedArgs& a, uint8_t* blur, uint64_t* ks_blur, uint64_t* ks_scan);
hipError_t launch_small_scan(hipStream_t st, const FusedArgs& a, const uint8_t* blur, uint64_t* ks_scan);
// Gaussian sizes above k_fused's on larger work images (fm_wide.hip): k_wide_blur (a workgroup per column strip
// sliding down an LDS ring of horizontal sums) + k_small_scan; coef: the context's taps
bool wide_supported(int ksize, const int32_t* coef);
int wide_lds_bytes(int ksize, const int32_t* coef);
hipError_t launch_wide(hipStream_t st, const FusedArgs& a, uint8_t* blur, uint64_t* ks_blur, uint64_t* ks_scan);
// the chain on the three colour channels (fm_rgb.hip, FM_FLAG_COLOUR_MOTION): k_rgb_blur (a workgroup per frame and
// 64 x 64 tile) + k_rgb_scan (three running averages; the channels' threshold bits ORed).  The kernels take their
// own argument struct, filled from a: a.bg_in / a.bg_out are [S][h][w][3] doubles here, and the element counts of
// OpenCV's SIMD rules (a.cvt_simd, a.acc_vec_end) are taken over 3hw, not from a.  blur: three channels,
// [F][3][x][nty * 64]
bool rgb_supported(int h, int w, int ksize);
int rgb_lds_bytes(int ksize);
hipError_t launch_rgb(hipStream_t st, const FusedArgs& a, uint8_t* blur, uint64_t* ks_blur, uint64_t* ks_scan);
// the Gaussian-mixture background model (fm_mog2.hip, FM_FLAG_MOG2): the blur of launch_small or launch_wide_blur,
// then k_mog2_scan (the scan around the pixel's five modes in registers) in place of the average's scan.  The
// state is updated in place: float planes [S][15][x][nty * 64] (field = 5 * {weight, mean, var} + mode;
// mog2_state_floats) and uint8 nmodes [S][x][nty * 64] (mog2_nmodes_bytes); alphaT: the learning rate of
// each of the batch's a.T * a.S frames, [T][S]
struct Mog2Dev {
    float* state;
    uint8_t* nmodes;
    const float* alphaT;
    fm_mog2_params prm;
};
size_t mog2_state_floats(int S, int w, int nty);
size_t mog2_nmodes_bytes(int S, int w, int nty);
hipError_t launch_small_blur(hipStream_t st, const FusedArgs& a, uint8_t* sblur, uint64_t* ks_blur);
hipError_t launch_wide_blur(hipStream_t st, const FusedArgs& a, uint8_t* wblur, uint64_t* ks_blur);
hipError_t launch_mog2_scan(hipStream_t st, const FusedArgs& a, const Mog2Dev& m, const uint8_t* blur, uint64_t* ks_scan);
// getBackgroundImage of stream s into out [h][w] (device memory)
hipError_t launch_mog2_background(hipStream_t st, const Mog2Dev& m, int s, int h, int w, int nty, uint8_t* out);
// a.tflag (one word per tile-frame) of all a.T * a.S frames from a.bits: after the 64 x 64 tile pixel kernels
// (launch_pix), ahead of either contour pass below
hipError_t launch_tile_flags(hipStream_t st, const FusedArgs& a);
// CCL over tile summaries; dilate = true: a.bits are threshold rows to dilate into a.dbits
// gate_wait / gate_done (optional): the labelling kernel waits for gate_wait (the previous batch's
// labelling) and gate_done is recorded after it, so that one batch's labelling runs at a time
hipError_t launch_tile_ccl(hipStream_t st, const FusedArgs& a, bool dilate, KernelTimer* timer,
                           hipEvent_t gate_wait = nullptr, hipEvent_t gate_done = nullptr);
// the whole contour pass of each frame in one workgroup (a.ntiles <= kFrameCclTiles; count[] sized 3F + 3, the
// slot-wide words count[2F], count[2F + 1], count[3F + 2] zero before the first batch: the kernel re-arms them)
hipError_t launch_frame_contours(hipStream_t st, const FusedArgs& a, bool dilate);
// every external-contour record of frame f of a finished batch (all of them, unlike the
// capped k_emit), into rec [cap][5]; *cnt must be 0 before
hipError_t launch_emit_all(hipStream_t st, const FusedArgs& a, int f, int32_t* rec, int32_t* cnt, int cap);
// 2 x contourArea of external contours by border following (fm_ccl.hip): jobs [n][3] = (frame, origin x,
// origin y); the dilated mask of frame f is dbits/candf (fused path, [F][ntiles]...) or mask [F][h*w] bytes
hipError_t launch_contour_area(hipStream_t st, const uint64_t* dbits, const uint8_t* candf, const uint8_t* mask, int ntiles,
                               int ntx, int h, int w, const int32_t* jobs, int n, int32_t* area2);
// CHAIN_APPROX_SIMPLE points of external contours by border following (fm_trace.hip).  jobs [n][8] =
// (frame, origin x, origin y, box x, box y, box w, box h, point offset); list: the contour indices of
// the register path, the LDS path, the big-window LDS path, then the unstaged path (n_path of each; the
// host sorts a box with trace_box_path); res [n][3] = (npts or -1, area2, steps), written by
// the count pass (emit = false) and read by the emit pass, which writes contour i's points at
// pts + 2 * offset_i and sets bits of *err when a walk disagrees with the count pass.
constexpr int kTracePaths = 4;
struct TraceArgs {
    const uint64_t* dbits;
    const uint8_t* candf;
    const uint8_t* mask;
    int ntiles, ntx, h, w;
    const int32_t* jobs;
    const int32_t* list;
    int n_path[kTracePaths];
    int32_t* res;
    int32_t* pts;
    int32_t* err;
};
int trace_box_path(int bw, int bh);  // 0 registers, 1 LDS, 2 big LDS window, 3 unstaged
struct KernelTimer;
// (timer: each path's launch timed under trace_count_<path> / trace_emit_<path>, FM_FLAG_PROFILE)
hipError_t launch_trace(hipStream_t st, const TraceArgs& t, bool emit, KernelTimer* timer);
// dilated bit rows of one frame -> mask bytes (VideoFrame.thresh) [h][w]; non-candidate tiles are 0
hipError_t launch_expand_bits(hipStream_t st, const uint64_t* dbits, const uint8_t* candf, uint8_t* out, int h, int w,
                              int ntx);

// Optional per-kernel timing.  FM_FLAG_PROFILE: events recorded on the launch stream around each
// kernel, read back after the stream syncs.  FM_FLAG_PROFILE_PIX: the pixel kernel and the INTER_AREA
// resize only, EVERY launch timed by in-kernel stamps (stamp(): no event packet enters the streams);
// other kernels on the pixel / input stream by events on one launch in kSample.
struct KernelTimer {
    bool enabled = false;
    bool pixel_only = false;
    static constexpr int kSample = 4;
    static constexpr int kStampRing = 4096;  // stamped launches held between two folds (more go untimed)
    std::vector<int64_t> calls;
    hipStream_t stream = nullptr;
    hipStream_t stream2 = nullptr;  // also timed in the pixel-only mode: the input stream's resize
    hipStream_t stream3 = nullptr;  // (the second input stream)
    std::vector<hipStream_t> extra; // other streams stamped kernels run on (the contour streams; dev-build stamps)
    struct Rec { int id; hipEvent_t a, b; hipStream_t st; };
    std::vector<Rec> pending;
    std::vector<hipEvent_t> pool;
    std::vector<const char*> names;
    std::vector<double> ms;
    std::vector<int64_t> launches;
    std::vector<double> ms_sq;      // sum of squared stamped launch times (ms^2)
    std::vector<int64_t> stamped;   // launches timed by stamps (ms_sq's count; `launches` adds event-timed ones)
    std::vector<double> stamped_ms; // their summed time (ms)
    struct Busy { double ms = 0; uint64_t s = 0, e = 0; bool open = false; };
    std::vector<Busy> busy;         // union of the stamped launch windows (closed part + the open interval)
    uint64_t* d_stamps = nullptr;   // device [kStampRing][2]: (first start, last end), ticks of 10 ns
    std::vector<int> stamp_ids;     // name id of ring entries [0, stamp_ids.size()) not yet folded
    int64_t unstamped = 0;          // launches that found the ring full
    int id_of(const char* name);
    int begin(const char* name, hipStream_t st = nullptr);  // token for end(), -1 when disabled
    void end(int token);
    void collect();                // folds in every pair whose end event has completed
    uint64_t* stamp(const char* name);  // this launch's stamp pair, nullptr when not stamping
    int fold_stamps();             // waits for the stamped streams, folds and re-arms the entries
    // One launch on st: stamped if stamping (launch gets the stamp pair), else bracketed by events.
    // name2: a launch of two stamped kernels (launch's second pair); unless both are stamped, events
    // bracket the two under ev_name.  stamps = false: a kernel that does not stamp (events only).
    template <class Launch>
    hipError_t timed(hipStream_t st, const char* name, Launch&& launch, bool stamps = true, const char* name2 = nullptr,
                     const char* ev_name = nullptr) {
        uint64_t* k1 = stamps ? stamp(name) : nullptr;
        uint64_t* k2 = stamps && name2 ? stamp(name2) : nullptr;
        const int tok = (k1 && (k2 || !name2)) ? -1 : begin(ev_name ? ev_name : name, st);
        const hipError_t e = launch(k1, k2);
        if (e == hipSuccess) end(tok);
        return e;
    }
    void reset();
    ~KernelTimer();
};

}  // namespace fm

// decode side (fm_jpeg.hip): queue the decode of n JPEGs into BGR frames at device address out on
// stream st; FM_* status, the message in fm_mjpeg_last_error
int fm_mjpeg_enqueue(fm_mjpeg* d, const uint8_t* const* jpegs, const size_t* sizes, int n, uint8_t* out, hipStream_t st);
