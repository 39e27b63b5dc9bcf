// fm_trace.hip — the CHAIN_APPROX_SIMPLE points of every external contour (FM_FLAG_CONTOUR_POINTS):
// the rest of what cv2.findContours(thresh, RETR_EXTERNAL, CHAIN_APPROX_SIMPLE) returns
// (fm.py:269-272), traced on the GPU (gfx950) from each record's start pixel on the batch's
// dilated mask.
//
// Measure, scan, write: a COUNT pass walks every outer border and returns the number of SIMPLE
// points, the shoelace sum and the steps walked; the host scans the counts (it builds the job list
// anyway) and sizes the point buffer; an EMIT pass walks again and writes point k of contour i at
// off[i] + k.  Both passes and all paths run ONE walker (walk_begin / walk_run: the
// neighbour rule of OpenCV's icvFetchContour, restated in oracle/fm_oracle.c fetch_contour) over a
// "pixel source" that returns the 8-neighbourhood of a pixel as one byte, bit d = the neighbour in
// direction code d: the rule's clockwise search is then a rotate and a count of trailing zeros,
// and a step costs one round of independent loads instead of up to eight dependent probes.
//
// The walk never leaves the contour's bounding box plus the 1-px pad, and the box is known from
// the record, so by the size of the padded box a contour takes one of these paths:
//   register  (box <= 6 x 6)         the padded 8 x 8 window is one uint64_t; one LANE per contour
//                                    (64 contours per wave: the dots of a dense lattice), the walk
//                                    touches no memory at all;
//   LDS       (window <= kWinWords)  one WAVE per contour copies the window's bit rows into its
//                                    8 KiB of LDS (all lanes, 32 pixels each), lane 0 walks on
//                                    LDS alone and buffers the points in LDS; the wave flushes
//                                    them 64 at a time (512 contiguous bytes);
//   big LDS   (window <= kBigWords)  the same kernel with one wave per workgroup and a 63.5 KiB
//                                    window (the moving objects of a 1080p frame: up to ~700 x 700);
//   unstaged  (anything larger)      one thread per contour behind a sliding window: the 64 x 18
//                                    block of the mask around the walker in the thread's slice of
//                                    LDS (32 x 16 of it the block proper, the rest overlap), refilled
//                                    by one round of independent loads when the walk leaves the
//                                    block.  Correct for a full 1920 x 1080 frame; one global
//                                    latency per up to 32 steps instead of several per step.
// Pixels of other components inside a window are harmless: the path depends only on which pixels
// are set.  A source answers 0 outside its window, and a walk that meets an empty neighbourhood,
// exceeds the step cap or (emit pass) yields another count than the count pass reports an error:
// no walk loops forever and no store leaves [off[i], off[i] + npts[i]).
#include "fm_internal.h"

namespace fm {
namespace tr {

constexpr int kTinyBox = 6;        // register path: box sides up to this (8 x 8 with the pad)
constexpr int kWaves = 4;          // LDS path: waves (= contours) per workgroup
constexpr int kWinWords = 2048;    // 32-bit words of one wave's window: 65536 pixels, e.g. 254 x 254
constexpr int kBigWords = 16256;   // the big window: with its point buffer exactly 64 KiB, e.g. 700 x 700
constexpr int kPtBuf = 64;         // points a wave buffers between two flushes
constexpr int kSlideRows = 16;     // unstaged path: rows of a block (cached with one row above and below)
constexpr int kJob = 8;            // ints per job: frame, origin x y, box x y w h, point offset
constexpr int kRes = 3;            // ints per result: npts (-1: no closed border), area2, steps

// the batch's dilated masks: 64 x 64 bit tiles (dbits, candf: [F][ntiles]) or bytes (mask: [F][h*w])
struct Mask {
    const uint64_t* dbits;
    const uint8_t* candf;
    const uint8_t* mask;
    int ntiles, ntx, h, w;
    __device__ __forceinline__ uint64_t tile_row(int f, int tx, int y) const {
        if (tx >= ntx) return 0ull;
        const size_t t = (size_t)f * ntiles + (size_t)(y >> 6) * ntx + tx;
        return candf[t] ? dbits[t * 64 + (y & 63)] : 0ull;
    }
    // pixels x0 .. x0 + 63 of row y (x0 = 16 mod 32, -16 <= x0 < w); 0 outside the image.  On the bit
    // tiles every load is unconditional (clamped addresses inside the batch's arrays, the values of
    // non-candidate tiles dropped afterwards), so the loads of many rows can be in flight together.
    __device__ __forceinline__ uint64_t window64(int f, int y, int x0) const {
        const bool yin = (unsigned)y < (unsigned)h;
        const int yc = yin ? y : 0;
        if (mask) {
            uint64_t v = 0;
            const uint8_t* r = mask + ((size_t)f * h + yc) * w;
            for (int i = 0; i < 64; i++)
                if (yin && (unsigned)(x0 + i) < (unsigned)w && r[x0 + i]) v |= 1ull << i;
            return v;
        }
        const int a = (x0 + 64) / 64 - 1;  // first tile column touched (-1: left of the image)
        const int sh = x0 - 64 * a;        // 16 or 48
        const int a0 = a < 0 ? 0 : a, a1 = a + 1 < ntx ? a + 1 : ntx - 1;
        const size_t row = (size_t)f * ntiles + (size_t)(yc >> 6) * ntx;
        const uint64_t w0 = dbits[(row + a0) * 64 + (yc & 63)], w1 = dbits[(row + a1) * 64 + (yc & 63)];
        const uint8_t c0 = candf[row + a0], c1 = candf[row + a1];
        uint64_t lo = (yin && a >= 0 && c0) ? w0 : 0ull, hi = (yin && a + 1 < ntx && c1) ? w1 : 0ull;
        const int wl = w - 64 * (ntx - 1);  // pixels of the last tile column inside the image
        const uint64_t lm = wl < 64 ? (1ull << wl) - 1ull : ~0ull;
        if (a == ntx - 1) lo &= lm;
        if (a + 1 == ntx - 1) hi &= lm;
        return (lo >> sh) | (hi << (64 - sh));
    }
    // pixels x .. x + n - 1 of row y as bits 0 .. n - 1 (n <= 32, x > -32; higher bits: further pixels
    // or 0); 0 outside the image
    __device__ __forceinline__ uint32_t row_bits(int f, int y, int x, int n = 32) const {
        if ((unsigned)y >= (unsigned)h || x >= w) return 0u;
        const int lead = x < 0 ? -x : 0;  // pixels left of the image
        x += lead;
        uint32_t v = 0;
        if (mask) {
            const uint8_t* r = mask + ((size_t)f * h + y) * w + x;
            const int m = w - x < n - lead ? w - x : n - lead;
            for (int i = 0; i < m; i++) v |= (r[i] ? 1u : 0u) << i;
        } else {
            const int tx = x >> 6, sh = x & 63;
            uint64_t lo = tile_row(f, tx, y) >> sh;
            if (sh > 32) lo |= tile_row(f, tx + 1, y) << (64 - sh);
            v = (uint32_t)lo;
            if (w - x < 32) v &= (1u << (w - x)) - 1u;
        }
        return v << lead;
    }
};

// three rows' (left, centre, right) bits -> the neighbourhood byte in direction-code order
// (code_dx / code_dy of the oracle: 0 = right, then counter-clockwise on the screen: up-right, up, ...)
__device__ __forceinline__ uint32_t nb_pack(uint32_t t, uint32_t m, uint32_t b) {
    return ((m >> 2) & 1u) | (((t >> 2) & 1u) << 1) | (((t >> 1) & 1u) << 2) | ((t & 1u) << 3) | ((m & 1u) << 4) |
           ((b & 1u) << 5) | (((b >> 1) & 1u) << 6) | (((b >> 2) & 1u) << 7);
}
__device__ __forceinline__ int dir_dx(int s) { return (int)((0x901Au >> (2 * s)) & 3u) - 1; }
__device__ __forceinline__ int dir_dy(int s) { return (int)((0xA901u >> (2 * s)) & 3u) - 1; }

// ---- pixel sources: nbhd(x, y) in image coordinates ----------------------------------------
struct SlideSrc {  // rows cy0 .. cy0 + kSlideRows + 1 of pixels 32 ckx - 16 .. 32 ckx + 47 at c[r * cs] (ckx < 0: none yet)
    Mask m;
    int f;
    uint64_t* c;
    int cs, ckx, cy0;
    __device__ __forceinline__ uint32_t nbhd(int x, int y) {
        if (x < 0 || y < 0) return 0u;
        const int kx = x >> 5, x0 = 32 * kx - 16;  // x - 1 .. x + 1 lie in pixels 15 .. 48 of the window
        const int y0 = (y & ~(kSlideRows - 1)) - 1;
        if (kx != ckx || y0 != cy0) {
            uint64_t v[kSlideRows + 2];
#pragma unroll
            for (int r = 0; r < kSlideRows + 2; r++) v[r] = m.window64(f, y0 + r, x0);
#pragma unroll
            for (int r = 0; r < kSlideRows + 2; r++) c[r * cs] = v[r];
            ckx = kx;
            cy0 = y0;
        }
        const uint64_t* p = c + (y - y0 - 1) * cs;
        const int b = x - x0 - 1;
        return nb_pack((uint32_t)(p[0] >> b) & 7u, (uint32_t)(p[cs] >> b) & 7u, (uint32_t)(p[2 * cs] >> b) & 7u);
    }
};
struct RegSrc {  // the padded window (ox, oy) .. (ox + 7, oy + 7), row r in bits 8r .. 8r + 7
    uint64_t win;
    int ox, oy;
    __device__ __forceinline__ void load(const Mask& m, int f) {
        win = 0;
        for (int r = 0; r < 8; r++) win |= (uint64_t)(m.row_bits(f, oy + r, ox, 8) & 0xFFu) << (8 * r);
    }
    __device__ __forceinline__ uint32_t nbhd(int x, int y) const {
        const int px = x - ox, py = y - oy;
        if (px < 1 || px > 6 || py < 1 || py > 6) return 0u;
        const uint64_t v = win >> (8 * (py - 1) + px - 1);
        return nb_pack((uint32_t)v & 7u, (uint32_t)(v >> 8) & 7u, (uint32_t)(v >> 16) & 7u);
    }
};
struct LdsSrc {  // the padded window (ox, oy) .. of bw + 2 x bh + 2 pixels, rows of `stride` words
    const uint32_t* w;
    int stride, ox, oy, bw, bh;
    __device__ __forceinline__ uint32_t row3(int r, int wd, int sh) const {
        const uint32_t* p = w + r * stride + wd;  // (wd + 1 <= stride - 1: the row's spare word)
        return (uint32_t)((((uint64_t)p[1] << 32) | p[0]) >> sh) & 7u;
    }
    __device__ __forceinline__ uint32_t nbhd(int x, int y) const {
        const int px = x - ox, py = y - oy;
        if (px < 1 || px > bw || py < 1 || py > bh) return 0u;
        const int wd = (px - 1) >> 5, sh = (px - 1) & 31;
        return nb_pack(row3(py - 1, wd, sh), row3(py, wd, sh), row3(py + 1, wd, sh));
    }
};

// ---- point sinks -----------------------------------------------------------------------------
struct CountSink {  // the SIMPLE points counted, their shoelace summed (cv2.contourArea, fm.py:679)
    long long a = 0;
    int np = 0, fx = 0, fy = 0, lx = 0, ly = 0;
    __device__ __forceinline__ bool full() const { return false; }
    __device__ __forceinline__ void point(int x, int y) {
        if (np == 0) {
            fx = x;
            fy = y;
        } else {
            a += (long long)lx * y - (long long)ly * x;
        }
        lx = x;
        ly = y;
        np++;
    }
    __device__ __forceinline__ int32_t area2() const {
        const long long c = np > 0 ? a + (long long)lx * fy - (long long)ly * fx : 0;
        return (int32_t)(c < 0 ? -c : c);
    }
};
struct StoreSink {  // straight to the contour's slice of the point buffer, never past its count
    int32_t* out;
    int limit, np = 0;
    __device__ __forceinline__ bool full() const { return false; }
    __device__ __forceinline__ void point(int x, int y) {
        if (np < limit) {
            out[2 * np] = x;
            out[2 * np + 1] = y;
        }
        np++;
    }
};
struct BufSink {  // kPtBuf points in LDS, flushed by the whole wave
    int32_t* buf;
    int n = 0;
    __device__ __forceinline__ bool full() const { return n >= kPtBuf; }
    __device__ __forceinline__ void point(int x, int y) {
        buf[2 * n] = x;
        buf[2 * n + 1] = y;
        n++;
    }
};

// ---- the walker ------------------------------------------------------------------------------
enum { WALK_RUN = 0, WALK_DONE = 1, WALK_ERR = -1 };
struct Walk {
    int x0, y0, x1, y1, x3, y3, s, prev_s, status;
    long long it, cap;
};

// icvFetchContour's start: the first non-zero neighbour clockwise from the left (outer border)
template <class Src, class Sink>
__device__ __forceinline__ void walk_begin(Walk& k, Src& src, Sink& sink, int x0, int y0, long long cap) {
    k.x0 = k.x3 = x0;
    k.y0 = k.y3 = y0;
    k.it = 0;
    k.cap = cap;
    const uint32_t n = src.nbhd(x0, y0);
    int s = -1;
    for (int i = 1; i < 8; i++) {
        const int d = (4 - i) & 7;
        if ((n >> d) & 1u) {
            s = d;
            break;
        }
    }
    if (s < 0) {  // an isolated pixel: one point
        sink.point(x0, y0);
        k.x1 = x0;
        k.y1 = y0;
        k.s = k.prev_s = 0;
        k.status = WALK_DONE;
        return;
    }
    k.x1 = x0 + dir_dx(s);
    k.y1 = y0 + dir_dy(s);
    k.s = s;
    k.prev_s = s ^ 4;
    k.status = WALK_RUN;
}

// border steps until the border closes, the sink is full, or the walk proves not to be one
template <class Src, class Sink>
__device__ __forceinline__ void walk_run(Walk& k, Src& src, Sink& sink) {
    while (k.status == WALK_RUN && !sink.full()) {
        const uint32_t n = src.nbhd(k.x3, k.y3);
        if (n == 0u || k.it++ > k.cap) {  // not a border start of this mask: report, never loop forever
            k.status = WALK_ERR;
            break;
        }
        // the first set neighbour among codes s + 1 .. 15 (mod 8)
        const uint32_t t = (n | (n << 8)) >> (k.s + 1);
        const int s = (k.s + 1 + __builtin_ctz(t)) & 7;
        const int x4 = k.x3 + dir_dx(s), y4 = k.y3 + dir_dy(s);
        if (s != k.prev_s) {  // CHAIN_APPROX_SIMPLE keeps the point where the direction changes
            sink.point(k.x3, k.y3);
            k.prev_s = s;
        }
        if (x4 == k.x0 && y4 == k.y0 && k.x3 == k.x1 && k.y3 == k.y1) {
            k.status = WALK_DONE;
            break;
        }
        k.x3 = x4;
        k.y3 = y4;
        k.s = (s + 4) & 7;
    }
}

struct Args {
    Mask m;
    const int32_t* jobs;  // [n][kJob]
    const int32_t* list;  // this path's contour indices
    int n;                // their number
    int32_t* res;         // [ncontours][kRes]
    int32_t* pts;         // emit pass: [total][2]
    int32_t* err;         // emit pass: error bits (1: a walk disagreed with the count pass, 2: window too large)
};

__device__ __forceinline__ long long step_cap(int w, int h) { return 4ll * (w + 2) * (h + 2) + 16; }

template <class Src>
__device__ __forceinline__ void count_one(const Args& a, Src& src, int i, const int32_t* j, long long cap) {
    CountSink sink;
    Walk k;
    walk_begin(k, src, sink, j[1], j[2], cap);
    walk_run(k, src, sink);
    int32_t* r = a.res + (size_t)i * kRes;
    r[0] = k.status == WALK_DONE ? sink.np : -1;
    r[1] = sink.area2();
    r[2] = (int32_t)(k.it > 0x7fffffffll ? 0x7fffffffll : k.it);
}
template <class Src>
__device__ __forceinline__ void store_one(const Args& a, Src& src, int i, const int32_t* j, long long cap) {
    const int npts = a.res[(size_t)i * kRes];
    StoreSink sink{a.pts + 2 * (size_t)(uint32_t)j[7], npts};
    Walk k;
    walk_begin(k, src, sink, j[1], j[2], cap);
    walk_run(k, src, sink);
    if (k.status != WALK_DONE || sink.np != npts) atomicOr(a.err, 1);
}

// register path: one lane per contour
template <bool EMIT>
__global__ __launch_bounds__(256) void k_trace_reg(Args a) {
    const int q = blockIdx.x * 256 + threadIdx.x;
    if (q >= a.n) return;
    const int i = a.list[q];
    const int32_t* j = a.jobs + (size_t)i * kJob;
    RegSrc src{0ull, j[3] - 1, j[4] - 1};
    src.load(a.m, j[0]);
    if (EMIT) store_one(a, src, i, j, step_cap(a.m.w, a.m.h));
    else count_one(a, src, i, j, step_cap(a.m.w, a.m.h));
}

// unstaged path: one thread per contour behind its sliding window
template <bool EMIT>
__global__ __launch_bounds__(64) void k_trace_global(Args a) {
    __shared__ uint64_t s_rows[kSlideRows + 2][64];  // [row][thread]: a thread's rows lie 512 B apart
    const int q = blockIdx.x * 64 + threadIdx.x;
    if (q >= a.n) return;
    const int i = a.list[q];
    const int32_t* j = a.jobs + (size_t)i * kJob;
    SlideSrc src{a.m, j[0], &s_rows[0][threadIdx.x], 64, -1, 0};
    if (EMIT) store_one(a, src, i, j, step_cap(a.m.w, a.m.h));
    else count_one(a, src, i, j, step_cap(a.m.w, a.m.h));
}

// a wave's LDS accesses complete in order; the compiler must keep them in program order too
__device__ __forceinline__ void wave_lds_order() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// LDS path: one wave per contour
template <bool EMIT, int WAVES, int WORDS>
__global__ __launch_bounds__(64 * WAVES) void k_trace_lds(Args a) {
    __shared__ uint32_t s_win[WAVES][WORDS];
    __shared__ int32_t s_pts[WAVES][2 * kPtBuf];
    const int wv = threadIdx.x >> 6, ln = threadIdx.x & 63;
    const int q = blockIdx.x * WAVES + wv;
    if (q >= a.n) return;  // (wave-uniform; no workgroup barrier below)
    const int i = a.list[q];
    const int32_t* j = a.jobs + (size_t)i * kJob;
    const int f = j[0], bw = j[5], bh = j[6];
    const int ox = j[3] - 1, oy = j[4] - 1;
    const int stride = ((bw + 2 + 31) >> 5) + 1, rows = bh + 2;
    if (stride * rows > WORDS) {  // (the host sorts such a box into another list)
        if (ln == 0) {
            if (EMIT) atomicOr(a.err, 2);
            else a.res[(size_t)i * kRes] = -1;
        }
        return;
    }
    uint32_t* win = s_win[wv];
    for (int e = ln; e < stride * rows; e += 64) {
        const int r = e / stride, wd = e - r * stride;
        win[e] = a.m.row_bits(f, oy + r, ox + 32 * wd);
    }
    wave_lds_order();
    LdsSrc src{win, stride, ox, oy, bw, bh};
    const long long cap = step_cap(a.m.w, a.m.h);
    if (!EMIT) {
        if (ln == 0) count_one(a, src, i, j, cap);
        return;
    }
    const int npts = a.res[(size_t)i * kRes];
    int32_t* out = a.pts + 2 * (size_t)(uint32_t)j[7];
    BufSink sink{s_pts[wv]};
    Walk k;
    k.status = WALK_RUN;
    if (ln == 0) walk_begin(k, src, sink, j[1], j[2], cap);
    int done = 0;  // points flushed
    for (;;) {
        if (ln == 0) walk_run(k, src, sink);
        wave_lds_order();
        const int nb = __shfl(sink.n, 0), status = __shfl(k.status, 0);
        // 2 * nb ints of contiguous points: lane l stores ints l and l + 64
        for (int e = ln; e < 2 * nb; e += 64)
            if (done + (e >> 1) < npts) out[2 * (size_t)done + e] = sink.buf[e];
        wave_lds_order();
        done += nb;
        sink.n = 0;
        if (status != WALK_RUN) {
            if (ln == 0 && (status != WALK_DONE || done != npts)) atomicOr(a.err, 1);
            break;
        }
        if (done > npts) {  // more points than counted: stop walking, report
            if (ln == 0) atomicOr(a.err, 1);
            break;
        }
    }
}

}  // namespace tr

int trace_box_path(int bw, int bh) {
    if (bw <= tr::kTinyBox && bh <= tr::kTinyBox) return 0;
    const long long words = ((long long)(((bw + 2 + 31) >> 5) + 1)) * (bh + 2);
    return words <= tr::kWinWords ? 1 : words <= tr::kBigWords ? 2 : 3;
}

template <bool EMIT>
static void launch_path(hipStream_t st, const tr::Args& a, int path) {
    const int n = a.n;
    if (path == 0) hipLaunchKernelGGL((tr::k_trace_reg<EMIT>), dim3((n + 255) / 256), dim3(256), 0, st, a);
    else if (path == 1)
        hipLaunchKernelGGL((tr::k_trace_lds<EMIT, tr::kWaves, tr::kWinWords>), dim3((n + tr::kWaves - 1) / tr::kWaves),
                           dim3(64 * tr::kWaves), 0, st, a);
    else if (path == 2) hipLaunchKernelGGL((tr::k_trace_lds<EMIT, 1, tr::kBigWords>), dim3(n), dim3(64), 0, st, a);
    else hipLaunchKernelGGL((tr::k_trace_global<EMIT>), dim3((n + 63) / 64), dim3(64), 0, st, a);
}

hipError_t launch_trace(hipStream_t st, const TraceArgs& t, bool emit, KernelTimer* timer) {
    static const char* const names[2][kTracePaths] = {
        {"trace_count_reg", "trace_count_lds", "trace_count_lds_big", "trace_count_unstaged"},
        {"trace_emit_reg", "trace_emit_lds", "trace_emit_lds_big", "trace_emit_unstaged"}};
    const tr::Mask m{t.dbits, t.candf, t.mask, t.ntiles, t.ntx, t.h, t.w};
    const int32_t* list = t.list;
    for (int path = 0; path < kTracePaths; path++) {
        const int n = t.n_path[path];
        if (n > 0) {
            const tr::Args a{m, t.jobs, list, n, t.res, t.pts, t.err};
            const int tok = timer ? timer->begin(names[emit ? 1 : 0][path], st) : -1;
            if (emit) launch_path<true>(st, a, path);
            else launch_path<false>(st, a, path);
            if (timer) timer->end(tok);
            const hipError_t e = hipGetLastError();
            if (e != hipSuccess) return e;
        }
        list += n;
    }
    return hipSuccess;
}

}  // namespace fm
