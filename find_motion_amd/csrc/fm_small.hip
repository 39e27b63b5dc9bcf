// fm_small.hip — the per-pixel motion chain for small work images (round 5): mode D, the reference
// CLI's default -B 100 (find_motion.py:1474, resize fm.py:492: 1080p -> 100 x 56, two 64 x 64 tiles per
// stream).  Reference chain per frame (fm.py): cvtColor 493, GaussianBlur 494, mask_off_areas 619-636,
// absdiff(convertScaleAbs) 250, threshold 257, accumulateWeighted 659.
//
// On a two-tile image k_pix5 (16 waves per tile, two workgroups) runs a batch's 256 frames one after
// another: 224 us per 256 frames alone, 355 us beside the next batch's resize (round 4), a latency chain
// with one LDS barrier per frame on 2 CUs.  But only the f64 running average is sequential in time
// (SURVEY.md §5); gray and blur of a frame depend on that frame alone.  So:
//
//   k_small_blur  one workgroup per frame (all T x S frames of the batch at once, over every CU):
//                 gray (fm.py:493), the k x k fixed-point Gaussian (fm.py:494, REFLECT_101), the keep-mask
//                 (masked pixels blur to 0, fm.py:619-636) -> blur bytes [F][x][y] (column-major, column
//                 stride CS = nty * 64), and it clears the frame's tile flags and the bit words of the
//                 columns past the image;
//   k_small_scan  fm_scan.h's scan_frames (one wave per stream, image column and 64-row tile row, lane = row,
//                 the frames in order) around the f64 background in a register: diff (convertScaleAbs +
//                 absdiff), threshold, accumulateWeighted; `d > t` is the lane's threshold bit.
//
// Same arithmetic as k_pix5 / the oracle: gray (1868 B + 9617 G + 4899 R + 8192) >> 14, blur
// (sum_y c_y sum_x c_x g + 2^15) >> 16 with OpenCV's 8-bit taps, q = sat_u8(rne(|(float)bg|)),
// d = |blur - q| > t, bg = fma(bg, 1 - a, blur * a) (scalar tail past acc_vec_end: blur * a + bg * (1 - a)),
// the stream's first frame bg := blur before the diff.
#include "fm_scan.h"

namespace fm {
namespace sm {

constexpr int BT = 256;  // k_small_blur threads

// H's row stride in dwords: odd, so that the vertical pass's 64 lanes (consecutive rows of one column)
// read 64 distinct banks (at w = 100 the unpadded stride put them on 16 banks: 4-way conflicts)
__host__ __device__ constexpr int h_stride(int w) { return w | 1; }

// LDS of k_small_blur: gray u8 [h][w], H u32 [h][h_stride(w)], reflected column / row indices
__host__ __device__ constexpr size_t blur_lds_bytes(int h, int w, int R) {
    return ((size_t)h * w + 3) / 4 * 4 + (size_t)h * h_stride(w) * 4 + (size_t)(w + 2 * R) * 4 +
           (size_t)(h + 2 * R) * 4;
}

__global__ __launch_bounds__(BT) void k_small_blur(FusedArgs a, uint8_t* __restrict__ sblur, int CS) {
    extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
    const int h = a.h, w = a.w, S = a.S, K = a.ksize, R = K >> 1;
    const int n = h * w, HS = h_stride(w);
    const size_t f = (size_t)a.t_begin * S + blockIdx.x;  // frame of this workgroup (t_begin * S + t * S + s)
    const int s = (int)(f % S);
    uint8_t* g = lds;
    uint32_t* H = reinterpret_cast<uint32_t*>(lds + (n + 3) / 4 * 4);
    int* xi = reinterpret_cast<int*>(H + (size_t)h * HS);  // [w + 2R]: reflected source column of x - R
    int* yi = xi + w + 2 * R;                 // [h + 2R]
    const int tid = threadIdx.x;
    kstamp_begin_grid(a.kstamp);
    for (int i = tid; i < w + 2 * R; i += BT) xi[i] = refl(i - R, w);
    for (int i = tid; i < h + 2 * R; i += BT) yi[i] = refl(i - R, h);
    clear_tile_frame(geom_of(a), f, tid, BT);  // the scan's precondition
    // gray: pixel quads as three dwords where the frame allows (4-B aligned), single pixels otherwise
    const uint8_t* src = a.src + f * (size_t)n * 3;
    const int nq = ((reinterpret_cast<uintptr_t>(src) & 3) == 0) ? n / 4 : 0;
    for (int q = tid; q < nq; q += BT) {
        const uint32_t* p = reinterpret_cast<const uint32_t*>(src) + 3 * q;
        const uint32_t d0 = p[0], d1 = p[1], d2 = p[2];
        const uint32_t v = gray_px(d0 & 0xFF, (d0 >> 8) & 0xFF, (d0 >> 16) & 0xFF) |
                           gray_px(d0 >> 24, d1 & 0xFF, (d1 >> 8) & 0xFF) << 8 |
                           gray_px((d1 >> 16) & 0xFF, d1 >> 24, d2 & 0xFF) << 16 |
                           gray_px((d2 >> 8) & 0xFF, (d2 >> 16) & 0xFF, d2 >> 24) << 24;
        reinterpret_cast<uint32_t*>(g)[q] = v;
    }
    for (int i = 4 * nq + tid; i < n; i += BT) g[i] = (uint8_t)gray_px(src[3 * i], src[3 * i + 1], src[3 * i + 2]);
    __syncthreads();
    // horizontal taps: H = sum_t c[t] * gray(y, x + t - R) (<= 255 * 256)
    for (int i = tid; i < n; i += BT) {
        const int y = i / w, x = i - y * w;
        const uint8_t* row = g + y * w;
        uint32_t acc = 0;
        for (int t = 0; t < K; t++) acc += (uint32_t)a.coef[t] * row[xi[x + t]];
        H[y * HS + x] = acc;
    }
    __syncthreads();
    // vertical taps, rounding, keep-mask; written column-major: thread i -> (x, y) with y fastest
    const bool hk = a.has_keep[s] != 0;
    const uint8_t* keep = a.keep + (size_t)s * n;
    uint8_t* out = sblur + f * (size_t)w * CS;
    for (int i = tid; i < n; i += BT) {
        const int x = i / h, y = i - x * h;
        uint32_t acc = 32768u;
        for (int t = 0; t < K; t++) acc += (uint32_t)a.coef[t] * H[yi[y + t] * HS + x];
        uint32_t blur = acc >> 16;
        if (hk && keep[y * w + x] == 0) blur = 0;
        out[x * CS + y] = (uint8_t)blur;
    }
    kstamp_end_wg(a.kstamp);
}

// the running average of one pixel: scan_frames' model of k_small_scan (after k_small_blur or k_wide_blur)
template <bool TAILK>
struct Average {
    struct Group { uint32_t b[PFD]; };
    const FusedArgs& a;
    const uint8_t* sblur;  // blur bytes [F][x][CS]
    int CS;
    double alpha, beta, bg;
    int thr, t0;
    bool tail, init0;
    size_t px, fstride;
    const uint8_t* base;
    __device__ __forceinline__ void open(const Lane& l) {
        alpha = a.alpha, beta = a.beta, thr = a.thresh, t0 = l.t0;
        const long long li = (long long)l.y * a.w + l.x;
        tail = TAILK && li >= a.acc_vec_end;  // accumulateWeighted's scalar tail
        init0 = a.init != nullptr && a.init[l.s] != 0;
        px = (size_t)l.s * a.h * a.w + li;
        bg = (l.valid && !init0) ? a.bg_in[px] : 0.0;
        // blur bytes of frame t of this pixel: sblur[((t * S + s) * w + x) * CS + y]
        fstride = (size_t)a.S * a.w * CS;
        base = sblur + (size_t)l.s * a.w * CS + (size_t)l.x * CS + l.y;
    }
    __device__ __forceinline__ void load(Group& r, int k, int tc) const { r.b[k] = base[(size_t)tc * fstride]; }
    __device__ __forceinline__ void step(const Group& r, int k, int t, bool& fg) {
        const uint32_t blur = r.b[k];
        const double bv = (init0 && t == t0) ? (double)blur : bg;
        const int q = min(max(__float2int_rn(fabsf(__double2float_rn(bv))), 0), 255);
        fg = abs((int)blur - q) > thr;
        // blur * alpha on the VALU (the pixel kernels' LDS table holds the same correctly rounded
        // product): a 256-entry f64 table read by 64 unrelated bytes averaged 1.95 bank-conflict
        // cycles per LDS cycle here, and the product is off the background's dependency chain
        const double bl = __dmul_rn((double)blur, alpha);
        bg = tail ? __dadd_rn(bl, __dmul_rn(bv, beta)) : __fma_rn(bv, beta, bl);
    }
    __device__ __forceinline__ void close(const Lane& l) const {
        if (l.valid) a.bg_out[px] = bg;
    }
};

template <bool TAILK>
__global__ __launch_bounds__(ST) void k_small_scan(FusedArgs a, const uint8_t* __restrict__ sblur, int CS) {
    scan_frames(geom_of(a), Average<TAILK>{a, sblur, CS});
}

}  // namespace sm

bool small_supported(int h, int w, int ksize) {
    return (long long)h * w <= 16384 && ksize <= kMaxK && sm::blur_lds_bytes(h, w, ksize >> 1) <= 64 * 1024;
}

// frames [a.t_begin, a.t_end) of the batch: blur of every frame in parallel, then the scan; a.init may mark
// first frames (bg := blur at t_begin).  ks1 / ks2: launch stamps of the two kernels (or nullptr)
hipError_t launch_small(hipStream_t st, const FusedArgs& a, uint8_t* sblur, uint64_t* ks1, uint64_t* ks2) {
    if (hipError_t e = launch_small_blur(st, a, sblur, ks1); e != hipSuccess) return e;
    return launch_small_scan(st, a, sblur, ks2);
}

// the blur alone (the Gaussian-mixture scan of fm_mog2.hip follows it too)
hipError_t launch_small_blur(hipStream_t st, const FusedArgs& a, uint8_t* sblur, uint64_t* ks) {
    const int CS = a.nty * 64;
    const int nf = (a.t_end - a.t_begin) * a.S;
    const size_t lds = sm::blur_lds_bytes(a.h, a.w, a.ksize >> 1);
    FusedArgs b = a;
    b.kstamp = ks;
    hipLaunchKernelGGL(sm::k_small_blur, dim3(nf), dim3(sm::BT), lds, st, b, sblur, CS);
    return hipGetLastError();
}

// the scan alone, over blur bytes [F][x][a.nty * 64] of frames [a.t_begin, a.t_end) that are already written and
// whose tile flags and padding bit words are cleared (k_small_blur, or fm_wide.hip's k_wide_blur)
hipError_t launch_small_scan(hipStream_t st, const FusedArgs& a, const uint8_t* sblur, uint64_t* ks) {
    const int CS = a.nty * 64;
    FusedArgs b = a;
    b.kstamp = ks;
    const int njobs = a.S * a.w * a.nty;
    const dim3 grid((njobs + ST / 64 - 1) / (ST / 64));
    if (a.acc_vec_end < (long long)a.h * a.w) hipLaunchKernelGGL(sm::k_small_scan<true>, grid, dim3(ST), 0, st, b, sblur, CS);
    else hipLaunchKernelGGL(sm::k_small_scan<false>, grid, dim3(ST), 0, st, b, sblur, CS);
    return hipGetLastError();
}

}  // namespace fm
