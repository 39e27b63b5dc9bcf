// fm_kernels.hip — gfx950 kernels of the motion-detection hot path.
//
// Stage map (reference = find_motion/find_motion.py, "fm.py"):
//   k_resize_area / k_resize_area_fast   imutils.resize(INTER_AREA)        fm.py:492
//   k_resize_area_up                     the same towards a larger image   fm.py:492
//   k_pixel                              cvtColor, GaussianBlur, mask,     fm.py:493-494, 619-662
//                                        convertScaleAbs+absdiff,
//                                        threshold, accumulateWeighted,
//                                        dilate(iterations=2)
//   k_ccl_*                              findContours(RETR_EXTERNAL) count fm.py:269-272
//                                        + boundingRect                    fm.py:792
//
// Bit-exactness notes: the file is compiled with -ffp-contract=off and every
// floating-point step that OpenCV performs with separate roundings is written
// with explicit __f*_rn / __d*_rn intrinsics; the fused accumulate step uses
// __fma_rn exactly where OpenCV's AVX2 body uses v_fma.
#include "fm_internal.h"

namespace fm {

// ---------------------------------------------------------------------------
// helpers
__device__ __forceinline__ int reflect101(int p, int len) {
    if ((unsigned)p < (unsigned)len) return p;
    if (len == 1) return 0;
    do {
        p = (p < 0) ? -p : 2 * len - 2 - p;
    } while ((unsigned)p >= (unsigned)len);
    return p;
}

__device__ __forceinline__ int gray_of(int b, int g, int r) {
    return (b * 1868 + g * 9617 + r * 4899 + 8192) >> 14;  // COLOR_BGR2GRAY, u8
}

__device__ __forceinline__ uint8_t sat_u8(int v) { return (uint8_t)min(max(v, 0), 255); }

// ---------------------------------------------------------------------------
// INTER_AREA, general (non-integer scale) path.  One workgroup per
// (destination row, frame); thread e owns destination element (dx, c) and
// runs OpenCV's sequential float chain: buf = sum_x S*alpha (in xtab order),
// sum = sum_y beta*buf (in ytab order), then saturate_cast (rne).
__global__ __launch_bounds__(256) void k_resize_area(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst,
                                                      int H, int W, int h, int w, const int32_t* __restrict__ xofs,
                                                      const int32_t* __restrict__ xcnt, const float* __restrict__ xwt,
                                                      int xtaps, const int32_t* __restrict__ yofs,
                                                      const int32_t* __restrict__ ycnt, const float* __restrict__ ywt,
                                                      int ytaps, uint64_t* kstamp) {
    kstamp_begin_grid(kstamp);
    const int dy = blockIdx.x;
    const size_t f = blockIdx.y;
    const uint8_t* S0 = src + f * (size_t)H * W * 3;
    uint8_t* D = dst + (f * h + dy) * (size_t)w * 3;
    const int sy0 = yofs[dy], ny = ycnt[dy];
    const float* wy = ywt + (size_t)dy * ytaps;
    for (int e = threadIdx.x; e < w * 3; e += blockDim.x) {
        const int dx = e / 3, c = e - dx * 3;
        const int sx0 = xofs[dx], nx = xcnt[dx];
        const float* wx = xwt + (size_t)dx * xtaps;
        float sum = 0.f;
        for (int j = 0; j < ny; j++) {
            const uint8_t* S = S0 + (size_t)(sy0 + j) * W * 3 + (size_t)sx0 * 3 + c;
            float buf = 0.f;
            for (int t = 0; t < nx; t++) buf = __fadd_rn(buf, __fmul_rn((float)S[t * 3], wx[t]));
            const float term = __fmul_rn(wy[j], buf);
            sum = (j == 0) ? term : __fadd_rn(sum, term);
        }
        D[e] = sat_u8(__float2int_rn(sum));
    }
    kstamp_end_wg(kstamp);
}

// INTER_AREA, general path, staged: one workgroup per (destination row, frame) walks
// that row's source rows in ytab order.  Each source row (3*W bytes) is read once with
// coalesced 16-B loads into LDS (double buffered: row j+1 is in flight into registers
// while row j is summed), the x weights sit in LDS for the whole walk, and thread e keeps
// the running sums of its destination elements (dx, c) = (e / 3, e % 3) in registers.
// The float chain per element is k_resize_area's, in the same order, so the bytes are
// identical.  Limits (else k_resize_area): 3*W % 16 == 0, 16-B aligned frames,
// 3*W <= RS_MAXROW, w*3 <= 256 * RS_EPT, w * xtaps floats <= RS_MAXWT.
constexpr int RS_T = 256, RS_EPT = 8, RS_CPT = 4;
constexpr int RS_MAXROW = RS_T * RS_CPT * 16;
constexpr int RS_MAXWT = 8192;
__global__ __launch_bounds__(RS_T) void k_resize_area_rows(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst,
                                                           int H, int W, int h, int w, const int32_t* __restrict__ xofs,
                                                           const int32_t* __restrict__ xcnt, const float* __restrict__ xwt,
                                                           int xtaps, const int32_t* __restrict__ yofs,
                                                           const int32_t* __restrict__ ycnt, const float* __restrict__ ywt,
                                                           int ytaps, uint64_t* kstamp) {
    kstamp_begin_grid(kstamp);
    extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
    const int rowb = 3 * W;                        // multiple of 16
    uint8_t* rows = lds;                           // [2][rowb]
    float* wt = reinterpret_cast<float*>(lds + 2 * rowb);  // [w][xtaps]
    const int dy = blockIdx.x;
    const size_t f = blockIdx.y;
    const int tid = threadIdx.x;
    const uint8_t* S0 = src + f * (size_t)H * rowb;
    for (int i = tid; i < w * xtaps; i += RS_T) wt[i] = xwt[i];
    const int sy0 = yofs[dy], ny = ycnt[dy];
    const int nch = rowb / 16;
    uint4 p0 = make_uint4(0, 0, 0, 0), p1 = p0, p2 = p0, p3 = p0;  // row prefetch (RS_CPT = 4 chunks)
    static_assert(RS_CPT == 4, "prefetch registers");
#define RS_LOAD_ROW(J)                                                                          \
    do {                                                                                        \
        const uint4* R_ = reinterpret_cast<const uint4*>(S0 + (size_t)(sy0 + (J)) * rowb);     \
        if (tid < nch) p0 = R_[tid];                                                            \
        if (tid + RS_T < nch) p1 = R_[tid + RS_T];                                              \
        if (tid + 2 * RS_T < nch) p2 = R_[tid + 2 * RS_T];                                      \
        if (tid + 3 * RS_T < nch) p3 = R_[tid + 3 * RS_T];                                      \
    } while (0)
#define RS_STORE_ROW(B)                                                                         \
    do {                                                                                        \
        uint4* L_ = reinterpret_cast<uint4*>(rows + (B) * rowb);                                \
        if (tid < nch) L_[tid] = p0;                                                            \
        if (tid + RS_T < nch) L_[tid + RS_T] = p1;                                              \
        if (tid + 2 * RS_T < nch) L_[tid + 2 * RS_T] = p2;                                      \
        if (tid + 3 * RS_T < nch) L_[tid + 3 * RS_T] = p3;                                      \
    } while (0)
    const int ne = w * 3;
    int sx0[RS_EPT], nx[RS_EPT], c3[RS_EPT];
    float sum[RS_EPT];
#pragma unroll
    for (int k = 0; k < RS_EPT; k++) {
        const int e = tid + RS_T * k;
        const int dx = e < ne ? e / 3 : 0;
        sx0[k] = xofs[dx];
        nx[k] = e < ne ? xcnt[dx] : 0;
        c3[k] = dx * xtaps;                   // weight row
        sum[k] = 0.f;
        sx0[k] = sx0[k] * 3 + (e < ne ? e - dx * 3 : 0);  // byte of tap 0 in the row
    }
    const float* wy = ywt + (size_t)dy * ytaps;
    RS_LOAD_ROW(0);
    for (int j = 0; j < ny; j++) {
        const int b = j & 1;
        __syncthreads();  // buffer b is free (row j-2 summed) and the weights are in
        RS_STORE_ROW(b);
        if (j + 1 < ny) RS_LOAD_ROW(j + 1);
        __syncthreads();
        const uint8_t* L = rows + b * rowb;
        const float wyj = wy[j];
#pragma unroll
        for (int k = 0; k < RS_EPT; k++) {
            if (RS_T * k < ne) {  // wave-uniform
                float buf = 0.f;
                const uint8_t* Lp = L + sx0[k];
                const float* wp = wt + c3[k];
                for (int t = 0; t < nx[k]; t++) buf = __fadd_rn(buf, __fmul_rn((float)Lp[3 * t], wp[t]));
                const float term = __fmul_rn(wyj, buf);
                sum[k] = (j == 0) ? term : __fadd_rn(sum[k], term);
            }
        }
    }
    uint8_t* D = dst + (f * h + dy) * (size_t)ne;
#pragma unroll
    for (int k = 0; k < RS_EPT; k++) {
        const int e = tid + RS_T * k;
        if (e < ne) D[e] = sat_u8(__float2int_rn(sum[k]));
    }
    kstamp_end_wg(kstamp);
#undef RS_LOAD_ROW
#undef RS_STORE_ROW
}

// INTER_AREA, general path, register-resident (round 4): one thread per destination pixel
// (dx, dy) of one frame, all three channels, no LDS and no barriers.  The thread walks its
// ycnt[dy] source rows two at a time; for each row pair it loads the 3*NT bytes of its x taps
// from both rows (per-frame buffer descriptor, 4-B aligned b128 loads, one v_alignbyte per
// dword to take out the 0..3-byte misalignment), and runs OpenCV's float chain on packed f32:
// lane (row j, row j+1) of one v_pk_mul_f32 / v_pk_add_f32 pair per (tap, channel), the tap
// weight broadcast.  The x weights (padded with zeros to NT: 0 * S = +0 and buf + 0 = buf, so
// the padding is exact) stay in registers for the whole walk.  The per-element order is
// k_resize_area's: buf = sum_x S*alpha in xtab order, sum = beta_0*buf_0 + beta_1*buf_1 + ...
// in ytab order, then saturate_cast (rne).
typedef float rs_f2 __attribute__((ext_vector_type(2)));
// (Non-temporal frame loads: mode D 492 vs 822 k frames/s -- neighbouring windows re-read a column; round 6,
// profiles/r06/r06i_nontemporal_ab.txt.)
constexpr int RN_T = 256;
template <int NT>
__global__ __launch_bounds__(RN_T) void k_resize_area_nt(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst,
                                                         int H, int W, int h, int w, const int32_t* __restrict__ xofs,
                                                         const int32_t* __restrict__ xcnt, const float* __restrict__ xwt,
                                                         int xtaps, const int32_t* __restrict__ yofs,
                                                         const int32_t* __restrict__ ycnt, const float* __restrict__ ywt,
                                                         int ytaps, const uint8_t* const* __restrict__ srcs,
                                                         uint64_t* kstamp) {
    kstamp_begin_grid(kstamp);
    constexpr int NB = 3 * NT;          // tap bytes of one row
    constexpr int NA = (NB + 3) / 4;    // aligned dwords holding them
    constexpr int ND = NA + 1;          // dwords loaded (a 0..3-byte misalignment)
    constexpr int NQ = ND / 4, NR = ND % 4;
    const int n = h * w;
    const int item = blockIdx.x * RN_T + threadIdx.x;
    const int it = item < n ? item : n - 1;
    const int dy = it / w, dx = it - dy * w;
    const uint32_t rowb = 3u * (uint32_t)W;
    const uint32_t fbytes = rowb * (uint32_t)H;
    const uint32_t lim = (fbytes + 3u) & ~3u;  // every dword holding a frame byte is in range
    // frame blockIdx.y: consecutive frames from src, or one address per frame (srcs: find_objects' ROI
    // frames, read where the engine left them)
    const uint8_t* F = srcs ? srcs[blockIdx.y] : src + (size_t)blockIdx.y * fbytes;
    const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc((void*)F, 0, (int)lim, 0x00020000);
    const int nx = xcnt[dx];
    float wx[NT];
#pragma unroll
    for (int t = 0; t < NT; t++) wx[t] = t < nx ? xwt[(size_t)dx * xtaps + t] : 0.f;
    const uint32_t b0 = 3u * (uint32_t)xofs[dx];
    const int sy0 = yofs[dy], ny = ycnt[dy];
    const float* wy = ywt + (size_t)dy * ytaps;
    float sum[3] = {0.f, 0.f, 0.f};
    for (int j = 0; j < ny; j += 2) {
        uint32_t o[2] = {(uint32_t)(sy0 + j) * rowb + b0, (uint32_t)(sy0 + j + 1) * rowb + b0};
        uint32_t al[2][NA];
#pragma unroll
        for (int r = 0; r < 2; r++) {
            const uint32_t a = o[r] & ~3u, sh = o[r] & 3u;
            uint32_t d[ND];
            if (a + 4u * ND <= lim) {
#pragma unroll
                for (int q = 0; q < NQ; q++) {
                    const auto v = __builtin_amdgcn_raw_buffer_load_b128(rs, (int)(a + 16u * q), 0, 0);
                    d[4 * q] = v[0]; d[4 * q + 1] = v[1]; d[4 * q + 2] = v[2]; d[4 * q + 3] = v[3];
                }
                if constexpr (NR == 1) {
                    d[4 * NQ] = __builtin_amdgcn_raw_buffer_load_b32(rs, (int)(a + 16u * NQ), 0, 0);
                } else if constexpr (NR == 2) {
                    const auto v = __builtin_amdgcn_raw_buffer_load_b64(rs, (int)(a + 16u * NQ), 0, 0);
                    d[4 * NQ] = v[0]; d[4 * NQ + 1] = v[1];
                } else if constexpr (NR == 3) {
                    const auto v = __builtin_amdgcn_raw_buffer_load_b96(rs, (int)(a + 16u * NQ), 0, 0);
                    d[4 * NQ] = v[0]; d[4 * NQ + 1] = v[1]; d[4 * NQ + 2] = v[2];
                }
            } else {  // the window runs past the frame (its last columns / a row past the walk): dwords
                      // wholly out of range read as 0 and carry zero weights or are discarded.  One dword
                      // per load, the step in soffset, so that the loads are not merged into multi-dword
                      // ones (whose range check would not be per dword on every target)
#pragma unroll
                for (int q = 0; q < ND; q++) d[q] = __builtin_amdgcn_raw_buffer_load_b32(rs, (int)a, 4 * q, 0);
            }
#pragma unroll
            for (int q = 0; q < NA; q++) al[r][q] = __builtin_amdgcn_alignbyte(d[q + 1], d[q], sh);
        }
        rs_f2 acc[3];
#pragma unroll
        for (int t = 0; t < NT; t++) {
#pragma unroll
            for (int c = 0; c < 3; c++) {
                const int k = 3 * t + c, q = k >> 2, s = 8 * (k & 3);
                const rs_f2 p = {(float)(uint8_t)(al[0][q] >> s), (float)(uint8_t)(al[1][q] >> s)};
                const rs_f2 m = p * wx[t];
                acc[c] = t == 0 ? m : acc[c] + m;  // 0 + m == m: OpenCV's zeroed buf
            }
        }
        const float by0 = wy[j];
#pragma unroll
        for (int c = 0; c < 3; c++) {
            const float term = __fmul_rn(by0, acc[c].x);
            sum[c] = j == 0 ? term : __fadd_rn(sum[c], term);
        }
        if (j + 1 < ny) {
            const float by1 = wy[j + 1];
#pragma unroll
            for (int c = 0; c < 3; c++) sum[c] = __fadd_rn(sum[c], __fmul_rn(by1, acc[c].y));
        }
    }
    if (item < n) {
        uint8_t* D = dst + ((size_t)blockIdx.y * n + item) * 3;
#pragma unroll
        for (int c = 0; c < 3; c++) D[c] = sat_u8(__float2int_rn(sum[c]));
    }
    kstamp_end_wg(kstamp);
}

// INTER_AREA integer-scale path (resizeAreaFast): 2x2 => (sum+2)>>2,
// otherwise cvRound(sum * (1.f/area)).
__global__ __launch_bounds__(256) void k_resize_area_fast(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst,
                                                           int H, int W, int h, int w, int sx, int sy, float inv_area,
                                                           uint64_t* kstamp) {
    kstamp_begin_grid(kstamp);
    const size_t f = blockIdx.y;
    const int n = h * w * 3;
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e < n) {
        const int c = e % 3, dx = (e / 3) % w, dy = e / (3 * w);
        const uint8_t* S = src + f * (size_t)H * W * 3;
        int sum = 0;
        for (int yy = 0; yy < sy; yy++)
            for (int xx = 0; xx < sx; xx++) sum += S[((size_t)(dy * sy + yy) * W + (dx * sx + xx)) * 3 + c];
        const int v = (sx == 2 && sy == 2) ? ((sum + 2) >> 2) : __float2int_rn(__fmul_rn((float)sum, inv_area));
        dst[f * (size_t)n + e] = sat_u8(v);
    }
    kstamp_end_wg(kstamp);
}

hipError_t launch_resize_area(hipStream_t st, const uint8_t* src, uint8_t* dst, int F, int H, int W, int h, int w,
                              const int32_t* xofs, const int32_t* xcnt, const float* xwt, int xtaps,
                              const int32_t* yofs, const int32_t* ycnt, const float* ywt, int ytaps,
                              const uint8_t* const* srcs, uint64_t* kstamp) {
    const int nt = (xtaps + 1) & ~1;
    if (nt <= 32 && (size_t)3 * W * H < (1u << 31)) {
        const dim3 g((h * w + RN_T - 1) / RN_T, F);
        switch (nt) {
#define RN_CASE(N)                                                                                                      \
    case N:                                                                                                            \
        hipLaunchKernelGGL(k_resize_area_nt<N>, g, dim3(RN_T), 0, st, src, dst, H, W, h, w, xofs, xcnt, xwt, xtaps, yofs, \
                           ycnt, ywt, ytaps, srcs, kstamp);                                                            \
        break;
            RN_CASE(2) RN_CASE(4) RN_CASE(6) RN_CASE(8) RN_CASE(10) RN_CASE(12) RN_CASE(14) RN_CASE(16)
            RN_CASE(18) RN_CASE(20) RN_CASE(22) RN_CASE(24) RN_CASE(26) RN_CASE(28) RN_CASE(30) RN_CASE(32)
#undef RN_CASE
        }
        return hipGetLastError();
    }
    if (srcs) return hipErrorInvalidValue;  // per-frame addresses: the register kernel only (callers gather)
    dim3 grid(h, F);
    const int rowb = 3 * W;
    if (rowb % 16 == 0 && ((uintptr_t)src & 15) == 0 && rowb <= RS_MAXROW && w * 3 <= RS_T * RS_EPT &&
        w * xtaps <= RS_MAXWT) {
        const int bytes = 2 * rowb + w * xtaps * 4;
        (void)hipFuncSetAttribute((const void*)k_resize_area_rows, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
        hipLaunchKernelGGL(k_resize_area_rows, grid, dim3(RS_T), bytes, st, src, dst, H, W, h, w, xofs, xcnt, xwt, xtaps,
                           yofs, ycnt, ywt, ytaps, kstamp);
    } else {
        hipLaunchKernelGGL(k_resize_area, grid, dim3(256), 0, st, src, dst, H, W, h, w, xofs, xcnt, xwt, xtaps, yofs,
                           ycnt, ywt, ytaps, kstamp);
    }
    return hipGetLastError();
}

hipError_t launch_resize_area_fast(hipStream_t st, const uint8_t* src, uint8_t* dst, int F, int H, int W, int h,
                                   int w, int sx, int sy, uint64_t* kstamp) {
    const int n = h * w * 3;
    dim3 grid((n + 255) / 256, F);
    const float inv_area = 1.f / (float)(sx * sy);
    hipLaunchKernelGGL(k_resize_area_fast, grid, dim3(256), 0, st, src, dst, H, W, h, w, sx, sy, inv_area, kstamp);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------
// INTER_AREA towards a larger image: cv::resize's 8-bit bilinear resizer with area-mode taps (fm_roi.cpp builds
// them).  All integer: D = S[s0] * a0 + S[s1] * a1 per source row, dst = (((b0 * (D0 >> 4)) >> 16) + ((b1 *
// (D1 >> 4)) >> 16) + 2) >> 2.  The output is the larger side, so the kernel is shaped by its stores.
//
// A workgroup takes p.rows destination rows of one span of p.cols destination columns of one frame:
//   1. the span's column table (s0 << 12 | a1 per destination column) and the band's row table go to LDS;
//   2. the source bytes the span reads, of every source row the band reads, go to LDS: aligned dword loads, all
//      of a thread's loads in flight before the first is stored (one byte load per lane and tap left a wave
//      waiting for memory once per element: 1.28 ms per 64 frames of 1280 x 720 -> 1920 x 1080); a dword that is
//      not wholly inside the frame is put together from the bytes that are, so no read passes a frame's last byte
//      or precedes its first;
//   3. the horizontal results D >> 4 (16 bits) go to LDS, once per source row however many destination rows use
//      it, a lane per destination pixel: its two source pixels are six consecutive bytes (where the first tap is
//      the row's last pixel the second coefficient is 0, so what follows it in LDS is multiplied by 0);
//   4. each lane takes one aligned dword of the destination (aligned in memory: a row starts at any byte when
//      3 * w is no multiple of 4) and stores it whole, a wave 256 contiguous bytes per store.  Where the span is
//      the full width the band's rows are one contiguous range and a dword may run from one row into the next;
//      a dword that the range only partly covers (its two ends, shared with the neighbouring workgroup) is
//      stored by bytes.  A lane's four horizontal results are 8 bytes of LDS at a 2-byte alignment, read as
//      three dwords (lanes 8 bytes apart: two lanes per bank) and shifted into place.
// (Workgroups of 1,024 threads, two a CU, took 0.77 ms where these take 0.61 ms per 64 frames of 1280 x 720 ->
// 1920 x 1080: more waves per CU did not help.  DESIGN.md 3.3.)
constexpr int RU_T = 256;

struct RuRow {
    const uint16_t *h0, *h1;  // the row's two source rows of horizontal results
    uint32_t b0, b1;
};
__device__ __forceinline__ RuRow ru_row(const uint32_t* yt, const uint16_t* Hs, int r, int sr0, int H, int hstride) {
    const uint32_t ty = yt[r];
    const int s0 = (int)(ty >> 12), s1 = min(s0 + 1, H - 1);
    const uint32_t b1 = ty & 0xfffu;
    return {Hs + (s0 - sr0) * hstride, Hs + (s1 - sr0) * hstride, 2048u - b1, b1};
}
__device__ __forceinline__ uint32_t ru_value(uint32_t d0, uint32_t d1, uint32_t b0, uint32_t b1) {
    return (((b0 * d0) >> 16) + ((b1 * d1) >> 16) + 2u) >> 2;
}

__global__ __launch_bounds__(RU_T) void k_resize_area_up(const uint8_t* __restrict__ src,
                                                         const uint8_t* const* __restrict__ srcs,
                                                         uint8_t* __restrict__ dst, int H, int W, int h, int w,
                                                         const uint32_t* __restrict__ xtab,
                                                         const uint32_t* __restrict__ ytab, AreaUpPlan p,
                                                         uint64_t* kstamp) {
    kstamp_begin_grid(kstamp);
    extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
    uint32_t* xt = reinterpret_cast<uint32_t*>(lds);          // [p.cols]
    uint32_t* yt = xt + p.cols;                               // [p.rows]
    uint16_t* Hs = reinterpret_cast<uint16_t*>(yt + p.rows);  // [p.nsrc][hstride], rows dword-aligned
    const int tid = threadIdx.x;
    const int band = blockIdx.x / p.nspans, span = blockIdx.x - band * p.nspans;
    const int y0 = band * p.rows, ny = min(p.rows, h - y0);
    const int x0 = span * p.cols, nx = min(p.cols, w - x0);
    const int segb = 3 * nx, hstride = area_up_hstride(p.cols);
    const size_t f = blockIdx.y, rowb = (size_t)3 * w;
    const uint8_t* S = srcs ? srcs[f] : src + f * (size_t)H * W * 3;

    for (int i = tid; i < nx; i += RU_T) xt[i] = xtab[x0 + i];
    for (int i = tid; i < ny; i += RU_T) yt[i] = ytab[y0 + i];
    __syncthreads();
    const int sr0 = (int)(yt[0] >> 12);
    const int ns = min((int)(yt[ny - 1] >> 12) + 1, H - 1) - sr0 + 1;
    if (ns > p.nsrc) return;  // (the plan covers every band: never taken)
    const int rstride = area_up_rawstride(p.cols);  // bytes between two rows of source bytes, a multiple of 4
    uint32_t* raw = reinterpret_cast<uint32_t*>(Hs + p.nsrc * hstride);  // [p.nsrc][rstride / 4]

    // the span's source columns c0 .. c1 of the band's source rows -> raw: row j holds the dwords from the aligned
    // address at or below the row segment's first byte, which lies lead(j) bytes into the first
    const int c0 = (int)(xt[0] >> 12), c1 = min((int)(xt[nx - 1] >> 12) + 1, W - 1);
    const int rawb = 3 * (c1 - c0 + 1);
    if (rawb + 12 > rstride) return;  // (at most cols + 1 source columns: never taken)
    const int ndw = (rawb + 6) >> 2, total = ns * ndw;
    const uint8_t* Send = S + (size_t)H * W * 3;
    const uint8_t* G0 = S + (size_t)sr0 * W * 3 + (size_t)3 * c0;
    const float dinv = 1.f / (float)ndw;
    constexpr int RU_U = 4;
    for (int base = 0; base < total; base += RU_T * RU_U) {
        uint32_t v[RU_U];
        int at[RU_U];
#pragma unroll
        for (int u = 0; u < RU_U; u++) {
            const int idx = base + u * RU_T + tid;
            at[u] = -1;
            v[u] = 0;
            if (idx < total) {
                int j = (int)((float)idx * dinv);  // idx / ndw (idx < 2^24: off by one at most)
                j -= j * ndw > idx;
                j += (j + 1) * ndw <= idx;
                const int i = idx - j * ndw;
                const uint8_t* G = G0 + (size_t)j * W * 3;
                const uint8_t* q = G - ((uintptr_t)G & 3) + 4 * i;
                if (q >= S && q + 4 <= Send) {
                    v[u] = *reinterpret_cast<const uint32_t*>(q);
                } else {
                    for (int b = 0; b < 4; b++)
                        if (q + b >= S && q + b < Send) v[u] |= (uint32_t)q[b] << (8 * b);
                }
                at[u] = j * (rstride >> 2) + i;
            }
        }
#pragma unroll
        for (int u = 0; u < RU_U; u++)
            if (at[u] >= 0) raw[at[u]] = v[u];
    }
    __syncthreads();

    // horizontal pass: every source row of the band, once; a lane per destination pixel
    for (int j = 0; j < ns; j++) {
        const int lead = (int)((uintptr_t)(G0 + (size_t)j * W * 3) & 3);
        const uint32_t* Rj = raw + j * (rstride >> 2);
        uint16_t* Hj = Hs + j * hstride;
        for (int dx = tid; dx < nx; dx += RU_T) {
            const uint32_t t = xt[dx];
            const uint32_t a1 = t & 0xfffu, a0 = 2048u - a1;
            const int off = lead + 3 * ((int)(t >> 12) - c0);
            const uint32_t* q = Rj + (off >> 2);
            const uint32_t d0 = q[0], d1 = q[1], d2 = q[2];
            const uint32_t lo = __builtin_amdgcn_alignbyte(d1, d0, (uint32_t)off & 3u);  // bytes off .. off + 3
            const uint32_t hi = __builtin_amdgcn_alignbyte(d2, d1, (uint32_t)off & 3u);  // bytes off + 4 .. off + 7
            uint16_t* o = Hj + 3 * dx;
            o[0] = (uint16_t)(((lo & 0xffu) * a0 + (lo >> 24) * a1) >> 4);
            o[1] = (uint16_t)((((lo >> 8) & 0xffu) * a0 + (hi & 0xffu) * a1) >> 4);
            o[2] = (uint16_t)((((lo >> 16) & 0xffu) * a0 + ((hi >> 8) & 0xffu) * a1) >> 4);
        }
    }
    __syncthreads();

    // vertical pass and stores.  Segments: the whole band when the span is the full width, else one per row
    const bool merged = p.nspans == 1;
    const int nseg = merged ? 1 : ny;
    const int seglen = merged ? ny * segb : segb;
    const float rinv = 1.f / (float)segb;
    uint8_t* band0 = dst + (f * h + y0) * rowb + (size_t)3 * x0;
    for (int sg = 0; sg < nseg; sg++) {
        uint8_t* A = band0 + (size_t)sg * rowb;
        const int lead = (int)((uintptr_t)A & 3);  // the segment starts `lead` bytes into its first dword
        const int nch = (lead + seglen + 3) >> 2;
        for (int ch = tid; ch < nch; ch += RU_T) {
            const int p0 = ch * 4 - lead;  // the dword's first byte, relative to the segment
            const int pb = max(p0, 0), pe = min(p0 + 4, seglen);
            int r = sg;
            if (merged) {  // pb / segb (pb < 2^24: exact in float, the quotient off by one at most)
                r = (int)((float)pb * rinv);
                r -= r * segb > pb;
                r += (r + 1) * segb <= pb;
            }
            int e = merged ? pb - r * segb : pb;
            RuRow rw = ru_row(yt, Hs, r, sr0, H, hstride);
            if (pe - pb == 4 && e + 4 <= segb) {
                const int eb = e & ~1;
                const uint32_t sh = (uint32_t)(e & 1) * 16u;
                const uint32_t* q0 = reinterpret_cast<const uint32_t*>(rw.h0 + eb);
                const uint32_t* q1 = reinterpret_cast<const uint32_t*>(rw.h1 + eb);
                const uint32_t u0 = q0[0], u1 = q0[1], u2 = q0[2], v0 = q1[0], v1 = q1[1], v2 = q1[2];
                const uint32_t ul = __builtin_amdgcn_alignbit(u1, u0, sh), uh = __builtin_amdgcn_alignbit(u2, u1, sh);
                const uint32_t vl = __builtin_amdgcn_alignbit(v1, v0, sh), vh = __builtin_amdgcn_alignbit(v2, v1, sh);
                const uint32_t out = ru_value(ul & 0xffffu, vl & 0xffffu, rw.b0, rw.b1) |
                                     ru_value(ul >> 16, vl >> 16, rw.b0, rw.b1) << 8 |
                                     ru_value(uh & 0xffffu, vh & 0xffffu, rw.b0, rw.b1) << 16 |
                                     ru_value(uh >> 16, vh >> 16, rw.b0, rw.b1) << 24;
                *reinterpret_cast<uint32_t*>(A + p0) = out;
            } else {
                for (int q = pb; q < pe; q++) {
                    A[q] = (uint8_t)ru_value(rw.h0[e], rw.h1[e], rw.b0, rw.b1);
                    if (++e == segb && q + 1 < pe) {  // (full-width spans only) into the next row
                        e = 0;
                        rw = ru_row(yt, Hs, ++r, sr0, H, hstride);
                    }
                }
            }
        }
    }
    kstamp_end_wg(kstamp);
}

hipError_t launch_resize_area_up(hipStream_t st, const uint8_t* src, uint8_t* dst, int F, int H, int W, int h, int w,
                                 const uint32_t* xtab, const uint32_t* ytab, const AreaUpPlan& p,
                                 const uint8_t* const* srcs, uint64_t* kstamp) {
    if (p.rows < 1 || p.cols < 1 || (long long)p.nspans * p.cols < w || p.lds > 64 * 1024 ||
        p.lds < 4 * p.cols + 4 * p.rows + p.nsrc * (2 * area_up_hstride(p.cols) + area_up_rawstride(p.cols)))
        return hipErrorInvalidValue;
    const dim3 grid((unsigned)(((h + p.rows - 1) / p.rows) * p.nspans), F);
    (void)hipFuncSetAttribute((const void*)k_resize_area_up, hipFuncAttributeMaxDynamicSharedMemorySize, p.lds);
    hipLaunchKernelGGL(k_resize_area_up, grid, dim3(RU_T), p.lds, st, src, srcs, dst, H, W, h, w, xtab, ytab, p, kstamp);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------
// Fused per-pixel chain for one frame of every stream.
//
// Tile = TW x TH output pixels of the dilated mask.  The dilation needs the
// threshold on the tile + 2 px halo (E region), the threshold needs the blur
// there, and the blur needs gray on E + r = ksize/2 (G region).  Stages:
//   G  : gray from BGR (REFLECT_101 indices)            LDS u8
//   Hs : horizontal taps  sum kx*g                      LDS u16 (<= 255*256)
//   E  : vertical taps, rounding, mask, diff, threshold LDS u8; background
//        updated for the tile interior only (bg_in -> bg_out ping-pong so a
//        neighbour's halo read never sees this frame's update)
//   dilate 5x5 as two separable max passes -> mask_out
constexpr int kTW = 64, kTH = 16, kPixThreads = 256;

__host__ __device__ constexpr int align16(int v) { return (v + 15) & ~15; }

struct PixelLayout {
    int GW, GH, EW, EH, offH, offE, offD, bytes;
    __host__ __device__ PixelLayout(int r) {
        GW = kTW + 4 + 2 * r;
        GH = kTH + 4 + 2 * r;
        EW = kTW + 4;
        EH = kTH + 4;
        offH = align16(GW * GH);
        offE = offH + align16(GH * EW * 2);
        offD = offE + align16(EH * EW);
        bytes = offD + align16(EH * kTW);
    }
};

struct PixelKArgs {
    PixelArgs a;
    const double* bg_in;
};

__global__ __launch_bounds__(kPixThreads) void k_pixel(PixelArgs a, const double* __restrict__ bg_in,
                                                        double* __restrict__ bg_out) {
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    const int r = a.ksize >> 1;
    const PixelLayout L(r);
    uint8_t* G = smem;
    uint16_t* Hs = reinterpret_cast<uint16_t*>(smem + L.offH);
    uint8_t* E = smem + L.offE;
    uint8_t* D = smem + L.offD;

    const int s = blockIdx.z;
    const int h = a.h, w = a.w;
    const int x0 = blockIdx.x * kTW, y0 = blockIdx.y * kTH;
    const size_t plane = (size_t)h * w;
    const uint8_t* src = a.src + (size_t)s * plane * 3;
    const size_t sbase = (size_t)s * plane;
    const bool has_keep = a.has_keep[s] != 0;
    const bool init = a.init != nullptr && a.init[s] != 0;
    const int k = a.ksize;

    // G: gray over the halo region
    for (int i = threadIdx.x; i < L.GW * L.GH; i += kPixThreads) {
        const int gy = i / L.GW, gx = i - gy * L.GW;
        const int y = reflect101(y0 - 2 - r + gy, h);
        const int x = reflect101(x0 - 2 - r + gx, w);
        const uint8_t* p = src + ((size_t)y * w + x) * 3;
        G[i] = (uint8_t)gray_of(p[0], p[1], p[2]);
    }
    __syncthreads();
    // Hs: horizontal pass (8 fraction bits, exact)
    for (int i = threadIdx.x; i < L.GH * L.EW; i += kPixThreads) {
        const int gy = i / L.EW, c = i - gy * L.EW;
        const uint8_t* g = G + gy * L.GW + c;
        uint32_t acc = 0;
        for (int t = 0; t < k; t++) acc += (uint32_t)a.coef[t] * g[t];
        Hs[i] = (uint16_t)acc;
    }
    __syncthreads();
    // E: vertical pass + mask + diff + threshold (+ background update inside)
    for (int i = threadIdx.x; i < L.EH * L.EW; i += kPixThreads) {
        const int ty = i / L.EW, tx = i - ty * L.EW;
        const int y = y0 - 2 + ty, x = x0 - 2 + tx;
        uint8_t th = 0;
        if (y >= 0 && y < h && x >= 0 && x < w) {
            uint32_t acc = 0;
            const uint16_t* hv = Hs + ty * L.EW + tx;
            for (int t = 0; t < k; t++) acc += (uint32_t)a.coef[t] * hv[t * L.EW];
            int blur = (int)((acc + 32768u) >> 16);
            const size_t li = (size_t)y * w + x;
            const size_t pix = sbase + li;
            if (has_keep && a.keep[pix] == 0) blur = 0;
            const double bgv = init ? (double)blur : bg_in[pix];
            int q = a.cvt_simd ? __float2int_rn(fabsf(__double2float_rn(bgv))) : __double2int_rn(fabs(bgv));
            q = min(max(q, 0), 255);
            const int d = abs(blur - q);
            th = d > a.thresh ? 255 : 0;
            if (ty >= 2 && ty < kTH + 2 && tx >= 2 && tx < kTW + 2) {
                const double bl = (double)blur;
                double nb;
                if ((long long)li < a.acc_vec_end)
                    nb = __fma_rn(bgv, a.beta, __dmul_rn(bl, a.alpha));
                else
                    nb = __dadd_rn(__dmul_rn(bl, a.alpha), __dmul_rn(bgv, a.beta));
                bg_out[pix] = nb;
                if (a.gray_out) {
                    a.gray_out[pix] = G[(ty + r) * L.GW + tx + r];
                    a.blur_out[pix] = (uint8_t)blur;
                    a.delta_out[pix] = (uint8_t)d;
                }
            }
        }
        E[i] = th;
    }
    __syncthreads();
    // dilate: horizontal 5-max over E rows
    for (int i = threadIdx.x; i < L.EH * kTW; i += kPixThreads) {
        const int ty = i / kTW, c = i - ty * kTW;
        const uint8_t* e = E + ty * L.EW + c;
        D[i] = max(max(max(e[0], e[1]), max(e[2], e[3])), e[4]);
    }
    __syncthreads();
    // dilate: vertical 5-max -> output
    for (int i = threadIdx.x; i < kTH * kTW; i += kPixThreads) {
        const int oy = i / kTW, ox = i - oy * kTW;
        const int y = y0 + oy, x = x0 + ox;
        if (y < h && x < w) {
            const uint8_t* d = D + oy * kTW + ox;
            const uint8_t m = max(max(max(d[0], d[kTW]), max(d[2 * kTW], d[3 * kTW])), d[4 * kTW]);
            a.mask_out[sbase + (size_t)y * w + x] = m;
        }
    }
}

int pixel_lds_bytes(int ksize) { return PixelLayout(ksize >> 1).bytes; }

hipError_t launch_pixel_pp(hipStream_t st, const PixelArgs& a, const double* bg_in, double* bg_out) {
    const int bytes = PixelLayout(a.ksize >> 1).bytes;
    if (bytes > 160 * 1024) return hipErrorInvalidValue;
    dim3 grid((a.w + kTW - 1) / kTW, (a.h + kTH - 1) / kTH, a.S);
    hipLaunchKernelGGL(k_pixel, grid, dim3(kPixThreads), bytes, st, a, bg_in, bg_out);
    return hipGetLastError();
}

hipError_t launch_pixel(hipStream_t st, const PixelArgs& a) { return launch_pixel_pp(st, a, a.bg, a.bg); }

// ---------------------------------------------------------------------------
// Connected components for findContours(RETR_EXTERNAL).
//
// Every pixel is labelled: foreground 8-connected, background 4-connected
// (Suzuki-Abe's connectivity pair), label = raster index of the component's
// raster-first pixel (union-find that always links the larger root under the
// smaller).  A foreground component has an external contour iff the
// background component left of its first pixel is the outer one, i.e. the
// component of the 1-px zero pad = every background component touching the
// image border.  That equals OpenCV's EXTERNAL scan (checked against the
// literal Suzuki-Abe restatement in oracle/fm_oracle.c).

__device__ __forceinline__ int lds_load(int* p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}
__device__ __forceinline__ int lfind(int* Lb, int x) {
    for (;;) {
        const int p = lds_load(&Lb[x]);
        if (p == x) return x;
        x = p;
    }
}
__device__ __forceinline__ void lunion(int* Lb, int a, int b) {
    for (;;) {
        a = lfind(Lb, a);
        b = lfind(Lb, b);
        if (a == b) return;
        if (a < b) {
            const int old = atomicMin(&Lb[b], a);
            if (old == b) return;
            b = old;
        } else {
            const int old = atomicMin(&Lb[a], b);
            if (old == a) return;
            a = old;
        }
    }
}

__device__ __forceinline__ int gload(int* p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ int gfind(int* Lg, int x) {
    for (;;) {
        const int p = gload(&Lg[x]);
        if (p == x) return x;
        x = p;
    }
}
__device__ __forceinline__ void gunion(int* Lg, int a, int b) {
    for (;;) {
        a = gfind(Lg, a);
        b = gfind(Lg, b);
        if (a == b) return;
        if (a < b) {
            const int old = atomicMin(&Lg[b], a);
            if (old == b) return;
            b = old;
        } else {
            const int old = atomicMin(&Lg[a], b);
            if (old == a) return;
            a = old;
        }
    }
}

constexpr int CB = kCclBlock;

__global__ __launch_bounds__(256) void k_ccl_local(CclArgs a) {
    __shared__ int Lb[CB * CB];
    __shared__ uint8_t M[CB * CB];
    const size_t f = blockIdx.z;
    const int h = a.h, w = a.w;
    const int bx = blockIdx.x * CB, by = blockIdx.y * CB;
    const uint8_t* mask = a.mask + f * (size_t)h * w;
    int32_t* label = a.label + f * (size_t)h * w;
    for (int p = threadIdx.x; p < CB * CB; p += 256) {
        const int ly = p / CB, lx = p % CB, y = by + ly, x = bx + lx;
        M[p] = (y < h && x < w) ? (mask[(size_t)y * w + x] ? 1 : 0) : 2;
        Lb[p] = p;
    }
    __syncthreads();
    for (int p = threadIdx.x; p < CB * CB; p += 256) {
        const int m = M[p];
        if (m == 2) continue;
        const int ly = p / CB, lx = p % CB;
        if (m == 1) {
            if (lx > 0 && M[p - 1] == 1) lunion(Lb, p, p - 1);
            if (ly > 0) {
                if (M[p - CB] == 1) lunion(Lb, p, p - CB);
                if (lx > 0 && M[p - CB - 1] == 1) lunion(Lb, p, p - CB - 1);
                if (lx < CB - 1 && M[p - CB + 1] == 1) lunion(Lb, p, p - CB + 1);
            }
        } else {
            if (lx > 0 && M[p - 1] == 0) lunion(Lb, p, p - 1);
            if (ly > 0 && M[p - CB] == 0) lunion(Lb, p, p - CB);
        }
    }
    __syncthreads();
    for (int p = threadIdx.x; p < CB * CB; p += 256) {
        if (M[p] == 2) continue;
        const int ly = p / CB, lx = p % CB;
        const int root = lfind(Lb, p);
        const int ry = root / CB, rx = root % CB;
        label[(size_t)(by + ly) * w + bx + lx] = (by + ry) * w + bx + rx;
    }
}

// Union across block edges: right-column pixels with E/NE/SE, bottom-row
// pixels with S/SE/SW (foreground), E / S (background).
__global__ __launch_bounds__(64) void k_ccl_merge(CclArgs a) {
    const size_t f = blockIdx.z;
    const int h = a.h, w = a.w;
    const uint8_t* mask = a.mask + f * (size_t)h * w;
    int32_t* L = a.label + f * (size_t)h * w;
    const int bx = blockIdx.x * CB, by = blockIdx.y * CB;
    const int t = threadIdx.x;
    int x, y;
    if (t < CB) {
        x = bx + CB - 1;
        y = by + t;
        if (x + 1 >= w || y >= h) return;
    } else {
        x = bx + (t - CB);
        y = by + CB - 1;
        if (y + 1 >= h || x >= w) return;
    }
    const int p = y * w + x;
    const bool fg = mask[p] != 0;
    auto link = [&](int xx, int yy, bool diag) {
        if (xx < 0 || xx >= w || yy < 0 || yy >= h) return;
        const int q = yy * w + xx;
        const bool qfg = mask[q] != 0;
        if (qfg != fg) return;
        if (!fg && diag) return;
        gunion(L, L[p], L[q]);
    };
    if (t < CB) {
        link(x + 1, y, false);
        link(x + 1, y - 1, true);
        link(x + 1, y + 1, true);
    } else {
        link(x, y + 1, false);
        link(x + 1, y + 1, true);
        link(x - 1, y + 1, true);
    }
}

__global__ __launch_bounds__(256) void k_ccl_flatten(CclArgs a) {
    const size_t f = blockIdx.y;
    const int n = a.h * a.w;
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    int32_t* L = a.label + f * (size_t)n;
    const int l = L[i];
    if (l != i) L[i] = gfind(L, l);
}

// Mark background components that touch the image border (== the pad's).
__global__ __launch_bounds__(256) void k_ccl_outer(CclArgs a) {
    const size_t f = blockIdx.y;
    const int h = a.h, w = a.w;
    const int per = 2 * w + 2 * h;
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= per) return;
    int x, y;
    if (i < w) { x = i; y = 0; }
    else if (i < 2 * w) { x = i - w; y = h - 1; }
    else if (i < 2 * w + h) { x = 0; y = i - 2 * w; }
    else { x = w - 1; y = i - 2 * w - h; }
    const size_t base = f * (size_t)h * w;
    const int p = y * w + x;
    if (a.mask[base + p] == 0) a.outer[base + a.label[base + p]] = 1;
}

// Foreground roots (raster-first pixels): external test + record allocation.
__global__ __launch_bounds__(256) void k_ccl_roots(CclArgs a) {
    const size_t f = blockIdx.y;
    const int h = a.h, w = a.w, n = h * w;
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const size_t base = f * (size_t)n;
    if (a.mask[base + i] == 0 || a.label[base + i] != i) return;
    const int y = i / w, x = i - y * w;
    const bool ext = (x == 0) || a.outer[base + a.label[base + i - 1]] != 0;
    int id = -1;
    if (ext) {
        id = atomicAdd(&a.count[f], 1);
        if (id < a.cap) {
            int32_t* r = a.rec + (f * a.cap + id) * 5;
            r[0] = i; r[1] = x; r[2] = y; r[3] = x; r[4] = y;
        }
    }
    a.cid[base + i] = id;
}

// Bounding boxes: only component-boundary pixels can hold an extreme.
__global__ __launch_bounds__(256) void k_ccl_bbox(CclArgs a) {
    const size_t f = blockIdx.y;
    const int h = a.h, w = a.w, n = h * w;
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const size_t base = f * (size_t)n;
    const uint8_t* m = a.mask + base;
    if (m[i] == 0) return;
    const int y = i / w, x = i - y * w;
    const bool left = (x == 0) || m[i - 1] == 0;
    const bool right = (x == w - 1) || m[i + 1] == 0;
    const bool down = (y == h - 1) || m[i + w] == 0;
    if (!(left || right || down)) return;
    const int id = a.cid[base + a.label[base + i]];
    if (id < 0 || id >= a.cap) return;
    int32_t* r = a.rec + (f * a.cap + id) * 5;
    if (left) atomicMin(&r[1], x);
    if (right) atomicMax(&r[3], x);
    if (down) atomicMax(&r[4], y);
}

hipError_t launch_ccl(hipStream_t st, const CclArgs& a, KernelTimer* tm) {
    const int F = a.F, h = a.h, w = a.w, n = h * w;
    dim3 gb((w + CB - 1) / CB, (h + CB - 1) / CB, F);
    hipError_t e;
    int tok = tm ? tm->begin("ccl_local", st) : -1;
    hipLaunchKernelGGL(k_ccl_local, gb, dim3(256), 0, st, a);
    if (tm) tm->end(tok);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    tok = tm ? tm->begin("ccl_merge", st) : -1;
    hipLaunchKernelGGL(k_ccl_merge, gb, dim3(64), 0, st, a);
    if (tm) tm->end(tok);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    dim3 gp((n + 255) / 256, F);
    tok = tm ? tm->begin("ccl_flatten", st) : -1;
    hipLaunchKernelGGL(k_ccl_flatten, gp, dim3(256), 0, st, a);
    if (tm) tm->end(tok);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    dim3 go((2 * w + 2 * h + 255) / 256, F);
    tok = tm ? tm->begin("ccl_outer", st) : -1;
    hipLaunchKernelGGL(k_ccl_outer, go, dim3(256), 0, st, a);
    if (tm) tm->end(tok);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    tok = tm ? tm->begin("ccl_roots", st) : -1;
    hipLaunchKernelGGL(k_ccl_roots, gp, dim3(256), 0, st, a);
    if (tm) tm->end(tok);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    tok = tm ? tm->begin("ccl_bbox", st) : -1;
    hipLaunchKernelGGL(k_ccl_bbox, gp, dim3(256), 0, st, a);
    if (tm) tm->end(tok);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------
// Retained source frames (fm_retain_frames): n copies of `bytes` bytes each in one launch, copy i from
// pairs[i].src to pairs[i].dst.  A destination is a pool entry and 16-byte aligned (the launcher's contract);
// a source is wherever its frame starts in a batch slot, (t * S + s) * bytes, so of any alignment.
// A workgroup takes one chunk (64 bytes per lane) of one frame: blockIdx.x = frame * chunks + chunk.
//   source 16-byte aligned: four 16-byte loads per lane, then the four stores (1 KiB per wave instruction);
//   any other source: the destination's dwords, each from the two aligned source dwords around it
//     (v_alignbit), four per lane in flight, 256 B per wave instruction.  Every dword read holds at
//     least one byte of the frame, so no read leaves the pages the frame lies in;
//   the last bytes % 16 of the frame: byte by byte.
// No atomics, no data-dependent indices, no LDS.
constexpr int kRetainLaneBytes = 64;
typedef uint32_t u32x4_t __attribute__((ext_vector_type(4)));
#define FM_GLOBAL __attribute__((address_space(1)))  // global (not flat) addressing of the table's addresses

struct RetainLoad16 {  // a 16-byte piece of a 16-byte aligned source
    typedef u32x4_t T;
    const uint8_t* s;
    __device__ __forceinline__ T operator()(size_t o) const { return *(const FM_GLOBAL T*)(s + o); }
};
struct RetainLoad4 {  // a dword of a source `sh` / 8 bytes past dword alignment, from the two aligned dwords around it
    typedef uint32_t T;
    const uint8_t* s;
    uint32_t sh;
    __device__ __forceinline__ T operator()(size_t o) const {
        const FM_GLOBAL uint32_t* q = (const FM_GLOBAL uint32_t*)((uintptr_t)(s + o) & ~(uintptr_t)3);
        const uint32_t lo = q[0];
        return sh ? __builtin_amdgcn_alignbit(q[1], lo, sh) : lo;  // (sh != 0: the piece's last byte lies in q[1])
    }
};

// a lane's four pieces, `step` bytes apart from byte o of the frame on, those that begin below vend: the loads, then
// the stores
template <class Load>
__device__ __forceinline__ void retain_pieces(const Load& load, uint8_t* d, size_t o, size_t step, size_t vend) {
    typedef typename Load::T T;
    const size_t o1 = o + step, o2 = o1 + step, o3 = o2 + step;
    if (o3 < vend) {  // all four (every chunk of a frame but its last): nothing between the loads
        const T w0 = load(o), w1 = load(o1), w2 = load(o2), w3 = load(o3);
        *(FM_GLOBAL T*)(d + o) = w0;
        *(FM_GLOBAL T*)(d + o1) = w1;
        *(FM_GLOBAL T*)(d + o2) = w2;
        *(FM_GLOBAL T*)(d + o3) = w3;
        return;
    }
    T v0 = {}, v1 = {}, v2 = {}, v3 = {};
    if (o < vend) v0 = load(o);
    if (o1 < vend) v1 = load(o1);
    if (o2 < vend) v2 = load(o2);
    if (o3 < vend) v3 = load(o3);
    if (o < vend) *(FM_GLOBAL T*)(d + o) = v0;
    if (o1 < vend) *(FM_GLOBAL T*)(d + o1) = v1;
    if (o2 < vend) *(FM_GLOBAL T*)(d + o2) = v2;
    if (o3 < vend) *(FM_GLOBAL T*)(d + o3) = v3;
}

__global__ __launch_bounds__(256) void k_retain_frames(const RetainPair* __restrict__ pairs, size_t bytes,
                                                        unsigned chunks) {
    const unsigned f = blockIdx.x / chunks, ch = blockIdx.x - f * chunks;
    const uint8_t* s = pairs[f].src;
    uint8_t* d = pairs[f].dst;
    const size_t chunk = (size_t)blockDim.x * kRetainLaneBytes;
    const size_t b0 = (size_t)ch * chunk;
    const size_t b1 = min(b0 + chunk, bytes);
    const size_t vend = b0 + ((b1 - b0) & ~(size_t)15);  // the end of the chunk's whole 16-byte pieces
    if (((uintptr_t)s & 15) == 0) {
        retain_pieces(RetainLoad16{s}, d, b0 + (size_t)threadIdx.x * 16, (size_t)blockDim.x * 16, vend);
    } else {
        const RetainLoad4 load{s, (uint32_t)((uintptr_t)s & 3) * 8u};
        const size_t step = (size_t)blockDim.x * 4;
        for (size_t o = b0 + (size_t)threadIdx.x * 4; o < vend; o += 4 * step) retain_pieces(load, d, o, step, vend);
    }
    for (size_t o = vend + threadIdx.x; o < b1; o += blockDim.x)
        ((FM_GLOBAL uint8_t*)d)[o] = ((const FM_GLOBAL uint8_t*)s)[o];
}

hipError_t launch_retain_frames(hipStream_t st, const RetainPair* pairs, int n, size_t bytes) {
    if (n < 1 || bytes == 0) return hipSuccess;
    const unsigned threads = bytes >= 16384 ? 256 : 64;  // a small frame: one wave per 4 KiB of it
    const size_t chunk = (size_t)threads * kRetainLaneBytes;
    const size_t chunks = (bytes + chunk - 1) / chunk;
    if (chunks * (size_t)n > 0x7fffffffull) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_retain_frames, dim3((unsigned)(chunks * (size_t)n)), dim3(threads), 0, st, pairs, bytes,
                       (unsigned)chunks);
    return hipGetLastError();
}

}  // namespace fm
