// fm_yuv.hip — YUV frames (NV12, I420, YUY2, UYVY) -> packed BGR on the input stream, in front of the
// unchanged hot path (fm_submit_yuv / fm_submit_yuv_list).
//
// cv2.cvtColor(yuv, COLOR_YUV2BGR_{NV12,I420,YUY2,UYVY}) restated (OpenCV imgproc color_yuv.simd.hpp,
// YUV420p2RGB8Invoker / YUV422toRGB8Invoker): BT.601 limited range in 20-bit fixed point, the chroma
// pair of a 2x1 (4:2:2) or 2x2 (4:2:0) pixel group replicated, never interpolated:
//   uu = U - 128, vv = V - 128, y = max(0, Y - 16) * 1220542
//   R = sat((y + 524288 + 1673527 vv) >> 20), G = sat((y + 524288 - 852492 vv - 409993 uu) >> 20),
//   B = sat((y + 524288 + 2116026 uu) >> 20)           (>> arithmetic: negative sums floor)
//
// Purely HBM-bound (1.5 or 2 B/px in, 3 B/px out).  One lane converts a run of kRun = 16 pixels: of both
// rows of a row pair for the 4:2:0 formats (the chroma of the pair is loaded once), of one row for the
// packed ones.  Luma and chroma come in as 16-byte loads (I420's two chroma planes as 8-byte ones), a row's
// 48 BGR bytes go out as three 16-byte stores; consecutive lanes take consecutive runs, so a wave reads
// 1 KiB of a luma row and writes 3 KiB of a BGR row.  A run that is cut by the image edge, or whose
// addresses are not aligned (a pitch or a surface offset that is no multiple of 16, W no multiple of 16 on
// the store side), goes through the byte-wise path instead.  The grid is flat over (frame, row group, run),
// capped and grid-strided; no LDS, no atomics.
#include <algorithm>

#include "fm_internal.h"

namespace fm {
namespace {

constexpr int kRun = 16;  // pixels per lane and row
constexpr int kCY = 1220542, kCRV = 1673527, kCGV = -852492, kCGU = -409993, kCBU = 2116026, kRound = 1 << 19;

// sat_u8(v >> 20), clamped before the shift: min(max(v >> 20, 0), 255) of two neighbouring channels packed
// into 16 bits is matched by hipcc (ROCm 7.2) to gfx950's v_ashr_pk_u8_i32, and on an MI355X the words built
// from such a pair came out with stray bits above bit 15 (B and G of every fourth pixel wrong).  The clamp
// first and a logical shift after it is the same function of v and is not matched.
__device__ __forceinline__ uint32_t sat8(int v) { return (uint32_t)min(max(v, 0), (255 << 20) | 0xFFFFF) >> 20; }

// the three chroma terms of one U, V pair (shared by the 2 or 4 pixels of its group)
struct Chroma {
    int r, g, b;
};
__device__ __forceinline__ Chroma chroma_terms(int U, int V) {
    const int uu = U - 128, vv = V - 128;
    return {kRound + kCRV * vv, kRound + kCGV * vv + kCGU * uu, kRound + kCBU * uu};
}
// one pixel -> B | G << 8 | R << 16
__device__ __forceinline__ uint32_t pixel_bgr(int Y, const Chroma& c) {
    const int y = max(0, Y - 16) * kCY;
    return sat8(y + c.b) | (sat8(y + c.g) << 8) | (sat8(y + c.r) << 16);
}

__device__ __forceinline__ int byte_of(const uint32_t* w, int i) { return (int)((w[i >> 2] >> ((i & 3) * 8)) & 255u); }

// kRun pixels (24-bit values) -> 48 packed bytes as three 16-byte stores; out is 16-byte aligned
__device__ __forceinline__ void store_run(uint8_t* out, const uint32_t (&px)[kRun]) {
    uint4* o = reinterpret_cast<uint4*>(out);
    uint32_t w[12];
#pragma unroll
    for (int g = 0; g < kRun / 4; g++) {  // 4 pixels -> 3 words
        const uint32_t p0 = px[4 * g], p1 = px[4 * g + 1], p2 = px[4 * g + 2], p3 = px[4 * g + 3];
        w[3 * g] = p0 | (p1 << 24);
        w[3 * g + 1] = (p1 >> 8) | (p2 << 16);
        w[3 * g + 2] = (p2 >> 16) | (p3 << 8);
    }
    o[0] = make_uint4(w[0], w[1], w[2], w[3]);
    o[1] = make_uint4(w[4], w[5], w[6], w[7]);
    o[2] = make_uint4(w[8], w[9], w[10], w[11]);
}

__device__ __forceinline__ void store_px(uint8_t* out, uint32_t p) {
    out[0] = (uint8_t)p;
    out[1] = (uint8_t)(p >> 8);
    out[2] = (uint8_t)(p >> 16);
}

// a load through the global address space (a frame address read from the device table would otherwise
// make every load of the frame a flat one)
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
template <class T>
__device__ __forceinline__ T gload(const void* p) {
    return *(const __attribute__((address_space(1))) T*)p;
}

__device__ __forceinline__ bool aligned(const void* p, uintptr_t n) { return ((uintptr_t)p & (n - 1)) == 0; }

template <int FMT>
__global__ __launch_bounds__(256) void k_yuv2bgr(YuvArgs a) {
    kstamp_begin(a.kstamp);
    constexpr bool planar = FMT == FM_YUV_NV12 || FMT == FM_YUV_I420;
    const size_t out_row = (size_t)a.W * 3;
    const long long step = (long long)gridDim.x * blockDim.x;
    for (long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x; idx < a.total; idx += step) {
        const int run = (int)(idx % a.runs);
        const long long rest = idx / a.runs;
        const int rg = (int)(rest % a.groups);
        const size_t f = (size_t)(rest / a.groups);
        const int x = run * kRun;
        const int npx = min(kRun, a.W - x);
        const uint8_t* fp = a.srcs ? a.srcs[f] : a.src + f * a.frame_stride;
        uint8_t* dp = a.dst + f * (size_t)a.H * out_row;
        if constexpr (planar) {
            const int y0 = 2 * rg;
            const uint8_t* l0 = fp + (size_t)y0 * a.pitch + x;
            const uint8_t* l1 = l0 + a.pitch;
            uint8_t* o0 = dp + (size_t)y0 * out_row + (size_t)x * 3;
            uint8_t* o1 = o0 + out_row;
            const uint8_t *cu, *cv;  // NV12: cu = the interleaved row, cv unused
            if constexpr (FMT == FM_YUV_NV12) {
                cu = fp + a.chroma_offset + (size_t)rg * a.pitch + x;
                cv = cu;
            } else {
                const size_t cp = (size_t)(a.pitch >> 1);
                cu = fp + a.chroma_offset + (size_t)rg * cp + (x >> 1);
                cv = cu + cp * (size_t)(a.H >> 1);
            }
            bool wide = npx == kRun && aligned(l0, 16) && aligned(l1, 16) && aligned(o0, 16) && aligned(o1, 16);
            if constexpr (FMT == FM_YUV_NV12) wide = wide && aligned(cu, 16);
            else wide = wide && aligned(cu, 8) && aligned(cv, 8);
            if (wide) {
                const u32x4 ya = gload<u32x4>(l0);
                const u32x4 yb = gload<u32x4>(l1);
                const uint32_t y0w[4] = {ya.x, ya.y, ya.z, ya.w}, y1w[4] = {yb.x, yb.y, yb.z, yb.w};
                uint32_t uw[2], vw[2], uvw[4];
                if constexpr (FMT == FM_YUV_NV12) {
                    const u32x4 c = gload<u32x4>(cu);
                    uvw[0] = c.x, uvw[1] = c.y, uvw[2] = c.z, uvw[3] = c.w;
                } else {
                    const u32x2 u = gload<u32x2>(cu), v = gload<u32x2>(cv);
                    uw[0] = u.x, uw[1] = u.y, vw[0] = v.x, vw[1] = v.y;
                }
                uint32_t p0[kRun], p1[kRun];
#pragma unroll
                for (int j = 0; j < kRun / 2; j++) {
                    int U, V;
                    if constexpr (FMT == FM_YUV_NV12) U = byte_of(uvw, 2 * j), V = byte_of(uvw, 2 * j + 1);
                    else U = byte_of(uw, j), V = byte_of(vw, j);
                    const Chroma c = chroma_terms(U, V);
                    p0[2 * j] = pixel_bgr(byte_of(y0w, 2 * j), c);
                    p0[2 * j + 1] = pixel_bgr(byte_of(y0w, 2 * j + 1), c);
                    p1[2 * j] = pixel_bgr(byte_of(y1w, 2 * j), c);
                    p1[2 * j + 1] = pixel_bgr(byte_of(y1w, 2 * j + 1), c);
                }
                store_run(o0, p0);
                store_run(o1, p1);
            } else {
                for (int i = 0; i < npx; i += 2) {  // W is even: whole pixel pairs
                    int U, V;
                    if constexpr (FMT == FM_YUV_NV12) U = gload<uint8_t>(cu + i), V = gload<uint8_t>(cu + i + 1);
                    else U = gload<uint8_t>(cu + (i >> 1)), V = gload<uint8_t>(cv + (i >> 1));
                    const Chroma c = chroma_terms(U, V);
                    store_px(o0 + 3 * i, pixel_bgr(gload<uint8_t>(l0 + i), c));
                    store_px(o0 + 3 * i + 3, pixel_bgr(gload<uint8_t>(l0 + i + 1), c));
                    store_px(o1 + 3 * i, pixel_bgr(gload<uint8_t>(l1 + i), c));
                    store_px(o1 + 3 * i + 3, pixel_bgr(gload<uint8_t>(l1 + i + 1), c));
                }
            }
        } else {
            constexpr int yi = FMT == FM_YUV_YUY2 ? 0 : 1;  // byte of Y0 in the 4-byte pair; U at 1 - yi, V at 3 - yi
            const uint8_t* l0 = fp + (size_t)rg * a.pitch + (size_t)x * 2;
            uint8_t* o0 = dp + (size_t)rg * out_row + (size_t)x * 3;
            if (npx == kRun && aligned(l0, 16) && aligned(o0, 16)) {
                const u32x4 qa = gload<u32x4>(l0), qb = gload<u32x4>(l0 + 16);
                const uint32_t w[8] = {qa.x, qa.y, qa.z, qa.w, qb.x, qb.y, qb.z, qb.w};
                uint32_t p0[kRun];
#pragma unroll
                for (int j = 0; j < kRun / 2; j++) {
                    const Chroma c = chroma_terms(byte_of(w, 4 * j + 1 - yi), byte_of(w, 4 * j + 3 - yi));
                    p0[2 * j] = pixel_bgr(byte_of(w, 4 * j + yi), c);
                    p0[2 * j + 1] = pixel_bgr(byte_of(w, 4 * j + 2 + yi), c);
                }
                store_run(o0, p0);
            } else {
                for (int i = 0; i < npx; i += 2) {
                    const uint8_t* q = l0 + 2 * i;
                    const Chroma c = chroma_terms(gload<uint8_t>(q + 1 - yi), gload<uint8_t>(q + 3 - yi));
                    store_px(o0 + 3 * i, pixel_bgr(gload<uint8_t>(q + yi), c));
                    store_px(o0 + 3 * i + 3, pixel_bgr(gload<uint8_t>(q + 2 + yi), c));
                }
            }
        }
    }
    kstamp_end_wg(a.kstamp);
}

}  // namespace

hipError_t launch_yuv2bgr(hipStream_t st, const YuvArgs& in) {
    YuvArgs a = in;
    const bool planar = a.format == FM_YUV_NV12 || a.format == FM_YUV_I420;
    a.runs = (a.W + kRun - 1) / kRun;
    a.groups = planar ? a.H / 2 : a.H;
    a.total = (long long)a.F * a.groups * a.runs;
    if (a.total <= 0) return hipSuccess;
    // memory-bound: enough workgroups to fill every CU several times over, the rest grid-strided
    const long long want = (a.total + 255) / 256;
    const dim3 grid((unsigned)std::min<long long>(want, 256 * 16)), block(256);
    switch (a.format) {
        case FM_YUV_NV12: hipLaunchKernelGGL(k_yuv2bgr<FM_YUV_NV12>, grid, block, 0, st, a); break;
        case FM_YUV_I420: hipLaunchKernelGGL(k_yuv2bgr<FM_YUV_I420>, grid, block, 0, st, a); break;
        case FM_YUV_YUY2: hipLaunchKernelGGL(k_yuv2bgr<FM_YUV_YUY2>, grid, block, 0, st, a); break;
        case FM_YUV_UYVY: hipLaunchKernelGGL(k_yuv2bgr<FM_YUV_UYVY>, grid, block, 0, st, a); break;
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

}  // namespace fm
