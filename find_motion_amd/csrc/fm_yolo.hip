// The YOLOv3 object stage: cvlib.detect_common_objects(frame.resized, ...) of
// find_motion.py:733-741 on the GPU, from the user's Darknet files.
//
//   k_yolo_blob    ROI frame (INTER_AREA, the Haar stage's kernels) -> 8-bit INTER_LINEAR to the
//                  network size -> R/B swap, * 0.00392 -> NCHW f32
//   k_conv         convolution as an implicit GEMM on v_mfma_f32_32x32x2_f32: M = Cout,
//                  N = batch * Hout * Wout, K = Cin * size^2; bias + leaky in the epilogue; the
//                  output may land at a channel offset of a wider buffer (a [route]'s)
//   k_maxpool, k_upsample, k_shortcut, k_copy     the layers without arithmetic
//   k_yolo_decode  the region layer in yolo mode; rows above the confidence, compacted
//
// By default everything is f32: the f32-input MFMA is a k-ordered fmaf chain, so a convolution output
// differs from exact arithmetic by at most (K + 3) * 2^-24 * (sum |w x| + |b|).
//
// FM_YOLO_F16 (fm_yolo_create_precision) keeps activations and weights as f16 and accumulates in f32 on
// v_mfma_f32_32x32x16_f16; its kernels (k_conv16 and the *16 ones) stand in a section of their own below
// and the f32 kernels are not touched by it.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <new>
#include <string>
#include <vector>

#include "../../include/find_motion_amd.h"
#include "fm_internal.h"
#include "fm_roi.h"

namespace fm {
namespace yolo {

typedef float f32x16 __attribute__((ext_vector_type(16)));

struct View {  // a layer's activations: frame b, channel c at p + b * bs + c * h * w
    float* p;
    size_t bs;
};

struct ConvArgs {
    const float* in;
    size_t in_bs;
    float* out;
    size_t out_bs;
    const float* wp;    // [Kpad][Mpad], zero padded
    const float* bias;  // [Cout]
    int Cin, H, W, Cout, Ho, Wo, stride, pad, leaky, K, Kpad, Mpad, N;
};

constexpr int BK = 16;  // k per LDS tile: 8 MFMAs of k = 2

// Block: 4 waves, each one 32 x 32 output tile; WM waves along M (Cout), 4 / WM along N.
// LDS rows are padded by 32 floats so that the two lane halves of an operand read (rows k and
// k + 1) fall on different banks.
template <int SIZE, int WM>
__global__ __launch_bounds__(256) void k_conv(ConvArgs a) {
    constexpr int BM = 32 * WM, BN = 32 * (4 / WM);
    constexpr int LDA = BM + 32, LDB = BN + 32;
    constexpr int NA = BK * BM / 256, NB = BK * BN / 256;  // elements per thread and tile
    constexpr int S2 = SIZE * SIZE;
    __shared__ float As[BK * LDA];
    __shared__ float Bs[BK * LDB];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int m0 = blockIdx.y * BM, n0 = blockIdx.x * BN;
    const int wm = (wave % WM) * 32, wn = (wave / WM) * 32;
    const int hw = a.Ho * a.Wo;
    // the loader's column of B: one output pixel
    const int bl = tid % BN, bk0 = tid / BN;
    const int n = n0 + bl;
    const bool nvalid = n < a.N;
    int iy0 = 0, ix0 = 0;
    const float* inb = a.in;
    if (nvalid) {
        const int b = n / hw, r = n - b * hw, oy = r / a.Wo, ox = r - oy * a.Wo;
        iy0 = oy * a.stride - a.pad;
        ix0 = ox * a.stride - a.pad;
        inb = a.in + (size_t)b * a.in_bs;
    }
    const int al = tid % BM, ak0 = tid / BM;
    float ra[NA], rb[NB];
    auto fetch = [&](int k0) {
#pragma unroll
        for (int i = 0; i < NA; i++) ra[i] = a.wp[(size_t)(k0 + ak0 + i * (256 / BM)) * a.Mpad + m0 + al];
#pragma unroll
        for (int i = 0; i < NB; i++) {
            const int k = k0 + bk0 + i * (256 / BN);
            float v = 0.f;
            if (nvalid && k < a.K) {
                const int c = k / S2, r = k - c * S2, ky = r / SIZE, kx = r - ky * SIZE;
                const int iy = iy0 + ky, ix = ix0 + kx;
                if (iy >= 0 && iy < a.H && ix >= 0 && ix < a.W) v = inb[((size_t)c * a.H + iy) * a.W + ix];
            }
            rb[i] = v;
        }
    };
    f32x16 acc;
#pragma unroll
    for (int i = 0; i < 16; i++) acc[i] = 0.f;
    fetch(0);
    for (int k0 = 0; k0 < a.Kpad; k0 += BK) {
#pragma unroll
        for (int i = 0; i < NA; i++) As[(ak0 + i * (256 / BM)) * LDA + al] = ra[i];
#pragma unroll
        for (int i = 0; i < NB; i++) Bs[(bk0 + i * (256 / BN)) * LDB + bl] = rb[i];
        __syncthreads();
        if (k0 + BK < a.Kpad) fetch(k0 + BK);
#pragma unroll
        for (int kk = 0; kk < BK; kk += 2) {
            const int k = kk + (lane >> 5);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(As[k * LDA + wm + (lane & 31)], Bs[k * LDB + wn + (lane & 31)],
                                                       acc, 0, 0, 0);
        }
        __syncthreads();
    }
    // C/D map: column = lane & 31, row = (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5)
    const int on = n0 + wn + (lane & 31);
    if (on >= a.N) return;
    const int b = on / hw, r = on - b * hw;
    float* ob = a.out + (size_t)b * a.out_bs + r;
#pragma unroll
    for (int i = 0; i < 16; i++) {
        const int m = m0 + wm + (i & 3) + 8 * (i >> 2) + 4 * (lane >> 5);
        if (m < a.Cout) {
            float v = acc[i] + a.bias[m];
            if (a.leaky) v = v > 0.f ? v : 0.1f * v;
            ob[(size_t)m * hw] = v;
        }
    }
}

// out(b, c, y, x) over total = n * C * Ho * Wo elements
__global__ void k_maxpool(const float* __restrict__ in, size_t in_bs, float* __restrict__ out, size_t out_bs, int C,
                          int H, int W, int Ho, int Wo, int stride, long long total) {
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= total) return;
    const int x = (int)(t % Wo), y = (int)((t / Wo) % Ho), c = (int)((t / ((long long)Wo * Ho)) % C);
    const int b = (int)(t / ((long long)Wo * Ho * C));
    const float* p = in + (size_t)b * in_bs + (size_t)c * H * W;
    const int y0 = y * stride, x0 = x * stride, y1 = min(y0 + 1, H - 1), x1 = min(x0 + 1, W - 1);
    const float v = fmaxf(fmaxf(p[(size_t)y0 * W + x0], p[(size_t)y0 * W + x1]),
                          fmaxf(p[(size_t)y1 * W + x0], p[(size_t)y1 * W + x1]));
    out[(size_t)b * out_bs + ((size_t)c * Ho + y) * Wo + x] = v;
}

__global__ void k_upsample(const float* __restrict__ in, size_t in_bs, float* __restrict__ out, size_t out_bs, int C,
                           int H, int W, long long total) {
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= total) return;
    const int Wo = 2 * W, Ho = 2 * H;
    const int x = (int)(t % Wo), y = (int)((t / Wo) % Ho), c = (int)((t / ((long long)Wo * Ho)) % C);
    const int b = (int)(t / ((long long)Wo * Ho * C));
    out[(size_t)b * out_bs + ((size_t)c * Ho + y) * Wo + x] =
        in[(size_t)b * in_bs + ((size_t)c * H + (y >> 1)) * W + (x >> 1)];
}

// per = C * H * W elements of each frame
__global__ void k_shortcut(const float* __restrict__ p, size_t p_bs, const float* __restrict__ q, size_t q_bs,
                           float* __restrict__ out, size_t out_bs, long long per, long long total) {
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= total) return;
    const long long b = t / per, e = t - b * per;
    out[b * out_bs + e] = p[b * p_bs + e] + q[b * q_bs + e];
}

__global__ void k_copy(const float* __restrict__ in, size_t in_bs, float* __restrict__ out, size_t out_bs,
                       long long per, long long total) {
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= total) return;
    const long long b = t / per, e = t - b * per;
    out[b * out_bs + e] = in[b * in_bs + e];
}

// roi: [n][rh][rw][3] BGR u8; xt[net_w], yt[net_h]: (first tap, second tap, coefficient 0, coefficient 1)
__global__ void k_yolo_blob(const uint8_t* __restrict__ roi, int rh, int rw, const int4* __restrict__ xt,
                            const int4* __restrict__ yt, const float* __restrict__ lut, float* __restrict__ out,
                            int net_h, int net_w, long long total) {
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= total) return;
    const int dx = (int)(t % net_w), dy = (int)((t / net_w) % net_h), b = (int)(t / ((long long)net_w * net_h));
    const int4 tx = xt[dx], ty = yt[dy];
    const uint8_t* r0 = roi + ((size_t)b * rh + ty.x) * rw * 3;
    const uint8_t* r1 = roi + ((size_t)b * rh + ty.y) * rw * 3;
#pragma unroll
    for (int ch = 0; ch < 3; ch++) {
        const int D0 = r0[tx.x * 3 + ch] * tx.z + r0[tx.y * 3 + ch] * tx.w;
        const int D1 = r1[tx.x * 3 + ch] * tx.z + r1[tx.y * 3 + ch] * tx.w;
        int v = (((ty.z * (D0 >> 4)) >> 16) + ((ty.w * (D1 >> 4)) >> 16) + 2) >> 2;
        v = min(max(v, 0), 255);
        out[(((size_t)b * 3 + (2 - ch)) * net_h + dy) * net_w + dx] = lut[v];
    }
}

__device__ __forceinline__ float sigmoidf(float x) { return 1.f / (1.f + expf(-x)); }

// One thread per (frame, anchor, cell).  cand: [n][cap_rows][9]; cnt[n].
__global__ void k_yolo_decode(const float* __restrict__ in, size_t in_bs, int rows, int cols, int A, int classes,
                              const float* __restrict__ anchors, float net_w, float net_h, float zero_thresh,
                              float confidence, int head, float* __restrict__ cand, int cap_rows,
                              int* __restrict__ cnt, long long total) {
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= total) return;
    const int cells = rows * cols;
    const int cell = (int)(t % cells), an = (int)((t / cells) % A), b = (int)(t / ((long long)cells * A));
    const int y = cell / cols, x = cell - y * cols;
    const float* p = in + (size_t)b * in_bs + (size_t)an * (5 + classes) * cells + cell;
    const float obj = sigmoidf(p[(size_t)4 * cells]);
    float best = 0.f;
    int cls = 0;
    for (int j = 0; j < classes; j++) {
        float s = obj * sigmoidf(p[(size_t)(5 + j) * cells]);
        if (s <= zero_thresh) s = 0.f;
        if (s > best) {
            best = s;
            cls = j;
        }
    }
    if (!(best > confidence)) return;
    const int slot = atomicAdd(&cnt[b], 1);
    if (slot >= cap_rows) return;
    float* o = cand + ((size_t)b * cap_rows + slot) * FM_YOLO_CAND;
    o[0] = (float)head;
    o[1] = (float)(cell * A + an);
    o[2] = ((float)x + sigmoidf(p[0])) / (float)cols;
    o[3] = ((float)y + sigmoidf(p[(size_t)cells])) / (float)rows;
    o[4] = expf(p[(size_t)2 * cells]) * anchors[2 * an] / net_w;
    o[5] = expf(p[(size_t)3 * cells]) * anchors[2 * an + 1] / net_h;
    o[6] = obj;
    o[7] = (float)cls;
    o[8] = best;
}

// ---- FM_YOLO_F16 ---------------------------------------------------------------------------------------------
// Activations are NHWC halves with the channels padded to a multiple of 8 by zeros, so that 8 consecutive k of
// the implicit GEMM (k = (ky, kx, c)) are 16 contiguous bytes of one tap.  The frames of a buffer follow each
// other without a gap, so a pixel is addressed by its index over all frames.
typedef _Float16 h8 __attribute__((ext_vector_type(8)));
typedef float f32x8 __attribute__((ext_vector_type(8)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));  // 16 bytes: 8 halves as they travel

struct View16 {  // pixel q (over all frames), channel c at p + q * ps + c; p and ps are multiples of 8 halves
    _Float16* p;
    int ps;
};

constexpr float H_MAX = 65504.f;

__device__ __forceinline__ _Float16 to_half(float v) {  // clamp, then v_cvt_f16_f32 (round to nearest even)
    return (_Float16)fminf(fmaxf(v, -H_MAX), H_MAX);
}

struct Conv16Args {
    const _Float16* in;
    int in_ps;
    _Float16* out;  // NHWC halves, or null:
    int out_ps;
    float* out32;  // NCHW f32 (a head's convolution)
    size_t out32_bs;
    const _Float16* wp;  // [Mpad][Kpad], zero padded
    const float* bias;   // [Cout]
    int Cp, H, W, Cout, Ho, Wo, stride, pad, leaky, Kpad, N;
};

constexpr int BK16 = 32;            // k per LDS tile: 2 MFMAs of k = 16
constexpr int LDC = BK16 / 8 + 1;   // LDS row in 16-byte chunks: 4 of data, 1 of padding against bank conflicts

// Block: 4 waves, WM along M (Cout) and 4 / WM along N (pixels); each wave MT x NT tiles of 32 x 32.  The MFMA's
// A operand is the activation tile (rows n) and B the weight tile (columns m), so that in the C/D map a lane
// holds one output channel and a register one pixel: 32 lanes store 32 consecutive halves of an NHWC pixel.
template <int SIZE, int WM, int MT, int NT>
__global__ __launch_bounds__(256) void k_conv16(Conv16Args a) {
    constexpr int WN = 4 / WM, BM = 32 * MT * WM, BN = 32 * NT * WN;
    constexpr int NA = (BM * 4 + 255) / 256, NB = BN * 4 / 256;  // 16-byte chunks per thread and tile
    constexpr int S2 = SIZE * SIZE;
    __shared__ u32x4 Ws[BM * LDC];
    __shared__ u32x4 Xs[BN * LDC];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int m0 = blockIdx.y * BM, n0 = blockIdx.x * BN;
    const int wm = (wave % WM) * 32 * MT, wn = (wave / WM) * 32 * NT;
    const int hw = a.Ho * a.Wo;
    // a thread loads chunk g (8 k) of rows tid / 4 + 64 i
    const int g = tid & 3, row = tid >> 2;
    const bool aload = BM * 4 >= 256 || tid < BM * 4;
    int iy0[NB], ix0[NB];
    const _Float16* inb[NB];
#pragma unroll
    for (int i = 0; i < NB; i++) {
        const int n = n0 + row + 64 * i;
        inb[i] = nullptr;
        iy0[i] = ix0[i] = 0;
        if (n < a.N) {
            const int b = n / hw, r = n - b * hw, oy = r / a.Wo, ox = r - oy * a.Wo;
            iy0[i] = oy * a.stride - a.pad;
            ix0[i] = ox * a.stride - a.pad;
            inb[i] = a.in + (size_t)b * a.H * a.W * a.in_ps;
        }
    }
    int tap = (8 * g) / a.Cp, c = 8 * g - tap * a.Cp;  // the chunk's k = tap * Cp + c
    const u32x4 zero = {0u, 0u, 0u, 0u};
    u32x4 ra[NA], rb[NB];
    auto fetch = [&](int k0) {
        if (aload) {
#pragma unroll
            for (int i = 0; i < NA; i++)
                ra[i] = *(const u32x4*)(a.wp + (size_t)(m0 + row + 64 * i) * a.Kpad + k0 + 8 * g);
        }
        const int ky = tap / SIZE, kx = tap - ky * SIZE;
#pragma unroll
        for (int i = 0; i < NB; i++) {
            const int iy = iy0[i] + ky, ix = ix0[i] + kx;
            u32x4 v = zero;
            if (inb[i] && tap < S2 && iy >= 0 && iy < a.H && ix >= 0 && ix < a.W)
                v = *(const u32x4*)(inb[i] + ((size_t)iy * a.W + ix) * a.in_ps + c);
            rb[i] = v;
        }
        c += BK16;
        while (c >= a.Cp) {
            c -= a.Cp;
            tap++;
        }
    };
    f32x16 acc[NT][MT];
#pragma unroll
    for (int j = 0; j < NT; j++)
#pragma unroll
        for (int m = 0; m < MT; m++)
#pragma unroll
            for (int i = 0; i < 16; i++) acc[j][m][i] = 0.f;
    fetch(0);
    for (int k0 = 0; k0 < a.Kpad; k0 += BK16) {
        if (aload) {
#pragma unroll
            for (int i = 0; i < NA; i++) Ws[(row + 64 * i) * LDC + g] = ra[i];
        }
#pragma unroll
        for (int i = 0; i < NB; i++) Xs[(row + 64 * i) * LDC + g] = rb[i];
        __syncthreads();
        if (k0 + BK16 < a.Kpad) fetch(k0 + BK16);
#pragma unroll
        for (int ks = 0; ks < BK16 / 16; ks++) {
            const int grp = 2 * ks + (lane >> 5);
            h8 wf[MT], xf[NT];
#pragma unroll
            for (int m = 0; m < MT; m++) wf[m] = __builtin_bit_cast(h8, Ws[(wm + 32 * m + (lane & 31)) * LDC + grp]);
#pragma unroll
            for (int j = 0; j < NT; j++) xf[j] = __builtin_bit_cast(h8, Xs[(wn + 32 * j + (lane & 31)) * LDC + grp]);
#pragma unroll
            for (int j = 0; j < NT; j++)
#pragma unroll
                for (int m = 0; m < MT; m++)
                    acc[j][m] = __builtin_amdgcn_mfma_f32_32x32x16_f16(xf[j], wf[m], acc[j][m], 0, 0, 0);
        }
        __syncthreads();
    }
    // C/D map: column (the channel) = lane & 31, row (the pixel) = (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5)
#pragma unroll
    for (int m = 0; m < MT; m++) {
        const int ch = m0 + wm + 32 * m + (lane & 31);
        if (ch >= a.Cout) continue;
        const float bias = a.bias[ch];
#pragma unroll
        for (int j = 0; j < NT; j++) {
#pragma unroll
            for (int i = 0; i < 16; i++) {
                const int n = n0 + wn + 32 * j + (i & 3) + 8 * (i >> 2) + 4 * (lane >> 5);
                if (n >= a.N) continue;
                float v = acc[j][m][i] + bias;
                if (a.leaky) v = v > 0.f ? v : 0.1f * v;
                if (a.out) {
                    a.out[(size_t)n * a.out_ps + ch] = to_half(v);
                } else {
                    const int b = n / hw, r = n - b * hw;
                    a.out32[(size_t)b * a.out32_bs + (size_t)ch * hw + r] = v;
                }
            }
        }
    }
}

// The layers without arithmetic over V channels a thread (8: one 16-byte access; 1: channel counts and
// offsets that are no multiples of 8).  total = pixels * C / V.
template <int V> struct HalfVec { typedef _Float16 type; };
template <> struct HalfVec<8> { typedef h8 type; };

template <int V>
__global__ void k_maxpool16(View16 in, View16 out, int C, int H, int W, int Ho, int Wo, int stride, long long total) {
    typedef typename HalfVec<V>::type T;
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= total) return;
    const int cg = C / V;
    const int c = (int)(t % cg) * V;
    const long long q = t / cg;
    const int x = (int)(q % Wo), y = (int)((q / Wo) % Ho);
    const long long b = q / ((long long)Wo * Ho);
    const int y0 = y * stride, x0 = x * stride, y1 = min(y0 + 1, H - 1), x1 = min(x0 + 1, W - 1);
    const _Float16* p = in.p + (size_t)b * H * W * in.ps + c;
    const T v00 = *(const T*)(p + ((size_t)y0 * W + x0) * in.ps), v01 = *(const T*)(p + ((size_t)y0 * W + x1) * in.ps);
    const T v10 = *(const T*)(p + ((size_t)y1 * W + x0) * in.ps), v11 = *(const T*)(p + ((size_t)y1 * W + x1) * in.ps);
    *(T*)(out.p + (size_t)q * out.ps + c) =
        __builtin_elementwise_max(__builtin_elementwise_max(v00, v01), __builtin_elementwise_max(v10, v11));
}

template <int V>
__global__ void k_upsample16(View16 in, View16 out, int C, int H, int W, long long total) {
    typedef typename HalfVec<V>::type T;
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= total) return;
    const int cg = C / V, Wo = 2 * W, Ho = 2 * H;
    const int c = (int)(t % cg) * V;
    const long long q = t / cg;
    const int x = (int)(q % Wo), y = (int)((q / Wo) % Ho);
    const long long b = q / ((long long)Wo * Ho);
    *(T*)(out.p + (size_t)q * out.ps + c) = *(const T*)(in.p + (((size_t)b * H + (y >> 1)) * W + (x >> 1)) * in.ps + c);
}

// f16(float(p) + float(q)): one f32 add, clamped, rounded to nearest even
template <int V>
__global__ void k_shortcut16(View16 p, View16 q, View16 out, int C, long long total) {
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= total) return;
    const int cg = C / V;
    const int c = (int)(t % cg) * V;
    const size_t px = (size_t)(t / cg);
    if constexpr (V == 8) {
        const f32x8 s = __builtin_convertvector(*(const h8*)(p.p + px * p.ps + c), f32x8) +
                        __builtin_convertvector(*(const h8*)(q.p + px * q.ps + c), f32x8);
        h8 o;
#pragma unroll
        for (int i = 0; i < 8; i++) o[i] = to_half(s[i]);
        *(h8*)(out.p + px * out.ps + c) = o;
    } else {
        out.p[px * out.ps + c] = to_half((float)p.p[px * p.ps + c] + (float)q.p[px * q.ps + c]);
    }
}

template <int V>
__global__ void k_copy16(View16 in, View16 out, int C, long long total) {
    typedef typename HalfVec<V>::type T;
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= total) return;
    const int cg = C / V;
    const int c = (int)(t % cg) * V;
    const size_t px = (size_t)(t / cg);
    *(T*)(out.p + px * out.ps + c) = *(const T*)(in.p + px * in.ps + c);
}

// [n][C][hw] f32 -> NHWC halves (round to nearest even, the padding zero); total = n * hw * Cp
__global__ void k_pack16(const float* __restrict__ in, _Float16* __restrict__ out, int C, int Cp, int hw, long long total) {
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= total) return;
    const int c = (int)(t % Cp);
    const long long q = t / Cp, b = q / hw, r = q - b * hw;
    out[t] = c < C ? (_Float16)in[((size_t)b * C + c) * hw + r] : (_Float16)0.f;
}

// a view -> [n][C][hw] f32 (the halves widened); total = n * C * hw
__global__ void k_unpack16(View16 in, float* __restrict__ out, int C, int hw, long long total) {
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= total) return;
    const int r = (int)(t % hw), c = (int)((t / hw) % C);
    const long long b = t / ((long long)hw * C);
    out[t] = (float)in.p[((size_t)b * hw + r) * in.ps + c];
}

// k_yolo_blob with each table value rounded to f16 and a pixel's (R, G, B, 0 x 5) stored as one 16 bytes
__global__ void k_yolo_blob16(const uint8_t* __restrict__ roi, int rh, int rw, const int4* __restrict__ xt,
                              const int4* __restrict__ yt, const float* __restrict__ lut, _Float16* __restrict__ out,
                              int net_h, int net_w, long long total) {
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= total) return;
    const int dx = (int)(t % net_w), dy = (int)((t / net_w) % net_h), b = (int)(t / ((long long)net_w * net_h));
    const int4 tx = xt[dx], ty = yt[dy];
    const uint8_t* r0 = roi + ((size_t)b * rh + ty.x) * rw * 3;
    const uint8_t* r1 = roi + ((size_t)b * rh + ty.y) * rw * 3;
    h8 o;
#pragma unroll
    for (int i = 0; i < 8; i++) o[i] = (_Float16)0.f;
#pragma unroll
    for (int ch = 0; ch < 3; ch++) {
        const int D0 = r0[tx.x * 3 + ch] * tx.z + r0[tx.y * 3 + ch] * tx.w;
        const int D1 = r1[tx.x * 3 + ch] * tx.z + r1[tx.y * 3 + ch] * tx.w;
        int v = (((ty.z * (D0 >> 4)) >> 16) + ((ty.w * (D1 >> 4)) >> 16) + 2) >> 2;
        v = min(max(v, 0), 255);
        o[2 - ch] = (_Float16)lut[v];
    }
    *(h8*)(out + (size_t)t * 8) = o;
}

struct Layer {
    fm_yolo_layer d{};
    int Cin = 0, Hin = 0, Win = 0;  // the previous layer's output
    int C = 0, H = 0, W = 0;        // this layer's output
    int alias = -1;                 // >= 0: the route whose buffer this layer writes into
    int alias_c = 0;                // at this channel
    bool in_place = false;          // a route whose sources wrote into its buffer
    DevBuf<float> buf;              // owned activations [max_frames][C][H][W] (empty: a view of another layer's)
    View v{nullptr, 0};
    DevBuf<float> wp;  // conv: packed weights
    DevBuf<float> bias;
    int K = 0, Kpad = 0, Mpad = 0, WM = 2;
    // FM_YOLO_F16: activations [max_frames][H][W][Cp] halves, Cp = C rounded up to 8, the padding zero
    int Cp = 0;
    bool f32_out = false;  // a head's convolution: NCHW f32 in buf / v, as in the f32 mode
    DevBuf<_Float16> buf16;
    View16 v16{nullptr, 0};
    DevBuf<_Float16> wp16;  // [Mpad16][Kpad16], k = (ky, kx, c) over the input's padded channels
    int K16 = 0, Kpad16 = 0, Mpad16 = 0;
};

}  // namespace yolo
}  // namespace fm

using namespace fm::yolo;

struct fm_yolo {
    int device = 0;
    fm::Stream stream;  // (before the buffers used on it: they are released first)
    std::string err;
    int precision = FM_YOLO_F32;
    int channels = 3, net_w = 0, net_h = 0, classes = 0, max_frames = 0;
    float zero_thresh = 0.f;
    std::vector<Layer> L;
    std::vector<int> heads;
    int total_rows = 0;
    fm::DevBuf<float> d_blob, d_anchors, d_lut, d_cand;
    fm::DevBuf<_Float16> d_blob16;  // FM_YOLO_F16: the network's input (d_blob stages fm_yolo_forward's f32 blob)
    fm::DevBuf<float> d_stage;      // FM_YOLO_F16: fm_yolo_layer_output's widened copy
    fm::DevBuf<int> d_cnt;
    fm::RoiStage roi{false};  // frames -> ROI (-> blob)
    fm::DevBuf<int4> d_xt, d_yt;
    int lin_key[2] = {0, 0};  // (rw, rh) the linear tables are for
    int last_n = 0;
    fm::Event ev[4];
    double ms[3] = {0., 0., 0.};

    ~fm_yolo() {
        if (stream || d_blob) {
            (void)hipSetDevice(device);
            if (stream) (void)hipStreamSynchronize(stream);
        }
    }
};

static inline unsigned nblk(long long total, int bs = 256) { return (unsigned)((total + bs - 1) / bs); }

// cv2.resize's 8-bit INTER_LINEAR taps of one axis: (first tap, second tap, coefficient 0, coefficient 1)
static void linear8u_taps(int ssize, int dsize, std::vector<int4>& out) {
    const double scale = (double)ssize / dsize;
    out.resize(dsize);
    for (int d = 0; d < dsize; d++) {
        float f = (float)((d + 0.5) * scale - 0.5);
        int s = (int)std::floor(f);
        f -= (float)s;
        if (s < 0) {
            s = 0;
            f = 0.f;
        }
        if (s >= ssize - 1) {
            s = ssize - 1;
            f = 0.f;
        }
        int4 t;
        t.x = s;
        t.y = std::min(s + 1, ssize - 1);
        t.z = (short)std::lrintf((1.f - f) * 2048.f);
        t.w = (short)std::lrintf(f * 2048.f);
        out[d] = t;
    }
}

static inline int round_up(int v, int m) { return (v + m - 1) / m * m; }

// What FM_YOLO_F16 adds to plan(): which convolutions store f32 for a head, the padded sizes, and the weights'
// range.  No HIP call.
static int plan16(fm_yolo* h, const fm_yolo_desc* d) {
    const int nl = (int)h->L.size();
    for (int i = 0; i < nl; i++) {
        Layer& l = h->L[i];
        l.Cp = round_up(l.C, 8);
        if (l.d.kind != FM_YOLO_CONV) continue;
        l.K16 = l.d.size * l.d.size * round_up(l.Cin, 8);
        l.Kpad16 = round_up(l.K16, BK16);
        l.Mpad16 = round_up(l.C, 128);
        const float* w = d->weights + l.d.weight_ofs;
        const long long nw = (long long)l.K * l.C;
        for (long long k = 0; k < nw; k++)
            if (!(std::fabs(w[k]) < 65520.f))  // rounds to an f16 infinity (or is none)
                return fm::failf(&h->err, FM_ENOTSUP, "layer %d: weight %lld (%g) is not finite in f16", i, k, (double)w[k]);
    }
    for (int i = 0; i < nl; i++) {
        if (h->L[i].d.kind != FM_YOLO_HEAD) continue;
        if (h->L[i - 1].d.kind != FM_YOLO_CONV)
            return fm::failf(&h->err, FM_ENOTSUP, "layer %d: in f16 a head reads a convolution's f32 output, layer %d is none", i, i - 1);
        h->L[i - 1].f32_out = true;
    }
    // a head's tensor is f32 and NCHW: nothing but the head reads it
    for (int i = 0; i < nl; i++) {
        const Layer& l = h->L[i];
        int src[2] = {-1, -1};
        if (l.d.kind == FM_YOLO_ROUTE) {
            src[0] = l.d.from[0];
            src[1] = l.d.from[1];
        } else if (l.d.kind != FM_YOLO_HEAD) {
            src[0] = i - 1;
            if (l.d.kind == FM_YOLO_SHORTCUT) src[1] = l.d.from[0];
        }
        for (int s : src)
            if (s >= 0 && (h->L[s].f32_out || h->L[s].d.kind == FM_YOLO_HEAD))
                return fm::failf(&h->err, FM_ENOTSUP, "layer %d: in f16 only a head reads layer %d, a head's f32 tensor", i, s);
    }
    return FM_OK;
}

// Shapes, aliasing and every consistency check: no HIP call.
static int plan(fm_yolo* h, const fm_yolo_desc* d) {
    if (!d->layers || d->n_layers < 1) return fm::failf(&h->err, FM_EINVAL, "no layers");
    if (d->net_w < 1 || d->net_h < 1 || d->channels < 1 || d->classes < 0 || d->max_frames < 1)
        return fm::failf(&h->err, FM_EINVAL, "net_w, net_h, channels and max_frames must be >= 1, classes >= 0");
    if (!(d->zero_thresh >= 0.f && d->zero_thresh < 1.f)) return fm::failf(&h->err, FM_EINVAL, "zero_thresh outside [0, 1)");
    if (d->n_weights < 0 || d->n_biases < 0 || d->n_anchors < 0 || (d->n_weights && !d->weights) ||
        (d->n_biases && !d->biases) || (d->n_anchors && !d->anchors))
        return fm::failf(&h->err, FM_EINVAL, "null weights, biases or anchors");
    h->channels = d->channels;
    h->net_w = d->net_w;
    h->net_h = d->net_h;
    h->classes = d->classes;
    h->max_frames = d->max_frames;
    h->zero_thresh = d->zero_thresh;
    h->L.resize(d->n_layers);
    const long long lim = (1ll << 31) - 1;
    if ((long long)d->max_frames * d->channels * d->net_h * d->net_w > lim)
        return fm::failf(&h->err, FM_EINVAL, "network input of %d frames exceeds 2^31 elements", d->max_frames);
    for (int i = 0; i < d->n_layers; i++) {
        Layer& l = h->L[i];
        l.d = d->layers[i];
        const fm_yolo_layer& q = l.d;
        l.Cin = i ? h->L[i - 1].C : d->channels;
        l.Hin = i ? h->L[i - 1].H : d->net_h;
        l.Win = i ? h->L[i - 1].W : d->net_w;
        switch (q.kind) {
        case FM_YOLO_CONV: {
            if (q.filters < 1 || (q.size != 1 && q.size != 3) || (q.stride != 1 && q.stride != 2) || q.pad < 0 ||
                q.pad > q.size / 2 || (q.leaky != 0 && q.leaky != 1))
                return fm::failf(&h->err, FM_EINVAL, "layer %d: convolution filters=%d size=%d stride=%d pad=%d leaky=%d", i,
                             q.filters, q.size, q.stride, q.pad, q.leaky);
            const long long K = (long long)l.Cin * q.size * q.size;
            if (q.weight_ofs < 0 || q.weight_ofs + K * q.filters > d->n_weights || q.bias_ofs < 0 ||
                q.bias_ofs + q.filters > d->n_biases || K > (1 << 24))
                return fm::failf(&h->err, FM_EINVAL, "layer %d: %d x %lld weights do not lie inside the arrays", i, q.filters, K);
            l.C = q.filters;
            l.H = (l.Hin + 2 * q.pad - q.size) / q.stride + 1;
            l.W = (l.Win + 2 * q.pad - q.size) / q.stride + 1;
            l.K = (int)K;
            l.Kpad = (l.K + BK - 1) / BK * BK;
            l.WM = q.filters <= 32 ? 1 : 2;
            l.Mpad = (q.filters + 32 * l.WM - 1) / (32 * l.WM) * (32 * l.WM);
            break;
        }
        case FM_YOLO_MAXPOOL:
            if (q.size != 2 || (q.stride != 1 && q.stride != 2))
                return fm::failf(&h->err, FM_EINVAL, "layer %d: maxpool size=%d stride=%d", i, q.size, q.stride);
            l.C = l.Cin;
            l.H = q.stride == 1 ? l.Hin : (l.Hin + 1) / 2;
            l.W = q.stride == 1 ? l.Win : (l.Win + 1) / 2;
            break;
        case FM_YOLO_UPSAMPLE:
            if (q.stride != 2) return fm::failf(&h->err, FM_EINVAL, "layer %d: upsample stride=%d", i, q.stride);
            l.C = l.Cin;
            l.H = 2 * l.Hin;
            l.W = 2 * l.Win;
            break;
        case FM_YOLO_ROUTE: {
            const int a = q.from[0], b = q.from[1];
            if (a < 0 || a >= i || b < -1 || b >= i)
                return fm::failf(&h->err, FM_EINVAL, "layer %d: route to layers %d, %d (only earlier layers)", i, a, b);
            l.C = h->L[a].C + (b >= 0 ? h->L[b].C : 0);
            l.H = h->L[a].H;
            l.W = h->L[a].W;
            if (b >= 0 && (h->L[b].H != l.H || h->L[b].W != l.W))
                return fm::failf(&h->err, FM_EINVAL, "layer %d: route joins %dx%d with %dx%d", i, l.W, l.H, h->L[b].W, h->L[b].H);
            break;
        }
        case FM_YOLO_SHORTCUT: {
            const int a = q.from[0];
            if (i == 0 || a < 0 || a >= i)
                return fm::failf(&h->err, FM_EINVAL, "layer %d: shortcut from layer %d (only earlier layers)", i, a);
            if (h->L[a].C != l.Cin || h->L[a].H != l.Hin || h->L[a].W != l.Win)
                return fm::failf(&h->err, FM_EINVAL, "layer %d: shortcut adds %dx%dx%d to %dx%dx%d", i, h->L[a].C, h->L[a].H,
                             h->L[a].W, l.Cin, l.Hin, l.Win);
            l.C = l.Cin;
            l.H = l.Hin;
            l.W = l.Win;
            break;
        }
        case FM_YOLO_HEAD:
            if (i == 0) return fm::failf(&h->err, FM_EINVAL, "layer 0: a head needs a layer before it");
            if (d->classes < 1) return fm::failf(&h->err, FM_EINVAL, "layer %d: a head needs classes >= 1", i);
            if (q.n_mask < 1 || q.anchor_ofs < 0 || (long long)q.anchor_ofs + q.n_mask > d->n_anchors)
                return fm::failf(&h->err, FM_EINVAL, "layer %d: head anchors %d..%d outside the %d given", i, q.anchor_ofs,
                             q.anchor_ofs + q.n_mask, d->n_anchors);
            if (l.Cin != q.n_mask * (d->classes + 5))
                return fm::failf(&h->err, FM_EINVAL, "layer %d: head with %d input channels, len(mask) * (classes + 5) = %d", i,
                             l.Cin, q.n_mask * (d->classes + 5));
            l.C = l.Cin;
            l.H = l.Hin;
            l.W = l.Win;
            h->heads.push_back(i);
            if ((long long)h->total_rows + (long long)q.n_mask * l.H * l.W > (1 << 24))
                return fm::failf(&h->err, FM_EINVAL, "more than 2^24 candidate rows");
            h->total_rows += q.n_mask * l.H * l.W;
            break;
        default:
            return fm::failf(&h->err, FM_EINVAL, "layer %d: unknown kind %d", i, q.kind);
        }
        if (l.H < 1 || l.W < 1) return fm::failf(&h->err, FM_EINVAL, "layer %d: empty output %dx%d", i, l.W, l.H);
        if ((long long)d->max_frames * l.C * l.H * l.W > lim)
            return fm::failf(&h->err, FM_EINVAL, "layer %d: %d frames of %dx%dx%d exceed 2^31 elements", i, d->max_frames, l.C,
                         l.H, l.W);
    }
    if (h->precision == FM_YOLO_F16) {
        if (int rc = plan16(h, d)) return rc;
    }
    // a route of two layers that write (not views, not yet placed elsewhere) takes them in place; in f16 the
    // second one's channel offset has to be a multiple of 8 (the 16-byte accesses), else the copy kernel serves
    for (int i = 0; i < d->n_layers; i++) {
        Layer& l = h->L[i];
        if (l.d.kind != FM_YOLO_ROUTE || l.d.from[1] < 0 || l.d.from[0] == l.d.from[1]) continue;
        bool ok = true;
        for (int s = 0; s < 2; s++) {
            const Layer& src = h->L[l.d.from[s]];
            ok = ok && src.alias < 0 && src.d.kind != FM_YOLO_ROUTE && src.d.kind != FM_YOLO_HEAD;
        }
        if (h->precision == FM_YOLO_F16 && h->L[l.d.from[0]].C % 8 != 0) ok = false;
        if (!ok) continue;
        l.in_place = true;
        h->L[l.d.from[0]].alias = i;
        h->L[l.d.from[0]].alias_c = 0;
        h->L[l.d.from[1]].alias = i;
        h->L[l.d.from[1]].alias_c = h->L[l.d.from[0]].C;
    }
    return FM_OK;
}

static View input_of(fm_yolo* h, int i) {
    if (i == 0) return View{h->d_blob, (size_t)h->channels * h->net_h * h->net_w};
    return h->L[i - 1].v;
}

static View16 input16_of(fm_yolo* h, int i) {
    if (i == 0) return View16{h->d_blob16, round_up(h->channels, 8)};
    return h->L[i - 1].v16;
}

template <int SIZE>
static void launch_conv16(const Conv16Args& a, hipStream_t st) {
    const auto blocks = [&](int bm, int bn) { return dim3((a.N + bn - 1) / bn, (a.Cout + bm - 1) / bm); };
    const dim3 big = blocks(128, 128);
    if (a.Cout <= 32) k_conv16<SIZE, 1, 1, 1><<<blocks(32, 128), 256, 0, st>>>(a);
    else if (a.Cout >= 128 && (long long)big.x * big.y >= 512) k_conv16<SIZE, 2, 2, 2><<<big, 256, 0, st>>>(a);
    else k_conv16<SIZE, 2, 1, 1><<<blocks(64, 64), 256, 0, st>>>(a);
}

// run_layers in FM_YOLO_F16, on the n frames in d_blob16
static int run_layers16(fm_yolo* h, int n) {
    for (size_t i = 0; i < h->L.size(); i++) {
        Layer& l = h->L[i];
        const View16 in = input16_of(h, (int)i);
        const long long px = (long long)n * l.H * l.W;
        // 8 channels a thread where every view involved starts and ends on a multiple of 8
        const auto go = [&](int C, auto k8, auto k1) {
            if (C % 8 == 0) k8(px * (C / 8));
            else k1(px * C);
        };
        switch (l.d.kind) {
        case FM_YOLO_CONV: {
            Conv16Args a;
            a.in = in.p;
            a.in_ps = in.ps;
            a.out = l.f32_out ? nullptr : l.v16.p;
            a.out_ps = l.v16.ps;
            a.out32 = l.f32_out ? l.v.p : nullptr;
            a.out32_bs = l.v.bs;
            a.wp = l.wp16;
            a.bias = l.bias;
            a.Cp = round_up(l.Cin, 8);
            a.H = l.Hin;
            a.W = l.Win;
            a.Cout = l.C;
            a.Ho = l.H;
            a.Wo = l.W;
            a.stride = l.d.stride;
            a.pad = l.d.pad;
            a.leaky = l.d.leaky;
            a.Kpad = l.Kpad16;
            a.N = (int)px;
            if (l.d.size == 1) launch_conv16<1>(a, h->stream);
            else launch_conv16<3>(a, h->stream);
            break;
        }
        case FM_YOLO_MAXPOOL:
            go(l.C,
               [&](long long t) { k_maxpool16<8><<<nblk(t), 256, 0, h->stream>>>(in, l.v16, l.C, l.Hin, l.Win, l.H, l.W, l.d.stride, t); },
               [&](long long t) { k_maxpool16<1><<<nblk(t), 256, 0, h->stream>>>(in, l.v16, l.C, l.Hin, l.Win, l.H, l.W, l.d.stride, t); });
            break;
        case FM_YOLO_UPSAMPLE:
            go(l.C, [&](long long t) { k_upsample16<8><<<nblk(t), 256, 0, h->stream>>>(in, l.v16, l.C, l.Hin, l.Win, t); },
               [&](long long t) { k_upsample16<1><<<nblk(t), 256, 0, h->stream>>>(in, l.v16, l.C, l.Hin, l.Win, t); });
            break;
        case FM_YOLO_SHORTCUT: {
            const View16 q = h->L[l.d.from[0]].v16;
            go(l.C, [&](long long t) { k_shortcut16<8><<<nblk(t), 256, 0, h->stream>>>(in, q, l.v16, l.C, t); },
               [&](long long t) { k_shortcut16<1><<<nblk(t), 256, 0, h->stream>>>(in, q, l.v16, l.C, t); });
            break;
        }
        case FM_YOLO_ROUTE: {
            if (l.in_place) break;
            int coff = 0;
            for (int s = 0; s < 2 && l.d.from[s] >= 0; s++) {
                const Layer& src = h->L[l.d.from[s]];
                const View16 dst{l.v16.p + coff, l.v16.ps};
                if (coff % 8 == 0 && src.C % 8 == 0)
                    k_copy16<8><<<nblk(px * (src.C / 8)), 256, 0, h->stream>>>(src.v16, dst, src.C, px * (src.C / 8));
                else  // an offset or a width off the 16 bytes: one channel a thread
                    k_copy16<1><<<nblk(px * src.C), 256, 0, h->stream>>>(src.v16, dst, src.C, px * src.C);
                coff += src.C;
            }
            break;
        }
        default:
            break;  // a head decodes its convolution's f32 tensor where it lies
        }
        FM_HIP_TRY(&h->err, hipGetLastError());
    }
    return FM_OK;
}

// The network on the n frames in d_blob: every launch on the detector's stream.
static int run_layers(fm_yolo* h, int n) {
    if (h->precision == FM_YOLO_F16) return run_layers16(h, n);
    for (size_t i = 0; i < h->L.size(); i++) {
        Layer& l = h->L[i];
        const View in = input_of(h, (int)i);
        const long long per = (long long)l.C * l.H * l.W, total = per * n;
        switch (l.d.kind) {
        case FM_YOLO_CONV: {
            ConvArgs a;
            a.in = in.p;
            a.in_bs = in.bs;
            a.out = l.v.p;
            a.out_bs = l.v.bs;
            a.wp = l.wp;
            a.bias = l.bias;
            a.Cin = l.Cin;
            a.H = l.Hin;
            a.W = l.Win;
            a.Cout = l.C;
            a.Ho = l.H;
            a.Wo = l.W;
            a.stride = l.d.stride;
            a.pad = l.d.pad;
            a.leaky = l.d.leaky;
            a.K = l.K;
            a.Kpad = l.Kpad;
            a.Mpad = l.Mpad;
            a.N = n * l.H * l.W;
            const int BM = 32 * l.WM, BN = 32 * (4 / l.WM);
            const dim3 grid((a.N + BN - 1) / BN, l.Mpad / BM);
            if (l.d.size == 1 && l.WM == 1) k_conv<1, 1><<<grid, 256, 0, h->stream>>>(a);
            else if (l.d.size == 1) k_conv<1, 2><<<grid, 256, 0, h->stream>>>(a);
            else if (l.WM == 1) k_conv<3, 1><<<grid, 256, 0, h->stream>>>(a);
            else k_conv<3, 2><<<grid, 256, 0, h->stream>>>(a);
            break;
        }
        case FM_YOLO_MAXPOOL:
            k_maxpool<<<nblk(total), 256, 0, h->stream>>>(in.p, in.bs, l.v.p, l.v.bs, l.C, l.Hin, l.Win, l.H, l.W,
                                                          l.d.stride, total);
            break;
        case FM_YOLO_UPSAMPLE:
            k_upsample<<<nblk(total), 256, 0, h->stream>>>(in.p, in.bs, l.v.p, l.v.bs, l.C, l.Hin, l.Win, total);
            break;
        case FM_YOLO_SHORTCUT: {
            const View q = h->L[l.d.from[0]].v;
            k_shortcut<<<nblk(total), 256, 0, h->stream>>>(in.p, in.bs, q.p, q.bs, l.v.p, l.v.bs, per, total);
            break;
        }
        case FM_YOLO_ROUTE: {
            if (l.in_place) break;
            size_t coff = 0;
            for (int s = 0; s < 2 && l.d.from[s] >= 0; s++) {
                const Layer& src = h->L[l.d.from[s]];
                const long long sper = (long long)src.C * src.H * src.W;
                k_copy<<<nblk(sper * n), 256, 0, h->stream>>>(src.v.p, src.v.bs, l.v.p + coff, l.v.bs, sper, sper * n);
                coff += (size_t)sper;
            }
            break;
        }
        default:
            break;  // a head decodes its input where it lies
        }
        FM_HIP_TRY(&h->err, hipGetLastError());
    }
    return FM_OK;
}

static int run_decode(fm_yolo* h, int n, float confidence) {
    FM_HIP_TRY(&h->err, hipMemsetAsync(h->d_cnt, 0, (size_t)h->max_frames * sizeof(int), h->stream));
    for (size_t k = 0; k < h->heads.size(); k++) {
        const Layer& l = h->L[h->heads[k]];
        const long long total = (long long)n * l.d.n_mask * l.H * l.W;
        k_yolo_decode<<<nblk(total), 256, 0, h->stream>>>(l.v.p, l.v.bs, l.H, l.W, l.d.n_mask, h->classes,
                                                          h->d_anchors + 2 * l.d.anchor_ofs, (float)h->net_w,
                                                          (float)h->net_h, h->zero_thresh, confidence, (int)k,
                                                          h->d_cand, h->total_rows, h->d_cnt, total);
        FM_HIP_TRY(&h->err, hipGetLastError());
    }
    return FM_OK;
}

// Waits for the stream, then copies each frame's candidates out sorted by (head, row).
static int collect(fm_yolo* h, int n, float* cand, int cap, int32_t* counts) {
    std::vector<int> cnt(n);
    FM_HIP_TRY(&h->err, hipMemcpyAsync(cnt.data(), h->d_cnt, (size_t)n * sizeof(int), hipMemcpyDeviceToHost, h->stream));
    FM_HIP_TRY(&h->err, hipStreamSynchronize(h->stream));
    std::vector<float> rows;
    std::vector<int> order;
    for (int b = 0; b < n; b++) {
        const int c = std::min(cnt[b], h->total_rows);
        counts[b] = c;
        if (!c) continue;
        rows.resize((size_t)c * FM_YOLO_CAND);
        FM_HIP_TRY(&h->err, hipMemcpy(rows.data(), h->d_cand + (size_t)b * h->total_rows * FM_YOLO_CAND,
                        rows.size() * sizeof(float), hipMemcpyDeviceToHost));
        order.resize(c);
        for (int i = 0; i < c; i++) order[i] = i;
        std::sort(order.begin(), order.end(), [&](int p, int q) {
            const float *x = &rows[(size_t)p * FM_YOLO_CAND], *y = &rows[(size_t)q * FM_YOLO_CAND];
            return x[0] != y[0] ? x[0] < y[0] : x[1] < y[1];
        });
        for (int i = 0; i < c && i < cap; i++)
            std::memcpy(cand + ((size_t)b * cap + i) * FM_YOLO_CAND, &rows[(size_t)order[i] * FM_YOLO_CAND],
                        FM_YOLO_CAND * sizeof(float));
    }
    return FM_OK;
}

static void read_ms(fm_yolo* h, int first, int last) {
    for (int s = 0; s < 3; s++) h->ms[s] = 0.;
    for (int s = first; s < last; s++) {
        float t = 0.f;
        if (hipEventElapsedTime(&t, h->ev[s], h->ev[s + 1]) == hipSuccess) h->ms[s] = t;
    }
}

// The rest of fm_yolo_create in FM_YOLO_F16: activations as zeroed NHWC halves (the zeros are the channel
// padding, which no kernel writes anything else to), weights rounded once to f16 and packed [Mpad][Kpad] with
// k = (ky, kx, c) over the input's padded channels.
static int create16(fm_yolo* h, const fm_yolo_desc* d) {
    const size_t blob = (size_t)h->max_frames * h->net_h * h->net_w * round_up(h->channels, 8);
    FM_HIP_TRY(&h->err, h->d_blob16.reserve(blob));
    FM_HIP_TRY(&h->err, hipMemsetAsync(h->d_blob16, 0, blob * sizeof(_Float16), h->stream));  // (ahead of every kernel)
    for (auto& l : h->L) {
        if (l.alias >= 0 || l.d.kind == FM_YOLO_HEAD) continue;
        if (l.f32_out) {
            const size_t per = (size_t)l.C * l.H * l.W;
            FM_HIP_TRY(&h->err, l.buf.reserve((size_t)h->max_frames * per));
            l.v = View{l.buf, per};
            continue;
        }
        const size_t count = (size_t)h->max_frames * l.H * l.W * l.Cp;
        FM_HIP_TRY(&h->err, l.buf16.reserve(count));
        FM_HIP_TRY(&h->err, hipMemsetAsync(l.buf16, 0, count * sizeof(_Float16), h->stream));
        l.v16 = View16{l.buf16, l.Cp};
    }
    for (size_t i = 0; i < h->L.size(); i++) {
        Layer& l = h->L[i];
        if (l.alias >= 0) {
            const Layer& r = h->L[l.alias];
            l.v16 = View16{r.buf16 + l.alias_c, r.Cp};
        } else if (l.d.kind == FM_YOLO_HEAD) {
            l.v = h->L[i - 1].v;
        }
    }
    std::vector<_Float16> wp;
    for (auto& l : h->L) {
        if (l.d.kind != FM_YOLO_CONV) continue;
        wp.assign((size_t)l.Mpad16 * l.Kpad16, (_Float16)0.f);
        const float* w = d->weights + l.d.weight_ofs;
        const int s2 = l.d.size * l.d.size, cp = round_up(l.Cin, 8);
        for (int m = 0; m < l.C; m++)
            for (int c = 0; c < l.Cin; c++)
                for (int t = 0; t < s2; t++)
                    wp[(size_t)m * l.Kpad16 + (size_t)t * cp + c] = (_Float16)w[((size_t)m * l.Cin + c) * s2 + t];
        FM_HIP_TRY(&h->err, l.wp16.reserve(wp.size()));
        FM_HIP_TRY(&h->err, hipMemcpy(l.wp16, wp.data(), wp.size() * sizeof(_Float16), hipMemcpyHostToDevice));
        FM_HIP_TRY(&h->err, l.bias.reserve((size_t)l.C));
        FM_HIP_TRY(&h->err, hipMemcpy(l.bias, d->biases + l.d.bias_ofs, (size_t)l.C * sizeof(float), hipMemcpyHostToDevice));
    }
    return FM_OK;
}

extern "C" {

int fm_yolo_create(int device, const fm_yolo_desc* d, fm_yolo** out) {
    return fm_yolo_create_precision(device, d, FM_YOLO_F32, out);
}

int fm_yolo_precision(const fm_yolo* h) { return h ? h->precision : FM_EINVAL; }

int fm_yolo_create_precision(int device, const fm_yolo_desc* d, int precision, fm_yolo** out) {
    if (!out) return FM_EINVAL;
    *out = nullptr;
    fm_yolo* h = new (std::nothrow) fm_yolo();
    if (!h) return FM_ENOMEM;
    *out = h;
    h->device = device;
    if (precision != FM_YOLO_F32 && precision != FM_YOLO_F16)
        return fm::failf(&h->err, FM_EINVAL, "precision %d (FM_YOLO_F32 or FM_YOLO_F16)", precision);
    h->precision = precision;
    if (!d) return fm::failf(&h->err, FM_EINVAL, "null description");
    if (device < 0) return fm::failf(&h->err, FM_EINVAL, "device %d", device);
    if (int rc = plan(h, d)) {
        h->L.clear();
        return rc;
    }
    int ndev = 0;
    FM_HIP_TRY(&h->err, hipGetDeviceCount(&ndev));
    if (device >= ndev) return fm::failf(&h->err, FM_EINVAL, "device %d of %d", device, ndev);
    FM_HIP_TRY(&h->err, hipSetDevice(device));
    FM_HIP_TRY(&h->err, hipStreamCreateWithFlags(h->stream.put(), hipStreamNonBlocking));
    for (auto& e : h->ev) FM_HIP_TRY(&h->err, hipEventCreate(e.put()));
    const size_t blob = (size_t)h->channels * h->net_h * h->net_w;
    FM_HIP_TRY(&h->err, h->d_blob.reserve((size_t)h->max_frames * blob));
    FM_HIP_TRY(&h->err, h->d_anchors.reserve(2 * (size_t)d->n_anchors));
    if (d->n_anchors)
        FM_HIP_TRY(&h->err, hipMemcpy(h->d_anchors, d->anchors, 2 * (size_t)d->n_anchors * sizeof(float), hipMemcpyHostToDevice));
    float lut[256];
    for (int v = 0; v < 256; v++) lut[v] = (float)((double)v * 0.00392);
    FM_HIP_TRY(&h->err, h->d_lut.reserve(256));
    FM_HIP_TRY(&h->err, hipMemcpy(h->d_lut, lut, sizeof lut, hipMemcpyHostToDevice));
    FM_HIP_TRY(&h->err, h->d_cnt.reserve((size_t)h->max_frames));
    FM_HIP_TRY(&h->err, h->d_cand.reserve(std::max<size_t>((size_t)h->max_frames * h->total_rows, 1) * FM_YOLO_CAND));
    if (precision == FM_YOLO_F16) return create16(h, d);
    // activations: a layer placed in a route's buffer and a head own none
    for (auto& l : h->L) {
        if (l.alias >= 0 || l.d.kind == FM_YOLO_HEAD) continue;
        const size_t per = (size_t)l.C * l.H * l.W;
        FM_HIP_TRY(&h->err, l.buf.reserve((size_t)h->max_frames * per));
        l.v = View{l.buf, per};
    }
    for (size_t i = 0; i < h->L.size(); i++) {
        Layer& l = h->L[i];
        if (l.alias >= 0) {
            const Layer& r = h->L[l.alias];
            l.v = View{r.buf + (size_t)l.alias_c * l.H * l.W, r.v.bs};
        } else if (l.d.kind == FM_YOLO_HEAD) {
            l.v = h->L[i - 1].v;
        }
    }
    // weights: [Cout][K] -> [Kpad][Mpad], zero padded, so that a tile's rows load contiguously
    std::vector<float> wp;
    for (auto& l : h->L) {
        if (l.d.kind != FM_YOLO_CONV) continue;
        wp.assign((size_t)l.Kpad * l.Mpad, 0.f);
        const float* w = d->weights + l.d.weight_ofs;
        for (int m = 0; m < l.C; m++)
            for (int k = 0; k < l.K; k++) wp[(size_t)k * l.Mpad + m] = w[(size_t)m * l.K + k];
        FM_HIP_TRY(&h->err, l.wp.reserve(wp.size()));
        FM_HIP_TRY(&h->err, hipMemcpy(l.wp, wp.data(), wp.size() * sizeof(float), hipMemcpyHostToDevice));
        FM_HIP_TRY(&h->err, l.bias.reserve((size_t)l.C));
        FM_HIP_TRY(&h->err, hipMemcpy(l.bias, d->biases + l.d.bias_ofs, (size_t)l.C * sizeof(float), hipMemcpyHostToDevice));
    }
    return FM_OK;
}

void fm_yolo_destroy(fm_yolo* h) { delete h; }

const char* fm_yolo_last_error(const fm_yolo* h) { return h ? h->err.c_str() : "null detector"; }

int fm_yolo_set_roi_upscale(fm_yolo* h, int on) {
    if (!h) return FM_EINVAL;
    h->roi.allow_upscale(on != 0);
    return FM_OK;
}

int fm_yolo_layer_shape(const fm_yolo* h, int layer, int* c, int* hh, int* w, int* rows) {
    if (!h || h->L.empty() || layer < -1 || layer >= (int)h->L.size()) return FM_EINVAL;
    if (c) *c = layer < 0 ? h->channels : h->L[layer].C;
    if (hh) *hh = layer < 0 ? h->net_h : h->L[layer].H;
    if (w) *w = layer < 0 ? h->net_w : h->L[layer].W;
    if (rows) *rows = h->total_rows;
    return FM_OK;
}

int fm_yolo_route_in_place(const fm_yolo* h, int layer) {
    if (!h || layer < 0 || layer >= (int)h->L.size() || h->L[layer].d.kind != FM_YOLO_ROUTE) return FM_EINVAL;
    return h->L[layer].in_place ? 1 : 0;
}

int fm_yolo_forward(fm_yolo* h, const float* blob, int n) {
    if (!h || !h->d_blob) return FM_EINVAL;
    if (!blob || n < 1) return fm::failf(&h->err, FM_EINVAL, "bad arguments (blob, n >= 1)");
    if (n > h->max_frames) return fm::failf(&h->err, FM_EINVAL, "%d frames, the detector was created for %d", n, h->max_frames);
    FM_HIP_TRY(&h->err, hipSetDevice(h->device));
    const size_t per = (size_t)h->channels * h->net_h * h->net_w;
    FM_HIP_TRY(&h->err, hipMemcpyAsync(h->d_blob, blob, (size_t)n * per * sizeof(float), hipMemcpyHostToDevice, h->stream));
    if (h->precision == FM_YOLO_F16) {
        const int cp = round_up(h->channels, 8), hw = h->net_h * h->net_w;
        const long long total = (long long)n * hw * cp;
        k_pack16<<<nblk(total), 256, 0, h->stream>>>(h->d_blob, h->d_blob16, h->channels, cp, hw, total);
        FM_HIP_TRY(&h->err, hipGetLastError());
    }
    FM_HIP_TRY(&h->err, hipEventRecord(h->ev[1], h->stream));
    if (int rc = run_layers(h, n)) return rc;
    FM_HIP_TRY(&h->err, hipEventRecord(h->ev[2], h->stream));
    FM_HIP_TRY(&h->err, hipStreamSynchronize(h->stream));
    h->last_n = n;
    read_ms(h, 1, 2);
    return FM_OK;
}

int fm_yolo_decode(fm_yolo* h, int n, float confidence, float* cand, int cap, int32_t* counts) {
    if (!h || !h->d_blob) return FM_EINVAL;
    if (n < 1 || cap < 0 || !counts || (cap > 0 && !cand)) return fm::failf(&h->err, FM_EINVAL, "bad arguments (counts[n], cand[n][cap][9])");
    if (n != h->last_n) return fm::failf(&h->err, FM_ESTATE, "%d frames asked for, the last call ran %d", n, h->last_n);
    FM_HIP_TRY(&h->err, hipSetDevice(h->device));
    FM_HIP_TRY(&h->err, hipEventRecord(h->ev[2], h->stream));
    if (int rc = run_decode(h, n, confidence)) return rc;
    FM_HIP_TRY(&h->err, hipEventRecord(h->ev[3], h->stream));
    if (int rc = collect(h, n, cand, cap, counts)) return rc;
    read_ms(h, 2, 3);
    return FM_OK;
}

int fm_yolo_layer_output(fm_yolo* h, int layer, float* out, size_t cap) {
    if (!h || !h->d_blob) return FM_EINVAL;
    if (layer < -1 || layer >= (int)h->L.size()) return fm::failf(&h->err, FM_EINVAL, "layer %d of %zu", layer, h->L.size());
    if (h->last_n < 1) return fm::failf(&h->err, FM_ESTATE, "no call yet");
    const View v = layer < 0 ? input_of(h, 0) : h->L[layer].v;
    const size_t per = layer < 0 ? (size_t)h->channels * h->net_h * h->net_w
                                 : (size_t)h->L[layer].C * h->L[layer].H * h->L[layer].W;
    const size_t total = per * h->last_n;
    if (!out || cap < total) return fm::failf(&h->err, FM_EINVAL, "layer %d holds %zu floats, room for %zu", layer, total, cap);
    FM_HIP_TRY(&h->err, hipSetDevice(h->device));
    if (h->precision == FM_YOLO_F16 && !(layer >= 0 && (h->L[layer].f32_out || h->L[layer].d.kind == FM_YOLO_HEAD))) {
        const View16 v16 = layer < 0 ? input16_of(h, 0) : h->L[layer].v16;
        const int C = layer < 0 ? h->channels : h->L[layer].C;
        FM_HIP_TRY(&h->err, h->d_stage.reserve(total));
        k_unpack16<<<nblk((long long)total), 256, 0, h->stream>>>(v16, h->d_stage, C, (int)(per / C), (long long)total);
        FM_HIP_TRY(&h->err, hipGetLastError());
        FM_HIP_TRY(&h->err, hipStreamSynchronize(h->stream));
        FM_HIP_TRY(&h->err, hipMemcpy(out, h->d_stage, total * sizeof(float), hipMemcpyDeviceToHost));
        return (int)total;
    }
    for (int b = 0; b < h->last_n; b++)
        FM_HIP_TRY(&h->err, hipMemcpy(out + (size_t)b * per, v.p + (size_t)b * v.bs, per * sizeof(float), hipMemcpyDeviceToHost));
    return (int)total;
}

double fm_yolo_last_ms(const fm_yolo* h, double* stages) {
    if (!h) return 0.;
    if (stages)
        for (int s = 0; s < 3; s++) stages[s] = h->ms[s];
    return h->ms[0] + h->ms[1] + h->ms[2];
}

}  // extern "C"

// frames -> ROI (INTER_AREA, as fm_haar_detect_frames) -> blob -> network -> decode
static int detect_impl(fm_yolo* h, const uint8_t* frames, const uint8_t* const* list, int n, int H, int W,
                       int on_device, int roi_w, float confidence, float* cand, int cap, int32_t* counts,
                       int* roi_h_out) {
    if (!h || !h->d_blob) return FM_EINVAL;
    if ((!frames && !list) || n < 1 || H < 1 || W < 1 || roi_w < 1 || cap < 0 || !counts || (cap > 0 && !cand))
        return fm::failf(&h->err, FM_EINVAL, "bad arguments (n >= 1, frame and ROI sizes >= 1, counts[n], cand[n][cap][9])");
    if (n > h->max_frames) return fm::failf(&h->err, FM_EINVAL, "%d frames, the detector was created for %d", n, h->max_frames);
    if (h->channels != 3) return fm::failf(&h->err, FM_EINVAL, "a network of %d input channels takes no BGR frames", h->channels);
    FM_HIP_TRY(&h->err, hipSetDevice(h->device));
    FM_HIP_TRY(&h->err, hipEventRecord(h->ev[0], h->stream));
    const uint8_t* roi = nullptr;
    int rh = 0, rc = h->roi.run(&h->err, h->stream, frames, list, n, H, W, on_device != 0, roi_w, &roi, &rh);
    if (roi_h_out) *roi_h_out = rh;
    if (rc) return rc;
    const int rw = roi_w;
    if (h->lin_key[0] != rw || h->lin_key[1] != rh) {
        std::vector<int4> xt, yt;
        linear8u_taps(rw, h->net_w, xt);
        linear8u_taps(rh, h->net_h, yt);
        FM_HIP_TRY(&h->err, hipStreamSynchronize(h->stream));
        h->lin_key[0] = 0;
        FM_HIP_TRY(&h->err, h->d_xt.reserve(xt.size()));
        FM_HIP_TRY(&h->err, h->d_yt.reserve(yt.size()));
        FM_HIP_TRY(&h->err, hipMemcpy(h->d_xt, xt.data(), xt.size() * sizeof(int4), hipMemcpyHostToDevice));
        FM_HIP_TRY(&h->err, hipMemcpy(h->d_yt, yt.data(), yt.size() * sizeof(int4), hipMemcpyHostToDevice));
        h->lin_key[0] = rw;
        h->lin_key[1] = rh;
    }
    const long long total = (long long)n * h->net_h * h->net_w;
    if (h->precision == FM_YOLO_F16)
        k_yolo_blob16<<<nblk(total), 256, 0, h->stream>>>(roi, rh, rw, h->d_xt, h->d_yt, h->d_lut, h->d_blob16, h->net_h,
                                                          h->net_w, total);
    else
        k_yolo_blob<<<nblk(total), 256, 0, h->stream>>>(roi, rh, rw, h->d_xt, h->d_yt, h->d_lut, h->d_blob, h->net_h,
                                                        h->net_w, total);
    FM_HIP_TRY(&h->err, hipGetLastError());
    FM_HIP_TRY(&h->err, hipEventRecord(h->ev[1], h->stream));
    if ((rc = run_layers(h, n))) return rc;
    FM_HIP_TRY(&h->err, hipEventRecord(h->ev[2], h->stream));
    if ((rc = run_decode(h, n, confidence))) return rc;
    FM_HIP_TRY(&h->err, hipEventRecord(h->ev[3], h->stream));
    h->last_n = n;
    if ((rc = collect(h, n, cand, cap, counts))) return rc;
    read_ms(h, 0, 3);
    return FM_OK;
}

extern "C" {

int fm_yolo_detect_frames(fm_yolo* h, const uint8_t* frames, int n, int H, int W, int on_device, int roi_w,
                          float confidence, float* cand, int cap, int32_t* counts, int* roi_h_out) {
    if (!frames) return h ? fm::failf(&h->err, FM_EINVAL, "null frames") : FM_EINVAL;
    return detect_impl(h, frames, nullptr, n, H, W, on_device, roi_w, confidence, cand, cap, counts, roi_h_out);
}

int fm_yolo_detect_frame_list(fm_yolo* h, const uint8_t* const* frames, int n, int H, int W, int roi_w,
                              float confidence, float* cand, int cap, int32_t* counts, int* roi_h_out) {
    if (!frames) return h ? fm::failf(&h->err, FM_EINVAL, "null frame list") : FM_EINVAL;
    for (int i = 0; i < n; i++)
        if (!frames[i]) return fm::failf(&h->err, FM_EINVAL, "frame %d: null address", i);
    return detect_impl(h, nullptr, frames, n, H, W, 1, roi_w, confidence, cand, cap, counts, roi_h_out);
}

}  // extern "C"
