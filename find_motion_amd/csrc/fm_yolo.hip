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
// Everything is f32: the f32-input MFMA is a k-ordered fmaf chain, so a convolution output differs
// from exact arithmetic by at most (K + 3) * 2^-24 * (sum |w x| + |b|).
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
};

}  // namespace yolo
}  // namespace fm

using namespace fm::yolo;

struct fm_yolo {
    int device = 0;
    fm::Stream stream;  // (before the buffers used on it: they are released first)
    std::string err;
    int channels = 3, net_w = 0, net_h = 0, classes = 0, max_frames = 0;
    float zero_thresh = 0.f;
    std::vector<Layer> L;
    std::vector<int> heads;
    int total_rows = 0;
    fm::DevBuf<float> d_blob, d_anchors, d_lut, d_cand;
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
    // a route of two layers that write (not views, not yet placed elsewhere) takes them in place
    for (int i = 0; i < d->n_layers; i++) {
        Layer& l = h->L[i];
        if (l.d.kind != FM_YOLO_ROUTE || l.d.from[1] < 0 || l.d.from[0] == l.d.from[1]) continue;
        bool ok = true;
        for (int s = 0; s < 2; s++) {
            const Layer& src = h->L[l.d.from[s]];
            ok = ok && src.alias < 0 && src.d.kind != FM_YOLO_ROUTE && src.d.kind != FM_YOLO_HEAD;
        }
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

// The network on the n frames in d_blob: every launch on the detector's stream.
static int run_layers(fm_yolo* h, int n) {
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

extern "C" {

int fm_yolo_create(int device, const fm_yolo_desc* d, fm_yolo** out) {
    if (!out) return FM_EINVAL;
    *out = nullptr;
    fm_yolo* h = new (std::nothrow) fm_yolo();
    if (!h) return FM_ENOMEM;
    *out = h;
    h->device = device;
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
