// fm_rgb.hip — the per-pixel motion chain on the three colour channels (FM_FLAG_COLOUR_MOTION): the chain the
// reference would run without its cvtColor line (fm.py:493), which its author asks for at the top of
// find_motion.py ("think about r/g/b channel motion detection, instead of just grayscale").  A mover whose gray
// level equals the background's -- BGR (0, 0, 100) on (0, 51, 0), both gray 30 -- never reaches frame_delta on
// the gray chain; here every OpenCV call of the chain runs on the 3-channel work image:
//   GaussianBlur 494 per channel (the same 8-bit taps, REFLECT_101, (... + 2^15) >> 16), mask_off_areas 619-636
//   (BLACK: 0 in all three channels), absdiff(convertScaleAbs) 250 and accumulateWeighted 659 element-wise over
//   the interleaved [h][w][3] arrays (so their SIMD rules count n = 3 h w elements: the float path of
//   convertScaleAbs when n >= 16, the fma body up to n - n % 16 and the two-rounding scalar tail behind it, which
//   can split a pixel's channels), threshold 257 per channel; the three planes are ORed into the one plane that
//   findContours needs before the dilation (dilation commutes with OR).
//
// The decomposition of fm_small.hip / fm_wide.hip: only the f64 running average is sequential in time.
//
//   k_rgb_blur  every frame of the launch in parallel, one workgroup per (frame, 64 x 64 tile): the tile's BGR
//               bytes plus a k/2 halo (reflected at any distance) go to LDS once, a plane per channel; horizontal
//               taps per channel into u16 sums (<= 255 * 256), four taps per v_dot4_u32_u8 on the row's dwords,
//               the sums of two consecutive rows kept in one dword; vertical taps on those row pairs, two taps
//               per v_dot2_u32_u16 (fm_wide.hip's packed taps, one v_readlane a step), rounding, keep-mask; the
//               tile's blur bytes are transposed in LDS and stored column-major, 16 rows a store, to the scratch
//               [F][3][x][CS] (k_small_blur's layout per channel, CS = nty * 64).  It clears the tile's flags and,
//               in the last tile column, the bit words of the columns past the image.
//   k_rgb_scan  fm_scan.h's scan_frames (one wave per stream, image column and 64-row tile row, lane = row, the
//               frames in order) around three f64 backgrounds in registers; per frame three blur bytes, three
//               diffs, and (dB > t) | (dG > t) | (dR > t) is the lane's threshold bit.
//               The background is read and written interleaved, [S][h][w][3]: the ABI's layout.
//
// No workgroup waits on another, no index depends on data, and the flag ORs are the only atomics.
#include "fm_scan.h"

namespace fm {
namespace rgb {

constexpr int kMaxKsize = 49;  // Gaussian sizes of the colour path (k_fused's limit)
constexpr int BT = 256;   // k_rgb_blur threads
constexpr int LC = 10;    // k_rgb_blur: pixels a thread loads together
constexpr int OTS = 68;   // bytes between two columns of the transposed tile in LDS (17 dwords: 64 lanes that
                          // write one dword each to 64 columns meet 64 banks)

// the kernels' own arguments (FusedArgs stays as it is)
struct RgbArgs {
    const uint8_t* src;       // work-size BGR frames [T][S][h][w][3]
    const double* bg_in;      // [S][h][w][3] background before the launch
    double* bg_out;           // [S][h][w][3] background after it
    const uint8_t* keep;      // [S][h*w]
    const uint8_t* has_keep;  // [S]
    const uint8_t* init;      // [S] or nullptr: 1 => bg := blur at the launch's first frame
    Geom g;
    int ksize, thresh;
    double alpha, beta;
    long long acc_vec_end;    // 3hw - 3hw % 16: elements below it take accumulateWeighted's fma body
    int32_t coef[kMaxKsize];
};

typedef unsigned short u16x2_t __attribute__((ext_vector_type(2)));

// Geometry of k_rgb_blur's tile for radius R (K = 2R + 1 taps): TW rows and columns with the halo; a raw row
// holds 64 + 4 M4 bytes, M4 = ceil(K / 4) steps of four taps (the bytes past TW meet zero taps)
__host__ __device__ constexpr int tile_w(int R) { return 64 + 2 * R; }
__host__ __device__ constexpr int steps4(int R) { return (2 * R + 1 + 3) / 4; }
__host__ __device__ constexpr int row_bytes(int R) { return 64 + 4 * steps4(R); }
// LDS of k_rgb_blur: the BGR tile with its halo, a plane per channel, u8 [3][TW][row_bytes] (later the transposed
// blur bytes u8 [3][64][OTS]); the horizontal sums of two consecutive rows in one dword, u16 [3][TW / 2][64][2]
// (before them the reflected source offsets of the tile's columns and rows, int [2][TW])
__host__ __device__ constexpr int raw_bytes(int R) {
    const int raw = 3 * tile_w(R) * row_bytes(R), ot = 3 * 64 * OTS;
    return ((raw > ot ? raw : ot) + 15) & ~15;
}
__host__ __device__ constexpr int blur_lds_bytes(int R) {
    return raw_bytes(R) + 3 * (tile_w(R) / 2) * 64 * 4;
}
static_assert(blur_lds_bytes(kMaxKsize >> 1) <= 160 * 1024, "k_rgb_blur's tile does not fit the LDS");

__global__ __launch_bounds__(BT) void k_rgb_blur(RgbArgs a, uint8_t* __restrict__ cblur, int CS) {
    extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
    const Geom& gm = a.g;
    const int h = gm.h, w = gm.w, S = gm.S, K = a.ksize, R = K >> 1, TW = tile_w(R), RB = row_bytes(R), NP = TW / 2;
    const int tid = threadIdx.x;
    const int fl = blockIdx.x / gm.ntiles, tile = blockIdx.x - fl * gm.ntiles;
    const size_t f = (size_t)gm.t_begin * S + fl;  // frame of the batch (t * S + s)
    const int s = (int)(f % S);
    const int ty = tile / gm.ntx, tx = tile - ty * gm.ntx;
    const int x0 = tx * 64, y0 = ty * 64;
    uint8_t* raw = lds;
    uint32_t* H2 = reinterpret_cast<uint32_t*>(lds + raw_bytes(R));  // [3][NP][64]: H of rows 2p (low half), 2p + 1
    int* xi = reinterpret_cast<int*>(H2);  // [TW] byte offset of the source column } until the tile is loaded, where H2
    int* yi = xi + TW;                     // [TW] source row                      } is written later (k = 5: 40,800 B,
                                           //                                        a fourth workgroup on the CU)
    kstamp_begin_grid(gm.kstamp);
    clear_tile_frame(gm, f, tile, tx, tid, BT);  // the scan's precondition
    for (int i = tid; i < TW; i += BT) {
        xi[i] = 3 * refl(x0 - R + i, w);
        yi[i] = refl(y0 - R + i, h);
    }
    // Lane l's taps, packed: four a dword as bytes for the horizontal pass (C4: taps 4l .. 4l + 3), two a dword
    // as u16 for the vertical pass on row pairs (E2: taps 2l, 2l + 1; O2: taps 2l - 1, 2l, for an output row
    // that starts on the odd row of a pair); taps past K are 0.  A step takes its taps with one v_readlane.
    // K = 1's single tap is 256, which no byte holds: 128 horizontally and 512 vertically give the same
    // 65536 v (H = 128 v fits its u16).
    uint32_t C4 = 0, E2 = 0, O2 = 0;
    {
        const int l = tid & 63;
        auto hc = [&](int t) { return (t < 0 || t >= K) ? 0u : K == 1 ? 128u : (uint32_t)a.coef[t]; };
        auto vc = [&](int t) { return (t < 0 || t >= K) ? 0u : K == 1 ? 512u : (uint32_t)a.coef[t]; };
        C4 = hc(4 * l) | (hc(4 * l + 1) << 8) | (hc(4 * l + 2) << 16) | (hc(4 * l + 3) << 24);
        E2 = vc(2 * l) | (vc(2 * l + 1) << 16);
        O2 = vc(2 * l - 1) | (vc(2 * l) << 16);
    }
    __syncthreads();
    // the tile and its halo, a plane per channel: LC pixels of a thread are loaded together (3 LC byte loads in
    // flight) and then stored; a thread's pixels are BT apart in the tile's raster order
    const uint8_t* src = a.src + f * (size_t)h * w * 3;
    const int PL = TW * RB;
    {
        const int dr = BT / TW, dc = BT - dr * TW;  // one step of BT pixels: dr rows and dc columns on
        int r = tid / TW, cc = tid - r * TW;
        for (int i0 = 0; i0 < TW * TW; i0 += BT * LC) {
            uint32_t vb[LC], vg[LC], vr[LC];
            int off[LC];
#pragma unroll
            for (int j = 0; j < LC; j++) {
                const int rl = min(r, TW - 1);  // (past the tile: a pixel of its last row, loaded and dropped)
                const uint8_t* p = src + (size_t)yi[rl] * w * 3 + xi[cc];
                vb[j] = p[0], vg[j] = p[1], vr[j] = p[2];
                off[j] = r < TW ? r * RB + cc : -1;
                cc += dc, r += dr;
                if (cc >= TW) cc -= TW, r++;
            }
#pragma unroll
            for (int j = 0; j < LC; j++)
                if (off[j] >= 0) {
                    raw[off[j]] = (uint8_t)vb[j];
                    raw[PL + off[j]] = (uint8_t)vg[j];
                    raw[2 * PL + off[j]] = (uint8_t)vr[j];
                }
        }
    }
    __syncthreads();
    // horizontal taps: H[c][r][x] = sum_t c[t] * raw[c][r][x + t] (<= 255 * 256: a u16).  A thread takes four
    // adjacent x of the two rows of a pair: per step of four taps one dword of each row, the four windows by
    // v_alignbyte, four taps per v_dot4_u32_u8
    const int M4 = steps4(R);
    for (int i = tid; i < 3 * NP * 16; i += BT) {
        const int g = i & 15, cp = i >> 4;  // cp = c * NP + p
        const uint32_t* r0 = reinterpret_cast<const uint32_t*>(raw + (size_t)(2 * cp) * RB) + g;
        const uint32_t* r1 = r0 + RB / 4;
        uint32_t e[4] = {0, 0, 0, 0}, o[4] = {0, 0, 0, 0};
        uint32_t d0 = r0[0], d1 = r1[0];
        for (int m = 0; m < M4; m++) {
            const uint32_t n0 = r0[m + 1], n1 = r1[m + 1];
            const uint32_t c4 = (uint32_t)__builtin_amdgcn_readlane((int)C4, m);
            e[0] = __builtin_amdgcn_udot4(d0, c4, e[0], false);
            o[0] = __builtin_amdgcn_udot4(d1, c4, o[0], false);
#pragma unroll
            for (int j = 1; j < 4; j++) {
                e[j] = __builtin_amdgcn_udot4(__builtin_amdgcn_alignbyte(n0, d0, j), c4, e[j], false);
                o[j] = __builtin_amdgcn_udot4(__builtin_amdgcn_alignbyte(n1, d1, j), c4, o[j], false);
            }
            d0 = n0, d1 = n1;
        }
        *reinterpret_cast<uint4*>(H2 + (size_t)cp * 64 + 4 * g) =
            make_uint4(e[0] | (o[0] << 16), e[1] | (o[1] << 16), e[2] | (o[2] << 16), e[3] | (o[3] << 16));
    }
    __syncthreads();
    // vertical taps, rounding, keep-mask: four adjacent rows per thread (two pairs), lanes along x.  Pair m of the
    // thread's R + 2 holds rows 4 yq + 2m and + 2m + 1: they meet taps 2m, 2m + 1 of output row 4 yq (E2[m]),
    // 2m - 1, 2m of row 4 yq + 1 (O2[m]), and the same taps one pair back of rows 4 yq + 2 and + 3; two taps per
    // v_dot2_u32_u16.  The bytes go to LDS transposed (every thread is past the barrier: the raw planes are free)
    const bool hk = a.has_keep[s] != 0;
    const uint8_t* keep = a.keep + (size_t)s * h * w;
    uint8_t* ot = raw;  // [3][64][OTS]
    auto dot2 = [](uint32_t hh, uint32_t tt, uint32_t acc) __attribute__((always_inline)) {
        return __builtin_amdgcn_udot2(__builtin_bit_cast(u16x2_t, hh), __builtin_bit_cast(u16x2_t, tt), acc, false);
    };
    for (int i = tid; i < 3 * 16 * 64; i += BT) {
        const int x = i & 63, yq = (i >> 6) & 15, c = i >> 10;
        const uint32_t* col = H2 + ((size_t)c * NP + 2 * yq) * 64 + x;
        uint32_t a0 = 32768u, a1 = 32768u, a2 = 32768u, a3 = 32768u;
        uint32_t ep = 0, op = 0;
        for (int m = 0; m < R + 2; m++) {
            const uint32_t pr = col[m * 64];
            const uint32_t em = (uint32_t)__builtin_amdgcn_readlane((int)E2, m);
            const uint32_t om = (uint32_t)__builtin_amdgcn_readlane((int)O2, m);
            a0 = dot2(pr, em, a0), a1 = dot2(pr, om, a1);
            a2 = dot2(pr, ep, a2), a3 = dot2(pr, op, a3);
            ep = em, op = om;
        }
        uint32_t v = (a0 >> 16) | ((a1 >> 16) << 8) | ((a2 >> 16) << 16) | ((a3 >> 16) << 24);
        if (hk && x0 + x < w) {
            const int gy = y0 + 4 * yq;
#pragma unroll
            for (int j = 0; j < 4; j++)
                if (gy + j < h && keep[(size_t)(gy + j) * w + x0 + x] == 0) v &= ~(0xFFu << (8 * j));
        }
        *reinterpret_cast<uint32_t*>(ot + (c * 64 + x) * OTS + 4 * yq) = v;
    }
    __syncthreads();
    // 16 rows of a column per store (rows past h, up to CS, are written and never read)
    for (int i = tid; i < 3 * 64 * 4; i += BT) {
        const int q = i & 3, cx = i >> 2, x = cx & 63, c = cx >> 6;
        if (x0 + x < w) {
            const uint32_t* p = reinterpret_cast<const uint32_t*>(ot + cx * OTS + 16 * q);
            *reinterpret_cast<uint4*>(cblur + ((f * 3 + c) * (size_t)w + x0 + x) * CS + y0 + 16 * q) =
                make_uint4(p[0], p[1], p[2], p[3]);
        }
    }
    kstamp_end_wg(gm.kstamp);
}

// TAILK: some elements take accumulateWeighted's scalar tail (3hw % 16 != 0); SIMD: convertScaleAbs's float path
// (3hw >= 16)
template <bool TAILK, bool SIMD>
struct Colour {  // scan_frames' model: the running averages of one pixel's three channels
    struct Group { uint32_t b[PFD][3]; };
    const RgbArgs& a;
    const uint8_t* cblur;  // blur bytes [F][3][x][CS]
    int CS;
    double alpha, beta, bg[3];
    int thr, t0;
    bool tail[3], init0;
    size_t e0, cstride, fstride;
    const uint8_t* base;
    __device__ __forceinline__ void open(const Lane& l) {
        alpha = a.alpha, beta = a.beta, thr = a.thresh, t0 = l.t0;
        const long long e = 3 * ((long long)l.y * a.g.w + l.x);  // element of channel B in the interleaved arrays
        e0 = (size_t)l.s * a.g.h * a.g.w * 3 + e;
        init0 = a.init != nullptr && a.init[l.s] != 0;
#pragma unroll
        for (int ch = 0; ch < 3; ch++) {
            tail[ch] = TAILK && e + ch >= a.acc_vec_end;  // accumulateWeighted's scalar tail, counted in elements
            bg[ch] = (l.valid && !init0) ? a.bg_in[e0 + ch] : 0.0;
        }
        // blur byte of channel ch of frame t of this pixel: cblur[(((t * S + s) * 3 + ch) * w + x) * CS + y]
        cstride = (size_t)a.g.w * CS, fstride = (size_t)a.g.S * 3 * cstride;
        base = cblur + (size_t)l.s * 3 * cstride + (size_t)l.x * CS + l.y;
    }
    __device__ __forceinline__ void load(Group& r, int k, int tc) const {
        const uint8_t* p = base + (size_t)tc * fstride;
#pragma unroll
        for (int ch = 0; ch < 3; ch++) r.b[k][ch] = p[ch * cstride];
    }
    __device__ __forceinline__ void step(const Group& r, int k, int t, bool& over) {
        const bool first = init0 && t == t0;
        over = false;
#pragma unroll
        for (int ch = 0; ch < 3; ch++) {
            const uint32_t blur = r.b[k][ch];
            const double bv = first ? (double)blur : bg[ch];
            const int qr = SIMD ? __float2int_rn(fabsf(__double2float_rn(bv))) : __double2int_rn(fabs(bv));
            const int q = min(max(qr, 0), 255);
            over |= abs((int)blur - q) > thr;
            const double bl = __dmul_rn((double)blur, alpha);
            bg[ch] = tail[ch] ? __dadd_rn(bl, __dmul_rn(bv, beta)) : __fma_rn(bv, beta, bl);
        }
    }
    __device__ __forceinline__ void close(const Lane& l) const {
        if (l.valid) {
#pragma unroll
            for (int ch = 0; ch < 3; ch++) a.bg_out[e0 + ch] = bg[ch];
        }
    }
};

template <bool TAILK, bool SIMD>
__global__ __launch_bounds__(ST) void k_rgb_scan(RgbArgs a, const uint8_t* __restrict__ cblur, int CS) {
    scan_frames(a.g, Colour<TAILK, SIMD>{a, cblur, CS});
}

}  // namespace rgb

bool rgb_supported(int h, int w, int ksize) {
    return ksize >= 1 && ksize <= rgb::kMaxKsize && (long long)((w + 63) / 64) * ((h + 63) / 64) <= 8192;
}

int rgb_lds_bytes(int ksize) { return rgb::blur_lds_bytes(ksize >> 1); }

// frames [a.t_begin, a.t_end) of the batch on the three channels: blur of every frame and tile in parallel, then
// the scan; a.init may mark first frames (bg := blur at t_begin); a.bg_in / a.bg_out hold [S][h][w][3] doubles.
// Of a, the fields of rgb::RgbArgs are read.  ks1 / ks2: launch stamps of the two kernels (or nullptr)
hipError_t launch_rgb(hipStream_t st, const FusedArgs& a, uint8_t* cblur, uint64_t* ks1, uint64_t* ks2) {
    if (!rgb_supported(a.h, a.w, a.ksize)) return hipErrorInvalidValue;
    rgb::RgbArgs r{};
    r.src = a.src;
    r.bg_in = a.bg_in;
    r.bg_out = a.bg_out;
    r.keep = a.keep;
    r.has_keep = a.has_keep;
    r.init = a.init;
    r.g = geom_of(a);
    r.ksize = a.ksize, r.thresh = a.thresh;
    r.alpha = a.alpha, r.beta = a.beta;
    const long long n3 = 3ll * a.h * a.w;  // the element count OpenCV's loops see
    r.acc_vec_end = n3 - n3 % 16;
    for (int i = 0; i < a.ksize; i++) r.coef[i] = a.coef[i];
    const int CS = a.nty * 64;
    const int nf = (a.t_end - a.t_begin) * a.S;
    const int lds = rgb::blur_lds_bytes(a.ksize >> 1);
    r.g.kstamp = ks1;
    (void)hipFuncSetAttribute((const void*)rgb::k_rgb_blur, hipFuncAttributeMaxDynamicSharedMemorySize, lds);
    hipLaunchKernelGGL(rgb::k_rgb_blur, dim3((unsigned)nf * (unsigned)a.ntiles), dim3(rgb::BT), lds, st, r, cblur, CS);
    if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
    r.g.kstamp = ks2;
    const int njobs = a.S * a.w * a.nty;
    const dim3 grid((njobs + ST / 64 - 1) / (ST / 64));
    const bool tailk = r.acc_vec_end < n3, simd = n3 >= 16;
    if (tailk && simd) hipLaunchKernelGGL((rgb::k_rgb_scan<true, true>), grid, dim3(ST), 0, st, r, cblur, CS);
    else if (simd) hipLaunchKernelGGL((rgb::k_rgb_scan<false, true>), grid, dim3(ST), 0, st, r, cblur, CS);
    else if (tailk) hipLaunchKernelGGL((rgb::k_rgb_scan<true, false>), grid, dim3(ST), 0, st, r, cblur, CS);
    else hipLaunchKernelGGL((rgb::k_rgb_scan<false, false>), grid, dim3(ST), 0, st, r, cblur, CS);
    return hipGetLastError();
}

}  // namespace fm
