// fm_jpeg_enc.hip — the write side of the path: BGR frames in HBM -> baseline JPEGs for the MJPG writer.
//
// The reference writes motion frames with cv2.VideoWriter (fm.py:447-546), constructor default codec 'MJPG'
// (fm.py:303).  This encoder produces, byte for byte, the file libjpeg-turbo writes through Pillow for the same
// pixels: Image.save(..., "JPEG", quality=q, subsampling=s[, restart_marker_blocks=n]) -- jpeg_set_quality(q,
// force_baseline), JDCT_ISLOW, the T.81 Annex K Huffman tables (not optimized), JFIF 1.01 APP0.  That is what
// videoio.MjpegAviWriter writes on the host, so a file written through this encoder is identical to it.  Pinned
// against Pillow by tests/test_jpeg_encode_host.py (numpy restatement tests/jpeg_encode_ref.py, fm_jpeg_header)
// and tests/test_gpu_jpeg_encode.py (this code).  cv2.VideoWriter's built-in MJPG encoder is OpenCV's own code,
// not libjpeg: parity with its bytes is unpinned, as the FFmpeg decode parity is on the read side.
// Supported: 8-bit BGR [H][W][3] frames up to 65535 x 65535, three components, Y at 1x1 (4:4:4), 2x1 (4:2:2) or
// 2x2 (4:2:0) with Cb, Cr at 1x1, quality 1..100, restart interval 0..65535 MCUs.  Not here: grayscale output,
// optimized Huffman tables, progressive, 12-bit.
//   k_enc_dct    four MCUs per workgroup: rgb_ycc_convert (jccolor.c, 16-bit fixed point) with edge replication
//           by clamped loads (columns on the full-resolution plane; chroma ROWS clamped after downsampling,
//           jcprepct.c), h2v1 / h2v2 downsampling with alternating bias (jcsample.c), jpeg_fdct_islow
//           (jfdctint.c) one lane per 8-sample row, then per column through LDS, quantization by plain division
//           (jcdctmgr.c); int16 coefficients in zigzag order, blocks in scan (MCU-interleaved) order, dummy blocks
//           (jccoefct.c: zero AC, the DC of the block before them in the MCU) included;
//   k_enc_bits   one lane per block: DC difference against the block's static predecessor, code length;
//   k_enc_scan   one workgroup per frame: exclusive prefix sum of the code lengths (each lane a contiguous run,
//           lane 0 combines the 256 run summaries), restart intervals starting on byte boundaries two bytes
//           after the padded end of the one before;
//   k_enc_emit   one lane per block writes its codes at its bit offset into the zeroed unstuffed stream (first
//           and last word by atomicOr, whole words by plain stores), pad bits and RSTn after an interval's last;
//   k_enc_ffcount / k_enc_stuff   per 4 KiB tile: count the 0xFF data bytes, then copy with 0x00 inserted.
// No workgroup waits on another: every prefix sum is done by one workgroup or on the host between launches.
// Sizes are known before anything is written: the unstuffed stream's after k_enc_scan, the output's after
// k_enc_ffcount; the buffers are grown to them (or the call fails) before the kernels that write them run.
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "fm_host.h"
#include "fm_internal.h"

namespace fm {
namespace je {

constexpr int kGroup = 4;          // MCUs per k_enc_dct workgroup
constexpr int kGroupBlocks = 24;   // blocks of kGroup 4:2:0 MCUs
constexpr int kBlockStride = 72;   // LDS dwords per block: 64 + 8 keeps the column pass conflict-free
constexpr int kTile = 4096;        // bytes of unstuffed stream per k_enc_stuff workgroup
constexpr int kThreads = 256;

struct EncGeom {
    int W, H, hs, vs;        // frame size, Y's sampling factors
    int mcux, nmcu, bpm, nblk;  // MCUs per row / frame, blocks per MCU / frame
    int ybw, ybh;            // Y's own block grid: blocks of an MCU outside it are dummy blocks
    int crows;               // chroma rows before replication: ceil(H / vs)
    int ib;                  // blocks per restart interval (0: no restart markers)
    int nint;                // restart intervals per frame
};

struct EncQuant {
    uint16_t q8[2][64];      // 8 x the quantization table (the DCT's output carries a factor of 8), natural order
};

struct EncHuff {             // code | length << 16
    uint32_t dc[2][16];
    uint32_t ac[2][256];
};

struct FrameInfo {
    unsigned long long ubase;  // byte offset of the frame's unstuffed stream (a multiple of kTile)
    unsigned long long obase;  // byte offset of the frame's stuffed scan in the output buffer
    uint32_t ubytes;           // unstuffed bytes
    uint32_t pad;
};

struct TileInfo {
    uint32_t frame;
    uint32_t tile;             // tile index inside the frame
    uint32_t out;              // output offset of the tile's first byte, from the frame's obase
    uint32_t pad;
};

__device__ const uint8_t kZig[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                                     41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                                     30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

// ---- colour, downsampling, DCT, quantization ---------------------------------------------------------------

__device__ inline int px_y(const uint8_t* p) { return (19595 * p[2] + 38470 * p[1] + 7471 * p[0] + 32768) >> 16; }
__device__ inline int px_c(const uint8_t* p, int comp) {
    const int r = p[2], g = p[1], b = p[0];
    return comp == 0 ? (-11059 * r - 21709 * g + 32768 * b + (128 << 16) + 32767) >> 16
                     : (32768 * r - 27439 * g - 5329 * b + (128 << 16) + 32767) >> 16;
}

// One pass of jpeg_fdct_islow over eight values (FIRST: the row pass, scaled up by PASS1_BITS).
template <bool FIRST>
__device__ inline void fdct8(int (&d)[8]) {
    constexpr int SH = FIRST ? 11 : 15;
    const int t0 = d[0] + d[7], t7 = d[0] - d[7], t1 = d[1] + d[6], t6 = d[1] - d[6];
    const int t2 = d[2] + d[5], t5 = d[2] - d[5], t3 = d[3] + d[4], t4 = d[3] - d[4];
    const int t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
    if (FIRST) {
        d[0] = (t10 + t11) << 2;
        d[4] = (t10 - t11) << 2;
    } else {
        d[0] = (t10 + t11 + 2) >> 2;
        d[4] = (t10 - t11 + 2) >> 2;
    }
    constexpr int R = 1 << (SH - 1);
    int z1 = (t12 + t13) * 4433;
    d[2] = (z1 + t13 * 6270 + R) >> SH;
    d[6] = (z1 - t12 * 15137 + R) >> SH;
    z1 = t4 + t7;
    int z2 = t5 + t6, z3 = t4 + t6, z4 = t5 + t7;
    const int z5 = (z3 + z4) * 9633;
    const int a4 = t4 * 2446, a5 = t5 * 16819, a6 = t6 * 25172, a7 = t7 * 12299;
    z1 *= -7373;
    z2 *= -20995;
    z3 = z3 * -16069 + z5;
    z4 = z4 * -3196 + z5;
    d[7] = (a4 + z1 + z3 + R) >> SH;
    d[5] = (a5 + z2 + z4 + R) >> SH;
    d[3] = (a6 + z2 + z3 + R) >> SH;
    d[1] = (a7 + z1 + z4 + R) >> SH;
}

// Whether block kb of MCU m is a dummy block (outside Y's own grid; chroma blocks never are).
__device__ inline bool is_dummy(const EncGeom& g, int m, int kb) {
    if (kb >= g.hs * g.vs) return false;
    const int mr = m / g.mcux, mc = m - mr * g.mcux;
    const int by = kb / g.hs, bx = kb - by * g.hs;
    return mc * g.hs + bx >= g.ybw || mr * g.vs + by >= g.ybh;
}

__global__ __launch_bounds__(kThreads) void k_enc_dct(const uint8_t* const* frames, EncGeom g, EncQuant q,
                                                       int16_t* __restrict__ coef) {
    __shared__ int s[kGroupBlocks * kBlockStride];
    __shared__ int16_t o[kGroupBlocks * 64];  // quantized, natural order
    const int tid = threadIdx.x, f = blockIdx.y;
    const int m0 = blockIdx.x * kGroup;
    const int nm = min(kGroup, g.nmcu - m0), nb = nm * g.bpm, ny = g.hs * g.vs;
    const uint8_t* img = frames[f];
    const size_t row = (size_t)g.W * 3;
    for (int e = tid; e < nb * 64; e += kThreads) {
        const int b = e >> 6, k = e & 63, sy = k >> 3, sx = k & 7;
        const int ml = b / g.bpm, kb = b - ml * g.bpm, m = m0 + ml;
        const int mr = m / g.mcux, mc = m - mr * g.mcux;
        int val;
        if (kb < ny) {
            const int by = kb / g.hs, bx = kb - by * g.hs;
            const int x = min((mc * g.hs + bx) * 8 + sx, g.W - 1), y = min((mr * g.vs + by) * 8 + sy, g.H - 1);
            val = px_y(img + y * row + (size_t)x * 3);
        } else {
            const int comp = kb - ny, cx = mc * 8 + sx, cy = min(mr * 8 + sy, g.crows - 1);
            const int x0 = min(cx * g.hs, g.W - 1), y0 = min(cy * g.vs, g.H - 1);
            val = px_c(img + y0 * row + (size_t)x0 * 3, comp);
            if (g.hs == 2) {
                const int x1 = min(cx * 2 + 1, g.W - 1);
                val += px_c(img + y0 * row + (size_t)x1 * 3, comp);
                if (g.vs == 2) {
                    const int y1 = min(cy * 2 + 1, g.H - 1);
                    val += px_c(img + y1 * row + (size_t)x0 * 3, comp) + px_c(img + y1 * row + (size_t)x1 * 3, comp);
                    val = (val + 1 + (cx & 1)) >> 2;  // bias 1, 2, 1, 2 along output columns
                } else {
                    val = (val + (cx & 1)) >> 1;      // bias 0, 1, 0, 1
                }
            }
        }
        s[b * kBlockStride + k] = val - 128;
    }
    __syncthreads();
    for (int t = tid; t < nb * 8; t += kThreads) {  // rows
        int* p = s + (t >> 3) * kBlockStride + (t & 7) * 8;
        int d[8];
#pragma unroll
        for (int i = 0; i < 8; i++) d[i] = p[i];
        fdct8<true>(d);
#pragma unroll
        for (int i = 0; i < 8; i++) p[i] = d[i];
    }
    __syncthreads();
    for (int t = tid; t < nb * 8; t += kThreads) {  // columns, quantization
        const int b = t >> 3, c = t & 7;
        const int* p = s + b * kBlockStride + c;
        int d[8];
#pragma unroll
        for (int i = 0; i < 8; i++) d[i] = p[i * 8];
        fdct8<false>(d);
        const int kb = b % g.bpm;
        const uint16_t* qt = q.q8[kb < ny ? 0 : 1];
#pragma unroll
        for (int i = 0; i < 8; i++) {
            const unsigned qv = qt[i * 8 + c];
            const unsigned a = ((unsigned)abs(d[i]) + (qv >> 1)) / qv;
            o[b * 64 + i * 8 + c] = (int16_t)(d[i] < 0 ? -(int)a : (int)a);
        }
    }
    __syncthreads();
    if (tid < nm)  // dummy blocks take the DC of the block before them in the MCU, in order
        for (int kb = 1; kb < ny; kb++)
            if (is_dummy(g, m0 + tid, kb)) o[(tid * g.bpm + kb) * 64] = o[(tid * g.bpm + kb - 1) * 64];
    __syncthreads();
    int16_t* out = coef + ((size_t)f * g.nblk + (size_t)m0 * g.bpm) * 64;
    for (int e = tid; e < nb * 64; e += kThreads) {
        const int b = e >> 6, k = e & 63;
        const int ml = b / g.bpm, kb = b - ml * g.bpm;
        const bool dummy = is_dummy(g, m0 + ml, kb);
        out[e] = dummy && k ? (int16_t)0 : o[b * 64 + kZig[k]];
    }
}

// ---- entropy coding --------------------------------------------------------------------------------------

// The DC difference of block b of a frame: against the previous block of the same component in scan order,
// against 0 at the start of the frame and of every restart interval.
__device__ inline int dc_diff(const int16_t* fc, const EncGeom& g, int b, int& slot) {
    const int m = b / g.bpm, kb = b - m * g.bpm, ny = g.hs * g.vs;
    slot = kb < ny ? 0 : 1;
    const bool start = m == 0 || (g.ib && (m * g.bpm) % g.ib == 0);
    int pb;
    if (kb > 0 && kb < ny)
        pb = b - 1;
    else if (start)
        pb = -1;
    else
        pb = kb == 0 ? b - g.bpm + ny - 1 : b - g.bpm;
    return (int)fc[(size_t)b * 64] - (pb < 0 ? 0 : (int)fc[(size_t)pb * 64]);
}

// jchuff.c encode_one_block over 64 zigzag coefficients: put(code, length) for every code and extra-bit field.
template <class Put>
__device__ inline void code_block(const int16_t* c, int diff, const uint32_t* dct, const uint32_t* act, Put& put) {
    int a = diff < 0 ? -diff : diff;
    int nb = 32 - __clz(a);
    uint32_t e = dct[nb];
    put(e & 0xffffu, (int)(e >> 16));
    if (nb) put((uint32_t)(diff < 0 ? diff - 1 : diff) & ((1u << nb) - 1), nb);
    int run = 0;
    const uint4* v4 = reinterpret_cast<const uint4*>(c);
    for (int j = 0; j < 8; j++) {
        const uint4 v = v4[j];
        const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int i = 0; i < 8; i++) {
            if (j == 0 && i == 0) continue;
            const int x = (int)(int16_t)(w[i >> 1] >> ((i & 1) * 16));
            if (x == 0) {
                run++;
                continue;
            }
            while (run > 15) {
                e = act[0xF0];
                put(e & 0xffffu, (int)(e >> 16));
                run -= 16;
            }
            a = x < 0 ? -x : x;
            nb = 32 - __clz(a);
            e = act[(run << 4) | nb];
            put(e & 0xffffu, (int)(e >> 16));
            put((uint32_t)(x < 0 ? x - 1 : x) & ((1u << nb) - 1), nb);
            run = 0;
        }
    }
    if (run > 0) {
        e = act[0];
        put(e & 0xffffu, (int)(e >> 16));
    }
}

__device__ inline void load_huff(const EncHuff* huff, uint32_t* sdc, uint32_t* sac) {
    for (int i = threadIdx.x; i < 32; i += kThreads) sdc[i] = huff->dc[i >> 4][i & 15];
    for (int i = threadIdx.x; i < 512; i += kThreads) sac[i] = huff->ac[i >> 8][i & 255];
    __syncthreads();
}

struct CountPut {
    uint32_t n = 0;
    __device__ void operator()(uint32_t, int len) { n += len; }
};

__global__ __launch_bounds__(kThreads) void k_enc_bits(const int16_t* __restrict__ coef, EncGeom g, const EncHuff* huff,
                                                        uint32_t* __restrict__ bits, long long total) {
    __shared__ uint32_t sdc[32], sac[512];
    load_huff(huff, sdc, sac);
    const long long gb = (long long)blockIdx.x * kThreads + threadIdx.x;
    if (gb >= total) return;
    const int f = (int)(gb / g.nblk), b = (int)(gb - (long long)f * g.nblk);
    const int16_t* fc = coef + (size_t)f * g.nblk * 64;
    int slot;
    const int diff = dc_diff(fc, g, b, slot);
    CountPut put;
    code_block(fc + (size_t)b * 64, diff, sdc + slot * 16, sac + slot * 256, put);
    bits[gb] = put.n;
}

// bits[f][b] (code length of block b) -> its bit offset in the frame's unstuffed stream; fbits[f] = the
// stream's length in bits before the final padding.  A block that starts a restart interval lies on a byte
// boundary, 16 bits (the RSTn marker) after the padded end of the block before it.
__global__ __launch_bounds__(kThreads) void k_enc_scan(uint32_t* __restrict__ bits, EncGeom g, uint32_t* __restrict__ fbits) {
    __shared__ uint32_t sh[kThreads], sa[kThreads], sb[kThreads], sp[kThreads];
    const int tid = threadIdx.x;
    uint32_t* p = bits + (size_t)blockIdx.x * g.nblk;
    const int per = (g.nblk + kThreads - 1) / kThreads;
    const int b0 = min(tid * per, g.nblk), b1 = min(b0 + per, g.nblk);
    // the run's summary: a bits before its first interval start; then, from that (byte-aligned) start, bb bits
    uint32_t h = 0, a = 0, bb = 0;
    int rem = g.ib ? b0 % g.ib : 1;
    for (int b = b0; b < b1; b++) {
        if (g.ib && b && rem == 0) {
            bb = h ? ((bb + 7) & ~7u) + 16 : 16;
            h = 1;
        }
        if (h)
            bb += p[b];
        else
            a += p[b];
        if (g.ib && ++rem == g.ib) rem = 0;
    }
    sh[tid] = h;
    sa[tid] = a;
    sb[tid] = bb;
    __syncthreads();
    if (tid == 0) {
        uint32_t pos = 0;
        for (int t = 0; t < kThreads; t++) {
            sp[t] = pos;
            pos = sh[t] ? ((pos + sa[t] + 7) & ~7u) + sb[t] : pos + sa[t];
        }
        fbits[blockIdx.x] = pos;
    }
    __syncthreads();
    uint32_t pos = sp[tid];
    rem = g.ib ? b0 % g.ib : 1;
    for (int b = b0; b < b1; b++) {
        if (g.ib && b && rem == 0) pos = ((pos + 7) & ~7u) + 16;
        const uint32_t n = p[b];
        p[b] = pos;
        pos += n;
        if (g.ib && ++rem == g.ib) rem = 0;
    }
}

// Big-endian bit writer into 32-bit words of a zeroed buffer.  The first and the last word it touches may be
// shared with the neighbouring blocks (atomicOr); every word in between is wholly this block's (plain store).
struct WordPut {
    uint32_t* w;
    unsigned long long acc = 0;
    int n;
    bool first = true;
    __device__ WordPut(uint32_t* base, unsigned long long bitpos) : w(base + (bitpos >> 5)), n((int)(bitpos & 31)) {}
    __device__ void operator()(uint32_t code, int len) {
        acc = (acc << len) | code;
        n += len;
        if (n >= 32) {
            const uint32_t v = __builtin_bswap32((uint32_t)(acc >> (n - 32)));
            if (first)
                atomicOr(w, v);
            else
                *w = v;
            first = false;
            w++;
            n -= 32;
        }
    }
    __device__ void finish() {
        if (n > 0) atomicOr(w, __builtin_bswap32((uint32_t)(acc << (32 - n))));
    }
};

__global__ __launch_bounds__(kThreads) void k_enc_emit(const int16_t* __restrict__ coef, EncGeom g, const EncHuff* huff,
                                                        const uint32_t* __restrict__ off, const FrameInfo* __restrict__ fi,
                                                        uint32_t* __restrict__ ustream, long long total) {
    __shared__ uint32_t sdc[32], sac[512];
    load_huff(huff, sdc, sac);
    const long long gb = (long long)blockIdx.x * kThreads + threadIdx.x;
    if (gb >= total) return;
    const int f = (int)(gb / g.nblk), b = (int)(gb - (long long)f * g.nblk);
    const int16_t* fc = coef + (size_t)f * g.nblk * 64;
    int slot;
    const int diff = dc_diff(fc, g, b, slot);
    WordPut put(ustream, fi[f].ubase * 8ull + off[gb]);
    code_block(fc + (size_t)b * 64, diff, sdc + slot * 16, sac + slot * 256, put);
    const bool last = b == g.nblk - 1;
    if (last || (g.ib && (b + 1) % g.ib == 0)) {  // the interval's last block: 1-bits to the byte boundary, RSTn
        const int fill = (8 - (put.n & 7)) & 7;   // words start on byte boundaries: n & 7 is the position mod 8
        if (fill) put((1u << fill) - 1, fill);
        if (!last) {
            put(0xFFu, 8);
            put(0xD0u | (uint32_t)((b / g.ib) & 7), 8);
        }
    }
    put.finish();
}

// ---- byte stuffing ---------------------------------------------------------------------------------------

// Whether the 0xFF at byte p of frame f's unstuffed stream (followed by D0..D7) is an RSTn marker's: markers
// end where a restart interval starts, and the intervals' first blocks' offsets are in `off`.
__device__ inline bool is_marker(const uint32_t* off, const EncGeom& g, int f, uint32_t p) {
    if (!g.ib) return false;
    const uint32_t* fo = off + (size_t)f * g.nblk;
    int lo = 1, hi = g.nint - 1;
    while (lo <= hi) {
        const int mid = (lo + hi) >> 1;
        const uint32_t s = fo[(size_t)mid * g.ib] >> 3;
        if (s == p + 2) return true;
        if (s < p + 2)
            lo = mid + 1;
        else
            hi = mid - 1;
    }
    return false;
}

// The 0xFF data bytes among this lane's 16 bytes of the tile (bit i of the result: byte i needs a 0x00 after it).
__device__ inline uint32_t stuff_mask(const uint8_t* us, const uint32_t* off, const EncGeom& g, int f, uint32_t ubytes,
                                      uint32_t p0, const uint4& v) {
    const uint32_t w[4] = {v.x, v.y, v.z, v.w};
    uint32_t mask = 0;
#pragma unroll
    for (int i = 0; i < 16; i++) {
        const uint32_t byte = (w[i >> 2] >> ((i & 3) * 8)) & 255u;
        const uint32_t p = p0 + i;
        if (byte != 0xFFu || p >= ubytes) continue;
        if (p + 1 < ubytes && (us[p + 1] & 0xF8u) == 0xD0u && is_marker(off, g, f, p)) continue;
        mask |= 1u << i;
    }
    return mask;
}

__global__ __launch_bounds__(kThreads) void k_enc_ffcount(const uint8_t* __restrict__ ustream, EncGeom g,
                                                           const uint32_t* __restrict__ off, const FrameInfo* __restrict__ fi,
                                                           const TileInfo* __restrict__ ti, uint32_t* __restrict__ count) {
    __shared__ uint32_t total;
    if (threadIdx.x == 0) total = 0;
    __syncthreads();
    const TileInfo t = ti[blockIdx.x];
    const FrameInfo F = fi[t.frame];
    const uint8_t* us = ustream + F.ubase;
    const uint32_t p0 = t.tile * kTile + threadIdx.x * 16;
    const uint4 v = *reinterpret_cast<const uint4*>(us + p0);
    const uint32_t m = stuff_mask(us, off, g, (int)t.frame, F.ubytes, p0, v);
    if (m) atomicAdd(&total, (uint32_t)__popc(m));
    __syncthreads();
    if (threadIdx.x == 0) count[blockIdx.x] = total;
}

__global__ __launch_bounds__(kThreads) void k_enc_stuff(const uint8_t* __restrict__ ustream, EncGeom g,
                                                         const uint32_t* __restrict__ off, const FrameInfo* __restrict__ fi,
                                                         const TileInfo* __restrict__ ti, uint8_t* __restrict__ out) {
    __shared__ uint32_t scan[kThreads];
    __shared__ uint8_t buf[2 * kTile];
    const int tid = threadIdx.x;
    const TileInfo t = ti[blockIdx.x];
    const FrameInfo F = fi[t.frame];
    const uint8_t* us = ustream + F.ubase;
    const uint32_t p0 = t.tile * kTile + tid * 16;
    const uint4 v = *reinterpret_cast<const uint4*>(us + p0);
    const uint32_t m = stuff_mask(us, off, g, (int)t.frame, F.ubytes, p0, v);
    const uint32_t valid = p0 >= F.ubytes ? 0u : min(16u, F.ubytes - p0);
    const uint32_t mine = valid + __popc(m);
    scan[tid] = mine;
    __syncthreads();
    for (int d = 1; d < kThreads; d <<= 1) {  // inclusive scan of the lanes' output byte counts
        const uint32_t x = tid >= d ? scan[tid - d] : 0u;
        __syncthreads();
        scan[tid] += x;
        __syncthreads();
    }
    uint32_t at = scan[tid] - mine;
    const uint32_t total = scan[kThreads - 1];
    const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int i = 0; i < 16; i++) {
        if ((uint32_t)i < valid) {
            buf[at++] = (uint8_t)(w[i >> 2] >> ((i & 3) * 8));
            if (m >> i & 1) buf[at++] = 0;
        }
    }
    __syncthreads();
    uint8_t* o = out + F.obase + t.out;
    for (uint32_t j = tid; j < total; j += kThreads) o[j] = buf[j];
}

// ---- host side ---------------------------------------------------------------------------------------------

// T.81 Annex K.1 quantization tables (natural order) and K.3 Huffman tables, as jcparam.c installs them.
const uint8_t kStdLuma[64] = {16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57,
                              69, 56, 14, 17, 22, 29, 51, 87, 80, 62, 18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64,
                              81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99};
const uint8_t kStdChroma[64] = {17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99,
                                99, 99, 47, 66, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99,
                                99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99};
const uint8_t kZigHost[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                              41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                              30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};
const uint8_t kDcBits[2][16] = {{0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0}, {0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0}};
const uint8_t kAcBits[2][16] = {{0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d}, {0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77}};
const uint8_t kAcHead0[40] = {0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51,
                              0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81, 0x91, 0xa1, 0x08, 0x23, 0x42, 0xb1, 0xc1,
                              0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16};
const uint8_t kAcHead1[43] = {0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61,
                              0x71, 0x13, 0x22, 0x32, 0x81, 0x08, 0x14, 0x42, 0x91, 0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33,
                              0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25, 0xf1};

// The symbols of table (cls, slot) in code order: the AC lists are an irregular head followed by every other
// (run, size) symbol, size 1..10, in increasing order.
std::vector<uint8_t> huff_vals(int cls, int slot) {
    std::vector<uint8_t> v;
    if (!cls) {
        for (int i = 0; i < 12; i++) v.push_back((uint8_t)i);
        return v;
    }
    bool used[256] = {};
    const uint8_t* head = slot ? kAcHead1 : kAcHead0;
    for (int k = 0; k < (slot ? 43 : 40); k++) {
        v.push_back(head[k]);
        used[head[k]] = true;
    }
    for (int rs = 0; rs < 256; rs++)
        if ((rs & 15) >= 1 && (rs & 15) <= 10 && !used[rs]) v.push_back((uint8_t)rs);
    return v;
}

void quant_table(int quality, int chroma, uint8_t (&q)[64]) {  // jpeg_set_quality(quality, force_baseline)
    const int scale = quality < 50 ? 5000 / quality : 200 - 2 * quality;
    const uint8_t* std_ = chroma ? kStdChroma : kStdLuma;
    for (int i = 0; i < 64; i++) q[i] = (uint8_t)std::min(255, std::max(1, (std_[i] * scale + 50) / 100));
}

void build_huff(EncHuff& H) {
    std::memset(&H, 0, sizeof H);
    for (int cls = 0; cls < 2; cls++)
        for (int slot = 0; slot < 2; slot++) {
            const uint8_t* bits = cls ? kAcBits[slot] : kDcBits[slot];
            const std::vector<uint8_t> vals = huff_vals(cls, slot);
            uint32_t code = 0;
            size_t k = 0;
            for (int len = 1; len <= 16; len++) {
                for (int i = 0; i < bits[len - 1]; i++, code++, k++)
                    (cls ? H.ac[slot] : H.dc[slot])[vals[k]] = code | ((uint32_t)len << 16);
                code <<= 1;
            }
        }
}

bool valid_settings(int width, int height, int quality, int subsampling, int restart_interval) {
    return width >= 1 && width <= 65535 && height >= 1 && height <= 65535 && quality >= 1 && quality <= 100 &&
           subsampling >= 0 && subsampling <= 2 && restart_interval >= 0 && restart_interval <= 65535;
}

// SOI, APP0 (JFIF 1.01, no units, density 1x1), DQT luma, DQT chroma, SOF0, DHT x 4, [DRI], SOS: jcmarker.c's order.
std::vector<uint8_t> make_header(int width, int height, int quality, int subsampling, int restart_interval) {
    std::vector<uint8_t> h = {0xFF, 0xD8, 0xFF, 0xE0, 0, 16, 'J', 'F', 'I', 'F', 0, 1, 1, 0, 0, 1, 0, 1, 0, 0};
    for (int t = 0; t < 2; t++) {
        uint8_t q[64];
        quant_table(quality, t, q);
        h.insert(h.end(), {0xFF, 0xDB, 0, 67, (uint8_t)t});
        for (int i = 0; i < 64; i++) h.push_back(q[kZigHost[i]]);
    }
    const int hs = subsampling ? 2 : 1, vs = subsampling == 2 ? 2 : 1;
    h.insert(h.end(), {0xFF, 0xC0, 0, 17, 8, (uint8_t)(height >> 8), (uint8_t)height, (uint8_t)(width >> 8), (uint8_t)width, 3,
                       1, (uint8_t)((hs << 4) | vs), 0, 2, 0x11, 1, 3, 0x11, 1});
    for (int t = 0; t < 4; t++) {
        const int cls = t & 1, slot = t >> 1;
        const std::vector<uint8_t> vals = huff_vals(cls, slot);
        const int len = 2 + 1 + 16 + (int)vals.size();
        h.insert(h.end(), {0xFF, 0xC4, (uint8_t)(len >> 8), (uint8_t)len, (uint8_t)((cls << 4) | slot)});
        const uint8_t* bits = cls ? kAcBits[slot] : kDcBits[slot];
        h.insert(h.end(), bits, bits + 16);
        h.insert(h.end(), vals.begin(), vals.end());
    }
    if (restart_interval) h.insert(h.end(), {0xFF, 0xDD, 0, 4, (uint8_t)(restart_interval >> 8), (uint8_t)restart_interval});
    h.insert(h.end(), {0xFF, 0xDA, 0, 12, 3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0});
    return h;
}

}  // namespace je
}  // namespace fm

using namespace fm::je;

struct fm_mjpeg_enc {
    int device = 0, max_frames = 0;
    EncGeom g{};
    EncQuant q{};
    size_t frame_bytes = 0;
    std::vector<uint8_t> header;
    std::string err;
    fm::Stream st;  // (before the buffers used on it: they are released first)
    fm::Event e0, e1;
    float last_ms = 0.f;
    int last_n = 0;                       // frames of the last successful call
    // device
    fm::DevBuf<EncHuff> d_huff;
    fm::DevBuf<const uint8_t*> d_list;    // [max_frames] frame addresses
    fm::DevBuf<uint8_t> d_in;             // staging for host frames (allocated by the first host call)
    fm::DevBuf<int16_t> d_coef;           // [max_frames][nblk][64]
    fm::DevBuf<uint32_t> d_bits;          // [max_frames][nblk] code lengths, then bit offsets
    fm::DevBuf<uint32_t> d_fbits;         // [max_frames]
    fm::DevBuf<FrameInfo> d_fi;           // [max_frames]
    fm::DevBuf<TileInfo> d_ti;            // one per tile; grows with d_tcount, h_ti and h_tcount
    fm::DevBuf<uint32_t> d_tcount;
    fm::DevBuf<uint8_t> d_u;              // unstuffed streams
    fm::DevBuf<uint8_t> d_out;            // stuffed scans
    // pinned host
    fm::PinBuf<const uint8_t*> h_list;
    fm::PinBuf<uint32_t> h_fbits;
    fm::PinBuf<FrameInfo> h_fi;
    fm::PinBuf<TileInfo> h_ti;
    fm::PinBuf<uint32_t> h_tcount;
    std::vector<uint32_t> scan_len;       // stuffed scan bytes per frame of the last call

    ~fm_mjpeg_enc() {
        if (st) (void)hipStreamSynchronize(st);
    }
};

namespace {

// Make a device buffer hold at least `need` bytes, a quarter more when it grows (contents are not kept).
int grow(fm_mjpeg_enc* e, fm::DevBuf<uint8_t>& b, size_t need, size_t count, const char* what) {
    if (b.reserve(need, count) == hipSuccess) return FM_OK;
    (void)hipGetLastError();
    return fm::failf(&e->err, FM_ENOMEM, "%s: %zu bytes of device memory not available", what, count);
}

// Encode the n frames whose device addresses are in e->h_list.
int encode_list(fm_mjpeg_enc* e, int n) {
    const EncGeom& g = e->g;
    hipStream_t st = e->st;
    e->last_n = 0;
    FM_HIP_TRY(&e->err, hipMemcpyAsync(e->d_list, e->h_list, n * sizeof(uint8_t*), hipMemcpyHostToDevice, st));
    FM_HIP_TRY(&e->err, hipEventRecord(e->e0, st));
    const long long total = (long long)n * g.nblk;
    const unsigned nbg = (unsigned)((total + kThreads - 1) / kThreads);
    k_enc_dct<<<dim3((g.nmcu + kGroup - 1) / kGroup, n), kThreads, 0, st>>>(e->d_list, g, e->q, e->d_coef);
    FM_HIP_TRY(&e->err, hipGetLastError());
    k_enc_bits<<<nbg, kThreads, 0, st>>>(e->d_coef, g, e->d_huff, e->d_bits, total);
    FM_HIP_TRY(&e->err, hipGetLastError());
    k_enc_scan<<<n, kThreads, 0, st>>>(e->d_bits, g, e->d_fbits);
    FM_HIP_TRY(&e->err, hipGetLastError());
    FM_HIP_TRY(&e->err, hipMemcpyAsync(e->h_fbits, e->d_fbits, n * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    FM_HIP_TRY(&e->err, hipStreamSynchronize(st));
    // the unstuffed streams' sizes are known: lay them out, one run of whole tiles per frame
    size_t u_total = 0, ntiles = 0;
    for (int f = 0; f < n; f++) {
        FrameInfo& F = e->h_fi[f];
        F.ubytes = (e->h_fbits[f] + 7) / 8;
        F.ubase = u_total;
        F.obase = 0;
        F.pad = 0;
        const size_t t = (F.ubytes + kTile - 1) / kTile;
        u_total += t * kTile;
        ntiles += t;
    }
    if (int rc = grow(e, e->d_u, u_total, u_total + u_total / 4, "unstuffed stream")) return rc;
    FM_HIP_TRY(&e->err, fm::reserve_all(ntiles, ntiles + ntiles / 4 + 64, e->d_ti, e->d_tcount, e->h_ti, e->h_tcount));
    size_t k = 0;
    for (int f = 0; f < n; f++)
        for (uint32_t t = 0; t < (e->h_fi[f].ubytes + kTile - 1) / kTile; t++) e->h_ti[k++] = TileInfo{(uint32_t)f, t, 0, 0};
    FM_HIP_TRY(&e->err, hipMemcpyAsync(e->d_fi, e->h_fi, n * sizeof(FrameInfo), hipMemcpyHostToDevice, st));
    FM_HIP_TRY(&e->err, hipMemcpyAsync(e->d_ti, e->h_ti, ntiles * sizeof(TileInfo), hipMemcpyHostToDevice, st));
    FM_HIP_TRY(&e->err, hipMemsetAsync(e->d_u, 0, u_total, st));  // k_enc_emit ORs into zeros: cleared for every call
    k_enc_emit<<<nbg, kThreads, 0, st>>>(e->d_coef, g, e->d_huff, e->d_bits, e->d_fi, (uint32_t*)e->d_u.get(), total);
    FM_HIP_TRY(&e->err, hipGetLastError());
    k_enc_ffcount<<<(unsigned)ntiles, kThreads, 0, st>>>(e->d_u, g, e->d_bits, e->d_fi, e->d_ti, e->d_tcount);
    FM_HIP_TRY(&e->err, hipGetLastError());
    FM_HIP_TRY(&e->err, hipMemcpyAsync(e->h_tcount, e->d_tcount, ntiles * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    FM_HIP_TRY(&e->err, hipStreamSynchronize(st));
    // the output's sizes are known: each tile's offset in its frame's scan, each frame's place in the buffer
    size_t o_total = 0;
    k = 0;
    e->scan_len.assign(n, 0);
    for (int f = 0; f < n; f++) {
        FrameInfo& F = e->h_fi[f];
        F.obase = o_total;
        uint32_t at = 0;
        for (uint32_t t = 0; t < (F.ubytes + kTile - 1) / kTile; t++, k++) {
            e->h_ti[k].out = at;
            at += std::min<uint32_t>(kTile, F.ubytes - t * kTile) + e->h_tcount[k];
        }
        e->scan_len[f] = at;
        o_total += ((size_t)at + 15) & ~(size_t)15;
    }
    if (int rc = grow(e, e->d_out, o_total, o_total + o_total / 4, "output")) return rc;
    FM_HIP_TRY(&e->err, hipMemcpyAsync(e->d_fi, e->h_fi, n * sizeof(FrameInfo), hipMemcpyHostToDevice, st));
    FM_HIP_TRY(&e->err, hipMemcpyAsync(e->d_ti, e->h_ti, ntiles * sizeof(TileInfo), hipMemcpyHostToDevice, st));
    k_enc_stuff<<<(unsigned)ntiles, kThreads, 0, st>>>(e->d_u, g, e->d_bits, e->d_fi, e->d_ti, e->d_out);
    FM_HIP_TRY(&e->err, hipGetLastError());
    FM_HIP_TRY(&e->err, hipEventRecord(e->e1, st));
    FM_HIP_TRY(&e->err, hipStreamSynchronize(st));
    FM_HIP_TRY(&e->err, hipEventElapsedTime(&e->last_ms, e->e0, e->e1));
    e->last_n = n;
    return FM_OK;
}

int check_call(fm_mjpeg_enc* e, const void* frames, int n) {
    if (!e) return FM_EINVAL;
    if (!e->d_coef) return fm::failf(&e->err, FM_ESTATE, "the encoder was not created");
    if (!frames) return fm::failf(&e->err, FM_EINVAL, "null frames");
    if (n < 1 || n > e->max_frames) return fm::failf(&e->err, FM_EINVAL, "%d frames, the encoder takes 1..%d per call", n, e->max_frames);
    return FM_OK;
}

}  // namespace

extern "C" {

int fm_jpeg_header(int width, int height, int quality, int subsampling, int restart_interval, uint8_t* out, size_t cap,
                   size_t* len) {
    if (len) *len = 0;
    if (!valid_settings(width, height, quality, subsampling, restart_interval)) return FM_EINVAL;
    const std::vector<uint8_t> h = make_header(width, height, quality, subsampling, restart_interval);
    if (len) *len = h.size();
    if (!out || cap < h.size()) return FM_EINVAL;
    std::memcpy(out, h.data(), h.size());
    return FM_OK;
}

int fm_mjpeg_enc_create(int device, int width, int height, int max_frames, int quality, int subsampling,
                        int restart_interval, fm_mjpeg_enc** out) {
    if (!out) return FM_EINVAL;
    fm_mjpeg_enc* e = new fm_mjpeg_enc();
    *out = e;
    if (!valid_settings(width, height, quality, subsampling, restart_interval) || max_frames < 1 || max_frames > 65535)
        return fm::failf(&e->err, FM_EINVAL, "bad settings: %dx%d, max_frames %d, quality %d (1..100), subsampling %d (0..2), "
                     "restart interval %d (0..65535)", width, height, max_frames, quality, subsampling, restart_interval);
    EncGeom& g = e->g;
    g.W = width, g.H = height;
    g.hs = subsampling ? 2 : 1, g.vs = subsampling == 2 ? 2 : 1;
    g.mcux = (width + 8 * g.hs - 1) / (8 * g.hs);
    const int mcuy = (height + 8 * g.vs - 1) / (8 * g.vs);
    const long long nmcu = (long long)g.mcux * mcuy;
    g.bpm = g.hs * g.vs + 2;
    if (nmcu * g.bpm > (1 << 20))  // a frame's bit offsets stay below 2^32 at the worst case of ~3500 bits a block
        return fm::failf(&e->err, FM_ENOTSUP, "%dx%d: more than 2^20 blocks per frame", width, height);
    g.nmcu = (int)nmcu, g.nblk = g.nmcu * g.bpm;
    g.ybw = (width + 7) / 8, g.ybh = (height + 7) / 8;
    g.crows = (height + g.vs - 1) / g.vs;
    g.ib = restart_interval && restart_interval < g.nmcu ? restart_interval * g.bpm : 0;
    g.nint = g.ib ? (g.nmcu + restart_interval - 1) / restart_interval : 1;
    for (int t = 0; t < 2; t++) {
        uint8_t q[64];
        quant_table(quality, t, q);
        for (int i = 0; i < 64; i++) e->q.q8[t][i] = (uint16_t)(q[i] * 8);
    }
    e->device = device, e->max_frames = max_frames;
    e->frame_bytes = (size_t)width * height * 3;
    e->header = make_header(width, height, quality, subsampling, restart_interval);
    FM_HIP_TRY(&e->err, hipSetDevice(device));
    FM_HIP_TRY(&e->err, hipStreamCreateWithFlags(e->st.put(), hipStreamNonBlocking));
    FM_HIP_TRY(&e->err, hipEventCreate(e->e0.put()));
    FM_HIP_TRY(&e->err, hipEventCreate(e->e1.put()));
    EncHuff H;
    build_huff(H);
    const size_t nb = (size_t)max_frames * g.nblk;
    FM_HIP_TRY(&e->err, e->d_huff.reserve(1));
    FM_HIP_TRY(&e->err, hipMemcpy(e->d_huff, &H, sizeof H, hipMemcpyHostToDevice));
    FM_HIP_TRY(&e->err, e->d_list.reserve(max_frames));
    FM_HIP_TRY(&e->err, e->d_bits.reserve(nb));
    FM_HIP_TRY(&e->err, e->d_fbits.reserve(max_frames));
    FM_HIP_TRY(&e->err, e->d_fi.reserve(max_frames));
    FM_HIP_TRY(&e->err, e->h_list.reserve(max_frames));
    FM_HIP_TRY(&e->err, e->h_fbits.reserve(max_frames));
    FM_HIP_TRY(&e->err, e->h_fi.reserve(max_frames));
    FM_HIP_TRY(&e->err, e->d_coef.reserve(nb * 64));  // last: check_call tests it
    return FM_OK;
}

void fm_mjpeg_enc_destroy(fm_mjpeg_enc* e) { delete e; }

const char* fm_mjpeg_enc_last_error(const fm_mjpeg_enc* e) { return e ? e->err.c_str() : "null encoder"; }

int fm_mjpeg_encode(fm_mjpeg_enc* e, const uint8_t* frames, int n, int on_device) {
    if (int rc = check_call(e, frames, n)) return rc;
    FM_HIP_TRY(&e->err, hipSetDevice(e->device));
    const uint8_t* base = frames;
    if (!on_device) {
        const size_t want = (size_t)e->max_frames * e->frame_bytes;
        if (int rc = grow(e, e->d_in, want, want, "frame staging")) return rc;
        FM_HIP_TRY(&e->err, hipMemcpyAsync(e->d_in, frames, (size_t)n * e->frame_bytes, hipMemcpyHostToDevice, e->st));
        base = e->d_in;
    }
    for (int i = 0; i < n; i++) e->h_list[i] = base + (size_t)i * e->frame_bytes;
    return encode_list(e, n);
}

int fm_mjpeg_encode_frame_list(fm_mjpeg_enc* e, const uint8_t* const* frames, int n) {
    if (int rc = check_call(e, frames, n)) return rc;
    for (int i = 0; i < n; i++)
        if (!frames[i]) return fm::failf(&e->err, FM_EINVAL, "null frame %d", i);
    FM_HIP_TRY(&e->err, hipSetDevice(e->device));
    for (int i = 0; i < n; i++) e->h_list[i] = frames[i];
    return encode_list(e, n);
}

int fm_mjpeg_enc_get(fm_mjpeg_enc* e, int frame, uint8_t* out, size_t cap, size_t* len) {
    if (len) *len = 0;
    if (!e) return FM_EINVAL;
    if (frame < 0 || frame >= e->last_n) return fm::failf(&e->err, FM_ESTATE, "frame %d: the last call encoded %d", frame, e->last_n);
    const size_t hl = e->header.size(), sl = e->scan_len[frame], need = hl + sl + 2;
    if (len) *len = need;
    if (!out || cap < need) return fm::failf(&e->err, FM_EINVAL, "frame %d needs %zu bytes, the buffer holds %zu", frame, need, cap);
    std::memcpy(out, e->header.data(), hl);
    FM_HIP_TRY(&e->err, hipSetDevice(e->device));
    FM_HIP_TRY(&e->err, hipMemcpyAsync(out + hl, e->d_out + e->h_fi[frame].obase, sl, hipMemcpyDeviceToHost, e->st));
    FM_HIP_TRY(&e->err, hipStreamSynchronize(e->st));
    out[hl + sl] = 0xFF;
    out[hl + sl + 1] = 0xD9;
    return FM_OK;
}

int fm_mjpeg_enc_coefficients(fm_mjpeg_enc* e, int frame, int16_t* out, size_t cap) {
    if (!e) return FM_EINVAL;
    if (frame < 0 || frame >= e->last_n) return fm::failf(&e->err, FM_ESTATE, "frame %d: the last call encoded %d", frame, e->last_n);
    const size_t need = (size_t)e->g.nblk * 64;
    if (!out || cap < need) return fm::failf(&e->err, FM_EINVAL, "frame %d has %zu coefficients, the buffer holds %zu", frame, need, cap);
    FM_HIP_TRY(&e->err, hipSetDevice(e->device));
    FM_HIP_TRY(&e->err, hipMemcpyAsync(out, e->d_coef + (size_t)frame * need, need * sizeof(int16_t), hipMemcpyDeviceToHost, e->st));
    FM_HIP_TRY(&e->err, hipStreamSynchronize(e->st));
    return (int)std::min<size_t>(need, 0x7fffffff);
}

double fm_mjpeg_enc_last_ms(const fm_mjpeg_enc* e) { return e ? (double)e->last_ms : 0.0; }

}  // extern "C"
