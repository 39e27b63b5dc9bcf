// fm_wide.hip — the per-pixel motion chain for Gaussian sizes above k_fused's (49) on work images of more
// than kFrameCclTiles tiles: the reference's default blur scale with a raised box (-B 1920 -b 20: k = 97,
// -B 3840: k = 193; fm.py:478-484).  The decomposition of fm_small.hip at any image size: only the f64
// running average is sequential in time, so
//
//   k_wide_blur   every frame of the launch in parallel, one workgroup per (frame, column strip, row band):
//                 gray (fm.py:493), the k x k fixed-point Gaussian (fm.py:494, REFLECT_101 at any distance), the
//                 keep-mask (masked pixels blur to 0, fm.py:619-636) -> blur bytes [F][x][y] (k_small_blur's
//                 column-major layout, column stride CS = nty * 64);
//   k_small_scan  (fm_small.hip, unchanged) the frames in order with the f64 background in a register:
//                 threshold bits as the tile's column words, tile flags, the background after the batch.
//
// k_wide_blur slides down its strip one image row at a time.  A row's gray bytes (the strip's columns plus rp
// columns of halo on either side, reflected) go to LDS once; every thread takes the horizontal sums H of its two
// adjacent columns from them (H = sum_x c_x gray <= 255 * 256: a u16) into an LDS ring of the last span + 1
// rows; the output row rp rows above is the vertical sum over the ring.  Neither gray nor H is ever recomputed
// inside a strip: per output pixel the kernel loads (SW + 2 rp) / SW gray pixels (1.16 at k = 97, SW = 512) and
// computes one H, times (rows + 2 rp) / rows where a frame is cut into row bands (only when a launch has too few
// frames and strips to fill the machine; each band warms its ring up over 2 rp rows).
//
// The taps are the context's coef[] with the zero ends trimmed (exact: OpenCV's 8-bit taps of a wide kernel are
// mostly 0..13 with zeros at both ends, k = 97: non-zero span 6..90): span = 2 rp + 1 taps stay.  Zeros inside
// the span are multiplied like any tap.  Every tap fits a byte, so lane l of each wave keeps taps 4 l .. 4 l + 3
// packed in one register and a step of four taps takes them with one v_readlane (taps read from the kernel
// arguments by a wave-uniform index cost a scalar load and a full lgkmcnt wait per tap: 13 k cycles per row).
//   horizontal  four taps per v_dot4_u32_u8 on gray dwords.  A thread's window starts at byte 2 tid of the row;
//               the row is kept twice, the second copy two bytes ahead, so even and odd threads both read
//               aligned dwords; the second column's bytes are the first's shifted by one (v_alignbyte).
//   vertical    the ring keeps a column's H of two consecutive rows in one dword, so two taps are one
//               v_dot2_u32_u16 and a thread's two columns one ds_read_b64 per row pair.  An output row whose
//               window starts on the odd row of a pair uses the taps shifted by one (a second packed register).
//
// Rows below the band's first output row and above its last come from refl() like the columns, so a radius
// larger than the image (k = 255 on 72 rows) walks back and forth over the same rows: correct at any distance.
#include "fm_scan.h"

namespace fm {
namespace wd {

constexpr int kLds = 160 * 1024;  // LDS of a gfx950 workgroup
typedef unsigned short u16x2_t __attribute__((ext_vector_type(2)));
constexpr int PD = 8;             // rows of a block: loaded together, a block ahead of the rows being summed
constexpr int GP = 4;             // gray pixels a thread loads per row, at most (make_geo checks)

// launch geometry of one (ksize, taps): NT threads own a strip of SW = 2 NT columns
struct Geo {
    int z = 0;      // first tap kept (coef[z .. z + span))
    int span = 1;   // taps kept (odd), rp = span / 2
    int rp = 0;
    int nt = 0;     // threads per workgroup: 256 or 128; 0: no geometry fits
    int gw = 0;     // gray bytes per row: SW + 2 rp
    int gwp = 0;    // bytes of one copy of the gray row: gw + 40 (the dwords read past it meet zero taps or are read ahead and dropped), to 64 mod 128
    int lds = 0;    // bytes: ring u16 [(span + 1) / 2][2 nt][2], gray u8 [PD][2][gwp]
};

inline Geo make_geo(int ksize, const int32_t* coef) {
    Geo g;
    int z = 0;
    while (z < ksize / 2 && coef[z] == 0 && coef[ksize - 1 - z] == 0) z++;
    g.z = z;
    g.span = ksize - 2 * z;
    g.rp = g.span / 2;
    for (int nt : {256, 128}) {
        const int gw = 2 * nt + 2 * g.rp;
        // (64 mod 128 bytes: the two copies, read by the even and the odd lanes of one ds_read_b32, 16 banks apart)
        const int gwp = (gw + 40 - 64 + 127) / 128 * 128 + 64;
        const int lds = (g.span + 1) * nt * 4 + PD * 2 * gwp;
        if (lds <= kLds && gw <= GP * nt) {
            g.nt = nt;
            g.gw = gw;
            g.gwp = gwp;
            g.lds = lds;
            break;
        }
    }
    return g;
}

struct Launch {
    int z, span, rp, gw, gwp;
    int band_rows;  // rows per band (a multiple of 64)
    int CS;         // column stride of the blur scratch: nty * 64
};

template <int NT>
__global__ __launch_bounds__(NT) void k_wide_blur(FusedArgs a, uint8_t* __restrict__ sblur, Launch L) {
    extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
    constexpr int SW = 2 * NT;
    const int h = a.h, w = a.w, S = a.S;
    const int span = L.span, rp = L.rp, GW = L.gw, CS = L.CS;
    const int tid = threadIdx.x;
    const size_t f = (size_t)a.t_begin * S + blockIdx.x;  // frame of the batch (t * S + s)
    const int s = (int)(f % S);
    const int x0 = blockIdx.y * SW;
    const int yb0 = blockIdx.z * L.band_rows;
    const int yb1 = min(yb0 + L.band_rows, h);
    const int yend = (yb1 + 15) & ~15;  // whole groups of 16 rows are stored (<= CS: rows past h are never read)
    const int RP = (span + 1) >> 1;  // row pairs of the ring (span + 1 rows)
    uint16_t* ring = reinterpret_cast<uint16_t*>(lds);  // [RP][SW][2]: H of (row pair, column, row of the pair)
    uint8_t* growA = lds + (size_t)RP * SW * 4;         // [PD][2][gwp]: gray of columns x0 - rp .. x0 + SW + rp - 1
    uint8_t* growB = growA + L.gwp;                     // (reflected) of PD rows, and the same two bytes ahead
    kstamp_begin_grid(a.kstamp);
    if (blockIdx.y == 0 && blockIdx.z == 0) clear_tile_frame(geom_of(a), f, tid, NT);  // the scan's precondition
    // the source byte offsets of this thread's gray pixels within a row (the same in every row)
    int sxo[GP];
#pragma unroll
    for (int k = 0; k < GP; k++) {
        const int i = tid + k * NT;
        sxo[k] = 3 * refl(x0 - rp + min(i, GW - 1), w);  // (past GW: a valid pixel, loaded and dropped)
    }
    const uint8_t* src = a.src + f * (size_t)h * w * 3;
    // The strip advances in blocks of PD rows: the block's source bytes are loaded together (one memory latency a
    // block; a row at a time, every row waited a whole one -- 3 us a row whatever k, a workgroup being alone on
    // its CU at most sizes), the next block's while this one is summed.
    uint32_t pb[PD][GP], pg[PD][GP], pr[PD][GP];
    auto load_block = [&](int vb) __attribute__((always_inline)) {
        // (unconditional, rows past the last included: a load under a branch is waited for where it is issued)
#pragma unroll
        for (int d = 0; d < PD; d++) {
            const uint8_t* row = src + (size_t)refl(vb + d, h) * w * 3;
#pragma unroll
            for (int k = 0; k < GP; k++) {
                pb[d][k] = row[sxo[k]];
                pg[d][k] = row[sxo[k] + 1];
                pr[d][k] = row[sxo[k] + 2];
            }
        }
    };
    // lane l's four taps 4 l .. 4 l + 3 of the kept ones, a byte each (E4), and 4 l - 1 .. 4 l + 2 (O4)
    uint32_t E4 = 0, O4 = 0;
    {
        const int l4 = 4 * (tid & 63);
#pragma unroll
        for (int q = 0; q < 4; q++) {
            const int te = l4 + q, to = l4 + q - 1;
            if (te < span) E4 |= (uint32_t)a.coef[L.z + te] << (8 * q);
            if (to >= 0 && to < span) O4 |= (uint32_t)a.coef[L.z + to] << (8 * q);
        }
    }
    const bool hk = a.has_keep[s] != 0;
    const uint8_t* keep = a.keep + (size_t)s * h * w;
    const int xa = x0 + 2 * tid, xb = xa + 1;  // this thread's columns
    uint8_t* out = sblur + f * (size_t)w * CS;
    uint32_t cur0 = 0, cur1 = 0;  // the blur bytes of 4 rows, then of 16 (q*), of either column
    uint32_t qa0 = 0, qa1 = 0, qa2 = 0, qb0 = 0, qb1 = 0, qb2 = 0;
    const int v0 = yb0 - rp, v1 = yend - 1 + rp;
    int slot = 0;  // ring row of image row v: (v - v0) % (span + 1)
    load_block(v0);
    for (int vb = v0; vb <= v1; vb += PD) {
        // (every thread is past the barrier behind the last H of the previous block: its gray rows are free)
#pragma unroll
        for (int d = 0; d < PD; d++)
#pragma unroll
            for (int k = 0; k < GP; k++)
                if (tid + k * NT < GW) {
                    const int i = tid + k * NT;
                    const uint8_t g = (uint8_t)gray_px(pb[d][k], pg[d][k], pr[d][k]);
                    growA[d * 2 * L.gwp + i] = g;
                    if (i >= 2) growB[d * 2 * L.gwp + i - 2] = g;
                }
        if (vb + PD <= v1) load_block(vb + PD);  // in flight during this block's arithmetic
        __syncthreads();  // the block's gray is in LDS; every thread has finished the previous block's last output row
        for (int d = 0; d < PD; d++) {
        const int v = vb + d;
        if (v > v1) break;  // (workgroup-uniform)
        const uint8_t* gA = growA + d * 2 * L.gwp;
        {   // H of columns xa, xb: gray bytes 2 tid + j and 2 tid + 1 + j, j = 0 .. span - 1, four taps a step
            const uint32_t* g4 = reinterpret_cast<const uint32_t*>((tid & 1) ? gA + L.gwp + 2 * tid - 2 : gA + 2 * tid);
            uint32_t h0 = 0, h1 = 0;
            // four steps an iteration, the next iteration's dwords read ahead of this one's sums (one wave on a
            // SIMD: nothing else covers the LDS latency); steps past the taps meet zero taps
            uint32_t c0 = g4[0], c1 = g4[1], c2 = g4[2], c3 = g4[3], c4 = g4[4];
            const int M4 = (span + 15) >> 4;
            for (int m = 0; m < 4 * M4; m += 4) {
                const uint32_t n1 = g4[m + 5], n2 = g4[m + 6], n3 = g4[m + 7], n4 = g4[m + 8];
                const uint32_t t0 = (uint32_t)__builtin_amdgcn_readlane((int)E4, m);
                const uint32_t t1 = (uint32_t)__builtin_amdgcn_readlane((int)E4, m + 1);
                const uint32_t t2 = (uint32_t)__builtin_amdgcn_readlane((int)E4, m + 2);
                const uint32_t t3 = (uint32_t)__builtin_amdgcn_readlane((int)E4, m + 3);
                h0 = __builtin_amdgcn_udot4(c0, t0, h0, false);
                h1 = __builtin_amdgcn_udot4(__builtin_amdgcn_alignbyte(c1, c0, 1), t0, h1, false);
                h0 = __builtin_amdgcn_udot4(c1, t1, h0, false);
                h1 = __builtin_amdgcn_udot4(__builtin_amdgcn_alignbyte(c2, c1, 1), t1, h1, false);
                h0 = __builtin_amdgcn_udot4(c2, t2, h0, false);
                h1 = __builtin_amdgcn_udot4(__builtin_amdgcn_alignbyte(c3, c2, 1), t2, h1, false);
                h0 = __builtin_amdgcn_udot4(c3, t3, h0, false);
                h1 = __builtin_amdgcn_udot4(__builtin_amdgcn_alignbyte(c4, c3, 1), t3, h1, false);
                c0 = c4, c1 = n1, c2 = n2, c3 = n3, c4 = n4;
            }
            uint16_t* hw = ring + ((size_t)(slot >> 1) * SW + 2 * tid) * 2 + (slot & 1);
            hw[0] = (uint16_t)h0;
            hw[2] = (uint16_t)h1;
        }
        // The ring holds rows v - span .. v.  One barrier a row: the next row's H goes to the ring row that this
        // row's sum reads under a zero tap only (slot + 1), and a thread reaches the row after that only through
        // the next barrier, behind every thread's sum of this row.
        __syncthreads();
        const int y = v - rp;
        if (y >= yb0) {  // (workgroup-uniform)
            uint32_t acc0 = 32768u, acc1 = 32768u;
            // the window's first row v - span + 1 is ring row slot + 2; from the pair that holds it, two pairs
            // (four taps) a step: the even-aligned taps, or the ones shifted by a row.  Pairs past the window
            // (the step count rounds up; they wrap inside the ring) meet zero taps.
            int rs = slot + 2;
            rs = rs >= span + 1 ? rs - (span + 1) : rs;
            const uint32_t tsel = (rs & 1) ? O4 : E4;
            int pr_ = rs >> 1;
            const uint2* ring2 = reinterpret_cast<const uint2*>(ring) + tid;  // pair row p: ring2[p * NT]
            const int G2 = (RP + 3) >> 2;  // four pairs an iteration
            auto next = [&](int p) __attribute__((always_inline)) { return p + 1 == RP ? 0 : p + 1; };
            auto pairs = [](uint32_t t4, uint32_t& ta, uint32_t& tb) __attribute__((always_inline)) {
                ta = (t4 & 0xFFu) | ((t4 & 0xFF00u) << 8);
                tb = ((t4 >> 16) & 0xFFu) | ((t4 >> 24) << 16);
            };
            auto dot2 = [](uint32_t hh, uint32_t tt, uint32_t acc) __attribute__((always_inline)) {
                return __builtin_amdgcn_udot2(__builtin_bit_cast(u16x2_t, hh), __builtin_bit_cast(u16x2_t, tt), acc, false);
            };
            // (the next iteration's four pair rows read ahead of this one's sums, as in the horizontal pass)
            uint2 r0, r1, r2, r3;
            auto read4 = [&]() __attribute__((always_inline)) {
                const int p0 = pr_, p1 = next(p0), p2 = next(p1), p3 = next(p2);
                pr_ = next(p3);
                r0 = ring2[p0 * NT], r1 = ring2[p1 * NT], r2 = ring2[p2 * NT], r3 = ring2[p3 * NT];
            };
            read4();
            for (int g = 0; g < 2 * G2; g += 2) {
                const uint2 q0 = r0, q1 = r1, q2 = r2, q3 = r3;
                read4();  // (past the last iteration: pair rows inside the ring, unused)
                uint32_t ta, tb, tc, td;
                pairs((uint32_t)__builtin_amdgcn_readlane((int)tsel, g), ta, tb);
                pairs((uint32_t)__builtin_amdgcn_readlane((int)tsel, g + 1), tc, td);
                acc0 = dot2(q0.x, ta, acc0), acc1 = dot2(q0.y, ta, acc1);
                acc0 = dot2(q1.x, tb, acc0), acc1 = dot2(q1.y, tb, acc1);
                acc0 = dot2(q2.x, tc, acc0), acc1 = dot2(q2.y, tc, acc1);
                acc0 = dot2(q3.x, td, acc0), acc1 = dot2(q3.y, td, acc1);
            }
            uint32_t b0 = acc0 >> 16, b1 = acc1 >> 16;
            if (hk && y < h) {
                if (xa < w && keep[(size_t)y * w + xa] == 0) b0 = 0;
                if (xb < w && keep[(size_t)y * w + xb] == 0) b1 = 0;
            }
            const int sh = 8 * (y & 3);
            cur0 |= b0 << sh;
            cur1 |= b1 << sh;
            if ((y & 3) == 3) {
                if ((y & 15) == 15) {  // rows y - 15 .. y of both columns: 16 bytes each, 16-byte aligned
                    uint8_t* o = out + (size_t)xa * CS + (y - 15);
                    if (xa < w) *reinterpret_cast<uint4*>(o) = make_uint4(qa0, qa1, qa2, cur0);
                    if (xb < w) *reinterpret_cast<uint4*>(o + CS) = make_uint4(qb0, qb1, qb2, cur1);
                }
                qa0 = qa1, qa1 = qa2, qa2 = cur0;
                qb0 = qb1, qb1 = qb2, qb2 = cur1;
                cur0 = cur1 = 0;
            }
        }
        slot = slot == span ? 0 : slot + 1;
        }
    }
    kstamp_end_wg(a.kstamp);
}

}  // namespace wd

bool wide_supported(int ksize, const int32_t* coef) {
    return ksize >= 1 && ksize <= kMaxK && wd::make_geo(ksize, coef).nt != 0;
}

int wide_lds_bytes(int ksize, const int32_t* coef) { return wd::make_geo(ksize, coef).lds; }

// frames [a.t_begin, a.t_end) of the batch: blur of every frame in parallel, then the scan; a.init may mark
// first frames (bg := blur at t_begin).  ks1 / ks2: launch stamps of the two kernels (or nullptr)
hipError_t launch_wide(hipStream_t st, const FusedArgs& a, uint8_t* wblur, uint64_t* ks1, uint64_t* ks2) {
    if (hipError_t e = launch_wide_blur(st, a, wblur, ks1); e != hipSuccess) return e;
    return launch_small_scan(st, a, wblur, ks2);
}

// the blur alone (the Gaussian-mixture scan of fm_mog2.hip follows it too)
hipError_t launch_wide_blur(hipStream_t st, const FusedArgs& a, uint8_t* wblur, uint64_t* ks1) {
    const wd::Geo g = wd::make_geo(a.ksize, a.coef);
    if (g.nt == 0) return hipErrorInvalidValue;
    const int nf = (a.t_end - a.t_begin) * a.S;
    const int sw = 2 * g.nt, strips = (a.w + sw - 1) / sw;
    // Row bands only where frames x strips leave CUs idle (a stream's first frame in its own launch, short
    // batches): each band recomputes 2 rp rows of H, so none is shorter than that, and all start on a tile row.
    const int min_rows = (std::max(32, 2 * g.rp) + 63) / 64 * 64;
    const long long wgs = (long long)nf * strips;
    int bands = (int)std::min<long long>((512 + wgs - 1) / wgs, std::max(1, a.h / min_rows));
    const int band_rows = ((a.h + bands - 1) / bands + 63) / 64 * 64;
    bands = (a.h + band_rows - 1) / band_rows;
    const wd::Launch L{g.z, g.span, g.rp, g.gw, g.gwp, band_rows, a.nty * 64};
    FusedArgs b = a;
    b.kstamp = ks1;
    const dim3 grid(nf, strips, bands);
    if (g.nt == 256) {
        (void)hipFuncSetAttribute((const void*)wd::k_wide_blur<256>, hipFuncAttributeMaxDynamicSharedMemorySize, g.lds);
        hipLaunchKernelGGL(wd::k_wide_blur<256>, grid, dim3(256), g.lds, st, b, wblur, L);
    } else {
        (void)hipFuncSetAttribute((const void*)wd::k_wide_blur<128>, hipFuncAttributeMaxDynamicSharedMemorySize, g.lds);
        hipLaunchKernelGGL(wd::k_wide_blur<128>, grid, dim3(128), g.lds, st, b, wblur, L);
    }
    return hipGetLastError();
}

}  // namespace fm
