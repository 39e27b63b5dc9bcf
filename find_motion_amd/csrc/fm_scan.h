// fm_scan.h — what the blur + scan pixel paths share (fm_small.hip, fm_wide.hip, fm_rgb.hip, fm_mog2.hip; device
// code, header only).  On these paths the blur of a frame depends on that frame alone and runs frame-parallel; only
// the per-pixel background model is sequential in time.  The scan that runs it is the same kernel around three
// models (the running average, three of them on the colour channels, the Gaussian mixture), and is written once
// here:
//
//   scan_frames   one wave per (stream, image column, 64-row tile row), lane = row: the launch's frames in order
//                 with the model's state in registers.  __ballot of a frame's foreground lanes is the tile's column
//                 word of threshold bits directly (word c = column c, bit r = row r: the contour pass's layout).  A
//                 block of 64 frames' words is held one frame per lane and stored at once, with the frames' flags
//                 ORed atomically into word 0 of each tile-frame's 8 (the reader ORs them) where a word has bits:
//                 no per-frame store, branch or address arithmetic (1,450 -> 1,002 instructions in k_small_scan,
//                 the scan 120 -> 65 us per 256 frames beside the resize, round 5).
//
// The scan's precondition -- the frame's tile flags and the bit words of the columns past the image are zero -- is
// the blur kernels' prologue, clear_tile_frame.
#pragma once

#include "fm_internal.h"

namespace fm {

constexpr int ST = 256;  // threads of a scan kernel (4 waves, each its own job)
constexpr int PFD = 8;   // frames per group of blur-byte loads
constexpr int NG = 2;    // groups in flight (4 and 8: scans 5 % shorter, mode D unchanged, round 5)

__device__ __forceinline__ int refl(int p, int len) {  // BORDER_REFLECT_101 (any distance)
    if ((unsigned)p < (unsigned)len) return p;
    if (len == 1) return 0;
    do {
        p = (p < 0) ? -p : 2 * len - 2 - p;
    } while ((unsigned)p >= (unsigned)len);
    return p;
}

__device__ __forceinline__ uint32_t gray_px(uint32_t b, uint32_t g, uint32_t r) {
    return (b * 1868u + g * 9617u + r * 4899u + 8192u) >> 14;
}

// blur bytes of `frames` frames: [F][channels][x][nty * 64], column-major with the rows padded to whole tiles
inline size_t scan_scratch_bytes(int w, int nty, size_t frames, int channels) {
    return frames * channels * (size_t)w * nty * 64;
}

// what every scan needs of a launch; the scan kernels' own argument structs embed it
struct Geom {
    uint64_t* bits;      // [F][ntiles][64] threshold bits, a word per tile column
    uint32_t* tflag;     // [F][ntiles][8] FLAG_* (word 0 is ORed into)
    int S, h, w;
    int t_begin, t_end;  // frames of the batch this launch processes
    int ntx, nty, ntiles;
    uint64_t* kstamp;
};

__host__ __device__ inline Geom geom_of(const FusedArgs& a) {
    return Geom{a.bits, a.tflag, a.S, a.h, a.w, a.t_begin, a.t_end, a.ntx, a.nty, a.ntiles, a.kstamp};
}

// Frame f's tile flags (the scan ORs into word 0 of each tile's 8) and the bit words of the columns past the image
// in the last tile column (no scan wave writes them), by the nt threads of a workgroup that owns the frame ...
__device__ __forceinline__ void clear_tile_frame(const Geom& g, size_t f, int tid, int nt) {
    for (int i = tid; i < g.ntiles * 8; i += nt) g.tflag[f * g.ntiles * 8 + i] = 0u;
    const int xpad = g.ntx * 64 - g.w;
    for (int i = tid; i < g.nty * xpad; i += nt) {
        const int ty = i / xpad, c = g.w - (g.ntx - 1) * 64 + (i - ty * xpad);
        g.bits[(f * g.ntiles + ty * g.ntx + g.ntx - 1) * 64 + c] = 0ull;
    }
}
// ... or the same of one tile (column tx of the tile grid) by a workgroup that owns the tile-frame
__device__ __forceinline__ void clear_tile_frame(const Geom& g, size_t f, int tile, int tx, int tid, int nt) {
    if (tid < 8) g.tflag[(f * g.ntiles + tile) * 8 + tid] = 0u;
    if (tx == g.ntx - 1)
        for (int c = g.w - tx * 64 + tid; c < 64; c += nt) g.bits[(f * g.ntiles + tile) * 64 + c] = 0ull;
}

// a scan wave's job as its model sees it
struct Lane {
    int s, x;    // stream, image column
    int y;       // this lane's image row, 0 where the row is past the image (a valid address, loaded and dropped)
    bool valid;  // the row is inside the image
    int t0;      // the launch's first frame
};

// The frames [g.t_begin, g.t_end) of one (stream, column, tile row) through a model.  A Model supplies
//   Group                    the registers of one group of PFD prefetched frames;
//   open(lane)               reads its state for this lane;
//   load(group, k, tc)       the loads of frame tc (clamped to the launch: unconditional) into entry k;
//   step(group, k, t, fg)    frame t of this lane's pixel from entry k: fg = foreground (rows past the image are
//                            masked here);
//   close(lane)              writes the state back where lane.valid.
// Everything is inlined into the kernel: the groups and the model's state stay in registers.  Two things keep the
// compiler's code that of a hand-written loop (k_rgb_scan otherwise takes 104 to 110 VGPRs for 81 to 90, a wave
// less per SIMD): the model is taken by value, a local of this function, and step reports through fg, not through
// a return value -- what an inlined function returns is computed at its end, below the model's background update,
// and the values the threshold test needs stay live across it.
template <class Model>
__device__ __forceinline__ void scan_frames(const Geom& g, Model m) {
    const int tid = threadIdx.x, ln = tid & 63;
    kstamp_begin_grid(g.kstamp);
    const int job = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * (ST / 64) + (tid >> 6)));
    const int njobs = g.S * g.w * g.nty;
    if (job < njobs) {
        const int s = job / (g.w * g.nty);
        const int rem = job - s * g.w * g.nty;
        const int ty = rem / g.w, x = rem - ty * g.w;
        const int y = ty * 64 + ln;
        const bool valid = y < g.h;
        const uint64_t vmask = __builtin_amdgcn_ballot_w64(valid);
        const int tile = ty * g.ntx + x / 64, c = x & 63;
        const int t0 = g.t_begin, t1 = g.t_end;
        const Lane lane{s, x, valid ? y : 0, valid, t0};
        m.open(lane);
        const uint32_t flagL = c < 2 ? (FLAG_L) : 0u, flagR = c >= 62 ? FLAG_R : 0u;
        // NG groups of PFD frames in flight (HBM latency is ~2 us beside the resize; one group of 8 frames ahead
        // left the scan waiting for every group)
        typename Model::Group rg[NG];
        // each frame's column word into lane (t - t0) % 64 of (wlo, whi); every 64 frames the
        // block's words are stored (one store, a frame per lane) and their flag words ORed into the tile-frame
        // flags (one atomic, lanes with bits): no per-frame store, branch or address arithmetic
        uint32_t wlo = 0, whi = 0;
        uint64_t* const bits0 = g.bits + ((size_t)s * g.ntiles + tile) * 64 + c;  // frame 0's word of (s, tile, c)
        uint32_t* const flag0 = g.tflag + ((size_t)s * g.ntiles + tile) * 8;
        const size_t bstride = (size_t)g.S * g.ntiles * 64, fstride8 = (size_t)g.S * g.ntiles * 8;
        auto flush = [&](int tb, int n) __attribute__((always_inline)) {  // frames tb .. tb + n - 1 in lanes 0 .. n - 1
            if (ln < n) {
                const size_t ft = (size_t)(tb + ln);
                const uint64_t word = ((uint64_t)whi << 32) | wlo;
                bits0[ft * bstride] = word;
                if (word) {
                    const uint32_t fl = FLAG_ANY | flagL | flagR |
                                        ((word & 3ull) ? (FLAG_T | (c < 2 ? FLAG_TL : 0u) | (c >= 62 ? FLAG_TR : 0u)) : 0u) |
                                        ((word >> 62) ? (FLAG_B | (c < 2 ? FLAG_BL : 0u) | (c >= 62 ? FLAG_BR : 0u)) : 0u);
                    atomicOr(&flag0[ft * fstride8], fl);
                }
            }
        };
        auto load_group = [&](typename Model::Group& r, int tg) __attribute__((always_inline)) {
#pragma unroll
            for (int k = 0; k < PFD; k++) m.load(r, k, min(tg + k, t1 - 1));  // clamped: unconditional
        };
        auto run_group = [&](const typename Model::Group& r, int tg) __attribute__((always_inline)) {
#pragma unroll
            for (int k = 0; k < PFD; k++) {
                const int t = tg + k;
                if (t >= t1) break;  // wave-uniform
                bool fg;
                m.step(r, k, t, fg);
                const uint64_t word = __builtin_amdgcn_ballot_w64(fg) & vmask;
                const int kb = (t - t0) & 63;
                const bool mine = ln == kb;
                wlo = mine ? (uint32_t)word : wlo;
                whi = mine ? (uint32_t)(word >> 32) : whi;
                if (kb == 63) flush(t - 63, 64);
            }
        };
        static_for<NG>([&](auto gi) { load_group(rg[decltype(gi)::value], t0 + decltype(gi)::value * PFD); });
        for (int tg = t0; tg < t1; tg += NG * PFD) {
            static_for<NG>([&](auto gi) {
                constexpr int G = decltype(gi)::value;
                run_group(rg[G], tg + G * PFD);
                load_group(rg[G], tg + (NG + G) * PFD);
            });
        }
        if (const int nrem = (t1 - t0) & 63) flush(t1 - nrem, nrem);  // the last, partial block
        m.close(lane);
    }
    kstamp_end_wg(g.kstamp);
}

}  // namespace fm
