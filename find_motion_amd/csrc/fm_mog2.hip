// fm_mog2.hip — a Gaussian-mixture background model (FM_FLAG_MOG2) in place of the running average: what a user
// gets who swaps cv2.createBackgroundSubtractorMOG2 into find_diff (fm.py:638-662), `fgmask = mog2.apply(frame.blur)`,
// then dilates and runs findContours as before.  The author's fifth TODO at the top of find_motion.py points at
// OpenCV's video module; this is its workhorse, restated from bgfg_gaussmix2.cpp (OpenCV 4.x) for one channel and
// five mixtures.  A pixel that alternates between two values (a flickering lamp, a swaying branch, an interlaced
// field) settles the average between them and fires on every frame; the mixture learns both and stays silent.
//
// The decomposition of fm_small.hip / fm_wide.hip: the blur of a frame depends on that frame alone and runs
// frame-parallel (k_small_blur or k_wide_blur, unchanged, blur bytes [F][x][CS] column-major); only the model is
// sequential in time.
//
//   k_mog2_scan        fm_scan.h's scan_frames: one wave per (stream, image column, 64-row tile row),
//                      lane = row, the frames of the launch in order.  The state of a pixel -- nmodes and five modes
//                      {weight, mean, variance} sorted by weight -- sits in 15 VGPRs + 1 for the launch's frames.
//                      Registers are not addressable, so every loop over modes is unrolled with compile-time
//                      indices and every data-dependent part (mode < nmodes, the bubble-up, mode - swaps, the new
//                      mode's slot) is a select; a mode no lane of the wave uses is skipped by a wave-uniform
//                      branch.  __ballot(mask == 255) is the tile's column word (a shadow, 127, is no foreground).
//   k_mog2_background  getBackgroundImage of one stream, a thread per pixel.
//
// State in HBM, structure-of-arrays and column-major like the blur bytes: float planes [S][15][x][CS] (field =
// 5 * {weight, mean, var} + mode) and uint8 nmodes [S][x][CS], so a wave's 64 lanes touch consecutive addresses.
// Mode m's three planes are loaded and stored only in lanes with m < nmodes: 1 + 12 nmodes bytes each way per
// pixel and launch.  Entries at mode >= nmodes are never read: their content is "don't care".  A pixel is owned by
// one lane of one wave and the launches of a context run in order on its pixel stream, so the state is updated in
// place.
//
// Every float operation is one separately rounded IEEE operation (-ffp-contract=off; the divisions are the
// compiler's correctly rounded sequence), in OpenCV's order, so the model is bit-identical to the scalar C++.
#include "fm_scan.h"

namespace fm {
namespace mg {

constexpr int NM = 5;     // mixtures: the register budget of k_mog2_scan
constexpr int BGT = 256;  // k_mog2_background threads

struct Mog2Args {
    const uint8_t* blur;   // [F][x][CS] blur bytes of the launch's batch
    float* state;          // [S][15][w][CS]
    uint8_t* nmodes;       // [S][w][CS]
    const float* alphaT;   // [T][S] learning rate of frame t of stream s, (float) of the double the host computed
    Geom g;
    float Tb, Tg, TB, var_init, var_min, var_max, CT, tau;
    int shadows;
};

struct Px {
    float w[NM], m[NM], v[NM];
    int nm;
};

__device__ __forceinline__ void swap_if(bool c, float& x, float& y) {
    const float t = x;
    x = c ? y : x;
    y = c ? t : y;
}

// One frame of one pixel: BackgroundSubtractorMOG2::apply's per-pixel body for blur value d at rate alphaT.
// Returns mask == 255.
__device__ __forceinline__ bool mog2_step(Px& p, float d, float alphaT, const Mog2Args& a) {
    const float alpha1 = 1.f - alphaT, prune = -alphaT * a.CT, nprune = -prune;
    bool bgd = false, fits = false;
    float total = 0.f;
#pragma unroll
    for (int M = 0; M < NM; M++) {
        const bool act = M < p.nm;  // (nmodes may have shrunk in an earlier iteration; it never grows here)
        if (__builtin_amdgcn_ballot_w64(act) == 0) break;  // wave-uniform: no lane has this mode
        float wg = alpha1 * p.w[M] + prune;
        const float var = p.v[M], dd = p.m[M] - d, dist2 = dd * dd;
        const bool look = act && !fits;
        bgd = bgd || (look && total < a.TB && dist2 < a.Tb * var);
        const bool fit = look && dist2 < a.Tg * var;
        fits = fits || fit;
        const float wf = wg + alphaT;
        wg = fit ? wf : wg;
        const float k = alphaT / wg;
        const float mn = p.m[M] - k * dd;
        float vn = var + k * (dist2 - var);
        vn = vn < a.var_min ? a.var_min : vn;  // MAX(varnew, varMin)
        vn = vn > a.var_max ? a.var_max : vn;  // MIN(varnew, varMax)
        p.m[M] = fit ? mn : p.m[M];
        p.v[M] = fit ? vn : p.v[M];
        // bubble up while the new weight is not below the neighbour's (w[M] still holds the old weight, which
        // travels with the swaps and is overwritten below)
        int swaps = 0;
        bool go = fit;
#pragma unroll
        for (int i = M; i > 0; i--) {
            go = go && !(wg < p.w[i - 1]);
            swaps += go ? 1 : 0;
            swap_if(go, p.w[i], p.w[i - 1]);
            swap_if(go, p.m[i], p.m[i - 1]);
            swap_if(go, p.v[i], p.v[i - 1]);
        }
        const bool pr = act && wg < nprune;
        wg = pr ? 0.f : wg;
        p.nm -= pr ? 1 : 0;
        const int dst = M - swaps;
#pragma unroll
        for (int j = 0; j <= M; j++) p.w[j] = (act && dst == j) ? wg : p.w[j];
        total = act ? total + wg : total;
    }
    const float inv = 1.f / total;
#pragma unroll
    for (int j = 0; j < NM; j++) p.w[j] = j < p.nm ? p.w[j] * inv : p.w[j];
    // no mode took the value: a new one, in place of the weakest when all five are in use
    const bool nw = !fits && alphaT > 0.f;
    if (__builtin_amdgcn_ballot_w64(nw) != 0) {
        const int slot = min(p.nm, NM - 1), nm2 = min(p.nm + 1, NM);
        p.nm = nw ? nm2 : p.nm;
#pragma unroll
        for (int j = 0; j < NM; j++) {
            const bool at = nw && j == slot, below = nw && j < slot;
            const float ws = p.w[j] * alpha1;
            p.w[j] = at ? (nm2 == 1 ? 1.f : alphaT) : below ? ws : p.w[j];
            p.m[j] = at ? d : p.m[j];
            p.v[j] = at ? a.var_init : p.v[j];
        }
        bool go = nw;
#pragma unroll
        for (int i = NM - 1; i > 0; i--) {
            const bool here = i <= slot;
            const bool sw = go && here && !(alphaT < p.w[i - 1]);
            go = here ? sw : go;
            swap_if(sw, p.w[i], p.w[i - 1]);
            swap_if(sw, p.m[i], p.m[i - 1]);
            swap_if(sw, p.v[i], p.v[i - 1]);
        }
    }
    // detectShadowGMM on the updated model, where the pixel is not background
    bool shadow = false;
    if (a.shadows && __builtin_amdgcn_ballot_w64(!bgd) != 0) {
        bool done = bgd;
        float t = 0.f;
#pragma unroll
        for (int M = 0; M < NM; M++) {
            const bool act = !done && M < p.nm;
            if (__builtin_amdgcn_ballot_w64(act) == 0) break;
            const float num = d * p.m[M], den = p.m[M] * p.m[M];
            const bool z = den == 0.f;
            const bool cand = act && !z && num <= den && num >= a.tau * den;
            const float aa = num / den;
            const float dD = aa * p.m[M] - d;
            const bool hit = cand && dD * dD < a.Tb * p.v[M] * aa * aa;
            shadow = shadow || hit;
            done = done || hit || (act && z);
            t = t + p.w[M];
            done = done || (act && t > a.TB);
        }
    }
    return !bgd && !shadow;
}

struct Mixture {  // scan_frames' model: the pixel's modes, and each frame's learning rate beside its blur byte
    struct Group {
        uint32_t b[PFD];
        float al[PFD];
    };
    const Mog2Args& a;
    int CS;
    Px p;
    size_t PS, fstride;
    float* sp;
    uint8_t* np;
    const uint8_t* base;
    const float* al;
    __device__ __forceinline__ void open(const Lane& l) {
        // the pixel's state: field f of stream s at state[((s * 15 + f) * w + x) * CS + y]
        PS = (size_t)a.g.w * CS;
        const size_t pix = (size_t)l.x * CS + l.y;
        sp = a.state + (size_t)l.s * 15 * PS + pix;
        np = a.nmodes + (size_t)l.s * PS + pix;
        p.nm = l.valid ? (int)*np : 0;
#pragma unroll
        for (int M = 0; M < NM; M++) {
            const bool has = M < p.nm;
            p.w[M] = has ? sp[(size_t)M * PS] : 0.f;
            p.m[M] = has ? sp[(size_t)(NM + M) * PS] : 0.f;
            p.v[M] = has ? sp[(size_t)(2 * NM + M) * PS] : 0.f;
        }
        // blur bytes of frame t of this pixel: blur[((t * S + s) * w + x) * CS + y]
        fstride = (size_t)a.g.S * a.g.w * CS;
        base = a.blur + (size_t)l.s * a.g.w * CS + (size_t)l.x * CS + l.y;
        al = a.alphaT + l.s;  // frame t: al[t * S] (wave-uniform)
    }
    __device__ __forceinline__ void load(Group& r, int k, int tc) const {
        r.b[k] = base[(size_t)tc * fstride];
        r.al[k] = al[(size_t)tc * a.g.S];
    }
    __device__ __forceinline__ void step(const Group& r, int k, int, bool& fg) {
        fg = mog2_step(p, (float)r.b[k], r.al[k], a);
    }
    __device__ __forceinline__ void close(const Lane& l) const {
        if (l.valid) {
            *np = (uint8_t)p.nm;
#pragma unroll
            for (int M = 0; M < NM; M++)
                if (M < p.nm) {
                    sp[(size_t)M * PS] = p.w[M];
                    sp[(size_t)(NM + M) * PS] = p.m[M];
                    sp[(size_t)(2 * NM + M) * PS] = p.v[M];
                }
        }
    }
};

__global__ __launch_bounds__(ST) void k_mog2_scan(Mog2Args a, int CS) {
    scan_frames(a.g, Mixture{a, CS});
}

// getBackgroundImage: the weighted mean of the strongest modes up to background_ratio, [h][w] row-major
__global__ __launch_bounds__(BGT) void k_mog2_background(const float* __restrict__ state, const uint8_t* __restrict__ nmodes,
                                                         uint8_t* __restrict__ out, int s, int h, int w, int CS, float TB) {
    const int i = blockIdx.x * BGT + threadIdx.x;
    if (i >= h * w) return;
    const int y = i / w, x = i - y * w;
    const size_t PS = (size_t)w * CS, pix = (size_t)x * CS + y;
    const float* sp = state + (size_t)s * 15 * PS + pix;
    const int nm = nmodes[(size_t)s * PS + pix];
    float mv = 0.f, total = 0.f;
    for (int M = 0; M < nm && M < NM; M++) {
        const float wt = sp[(size_t)M * PS];
        mv = mv + wt * sp[(size_t)(NM + M) * PS];
        total = total + wt;
        if (total > TB) break;
    }
    const float inv = 1.f / total;
    const int q = nm ? min(max(__float2int_rn(mv * inv), 0), 255) : 0;
    out[i] = (uint8_t)q;
}

}  // namespace mg

size_t mog2_state_floats(int S, int w, int nty) { return (size_t)S * 15 * w * nty * 64; }
size_t mog2_nmodes_bytes(int S, int w, int nty) { return (size_t)S * w * nty * 64; }

// the scan of frames [a.t_begin, a.t_end) over blur bytes [F][x][a.nty * 64] that are already written and whose
// tile flags and padding bit words are cleared (k_small_blur or k_wide_blur); m.alphaT holds a.T * a.S rates
hipError_t launch_mog2_scan(hipStream_t st, const FusedArgs& a, const Mog2Dev& m, const uint8_t* blur, uint64_t* ks) {
    mg::Mog2Args r{};
    r.blur = blur;
    r.state = m.state;
    r.nmodes = m.nmodes;
    r.alphaT = m.alphaT;
    r.g = geom_of(a);
    r.g.kstamp = ks;
    r.Tb = m.prm.var_threshold, r.Tg = m.prm.var_threshold_gen, r.TB = m.prm.background_ratio;
    r.var_init = m.prm.var_init, r.var_min = m.prm.var_min, r.var_max = m.prm.var_max;
    r.CT = m.prm.complexity_reduction, r.tau = m.prm.shadow_tau;
    r.shadows = m.prm.detect_shadows != 0;
    const int njobs = a.S * a.w * a.nty;
    const dim3 grid((njobs + ST / 64 - 1) / (ST / 64));
    hipLaunchKernelGGL(mg::k_mog2_scan, grid, dim3(ST), 0, st, r, a.nty * 64);
    return hipGetLastError();
}

hipError_t launch_mog2_background(hipStream_t st, const Mog2Dev& m, int s, int h, int w, int nty, uint8_t* out) {
    const int n = h * w;
    hipLaunchKernelGGL(mg::k_mog2_background, dim3((n + mg::BGT - 1) / mg::BGT), dim3(mg::BGT), 0, st, m.state, m.nmodes, out,
                       s, h, w, nty * 64, m.prm.background_ratio);
    return hipGetLastError();
}

}  // namespace fm
