// fm_roi.cpp — the INTER_AREA path decision and the detectors' frames -> ROI stage.  Host code.
#include "fm_roi.h"

#include <cmath>
#include <cstring>

namespace fm {

AreaMode area_resize_mode(int src_w, int src_h, int dst_w, int dst_h) {
    AreaMode m;
    if (dst_h == src_h && dst_w == src_w) return m;
    m.sx = 1. / ((double)dst_w / src_w), m.sy = 1. / ((double)dst_h / src_h);
    m.isx = (int)std::lrint(m.sx), m.isy = (int)std::lrint(m.sy);
    if (!(m.sx >= 1 && m.sy >= 1))
        m.kind = AreaMode::Upscale;
    else if (std::fabs(m.sx - m.isx) < 2.220446049250313e-16 && std::fabs(m.sy - m.isy) < 2.220446049250313e-16)
        m.kind = AreaMode::Fast;
    else
        m.kind = AreaMode::General;
    return m;
}

bool build_area_up_axis(int ssize, int dsize, AreaUpAxis& A) {
    if (ssize < 1 || dsize < 1 || ssize >= (1 << 20)) return false;
    A.s0.resize(dsize), A.s1.resize(dsize), A.a0.resize(dsize), A.a1.resize(dsize), A.tab.resize(dsize);
    const double inv = (double)dsize / ssize, scale = 1. / inv;
    for (int dx = 0; dx < dsize; dx++) {
        int sx = (int)std::floor(dx * scale);
        float fx = (float)((dx + 1) - (sx + 1) * inv);
        fx = fx <= 0 ? 0.f : fx - std::floor(fx);
        if (sx < 0) sx = 0, fx = 0.f;
        if (sx >= ssize - 1) sx = ssize - 1, fx = 0.f;
        A.s0[dx] = sx;
        A.s1[dx] = std::min(sx + 1, ssize - 1);
        A.a0[dx] = (int16_t)std::lrintf((1.f - fx) * 2048.f);  // cvRound: to nearest, ties to even
        A.a1[dx] = (int16_t)std::lrintf(fx * 2048.f);
        A.tab[dx] = (uint32_t)sx << 12 | (uint32_t)A.a1[dx];
    }
    return true;
}

// The source rows a band of r destination rows reads: from its first row's first tap to its last row's second.
static int band_source_rows(const AreaUpAxis& ay, int r) {
    const int h = (int)ay.s0.size();
    int ns = 1;
    for (int y0 = 0; y0 < h; y0 += r) ns = std::max(ns, ay.s1[std::min(y0 + r, h) - 1] - ay.s0[y0] + 1);
    return ns;
}

AreaUpPlan plan_area_up(const AreaUpAxis& ay, int w) {
    // spans of at most 1,024 columns, equal to within one; then as many rows (up to 32) as keep the column table
    // and the rows' source bytes and 16-bit horizontal results within 48 KiB, so that three workgroups fit a CU's LDS
    constexpr int kMaxCols = 1024, kMaxRows = 32, kLds = 48 * 1024;
    AreaUpPlan p{};
    p.nspans = (w + kMaxCols - 1) / kMaxCols;
    p.cols = (w + p.nspans - 1) / p.nspans;
    p.nspans = (w + p.cols - 1) / p.cols;
    auto lds = [&](int r, int ns) { return 4 * p.cols + 4 * r + ns * (2 * area_up_hstride(p.cols) + area_up_rawstride(p.cols)); };
    p.rows = 1;
    for (int r = std::min<int>(kMaxRows, (int)ay.s0.size()); r > 1; r--)
        if (lds(r, band_source_rows(ay, r)) <= kLds) {
            p.rows = r;
            break;
        }
    p.nsrc = band_source_rows(ay, p.rows);
    p.lds = lds(p.rows, p.nsrc);
    return p;
}

// one tap table at its exact size
template <class T>
static hipError_t upload(DevBuf<T>& b, const std::vector<T>& v) {
    b.reset();
    if (hipError_t e = b.reserve(v.size())) return e;
    return hipMemcpy(b.get(), v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice);
}

int RoiStage::run(std::string* err, hipStream_t st, const uint8_t* frames, const uint8_t* const* list, int n, int H,
                  int W, bool on_device, int roi_w, const uint8_t** roi, int* roi_h) {
    const int rw = roi_w, rh = (int)(H * ((double)roi_w / (double)W));  // imutils.resize(raw, width=roi_w)
    if (roi_h) *roi_h = rh;
    if (rh < 1) return failf(err, FM_EINVAL, "ROI height 0 for a %dx%d frame", W, H);
    const AreaMode m = area_resize_mode(W, H, rw, rh);
    if (m.kind == AreaMode::Upscale && !allow_upscale_)
        return failf(err, FM_ENOTSUP, "frame width %d < ROI width %d: INTER_AREA upscaling is not supported", W, rw);
    const size_t fb = (size_t)H * W * 3;
    const uint8_t* src = frames;
    const uint8_t* const* dlist = nullptr;
    auto gather = [&]() -> int {
        FM_HIP_TRY(err, raw_.reserve(n * fb));
        for (int i = 0; i < n; i++)
            FM_HIP_TRY(err, hipMemcpyAsync(raw_.get() + (size_t)i * fb, list[i], fb, hipMemcpyDeviceToDevice, st));
        src = raw_.get();
        dlist = nullptr;
        return FM_OK;
    };
    if (list && list_in_place_) {
        // from page-locked memory: a pageable source made this small copy cost ~0.5 ms of host time per
        // call beside a busy pixel stream (FM_HAAR_TIMES); the previous call's copy is done
        FM_HIP_TRY(err, reserve_all((size_t)n, (size_t)n, list_, hlist_));
        std::memcpy((void*)hlist_.get(), list, (size_t)n * sizeof(const uint8_t*));
        FM_HIP_TRY(err, hipMemcpyAsync(list_.get(), hlist_.get(), (size_t)n * sizeof(const uint8_t*), hipMemcpyHostToDevice, st));
        dlist = list_.get();
    } else if (list) {
        if (int rc = gather()) return rc;
    } else if (!on_device) {
        FM_HIP_TRY(err, raw_.reserve(n * fb));
        FM_HIP_TRY(err, hipMemcpyAsync(raw_.get(), frames, n * fb, hipMemcpyHostToDevice, st));
        src = raw_.get();
    }
    if (m.kind == AreaMode::Identity) {
        if (dlist)
            if (int rc = gather()) return rc;
        *roi = src;
        return FM_OK;
    }
    FM_HIP_TRY(err, roi_.reserve((size_t)n * rh * rw * 3));
    if (m.kind == AreaMode::Fast) {
        if (dlist)
            if (int rc = gather()) return rc;
        FM_HIP_TRY(err, launch_resize_area_fast(st, src, roi_.get(), n, H, W, rh, rw, m.isx, m.isy));
    } else if (m.kind == AreaMode::Upscale) {
        const int key[4] = {W, H, rw, rh};
        if (!std::equal(key, key + 4, area_key_)) {
            area_key_[0] = 0;
            AreaUpAxis ux, uy;
            if (!build_area_up_axis(W, rw, ux) || !build_area_up_axis(H, rh, uy))
                return failf(err, FM_ENOTSUP, "frame %dx%d too large for the INTER_AREA upscaling tables", W, H);
            FM_HIP_TRY(err, hipStreamSynchronize(st));
            FM_HIP_TRY(err, upload(upx_, ux.tab));
            FM_HIP_TRY(err, upload(upy_, uy.tab));
            up_ = plan_area_up(uy, rw);
            std::copy(key, key + 4, area_key_);
        }
        // (a frame list is read where its frames lie)
        FM_HIP_TRY(err, launch_resize_area_up(st, src, roi_.get(), n, H, W, rh, rw, upx_.get(), upy_.get(), up_, dlist));
    } else {
        const int key[4] = {W, H, rw, rh};
        if (!std::equal(key, key + 4, area_key_)) {
            area_key_[0] = 0;  // no geometry while the tables change: a failure below leaves them unused
            if (!build_area_axis(W, rw, m.sx, ax_) || !build_area_axis(H, rh, m.sy, ay_))
                return failf(err, FM_ENOTSUP, "INTER_AREA table with non-consecutive taps");
            FM_HIP_TRY(err, hipStreamSynchronize(st));
            FM_HIP_TRY(err, upload(xofs_, ax_.ofs));
            FM_HIP_TRY(err, upload(xcnt_, ax_.cnt));
            FM_HIP_TRY(err, upload(xwt_, ax_.wt));
            FM_HIP_TRY(err, upload(yofs_, ay_.ofs));
            FM_HIP_TRY(err, upload(ycnt_, ay_.cnt));
            FM_HIP_TRY(err, upload(ywt_, ay_.wt));
            std::copy(key, key + 4, area_key_);
        }
        const bool direct = dlist && ((ax_.max_taps + 1) & ~1) <= 32 && fb < (1u << 31);
        if (dlist && !direct)
            if (int rc = gather()) return rc;
        FM_HIP_TRY(err, launch_resize_area(st, src, roi_.get(), n, H, W, rh, rw, xofs_.get(), xcnt_.get(), xwt_.get(),
                                           ax_.max_taps, yofs_.get(), ycnt_.get(), ywt_.get(), ay_.max_taps, dlist));
    }
    *roi = roi_.get();
    return FM_OK;
}

}  // namespace fm
