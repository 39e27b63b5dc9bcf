// fm_roi.h — cv2.resize(INTER_AREA)'s choice of path, and the frames -> ROI stage of the detectors
// (find_objects' imutils.resize(raw, width=roi_w)), fm_roi.cpp.
#pragma once

#include "fm_host.h"
#include "fm_internal.h"

namespace fm {

// cv::resize: a copy at equal sizes; INTER_AREA needs scale >= 1 on both axes (Upscale otherwise) and
// takes the integer-factor path when both scales are whole numbers (isx, isy).
struct AreaMode {
    enum Kind { Identity, Fast, General, Upscale } kind = Identity;
    double sx = 1., sy = 1.;
    int isx = 1, isy = 1;
};
AreaMode area_resize_mode(int src_w, int src_h, int dst_w, int dst_h);

// AreaMode::Upscale: cv::resize runs its 8-bit bilinear resizer with "area mode" taps.  Per destination index
// the two source indices (s1 clamped to the last one) and the 11-bit fixed-point coefficients (a0 + a1 ==
// 2048); tab[d] = s0 << 12 | a1 is what k_resize_area_up reads.  false for an axis whose source index does
// not fit in 20 bits.  ([OCV] restated from resize.cpp; parity to cv2 is not pinned.)
struct AreaUpAxis {
    std::vector<int32_t> s0, s1, a0, a1;
    std::vector<uint32_t> tab;
};
bool build_area_up_axis(int ssize, int dsize, AreaUpAxis& A);
// k_resize_area_up's tiling of a w-wide destination whose rows follow ay (fm_kernels.hip).
AreaUpPlan plan_area_up(const AreaUpAxis& ay, int w);

// n BGR frames resized to width roi_w on a stream, with every buffer the stage needs: the staging copy of
// host frames or of a gathered frame list, the ROI frames, the list's address table, the general path's
// six tap tables (two for an enlarging resize).  All grow-only at their exact size; the tables are kept per (W, H, w, h).
class RoiStage {
public:
    // list_in_place: a frame list is read where its frames lie (k_resize_area_nt's address table) when the
    // general path's taps allow it; otherwise, and always without the flag, the list is gathered first.
    explicit RoiStage(bool list_in_place) : list_in_place_(list_in_place) {}
    // frames narrower than the ROI are enlarged (AreaMode::Upscale) instead of refused; off by default
    void allow_upscale(bool on) { allow_upscale_ = on; }

    // Consecutive [n][H][W][3] frames at `frames` (host memory, or device memory when on_device), or --
    // list != nullptr -- the n device frames at list[i].  Everything is queued on st (a change of the tap
    // tables waits for it first); *roi is the device address of the n ROI frames of *roi_h rows, the
    // source itself when the sizes are equal.  The list staging is reused by the next call: the caller
    // synchronises st between calls.
    int run(std::string* err, hipStream_t st, const uint8_t* frames, const uint8_t* const* list, int n, int H, int W,
            bool on_device, int roi_w, const uint8_t** roi, int* roi_h);

private:
    bool list_in_place_;
    bool allow_upscale_ = false;
    DevBuf<uint8_t> raw_, roi_;
    DevBuf<const uint8_t*> list_;  // the frames' device addresses
    PinBuf<const uint8_t*> hlist_;  // their page-locked staging copy (an asynchronous DMA)
    DevBuf<int32_t> xofs_, xcnt_, yofs_, ycnt_;
    DevBuf<float> xwt_, ywt_;
    int area_key_[4] = {0, 0, 0, 0};  // (W, H, w, h) the tap tables are for; W == 0 while they change
    AreaAxis ax_, ay_;
    DevBuf<uint32_t> upx_, upy_;  // the Upscale branch's tables, under the same key
    AreaUpPlan up_{};
};

}  // namespace fm
