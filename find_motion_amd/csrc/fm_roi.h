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

// n BGR frames resized to width roi_w on a stream, with every buffer the stage needs: the staging copy of
// host frames or of a gathered frame list, the ROI frames, the list's address table, the general path's
// six tap tables.  All grow-only at their exact size; the tables are kept per (W, H, w, h).
class RoiStage {
public:
    // list_in_place: a frame list is read where its frames lie (k_resize_area_nt's address table) when the
    // general path's taps allow it; otherwise, and always without the flag, the list is gathered first.
    explicit RoiStage(bool list_in_place) : list_in_place_(list_in_place) {}

    // Consecutive [n][H][W][3] frames at `frames` (host memory, or device memory when on_device), or --
    // list != nullptr -- the n device frames at list[i].  Everything is queued on st (a change of the tap
    // tables waits for it first); *roi is the device address of the n ROI frames of *roi_h rows, the
    // source itself when the sizes are equal.  The list staging is reused by the next call: the caller
    // synchronises st between calls.
    int run(std::string* err, hipStream_t st, const uint8_t* frames, const uint8_t* const* list, int n, int H, int W,
            bool on_device, int roi_w, const uint8_t** roi, int* roi_h);

private:
    bool list_in_place_;
    DevBuf<uint8_t> raw_, roi_;
    DevBuf<const uint8_t*> list_;  // the frames' device addresses
    PinBuf<const uint8_t*> hlist_;  // their page-locked staging copy (an asynchronous DMA)
    DevBuf<int32_t> xofs_, xcnt_, yofs_, ycnt_;
    DevBuf<float> xwt_, ywt_;
    int area_key_[4] = {0, 0, 0, 0};  // (W, H, w, h) the tap tables are for; W == 0 while they change
    AreaAxis ax_, ay_;
};

}  // namespace fm
