// fm_tables.cpp — the host-side tables OpenCV builds per call, built once per context:
// the INTER_AREA taps and the fixed-point Gaussian taps.  Plain host code.
#include <algorithm>
#include <cmath>

#include "fm_internal.h"

namespace fm {

// computeResizeAreaTab (OpenCV imgproc resize.cpp) restated on the product
// side: for each destination index the weights over consecutive source
// indices, in the order OpenCV accumulates them.
bool build_area_axis(int ssize, int dsize, double scale, AreaAxis& A) {
    A.n_dst = dsize;
    std::vector<std::vector<std::pair<int, float>>> taps(dsize);
    for (int dx = 0; dx < dsize; dx++) {
        const double fsx1 = dx * scale, fsx2 = fsx1 + scale;
        const double cell = std::min(scale, ssize - fsx1);
        int sx1 = (int)std::ceil(fsx1), sx2 = (int)std::floor(fsx2);
        sx2 = std::min(sx2, ssize - 1);
        sx1 = std::min(sx1, sx2);
        auto& t = taps[dx];
        if (sx1 - fsx1 > 1e-3) t.emplace_back(sx1 - 1, (float)((sx1 - fsx1) / cell));
        for (int sx = sx1; sx < sx2; sx++) t.emplace_back(sx, (float)(1.0 / cell));
        if (fsx2 - sx2 > 1e-3) t.emplace_back(sx2, (float)(std::min(std::min(fsx2 - sx2, 1.), cell) / cell));
    }
    A.max_taps = 1;
    for (auto& t : taps) A.max_taps = std::max<int>(A.max_taps, (int)t.size());
    A.ofs.assign(dsize, 0);
    A.cnt.assign(dsize, 0);
    A.wt.assign((size_t)dsize * A.max_taps, 0.f);
    for (int d = 0; d < dsize; d++) {
        auto& t = taps[d];
        if (t.empty()) return false;
        A.ofs[d] = t[0].first;
        A.cnt[d] = (int)t.size();
        for (size_t j = 0; j < t.size(); j++) {
            if (t[j].first != t[0].first + (int)j) return false;  // taps must be consecutive
            A.wt[(size_t)d * A.max_taps + j] = t[j].second;
        }
    }
    return true;
}

// getGaussianKernelBitExact + getGaussianKernelFixedPoint_ED (OpenCV imgproc
// smooth.dispatch.cpp) restated: the 8-bit fixed-point taps GaussianBlur
// uses for CV_8U with sigma = 0.
bool gaussian_taps(int n, std::vector<int32_t>& out) {
    if (n < 1 || (n & 1) == 0 || n > kMaxK) return false;
    std::vector<double> kd(n);
    switch (n) {
        case 1: kd = {1.0}; break;
        case 3: kd = {0.25, 0.5, 0.25}; break;
        case 5: kd = {0.0625, 0.25, 0.375, 0.25, 0.0625}; break;
        case 7: kd = {0.03125, 0.109375, 0.21875, 0.28125, 0.21875, 0.109375, 0.03125}; break;
        case 9: kd = {4 / 256., 13 / 256., 30 / 256., 51 / 256., 60 / 256., 51 / 256., 30 / 256., 13 / 256., 4 / 256.}; break;
        default: {
            const double sigma = std::fma((double)n, 0.15, 0.35);
            const double scale2 = -0.125 / (sigma * sigma);
            const int half = (n - 1) / 2;
            std::vector<double> v(half);
            double sum = 0;
            for (int i = 0, x = 1 - n; i < half; i++, x += 2) {
                v[i] = std::exp((double)(x * x) * scale2);
                sum += v[i];
            }
            sum = sum * 2 + 1;
            for (int i = 0; i < half; i++) kd[i] = kd[n - 1 - i] = v[i] / sum;
            kd[half] = 1 / sum;
        }
    }
    out.assign(n, 0);
    const int half = n / 2;
    double err = 0;
    int64_t s = 0;
    for (int i = 0; i < half; i++) {
        const double adj = kd[i] * 256 + err;
        const int64_t v0 = (int64_t)std::nearbyint(adj);
        err = adj - (double)v0;
        out[i] = out[n - 1 - i] = (int32_t)v0;
        s += v0;
    }
    out[half] = (int32_t)(256 - 2 * s);
    return true;
}

}  // namespace fm
