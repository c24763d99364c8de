// cv2.resize(..., (298, 224)) with INTER_LINEAR of the 36x48 energy-map grid, as the localisation metric (localize.hip)
// and the overlay renderer (render.hip) both restate it: the grid constants, the 8 x 28-row band split of the frame, and
// OpenCV's coefficient rule.  Include it after `#pragma clang fp contract(off)`: the arithmetic is OpenCV's only unfused.
#pragma once
#include <math.h>

namespace acimg {

constexpr int LOC_H = 36, LOC_W = 48, LOC_P = LOC_H * LOC_W;
constexpr int FRAME_H = 224, FRAME_W = 298;
constexpr int BOX_BANDS = 8, BAND_ROWS = FRAME_H / BOX_BANDS;   // 28 output rows per workgroup
constexpr int BAND_SRC_ROWS = 8;                                 // the bands need 5 or 6 source rows
static_assert(BAND_ROWS * BOX_BANDS == FRAME_H, "bands tile the frame");

// cv::resize INTER_LINEAR coefficients of one output coordinate (resize.cpp, the !area_mode branch): source index s and
// float32 weights (w0, w1) on s and s1 = min(s + 1, n_in - 1); f = 0 where the border clamps s.
__host__ __device__ inline void linear_coef(int d, double scale, int n_in, int& s, int& s1, float& w0, float& w1) {
    float f = (float)((d + 0.5) * scale - 0.5);
    s = (int)floorf(f);
    f -= (float)s;
    if (s < 0) {
        s = 0;
        f = 0.f;
    }
    if (s >= n_in - 1) {
        s = n_in - 1;
        f = 0.f;
    }
    s1 = s + 1 < n_in ? s + 1 : n_in - 1;
    w0 = 1.f - f;
    w1 = f;
}

// cv::resize: inv_scale = dsize / ssize, scale = 1 / inv_scale (host fp64, as OpenCV computes it)
inline double resize_scale_x() { return 1.0 / ((double)FRAME_W / LOC_W); }
inline double resize_scale_y() { return 1.0 / ((double)FRAME_H / LOC_H); }

// every band's source rows fit the BAND_SRC_ROWS-row LDS table (a property of the constants, checked where it is used)
inline int band_rows_needed(int band) {
    int lo, hi, t;
    float w0, w1;
    linear_coef(band * BAND_ROWS, resize_scale_y(), LOC_H, lo, t, w0, w1);
    linear_coef(band * BAND_ROWS + BAND_ROWS - 1, resize_scale_y(), LOC_H, t, hi, w0, w1);
    return hi - lo + 1;
}

}  // namespace acimg
