// cv2.resize(..., INTER_CUBIC) of 8-bit frames, as convert_data.py:66 calls it: the scalar fixed-point path of OpenCV's
// resize.cpp restated - the position and float32 weight rule of one output coordinate (interpolateCubic), the int16
// weights, and the two int32 passes' arithmetic.  Include it after `#pragma clang fp contract(off)`: the arithmetic is
// OpenCV's only unfused.
#pragma once
#include <math.h>
#include <stdint.h>

namespace acimg {

constexpr int CUBIC_TAPS = 4;
constexpr int CUBIC_COEF_BITS = 11;                         // INTER_RESIZE_COEF_BITS: weights are rint(c * 2048)
constexpr int CUBIC_SHIFT = 2 * CUBIC_COEF_BITS;            // both passes' scale leaves in one shift
constexpr int CUBIC_DELTA = 1 << (CUBIC_SHIFT - 1);

// cv::resize: inv_scale = dsize / ssize, scale = 1 / inv_scale (host fp64, as OpenCV computes it)
inline double cubic_scale(int n_in, int n_out) { return 1.0 / ((double)n_out / n_in); }

// One output coordinate d: the source index s of tap 1 (taps are s - 1 .. s + 2, NOT clamped here: cubic keeps s and f
// at the border and clamps each tap) and the four int16 weights.  Their sum is 2047, 2048 or 2049: OpenCV does not fix
// it up.
inline void cubic_coef(int d, double scale, int& s, int16_t w[CUBIC_TAPS]) {
    const float A = -0.75f;
    float f = (float)((d + 0.5) * scale - 0.5);
    s = (int)floorf(f);
    f -= (float)s;
    float c[CUBIC_TAPS];
    c[0] = ((A * (f + 1) - 5 * A) * (f + 1) + 8 * A) * (f + 1) - 4 * A;
    c[1] = ((A + 2) * f - (A + 3)) * f * f + 1;
    c[2] = ((A + 2) * (1 - f) - (A + 3)) * (1 - f) * (1 - f) + 1;
    c[3] = 1.f - c[0] - c[1] - c[2];
    for (int k = 0; k < CUBIC_TAPS; ++k) {
        const long r = lrintf(c[k] * 2048.0f);              // half to even (the default rounding mode), as cvRound
        w[k] = (int16_t)(r < -32768 ? -32768 : r > 32767 ? 32767 : r);
    }
}

// tap k of an output coordinate whose tap 1 is s
inline int cubic_tap(int s, int k, int n_in) {
    const int t = s - 1 + k;
    return t < 0 ? 0 : t >= n_in ? n_in - 1 : t;
}

// FixedPtCast<int, uchar, 22> of the vertical pass's sum
__host__ __device__ inline uint8_t cubic_cast(int v) {
    const int r = (v + CUBIC_DELTA) >> CUBIC_SHIFT;
    return (uint8_t)(r < 0 ? 0 : r > 255 ? 255 : r);
}

}  // namespace acimg
