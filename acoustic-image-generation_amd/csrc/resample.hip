// Band-limited sample-rate conversion of one mono clip on the GPU: the windowed-sinc interpolation of resampy's
// `resample_f` that `librosa.core.resample(data * 1.0, fs, 12288)` runs in convert_data2.py:35, then `np.int32(...)`.
// The caller passes the filter's right wing `win` (already multiplied by the ratio when downsampling) and its first
// differences `delta` (a 0 appended), both fp64 [nwin], built once on the host (acimg/convert_boxes.py: sinc_window);
// `num_table` entries lie between two zero crossings.  ONE THREAD per output sample t, fp64, every product and sum rounded
// on its own (`fp contract(off)`: no fused multiply-adds), so that tests/resample_ref.py restates it bit for bit:
//     time = t * (1 / ratio);  n = (long)time;  scale = min(1, ratio);  step = (int)(scale * num_table)
//     left wing:   frac = scale * (time - n);  pos = frac * num_table;  o = (int)pos;  eta = pos - o
//                  for i in 0 .. min(n + 1, (nwin - o) / step) - 1:   y += (win[o + i step] + eta delta[o + i step]) * x[n - i]
//     right wing:  frac = scale - frac;  pos, o, eta as above
//                  for k in 0 .. min(len - n - 1, (nwin - o) / step) - 1:   y += (...) * x[n + k + 1]
// (resampy advances `time` by repeated addition; the product makes the samples independent - DESIGN section 8.)
// Samples t >= n_calc = (long)(len * ratio) are the zeros librosa pads to ceil(len * ratio) with.  yi = y truncated toward
// zero and clamped to the int32 range.  No atomics: bit-identical from run to run.
#include <cmath>

#include "common.hpp"

namespace acimg {

__global__ __launch_bounds__(256) void resample_sinc_kernel(const int32_t* x, long len, const double* win, const double* delta,
                                                            int nwin, int num_table, int step, double scale, double time_inc,
                                                            long n_calc, long n_out, double* y, int32_t* yi) {
    // every product and sum below is rounded on its own: with contraction on, the compiler fuses weight * x into the sum
    // (and eta * delta into the weight), and the last bits leave the restatement's
#pragma clang fp contract(off)
    const long t = (long)blockIdx.x * 256 + threadIdx.x;
    if (t >= n_out) return;
    double acc = 0.0;
    const double time = (double)t * time_inc;
    const long n = (long)time;
    if (t < n_calc && n < len) {   // n < len always holds for t < n_calc; the test keeps every read inside x
        double frac = scale * (time - (double)n);
        double pos = frac * (double)num_table;
        int o = (int)pos;
        double eta = pos - (double)o;
        long taps = o <= nwin ? (nwin - o) / step : 0;
        if (taps > n + 1) taps = n + 1;
        for (long i = 0; i < taps; ++i) {
            const long w = o + i * step;
            const double weight = win[w] + eta * delta[w];
            acc = acc + weight * (double)x[n - i];
        }
        frac = scale - frac;
        pos = frac * (double)num_table;
        o = (int)pos;
        eta = pos - (double)o;
        taps = o <= nwin ? (nwin - o) / step : 0;
        if (taps > len - n - 1) taps = len - n - 1;
        for (long k = 0; k < taps; ++k) {
            const long w = o + k * step;
            const double weight = win[w] + eta * delta[w];
            acc = acc + weight * (double)x[n + k + 1];
        }
    }
    if (y) y[t] = acc;
    if (yi) yi[t] = acc >= 2147483647.0 ? INT32_MAX : (acc <= -2147483648.0 ? INT32_MIN : (int32_t)acc);
}

}  // namespace acimg

using namespace acimg;

extern "C" {

long acimg_resample_length(long len, int rate_in, int rate_out, long* computed) {
    if (len < 1 || rate_in < 1 || rate_out < 1) return 0;
    const double ratio = (double)rate_out / (double)rate_in;
    const double exact = (double)len * ratio;
    if (!(exact < 9.0e15)) return 0;
    if (computed) *computed = (long)exact;
    return (long)std::ceil(exact);
}

int acimg_resample_sinc(const int32_t* x, long len, int rate_in, int rate_out, const double* win, const double* delta, int nwin,
                        int num_table, double* y, int32_t* yi, long n_out, void* stream) {
    if (!x || !win || !delta || (!y && !yi)) return fail(ACIMG_EINVAL, "resample_sinc: null argument");
    if (len < 1 || rate_in < 1 || rate_out < 1)
        return fail(ACIMG_EINVAL, "resample_sinc: %ld samples from %d Hz to %d Hz", len, rate_in, rate_out);
    if (num_table < 1 || nwin < 2) return fail(ACIMG_EINVAL, "resample_sinc: a filter of %d entries, %d per crossing", nwin, num_table);
    long n_calc = 0;
    const long want = acimg_resample_length(len, rate_in, rate_out, &n_calc);
    if (want < 1 || n_out != want)
        return fail(ACIMG_EINVAL, "resample_sinc: n_out = %ld, %ld samples at %d Hz give %ld at %d Hz", n_out, len, rate_in, want,
                    rate_out);
    const double ratio = (double)rate_out / (double)rate_in;
    const double scale = ratio < 1.0 ? ratio : 1.0;
    const int step = (int)(scale * num_table);
    if (step < 1) return fail(ACIMG_EINVAL, "resample_sinc: a ratio of %g leaves no table step at %d entries per crossing", ratio, num_table);
    const long grid = (n_out + 255) / 256;
    if (grid > (long)INT32_MAX) return fail(ACIMG_EINVAL, "resample_sinc: %ld samples exceed the grid", n_out);
    hipLaunchKernelGGL(resample_sinc_kernel, dim3((unsigned)grid), dim3(256), 0, (hipStream_t)stream, x, len, win, delta, nwin,
                       num_table, step, scale, 1.0 / ratio, n_calc, n_out, y, yi);
    return check_launch("resample_sinc");
}

}  // extern "C"
