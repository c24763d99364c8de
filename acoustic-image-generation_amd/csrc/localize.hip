// Bounding-box localisation metric of the Flickr-SoundNet evaluation (showimages_bb.py:286-320) on the GPU.
//
// Per sample: the find_logen energy map [36][48] -> mean-threshold mask m2 -> cv2.resize(m2 * 1.0, (298, 224)) with the
// default INTER_LINEAR on a float64 image -> keep > 0.5 -> weighted IoU against the consensus map of up to three
// annotators' boxes (each filled rectangle adds 0.5, the sum is capped at 1).
//
// Exactness: the mask is binary and the consensus map holds 0, 0.5 or 1, so numerator and denominator are multiples of
// 0.5 and are counted as integer half-units (deterministic whatever the order).  The resize is OpenCV's arithmetic:
// float32 weights (1 - f, f) from f = (float)((d + 0.5) * scale - 0.5) - floor, clamped at the borders, applied in
// float64 without fused multiply-adds (this file is compiled with contraction off), so the > 0.5 decision on the tie
// columns 74 and 223 (f = 0.5) is the one the float64 CPU arithmetic makes.
//
// Launch: 8 workgroups per sample, each 28 output rows x 298 columns; each recomputes the sample's mean (the same fp64
// reduction order as mask_iou_kernel, so both metrics threshold identically), holds the 36x48 mask and the horizontal
// pass of the <= 6 source rows its band needs in LDS, and writes one (num, den) pair to the caller's workspace; a
// second launch sums the 8 pairs of each sample in a fixed order.  No atomics.
#include "common.hpp"

#pragma clang fp contract(off)

#include "resize_linear.hpp"

namespace acimg {

__device__ __forceinline__ int wave_sum_i(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

__global__ __launch_bounds__(256) void box_iou_partial_kernel(const float* logen, const int32_t* boxes, double scale_x,
                                                              double scale_y, int* part, uint8_t* mask_out) {
    __shared__ double sm[4];
    __shared__ int smi[8];
    __shared__ uint8_t m[LOC_P];
    __shared__ double h[BAND_SRC_ROWS][FRAME_W];
    __shared__ int rs0[BAND_ROWS], rs1[BAND_ROWS];
    __shared__ float rw0[BAND_ROWS], rw1[BAND_ROWS];
    __shared__ int bx[3][4];
    const int tid = threadIdx.x, wid = tid >> 6, lane = tid & 63;
    const int band = blockIdx.x, n = blockIdx.y;
    const float* map = logen + (long)n * LOC_P;

    // mean(map): mask_iou_kernel's fp64 reduction, term for term
    double s = 0.0;
    for (int i = tid; i < LOC_P; i += 256) s += (double)map[i];
    s = wave_sum_d(s);
    if (lane == 0) sm[wid] = s;
    __syncthreads();
    const double mean = (sm[0] + sm[1] + sm[2] + sm[3]) / (double)LOC_P;
    for (int i = tid; i < LOC_P; i += 256) m[i] = (double)map[i] > mean ? 1 : 0;

    // boxes [4][3] = xmin, xmax, ymin, ymax of annotators 0..2: cv2.rectangle(thickness=-1) fills the closed rectangle
    // between the two corners, clipped to the frame; xmax == 0 means "no annotator"
    if (tid < 3) {
        const int32_t* b = boxes + (long)n * 12;
        const int xa = b[tid], xb = b[3 + tid], ya = b[6 + tid], yb = b[9 + tid];
        int x0 = xa < xb ? xa : xb, x1 = xa < xb ? xb : xa, y0 = ya < yb ? ya : yb, y1 = ya < yb ? yb : ya;
        x0 = x0 < 0 ? 0 : x0;
        y0 = y0 < 0 ? 0 : y0;
        x1 = x1 > FRAME_W - 1 ? FRAME_W - 1 : x1;
        y1 = y1 > FRAME_H - 1 ? FRAME_H - 1 : y1;
        if (xb == 0 || x0 > x1 || y0 > y1) x0 = y0 = 1, x1 = y1 = 0;   // empty
        bx[tid][0] = x0;
        bx[tid][1] = x1;
        bx[tid][2] = y0;
        bx[tid][3] = y1;
    }
    // vertical coefficients of the band's rows; the first source row the band reads
    const int oy0 = band * BAND_ROWS;
    int r_lo, unused;
    float f0, f1;
    linear_coef(oy0, scale_y, LOC_H, r_lo, unused, f0, f1);
    if (tid < BAND_ROWS) {
        int a, b;
        float w0, w1;
        linear_coef(oy0 + tid, scale_y, LOC_H, a, b, w0, w1);
        rs0[tid] = a - r_lo;
        rs1[tid] = b - r_lo;
        rw0[tid] = w0;
        rw1[tid] = w1;
    }
    __syncthreads();

    // horizontal pass of source rows r_lo .. r_lo + BAND_SRC_ROWS - 1 (clamped): h = w0 * m[sx] + w1 * m[sx1] in fp64
    for (int i = tid; i < BAND_SRC_ROWS * FRAME_W; i += 256) {
        const int r = i / FRAME_W, dx = i - r * FRAME_W;
        const int sr = r_lo + r < LOC_H ? r_lo + r : LOC_H - 1;
        int sx, sx1;
        float w0, w1;
        linear_coef(dx, scale_x, LOC_W, sx, sx1, w0, w1);
        h[r][dx] = (double)w0 * (double)m[sr * LOC_W + sx] + (double)w1 * (double)m[sr * LOC_W + sx1];
    }
    __syncthreads();

    int num = 0, den = 0;
    uint8_t* mo = mask_out ? mask_out + (long)n * FRAME_H * FRAME_W + (long)oy0 * FRAME_W : nullptr;
    for (int p = tid; p < BAND_ROWS * FRAME_W; p += 256) {
        const int yl = p / FRAME_W, dx = p - yl * FRAME_W, dy = oy0 + yl;
        const double v = (double)rw0[yl] * h[rs0[yl]][dx] + (double)rw1[yl] * h[rs1[yl]][dx];
        const int on = v > 0.5 ? 1 : 0;
        int c = 0;
#pragma unroll
        for (int k = 0; k < 3; ++k)
            c += (dx >= bx[k][0] && dx <= bx[k][1] && dy >= bx[k][2] && dy <= bx[k][3]) ? 1 : 0;
        c = c > 2 ? 2 : c;                       // mtot in half-units, capped at 1
        num += on ? c : 0;                       // sum(logical_and(mtot, m2) * mtot)
        den += (on || c) ? (c == 1 ? 1 : 2) : 0; // sum(logical_or(mtot, m2) + mtot - (mtot > 0))
        if (mo) mo[p] = (uint8_t)on;
    }
    num = wave_sum_i(num);
    den = wave_sum_i(den);
    if (lane == 0) {
        smi[wid] = num;
        smi[4 + wid] = den;
    }
    __syncthreads();
    if (tid == 0) {
        int* dst = part + ((long)n * BOX_BANDS + band) * 2;
        dst[0] = smi[0] + smi[1] + smi[2] + smi[3];
        dst[1] = smi[4] + smi[5] + smi[6] + smi[7];
    }
}

// per sample: the 8 band pairs in band order -> counts (half-units) and iou = num / den (0 / 0 -> NaN, like NumPy)
__global__ __launch_bounds__(256) void box_iou_finish_kernel(const int* part, int N, float* iou, int32_t* counts) {
    const int n = blockIdx.x * 256 + threadIdx.x;
    if (n >= N) return;
    int num = 0, den = 0;
    for (int b = 0; b < BOX_BANDS; ++b) {
        num += part[((long)n * BOX_BANDS + b) * 2];
        den += part[((long)n * BOX_BANDS + b) * 2 + 1];
    }
    if (counts) {
        counts[2 * n] = num;
        counts[2 * n + 1] = den;
    }
    iou[n] = den ? (float)((double)num / (double)den) : __builtin_nanf("");
}

}  // namespace acimg

using namespace acimg;

extern "C" {

size_t acimg_box_iou_workspace(int N) { return N > 0 ? (size_t)N * BOX_BANDS * 2 * sizeof(int) : 0; }

int acimg_box_iou(const float* logen, const int32_t* boxes, int N, float* iou, int32_t* counts, uint8_t* mask_out,
                  void* ws, size_t ws_bytes, void* stream) {
    if (N <= 0) return fail(ACIMG_EINVAL, "box_iou: N must be positive");
    if (N > 65535) return fail(ACIMG_EINVAL, "box_iou: N = %d exceeds the grid's y extent", N);
    if (!logen || !boxes || !iou || !ws) return fail(ACIMG_EINVAL, "box_iou: null argument");
    if (ws_bytes < acimg_box_iou_workspace(N))
        return fail(ACIMG_EWORKSPACE, "box_iou: workspace %zu < %zu bytes", ws_bytes, acimg_box_iou_workspace(N));
    const double scale_x = resize_scale_x(), scale_y = resize_scale_y();
    for (int b = 0; b < BOX_BANDS; ++b)   // every band's source rows fit the LDS table
        if (band_rows_needed(b) > BAND_SRC_ROWS)
            return fail(ACIMG_EINVAL, "box_iou: band %d needs %d source rows", b, band_rows_needed(b));
    hipStream_t s = (hipStream_t)stream;
    int* part = (int*)ws;
    hipLaunchKernelGGL(box_iou_partial_kernel, dim3(BOX_BANDS, N), dim3(256), 0, s, logen, boxes, scale_x, scale_y, part,
                       mask_out);
    int rc = check_launch("box_iou");
    if (rc) return rc;
    hipLaunchKernelGGL(box_iou_finish_kernel, dim3(cdiv(N, 256)), dim3(256), 0, s, part, N, iou, counts);
    return check_launch("box_iou (finish)");
}

}  // extern "C"
