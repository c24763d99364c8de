// Localisation overlay on the GPU: the picture showvideo.py:213-233, showimages.py:136-154 and showimages_bb.py:240-285
// draw - the jet-coloured energy map of an acoustic image at alpha 0.7 over the grey video frame - as RGB8 pixels at the
// frame's native 224 x 298.
//
// Per sample: grey g of the frame (fp32, every product and sum rounded on its own), the annotators' 3-pixel box outlines
// painted as g = 1, the energy map resized to the frame in float64 (the cv2.resize restatement of localize.hip, without
// its threshold), each layer autoscaled over the sample (min / max: order-free), turned into a table index with an
// IEEE-correct division (fp32 for grey, fp64 for the map), and the two table colours blended in integer arithmetic.
// This file is compiled with contraction off, so a - b * c never becomes one fused operation.
//
// Launch: 8 workgroups per sample, each 28 output rows x 298 columns, the structure of box_iou_partial_kernel: the 36x48
// map and the horizontal pass of the <= 6 source rows the band needs live in LDS.  The first launch leaves each band's
// (vmin, vmax, gmin, gmax) in the caller's workspace; the second reduces the sample's 8 records (min and max: the same
// value in any order), recomputes g and v with the same code, stages the band's 28 x 894 output bytes in LDS at the
// destination's own 16-byte phase and writes them as aligned 16-byte stores (single bytes only at a row's two ends).
// No atomics.
#include "common.hpp"

#pragma clang fp contract(off)

#include "resize_linear.hpp"

namespace acimg {

constexpr int ROW_OUT = FRAME_W * 3;                       // 894 bytes written per row
constexpr int STAGE_CHUNKS = (ROW_OUT + 15 + 15) / 16;     // 16-byte chunks that cover 894 bytes at any phase: 57
constexpr int STAGE_ROW = STAGE_CHUNKS * 16;               // 912
constexpr int BOX_LO = -16, BOX_HI = 1024;                 // corners are clamped here first: the outline inside the frame
                                                           // does not change and x0 - 1, x1 + 1 cannot overflow

struct BandExtent {   // what one band leaves in the workspace
    double vmin, vmax;
    float gmin, gmax;
};
static_assert(sizeof(BandExtent) == 24, "workspace record");

__device__ __forceinline__ float wave_min_f(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fminf(v, __shfl_xor(v, o, 64));
    return v;
}
__device__ __forceinline__ float wave_max_f(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
    return v;
}
__device__ __forceinline__ double wave_min_d(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmin(v, __shfl_xor(v, o, 64));
    return v;
}
__device__ __forceinline__ double wave_max_d(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o, 64));
    return v;
}

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// table index of a value in its layer's range: trunc(t * 256) of t = (a - amin) / (amax - amin), 256 -> 255, a flat
// layer -> 0; clamped so that no input reads outside the table
template <typename T>
__device__ __forceinline__ int lut_index(T a, T amin, T amax) {
    if (amax == amin) return 0;
    const T t = (a - amin) / (amax - amin);
    const T s = t * (T)256;
    int i = s == (T)256 ? 255 : (int)s;
    if (!(s >= (T)0)) i = 0;          // negative or NaN
    if (s > (T)256) i = 255;
    return clampi(i, 0, 255);
}

// The band's state in LDS: map, horizontal pass, row coefficients, outlines.  One code path serves both launches.
struct BandShared {
    float map[LOC_P];
    double h[BAND_SRC_ROWS][FRAME_W];
    int rs0[BAND_ROWS], rs1[BAND_ROWS];
    float rw0[BAND_ROWS], rw1[BAND_ROWS];
    int bx[3][4];      // x0, x1, y0, y1 of each annotator's outline rule; x0 > x1 = absent
};

__device__ __forceinline__ void band_setup(BandShared& sh, const float* logen, const int32_t* boxes, double scale_x,
                                           double scale_y, int band, int n, int tid) {
    const float* map = logen + (long)n * LOC_P;
    for (int i = tid; i < LOC_P; i += 256) sh.map[i] = map[i];
    if (tid < 3) {
        int x0 = 1, x1 = 0, y0 = 1, y1 = 0;
        if (boxes) {
            const int32_t* b = boxes + (long)n * 12;
            const int xa = b[tid], xb = b[3 + tid], ya = b[6 + tid], yb = b[9 + tid];
            if (xb != 0) {   // xmax == 0 means "no annotator"
                x0 = clampi(xa < xb ? xa : xb, BOX_LO, BOX_HI);
                x1 = clampi(xa < xb ? xb : xa, BOX_LO, BOX_HI);
                y0 = clampi(ya < yb ? ya : yb, BOX_LO, BOX_HI);
                y1 = clampi(ya < yb ? yb : ya, BOX_LO, BOX_HI);
            }
        }
        sh.bx[tid][0] = x0;
        sh.bx[tid][1] = x1;
        sh.bx[tid][2] = y0;
        sh.bx[tid][3] = y1;
    }
    const int oy0 = band * BAND_ROWS;
    int r_lo, unused;
    float f0, f1;
    linear_coef(oy0, scale_y, LOC_H, r_lo, unused, f0, f1);
    if (tid < BAND_ROWS) {
        int a, b;
        float w0, w1;
        linear_coef(oy0 + tid, scale_y, LOC_H, a, b, w0, w1);
        sh.rs0[tid] = a - r_lo;
        sh.rs1[tid] = b - r_lo;
        sh.rw0[tid] = w0;
        sh.rw1[tid] = w1;
    }
    __syncthreads();
    // horizontal pass of source rows r_lo .. r_lo + BAND_SRC_ROWS - 1 (clamped): h = w0 * m[sx] + w1 * m[sx1] in fp64
    for (int i = tid; i < BAND_SRC_ROWS * FRAME_W; i += 256) {
        const int r = i / FRAME_W, dx = i - r * FRAME_W;
        const int sr = r_lo + r < LOC_H ? r_lo + r : LOC_H - 1;
        int sx, sx1;
        float w0, w1;
        linear_coef(dx, scale_x, LOC_W, sx, sx1, w0, w1);
        sh.h[r][dx] = (double)w0 * (double)sh.map[sr * LOC_W + sx] + (double)w1 * (double)sh.map[sr * LOC_W + sx1];
    }
    __syncthreads();
}

// resized energy value of band row yl, column dx
__device__ __forceinline__ double band_value(const BandShared& sh, int yl, int dx) {
    return (double)sh.rw0[yl] * sh.h[sh.rs0[yl]][dx] + (double)sh.rw1[yl] * sh.h[sh.rs1[yl]][dx];
}

// grey of frame pixel (dx, dy) with the outlines painted: cv2.cvtColor(COLOR_BGR2GRAY) on a float image, then 1 on a
// 3-pixel line around every present annotator's box
__device__ __forceinline__ float band_grey(const BandShared& sh, const float* px, int dx, int dy) {
    const float f0 = px[0], f1 = px[1], f2 = px[2];
    float g = (f0 * 0.114f + f1 * 0.587f) + f2 * 0.299f;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const int x0 = sh.bx[k][0], x1 = sh.bx[k][1], y0 = sh.bx[k][2], y1 = sh.bx[k][3];
        const bool present = x0 <= x1;
        const bool outer = dx >= x0 - 1 && dx <= x1 + 1 && dy >= y0 - 1 && dy <= y1 + 1;
        const bool inner = dx >= x0 + 2 && dx <= x1 - 2 && dy >= y0 + 2 && dy <= y1 - 2;
        if (present && outer && !inner) g = 1.0f;
    }
    return g;
}

__global__ __launch_bounds__(256) void overlay_extent_kernel(const float* frames, int ldf, const float* logen,
                                                             const int32_t* boxes, double scale_x, double scale_y,
                                                             BandExtent* part) {
    __shared__ BandShared sh;
    __shared__ float smf[8];
    __shared__ double smd[8];
    const int tid = threadIdx.x, wid = tid >> 6, lane = tid & 63;
    const int band = blockIdx.x, n = blockIdx.y;
    band_setup(sh, logen, boxes, scale_x, scale_y, band, n, tid);
    const int oy0 = band * BAND_ROWS;
    const float* fr = frames + ((long)n * FRAME_H + oy0) * FRAME_W * ldf;
    float gmin = __builtin_inff(), gmax = -__builtin_inff();
    double vmin = __builtin_inf(), vmax = -__builtin_inf();
    for (int p = tid; p < BAND_ROWS * FRAME_W; p += 256) {
        const int yl = p / FRAME_W, dx = p - yl * FRAME_W;
        const float g = band_grey(sh, fr + (long)p * ldf, dx, oy0 + yl);
        const double v = band_value(sh, yl, dx);
        gmin = fminf(gmin, g);
        gmax = fmaxf(gmax, g);
        vmin = fmin(vmin, v);
        vmax = fmax(vmax, v);
    }
    gmin = wave_min_f(gmin);
    gmax = wave_max_f(gmax);
    vmin = wave_min_d(vmin);
    vmax = wave_max_d(vmax);
    if (lane == 0) {
        smf[wid] = gmin;
        smf[4 + wid] = gmax;
        smd[wid] = vmin;
        smd[4 + wid] = vmax;
    }
    __syncthreads();
    if (tid == 0) {
        BandExtent e;
        e.vmin = fmin(fmin(smd[0], smd[1]), fmin(smd[2], smd[3]));
        e.vmax = fmax(fmax(smd[4], smd[5]), fmax(smd[6], smd[7]));
        e.gmin = fminf(fminf(smf[0], smf[1]), fminf(smf[2], smf[3]));
        e.gmax = fmaxf(fmaxf(smf[4], smf[5]), fmaxf(smf[6], smf[7]));
        part[(long)n * BOX_BANDS + band] = e;
    }
}

__global__ __launch_bounds__(256) void overlay_paint_kernel(const float* frames, int ldf, const float* logen,
                                                            const int32_t* boxes, double scale_x, double scale_y,
                                                            const BandExtent* part, const uint8_t* lut_base,
                                                            const uint8_t* lut_over, int alpha_num, int alpha_den,
                                                            uint8_t* out, long row_bytes, long image_bytes) {
    __shared__ BandShared sh;
    __shared__ __attribute__((aligned(16))) uint8_t stage[BAND_ROWS][STAGE_ROW];
    __shared__ uint8_t lut[2][256 * 3];
    __shared__ BandExtent ext;
    const int tid = threadIdx.x;
    const int band = blockIdx.x, n = blockIdx.y;
    for (int i = tid; i < 256 * 3; i += 256) {
        lut[0][i] = lut_base[i];
        lut[1][i] = lut_over[i];
    }
    if (tid == 0) {   // the sample's extents: 8 band records, min / max (any order gives the same value)
        BandExtent e = part[(long)n * BOX_BANDS];
        for (int b = 1; b < BOX_BANDS; ++b) {
            const BandExtent q = part[(long)n * BOX_BANDS + b];
            e.vmin = fmin(e.vmin, q.vmin);
            e.vmax = fmax(e.vmax, q.vmax);
            e.gmin = fminf(e.gmin, q.gmin);
            e.gmax = fmaxf(e.gmax, q.gmax);
        }
        ext = e;
    }
    band_setup(sh, logen, boxes, scale_x, scale_y, band, n, tid);   // its barriers publish lut and ext too
    const int oy0 = band * BAND_ROWS;
    const float* fr = frames + ((long)n * FRAME_H + oy0) * FRAME_W * ldf;
    uint8_t* dst = out + (long)n * image_bytes + (long)oy0 * row_bytes;
    const float gmin = ext.gmin, gmax = ext.gmax;
    const double vmin = ext.vmin, vmax = ext.vmax;
    const int wb = alpha_den - alpha_num, half = alpha_den / 2;
    for (int p = tid; p < BAND_ROWS * FRAME_W; p += 256) {
        const int yl = p / FRAME_W, dx = p - yl * FRAME_W;
        const float g = band_grey(sh, fr + (long)p * ldf, dx, oy0 + yl);
        const double v = band_value(sh, yl, dx);
        const int ig = lut_index<float>(g, gmin, gmax) * 3, iv = lut_index<double>(v, vmin, vmax) * 3;
        const int phase = (int)((uintptr_t)(dst + (long)yl * row_bytes) & 15);
        uint8_t* q = &stage[yl][phase + dx * 3];
#pragma unroll
        for (int c = 0; c < 3; ++c)
            q[c] = (uint8_t)((alpha_num * (int)lut[1][iv + c] + wb * (int)lut[0][ig + c] + half) / alpha_den);
    }
    __syncthreads();
    // row yl occupies stage[yl][phase .. phase + 894): chunk j of the row is the aligned 16 bytes at (row address - phase)
    // + 16 j; whole chunks go out as one 16-byte store, the two ragged ends byte by byte
    for (int i = tid; i < BAND_ROWS * STAGE_CHUNKS; i += 256) {
        const int yl = i / STAGE_CHUNKS, j = i - yl * STAGE_CHUNKS;
        uint8_t* row = dst + (long)yl * row_bytes;
        const int phase = (int)((uintptr_t)row & 15);
        const int lo = j * 16, hi = lo + 16, end = phase + ROW_OUT;
        if (lo >= end) continue;
        if (lo >= phase && hi <= end) {
            *reinterpret_cast<uint4*>(row - phase + lo) = *reinterpret_cast<const uint4*>(&stage[yl][lo]);
        } else {
            const int a = lo > phase ? lo : phase, b = hi < end ? hi : end;
            for (int k = a; k < b; ++k) row[k - phase] = stage[yl][k];
        }
    }
}

}  // namespace acimg

using namespace acimg;

extern "C" {

size_t acimg_overlay_render_workspace(int N) { return N > 0 ? (size_t)N * BOX_BANDS * sizeof(BandExtent) : 0; }

int acimg_overlay_render(const float* frames, int ldf, const float* logen, const int32_t* boxes, const uint8_t* lut_base,
                         const uint8_t* lut_over, int alpha_num, int alpha_den, uint8_t* out, long row_bytes,
                         long image_bytes, int N, void* ws, size_t ws_bytes, void* stream) {
    if (N <= 0) return fail(ACIMG_EINVAL, "overlay_render: N must be positive");
    if (N > 65535) return fail(ACIMG_EINVAL, "overlay_render: N = %d exceeds the grid's y extent", N);
    if (!frames || !logen || !lut_base || !lut_over || !out || !ws) return fail(ACIMG_EINVAL, "overlay_render: null argument");
    if (ldf < 3) return fail(ACIMG_EINVAL, "overlay_render: ldf = %d < 3 floats per pixel", ldf);
    if (row_bytes < ROW_OUT) return fail(ACIMG_EINVAL, "overlay_render: row_bytes = %ld < %d", row_bytes, ROW_OUT);
    if (image_bytes < (FRAME_H - 1) * row_bytes + ROW_OUT)
        return fail(ACIMG_EINVAL, "overlay_render: image_bytes = %ld holds no %d rows of %ld bytes", image_bytes, FRAME_H,
                    row_bytes);
    if (alpha_den < 1 || alpha_den > 255 || alpha_num < 0 || alpha_num > alpha_den)
        return fail(ACIMG_EINVAL, "overlay_render: alpha %d / %d outside 0 <= num <= den, 1 <= den <= 255", alpha_num,
                    alpha_den);
    if (reinterpret_cast<uintptr_t>(ws) & 7u) return fail(ACIMG_EINVAL, "overlay_render: workspace not 8-byte aligned");
    if (ws_bytes < acimg_overlay_render_workspace(N))
        return fail(ACIMG_EWORKSPACE, "overlay_render: workspace %zu < %zu bytes", ws_bytes,
                    acimg_overlay_render_workspace(N));
    const double scale_x = resize_scale_x(), scale_y = resize_scale_y();
    for (int b = 0; b < BOX_BANDS; ++b)   // every band's source rows fit the LDS table
        if (band_rows_needed(b) > BAND_SRC_ROWS)
            return fail(ACIMG_EINVAL, "overlay_render: band %d needs %d source rows", b, band_rows_needed(b));
    hipStream_t s = (hipStream_t)stream;
    BandExtent* part = (BandExtent*)ws;
    hipLaunchKernelGGL(overlay_extent_kernel, dim3(BOX_BANDS, N), dim3(256), 0, s, frames, ldf, logen, boxes, scale_x,
                       scale_y, part);
    int rc = check_launch("overlay_render (extent)");
    if (rc) return rc;
    hipLaunchKernelGGL(overlay_paint_kernel, dim3(BOX_BANDS, N), dim3(256), 0, s, frames, ldf, logen, boxes, scale_x,
                       scale_y, part, lut_base, lut_over, alpha_num, alpha_den, out, row_bytes, image_bytes);
    return check_launch("overlay_render (paint)");
}

}  // extern "C"
