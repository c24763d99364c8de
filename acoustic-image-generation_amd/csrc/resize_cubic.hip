// cv2.resize(frame, (new_w, new_h), INTER_CUBIC) of 8-bit 3-channel frames with the central crop of convert_data.py:
// 120-138 fused in: the resize behind `python -m acimg.convert` (_read_video_frame, convert_data.py:141-158).  The
// definition is OpenCV's scalar fixed-point path (resize_cubic.hpp); tests/convert_ref.py restates it
// bit for bit.
//
// acimg_resize_cubic_tables (host): the tap indices and int16 weights of a run of output coordinates.  The caller asks
//   for the rows and columns of the crop window only, so cropping is a choice of tables and costs nothing.
// acimg_resize_cubic_u8: one workgroup of 1024 threads per (band of RC_BAND output rows, column tile, frame).
//   1. the band's row taps and the tile's column taps go to LDS, each index clamped to the frame (the tables live on
//      the device, so the host cannot vouch for them: a foreign table gives foreign pixels, never a foreign address);
//   2. horizontal pass: one thread per (source row the band needs, output column) reads its 4 x 3 source bytes - byte
//      loads, because a BMP's pixel offset of 54 and its row padding leave nothing aligned - and writes three int32 sums
//      to the LDS tile [row][column][channel] (lanes 3 dwords apart: conflict-free);
//   3. vertical pass: one thread per output byte reads its four int32 out of LDS (consecutive lanes, consecutive dwords),
//      applies (v + 2^21) >> 22 and the clamp, and stores the byte.
//   A band whose source rows do not fit the tile (a steeper reduction than the 480 -> 224 it is sized for) is worked off
//   in several chunks of whole output rows, the rows shared by two chunks being formed twice.
// Integer arithmetic, no atomics, no workspace; every output byte is written by exactly one thread: bit-identical from
// run to run.
#include "common.hpp"

#pragma clang fp contract(off)

#include "resize_cubic.hpp"

namespace acimg {

// two workgroups per CU (the LDS decides) are 8 waves per SIMD at 48 VGPRs; 256 threads measured 1.12 - 1.21 x slower
constexpr int RC_THREADS = 1024;
constexpr int RC_BAND = 8;            // output rows per workgroup: 28 bands of a 224-row frame, 336 workgroups at 12 frames
constexpr int RC_COLS = 320;          // widest column tile (298 output columns are one tile)
// LDS per workgroup: 18432 int32 of tile + the tables below = 81664 bytes, two workgroups per CU.  At 298 columns the
// tile holds 20 source rows; a band of 8 rows at 480 -> 224 needs 19.
constexpr int RC_TILE_INTS = 18432;
constexpr int RC_MAX_DIM = 65535;     // of every size: byte offsets inside a row and the grid stay far inside int32

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : v > hi ? hi : v; }

__global__ __launch_bounds__(RC_THREADS, 8) void resize_cubic_u8_kernel(
    const uint8_t* __restrict__ src, size_t frame_stride, size_t pixel_offset, long row_stride, int H, int W,
    const int32_t* __restrict__ idx_y, const int16_t* __restrict__ coef_y, const int32_t* __restrict__ idx_x,
    const int16_t* __restrict__ coef_x, int OH, int OW, int CW, int S, uint8_t* __restrict__ out) {
    __shared__ int tile[RC_TILE_INTS];
    __shared__ __attribute__((aligned(16))) int s_tx[RC_COLS * CUBIC_TAPS];      // byte offset of each column tap in a row
    __shared__ short s_wx[RC_COLS * CUBIC_TAPS];
    __shared__ int s_ty[RC_BAND * CUBIC_TAPS];
    __shared__ int s_wy[RC_BAND * CUBIC_TAPS];

    const int tid = threadIdx.x;
    const int r0 = blockIdx.x * RC_BAND, r1 = min(r0 + RC_BAND, OH);
    const int x0 = blockIdx.y * CW, cw = min(CW, OW - x0);
    const uint8_t* frame = src + (size_t)blockIdx.z * frame_stride + pixel_offset;
    uint8_t* dst = out + (size_t)blockIdx.z * OH * OW * 3;

    for (int i = tid; i < (r1 - r0) * CUBIC_TAPS; i += RC_THREADS) {
        s_ty[i] = clampi(idx_y[r0 * CUBIC_TAPS + i], 0, H - 1);
        s_wy[i] = coef_y[r0 * CUBIC_TAPS + i];
    }
    for (int i = tid; i < cw * CUBIC_TAPS; i += RC_THREADS) {
        s_tx[i] = clampi(idx_x[x0 * CUBIC_TAPS + i], 0, W - 1) * 3;
        s_wx[i] = coef_x[x0 * CUBIC_TAPS + i];
    }
    __syncthreads();

    const int row_ints = cw * 3;
    int r = r0;
    while (r < r1) {      // uniform: every thread walks the same chunks
        // the chunk: output rows r .. re - 1, whose taps all lie in the S source rows from `base`
        const int* t = s_ty + (r - r0) * CUBIC_TAPS;
        const int base = min(min(t[0], t[1]), min(t[2], t[3]));
        int re = r, top = base;
        while (re < r1) {
            const int* u = s_ty + (re - r0) * CUBIC_TAPS;
            const int lo = min(min(u[0], u[1]), min(u[2], u[3])), hi = max(max(u[0], u[1]), max(u[2], u[3]));
            if (lo < base || hi >= base + S) break;
            top = max(top, hi);
            ++re;
        }
        if (re == r) {    // one row's taps wider than the tile: no cubic table is; the taps clamp into the tile below
            re = r + 1;
            top = min(base + S - 1, H - 1);
        }
        const int nrows = top - base + 1;

        for (int i = tid; i < nrows * cw; i += RC_THREADS) {
            const int row = i / cw, x = i - row * cw;
            const uint8_t* p = frame + (long)(base + row) * row_stride;
            const int4 o = *reinterpret_cast<const int4*>(s_tx + x * CUBIC_TAPS);
            const short* w = s_wx + x * CUBIC_TAPS;
            const int w0 = w[0], w1 = w[1], w2 = w[2], w3 = w[3];
            int* d = tile + row * row_ints + x * 3;
#pragma unroll
            for (int c = 0; c < 3; ++c)
                d[c] = (int)p[o.x + c] * w0 + (int)p[o.y + c] * w1 + (int)p[o.z + c] * w2 + (int)p[o.w + c] * w3;
        }
        __syncthreads();

        for (int j = tid; j < (re - r) * row_ints; j += RC_THREADS) {
            const int rr = j / row_ints, e = j - rr * row_ints;
            const int* u = s_ty + (r - r0 + rr) * CUBIC_TAPS;
            const int* w = s_wy + (r - r0 + rr) * CUBIC_TAPS;
            int v = 0;
#pragma unroll
            for (int k = 0; k < CUBIC_TAPS; ++k) v += tile[clampi(u[k] - base, 0, nrows - 1) * row_ints + e] * w[k];
            dst[((size_t)(r + rr) * OW + x0) * 3 + e] = cubic_cast(v);
        }
        __syncthreads();
        r = re;
    }
}

}  // namespace acimg

using namespace acimg;

extern "C" {

int acimg_resize_cubic_tables(int n_in, int n_out, int first, int count, int32_t* idx, int16_t* coef) {
    if (!idx || !coef) return fail(ACIMG_EINVAL, "resize_cubic_tables: null argument");
    if (n_in < 1 || n_in > RC_MAX_DIM || n_out < 1 || n_out > RC_MAX_DIM)
        return fail(ACIMG_EINVAL, "resize_cubic_tables: sizes %d -> %d outside 1..%d", n_in, n_out, RC_MAX_DIM);
    if (first < 0 || count < 1 || count > n_out - first)
        return fail(ACIMG_EINVAL, "resize_cubic_tables: window [%d, %d + %d) outside the %d output coordinates", first, first,
                    count, n_out);
    const double scale = cubic_scale(n_in, n_out);
    for (int i = 0; i < count; ++i) {
        int s;
        cubic_coef(first + i, scale, s, coef + (size_t)i * CUBIC_TAPS);
        for (int k = 0; k < CUBIC_TAPS; ++k) idx[(size_t)i * CUBIC_TAPS + k] = cubic_tap(s, k, n_in);
    }
    return ACIMG_OK;
}

int acimg_resize_cubic_u8(const uint8_t* src, size_t frame_stride, size_t pixel_offset, long row_stride, int n, int H, int W,
                          const int32_t* idx_y, const int16_t* coef_y, const int32_t* idx_x, const int16_t* coef_x, int OH,
                          int OW, uint8_t* out, void* stream) {
    if (!src || !idx_y || !coef_y || !idx_x || !coef_x || !out) return fail(ACIMG_EINVAL, "resize_cubic_u8: null argument");
    if (n < 1 || H < 1 || W < 1 || OH < 1 || OW < 1 || H > RC_MAX_DIM || W > RC_MAX_DIM || OH > RC_MAX_DIM || OW > RC_MAX_DIM)
        return fail(ACIMG_EINVAL, "resize_cubic_u8: n = %d, %d x %d -> %d x %d: every size is 1..%d", n, H, W, OH, OW,
                    RC_MAX_DIM);
    const long row_bytes = 3L * W, pitch = row_stride < 0 ? -row_stride : row_stride;
    if (pitch < row_bytes)
        return fail(ACIMG_EINVAL, "resize_cubic_u8: row_stride = %ld holds fewer than the %ld bytes of a row", row_stride,
                    row_bytes);
    // the frame's first and last byte relative to its start: the top row is at pixel_offset, the others row_stride apart
    const size_t span = (size_t)(H - 1) * (size_t)pitch;
    const bool fits = row_stride < 0 ? pixel_offset >= span && pixel_offset <= frame_stride &&
                                           (size_t)row_bytes <= frame_stride - pixel_offset
                                     : pixel_offset <= frame_stride && span + (size_t)row_bytes <= frame_stride - pixel_offset;
    if (!fits)
        return fail(ACIMG_EINVAL, "resize_cubic_u8: a %d x %d frame at offset %zu with row_stride %ld overruns frame_stride = %zu",
                    H, W, pixel_offset, row_stride, frame_stride);
    const int tiles = cdiv(OW, RC_COLS), CW = cdiv(OW, tiles), S = RC_TILE_INTS / (CW * 3), bands = cdiv(OH, RC_BAND);
    static_assert(RC_TILE_INTS / (RC_COLS * 3) >= CUBIC_TAPS + RC_BAND, "a tile holds a band's rows at any enlargement");
    static_assert(RC_MAX_DIM / RC_COLS < 65535, "the column tiles fit the grid's y");
    for (int done = 0; done < n; done += 65535) {      // frames are the grid's z: 65535 per launch
        const int m = n - done < 65535 ? n - done : 65535;
        hipLaunchKernelGGL(resize_cubic_u8_kernel, dim3(bands, tiles, m), dim3(RC_THREADS), 0, (hipStream_t)stream,
                           src + (size_t)done * frame_stride, frame_stride, pixel_offset, row_stride, H, W, idx_y, coef_y, idx_x,
                           coef_x, OH, OW, CW, S, out + (size_t)done * OH * OW * 3);
        const int rc = check_launch("resize_cubic_u8");
        if (rc != ACIMG_OK) return rc;
    }
    return ACIMG_OK;
}

}  // extern "C"
