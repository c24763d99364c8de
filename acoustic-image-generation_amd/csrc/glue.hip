// Layout and pooling glue between the layers of the acoustic-image models for gfx950 (MI355X): HBM-bound single passes, none
// of them batch norm, loss or optimizer.  This file owns
//   pad_channels_kernel, pad_image_kernel, tile_mfcc_kernel      acimg_pad_channels, acimg_pad_image, acimg_tile_mfcc
//   minmax_part / _apply / _bwd_part / _bwd_kernel               acimg_minmax_fwd, acimg_minmax_bwd, acimg_minmax_workspace
//   grad_slice_kernel                                            acimg_grad_slice (strided copy / accumulate, optional ReLU mask)
//   maxpool_fwd_kernel, maxpool_relu_bwd_kernel,                 acimg_maxpool_fwd, acimg_maxpool_relu_bwd, acimg_spatial_sum,
//   spatial_sum_kernel, spatial_sum_relu_bwd_kernel              acimg_spatial_sum_relu_bwd (the DualCamNet classifier's pooling)
// Callers: acimg/ops.py.
#include "common.hpp"

namespace acimg {

__global__ __launch_bounds__(256) void pad_channels_kernel(const float* x, float* y, long pixels,
                                                           int C, int Cp) {
    for (long idx = (long)blockIdx.x * 256 + threadIdx.x; idx < pixels * Cp; idx += (long)gridDim.x * 256) {
        const long p = idx / Cp;
        const int c = (int)(idx - p * Cp);
        y[idx] = c < C ? x[p * C + c] : 0.f;
    }
}

// [N,H,W,C] -> interior of a zeroed [N,Hp,Wp,Cp] image at (pt, pl); the border and the pad channels are never
// written (the caller zeroes the buffer once)
__global__ __launch_bounds__(256) void pad_image_kernel(const float* x, float* y, int H, int W, int C, int Cp,
                                                        int Hp, int Wp, int pt, int pl, long pixels) {
    // one pixel per thread: C contiguous floats in, one (zero-padded) Cp-float pixel out
    for (long p = (long)blockIdx.x * 256 + threadIdx.x; p < pixels; p += (long)gridDim.x * 256) {
        const int w = (int)(p % W);
        const long q = p / W;
        const int h = (int)(q % H);
        const long n = q / H;
        const float* src = x + p * C;
        float* dst = y + ((n * Hp + h + pt) * Wp + w + pl) * Cp;
        if (C == 3 && Cp == 4) {
            *reinterpret_cast<float4*>(dst) = make_float4(src[0], src[1], src[2], 0.f);
        } else {
            for (int c = 0; c < C; ++c) dst[c] = src[c];
        }
    }
}

__global__ __launch_bounds__(256) void tile_mfcc_kernel(const float* mfcc, float* out, int HW, int C,
                                                        long total) {
    for (long idx = (long)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (long)gridDim.x * 256) {
        const int c = (int)(idx % C);
        const long n = idx / ((long)HW * C);
        out[idx] = mfcc[n * C + c];
    }
}

// ------------------------------------------------------------------------------------------
// per-sample min-max normalisation; S pixel chunks per sample (grid S x N), two phases each way:
// partial (min, max) / partial gradient sums per chunk into the workspace, then every chunk combines the S
// partials of its sample in a fixed order and does its share of the elementwise work.  Tie counts are
// integer-valued float atomics (exact, order-independent), so results are bit-reproducible.
// ------------------------------------------------------------------------------------------
static inline int minmax_chunks(int P, int C) {
    long s = ((long)P * C + 2047) / 2048;
    if (s > 32) s = 32;
    if (s > P) s = P;
    if (s < 1) s = 1;
    const int ppc = (P + (int)s - 1) / (int)s;
    return (P + ppc - 1) / ppc;
}

__global__ __launch_bounds__(256) void minmax_part_kernel(const float* x, int ldx, float* part, float* mm,
                                                          int P, int C, int ppc) {
    __shared__ float sm[32];
    const int n = blockIdx.y, sidx = blockIdx.x, S = gridDim.x;
    const int p0 = sidx * ppc, np = min(ppc, P - p0);
    const float* xs = x + ((long)n * P + p0) * ldx;
    const int cnt = np * C;
    float mn = INFINITY, mx = -INFINITY;
    for (int i = threadIdx.x; i < cnt; i += 256) {
        const int p = i / C, c = i - p * C;
        const float v = xs[(long)p * ldx + c];
        mn = fminf(mn, v);
        mx = fmaxf(mx, v);
    }
    mn = wave_min(mn);
    mx = wave_max(mx);
    const int wid = threadIdx.x >> 6, lane = threadIdx.x & 63;
    if (lane == 0) {
        sm[wid] = mn;
        sm[4 + wid] = mx;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        part[((long)n * S + sidx) * 2 + 0] = fminf(fminf(sm[0], sm[1]), fminf(sm[2], sm[3]));
        part[((long)n * S + sidx) * 2 + 1] = fmaxf(fmaxf(sm[4], sm[5]), fmaxf(sm[6], sm[7]));
        if (sidx == 0) {
            mm[n * 4 + 2] = 0.f;
            mm[n * 4 + 3] = 0.f;
        }
    }
}

__global__ __launch_bounds__(256) void minmax_apply_kernel(const float* x, int ldx, float* out, int ldo,
                                                           const float* part, float* mm, int P, int C, int ppc) {
    __shared__ float sm[32];
    const int n = blockIdx.y, sidx = blockIdx.x, S = gridDim.x;
    float mn = INFINITY, mx = -INFINITY;
    for (int k = 0; k < S; ++k) {
        mn = fminf(mn, part[((long)n * S + k) * 2 + 0]);
        mx = fmaxf(mx, part[((long)n * S + k) * 2 + 1]);
    }
    const float D = mx - mn;
    const int p0 = sidx * ppc, np = min(ppc, P - p0);
    const float* xs = x + ((long)n * P + p0) * ldx;
    float* os = out + ((long)n * P + p0) * ldo;
    const int cnt = np * C;
    float cmin = 0.f, cmax = 0.f;
    for (int i = threadIdx.x; i < cnt; i += 256) {
        const int p = i / C, c = i - p * C;
        const float v = xs[(long)p * ldx + c];
        cmin += (v == mn) ? 1.f : 0.f;
        cmax += (v == mx) ? 1.f : 0.f;
        os[(long)p * ldo + c] = (v - mn) / D;
    }
    cmin = block_sum(cmin, sm);
    cmax = block_sum(cmax, sm);
    if (threadIdx.x == 0) {
        if (sidx == 0) {
            mm[n * 4 + 0] = mn;
            mm[n * 4 + 1] = mx;
        }
        if (cmin != 0.f) atomicAdd(&mm[n * 4 + 2], cmin);
        if (cmax != 0.f) atomicAdd(&mm[n * 4 + 3], cmax);
    }
}

__global__ __launch_bounds__(256) void minmax_bwd_part_kernel(const float* x, int ldx, const float* go, int ldgo,
                                                              const float* mm, float* part, int P, int C, int ppc) {
    __shared__ float sm[32];
    const int n = blockIdx.y, sidx = blockIdx.x, S = gridDim.x;
    const int p0 = sidx * ppc, np = min(ppc, P - p0);
    const float* xs = x + ((long)n * P + p0) * ldx;
    const float* gs = go + ((long)n * P + p0) * ldgo;
    const float mn = mm[n * 4 + 0], D = mm[n * 4 + 1] - mn;
    const int cnt = np * C;
    float s1 = 0.f, s2 = 0.f;
    for (int i = threadIdx.x; i < cnt; i += 256) {
        const int p = i / C, c = i - p * C;
        const float g = gs[(long)p * ldgo + c];
        const float o = (xs[(long)p * ldx + c] - mn) / D;
        s1 += g;
        s2 += g * o;
    }
    s1 = block_sum(s1, sm);
    s2 = block_sum(s2, sm);
    if (threadIdx.x == 0) {
        part[((long)n * S + sidx) * 2 + 0] = s1;
        part[((long)n * S + sidx) * 2 + 1] = s2;
    }
}

__global__ __launch_bounds__(256) void minmax_bwd_kernel(const float* x, int ldx, const float* go,
                                                         int ldgo, const float* mm, const float* part, float* gx,
                                                         int ldgx, int P, int C, int ppc, int accumulate,
                                                         int mask_relu) {
    const int n = blockIdx.y, sidx = blockIdx.x, S = gridDim.x;
    const int p0 = sidx * ppc, np = min(ppc, P - p0);
    const float* xs = x + ((long)n * P + p0) * ldx;
    const float* gs = go + ((long)n * P + p0) * ldgo;
    float* gxs = gx + ((long)n * P + p0) * ldgx;
    const float mn = mm[n * 4 + 0], mx = mm[n * 4 + 1], cmin = mm[n * 4 + 2], cmax = mm[n * 4 + 3];
    const float D = mx - mn;
    float s1 = 0.f, s2 = 0.f;
    for (int k = 0; k < S; ++k) {
        s1 += part[((long)n * S + k) * 2 + 0];
        s2 += part[((long)n * S + k) * 2 + 1];
    }
    const float gmin = -(s1 - s2) / D / cmin;
    const float gmax = -s2 / D / cmax;
    const int cnt = np * C;
    for (int i = threadIdx.x; i < cnt; i += 256) {
        const int p = i / C, c = i - p * C;
        const float v = xs[(long)p * ldx + c];
        float g = gs[(long)p * ldgo + c] / D;
        if (v == mn) g += gmin;
        if (v == mx) g += gmax;
        if (accumulate) g += gxs[(long)p * ldgx + c];
        if (mask_relu && !(v > 0.f)) g = 0.f;
        gxs[(long)p * ldgx + c] = g;
    }
}

// dst[p][c] = [accumulate ? dst : 0] + src[p][c], zeroed where mask[p][c] <= 0 (mask optional)
__global__ __launch_bounds__(256) void grad_slice_kernel(const float* src, int ldsrc, float* dst, int lddst,
                                                         const float* mask, int ldmask, long pixels, int C,
                                                         int accumulate) {
    const long total = pixels * C;
    for (long idx = (long)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (long)gridDim.x * 256) {
        const long p = idx / C;
        const int c = (int)(idx - p * C);
        float v = src[p * ldsrc + c];
        if (accumulate) v += dst[p * lddst + c];
        if (mask && !(mask[p * ldmask + c] > 0.f)) v = 0.f;
        dst[p * lddst + c] = v;
    }
}

// ------------------------------------------------------------------------------------------
// DualCamNet classifier pieces (models/dualcamnet.py:82-106, models/base.py:34-38): non-overlapping VALID max
// pooling and the spatial reduce_sum (the clip-level softmax cross-entropy of the same head: loss.hip).
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void maxpool_fwd_kernel(const float* x, int ldx, float* y, int ldy, int H, int W,
                                                          int C, int OH, int OW, int k, long total) {
    for (long idx = (long)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (long)gridDim.x * 256) {
        const int c = (int)(idx % C);
        long t = idx / C;
        const int ow = (int)(t % OW);
        t /= OW;
        const int oh = (int)(t % OH);
        const long n = t / OH;
        float m = -INFINITY;
        for (int r = 0; r < k; ++r)
            for (int q = 0; q < k; ++q)
                m = fmaxf(m, x[((n * H + oh * k + r) * W + ow * k + q) * ldx + c]);
        y[((n * OH + oh) * OW + ow) * ldy + c] = m;
    }
}

// gx = gradient w.r.t. the PRE-activation of the ReLU layer that feeds the pool: the window's gradient goes to
// its first maximum (tf.nn.max_pool's argmax) and only where the activation is positive
__global__ __launch_bounds__(256) void maxpool_relu_bwd_kernel(const float* x, int ldx, const float* gy, int ldgy,
                                                               float* gx, int ldgx, int H, int W, int C, int OH,
                                                               int OW, int k, long total) {
    for (long idx = (long)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (long)gridDim.x * 256) {
        const int c = (int)(idx % C);
        long t = idx / C;
        const int w = (int)(t % W);
        t /= W;
        const int h = (int)(t % H);
        const long n = t / H;
        const int oh = h / k, ow = w / k;
        float g = 0.f;
        const float v = x[((n * H + h) * W + w) * ldx + c];
        if (oh < OH && ow < OW && v > 0.f) {
            bool take = true;
            for (int r = 0; r < k; ++r)
                for (int q = 0; q < k; ++q) {
                    const int hh = oh * k + r, ww = ow * k + q;
                    const float u = x[((n * H + hh) * W + ww) * ldx + c];
                    const bool before = hh < h || (hh == h && ww < w);
                    if (u > v || (u == v && before)) take = false;
                }
            if (take) g = gy[((n * OH + oh) * OW + ow) * ldgy + c];
        }
        gx[((n * H + h) * W + w) * ldgx + c] = g;
    }
}

// y[n][c] = sum_p x[n][p][c]; one workgroup per (sample, 64-channel group)
__global__ __launch_bounds__(256) void spatial_sum_kernel(const float* x, int ldx, float* y, int P, int C) {
    __shared__ float red[4][64];
    const int n = blockIdx.x, c = blockIdx.y * 64 + (threadIdx.x & 63), rg = threadIdx.x >> 6;
    float s = 0.f;
    if (c < C)
        for (int p = rg; p < P; p += 4) s += x[((long)n * P + p) * ldx + c];
    red[rg][threadIdx.x & 63] = s;
    __syncthreads();
    if (rg == 0 && c < C) y[(long)n * C + c] = red[0][threadIdx.x] + red[1][threadIdx.x] + red[2][threadIdx.x] + red[3][threadIdx.x];
}

__global__ __launch_bounds__(256) void spatial_sum_relu_bwd_kernel(const float* x, int ldx, const float* gy, float* gx,
                                                                   int ldgx, int P, int C, long total) {
    for (long idx = (long)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (long)gridDim.x * 256) {
        const int c = (int)(idx % C);
        const long np = idx / C;
        const long n = np / P;
        gx[np * ldgx + c] = x[np * ldx + c] > 0.f ? gy[n * C + c] : 0.f;
    }
}

}  // namespace acimg

using namespace acimg;

extern "C" {

int acimg_pad_channels(const float* x, float* y, long pixels, int C, int Cp, void* stream) {
    hipLaunchKernelGGL(pad_channels_kernel, dim3(ew_grid(pixels * Cp)), dim3(256), 0,
                       (hipStream_t)stream, x, y, pixels, C, Cp);
    return check_launch("pad_channels");
}

int acimg_pad_image(const float* x, float* y, int N, int H, int W, int C, int Cp, int Hp, int Wp, int pad_t,
                    int pad_l, void* stream) {
    if (!x || !y || C > Cp || pad_t < 0 || pad_l < 0 || H + pad_t > Hp || W + pad_l > Wp)
        return fail(ACIMG_EINVAL, "pad_image: the image does not fit the padded frame");
    const long pixels = (long)N * H * W;
    if (C == 3 && Cp == 4 && !aligned16(y)) return fail(ACIMG_EINVAL, "pad_image: the frame must be 16-byte aligned");
    hipLaunchKernelGGL(pad_image_kernel, dim3(ew_grid(pixels)), dim3(256), 0, (hipStream_t)stream, x, y, H, W, C, Cp,
                       Hp, Wp, pad_t, pad_l, pixels);
    return check_launch("pad_image");
}

int acimg_tile_mfcc(const float* mfcc, float* out, int N, int HW, int C, void* stream) {
    const long total = (long)N * HW * C;
    hipLaunchKernelGGL(tile_mfcc_kernel, dim3(ew_grid(total)), dim3(256), 0, (hipStream_t)stream, mfcc,
                       out, HW, C, total);
    return check_launch("tile_mfcc");
}

size_t acimg_minmax_workspace(int N, int P, int C) {
    if (N <= 0 || P <= 0 || C <= 0) return 0;
    return (size_t)N * minmax_chunks(P, C) * 2 * sizeof(float);
}

int acimg_minmax_fwd(const float* x, int ldx, float* out, int ldo, float* mm, int N, int P, int C, void* ws,
                     size_t ws_bytes, void* stream) {
    if (!x || !out || !mm || N <= 0 || P <= 0 || C <= 0) return fail(ACIMG_EINVAL, "minmax_fwd: bad argument");
    if (!ws || ws_bytes < acimg_minmax_workspace(N, P, C))
        return fail(ACIMG_EWORKSPACE, "minmax_fwd: workspace %zu < %zu", ws_bytes, acimg_minmax_workspace(N, P, C));
    const int S = minmax_chunks(P, C), ppc = cdiv(P, S);
    float* part = static_cast<float*>(ws);
    hipLaunchKernelGGL(minmax_part_kernel, dim3(S, N), dim3(256), 0, (hipStream_t)stream, x, ldx, part, mm, P, C, ppc);
    hipLaunchKernelGGL(minmax_apply_kernel, dim3(S, N), dim3(256), 0, (hipStream_t)stream, x, ldx, out, ldo, part,
                       mm, P, C, ppc);
    return check_launch("minmax_fwd");
}

int acimg_minmax_bwd(const float* x, int ldx, const float* go, int ldgo, const float* mm,
                     float* gx, int ldgx, int N, int P, int C, int accumulate, int mask_relu, void* ws,
                     size_t ws_bytes, void* stream) {
    if (!x || !go || !mm || !gx || N <= 0 || P <= 0 || C <= 0) return fail(ACIMG_EINVAL, "minmax_bwd: bad argument");
    if (!ws || ws_bytes < acimg_minmax_workspace(N, P, C))
        return fail(ACIMG_EWORKSPACE, "minmax_bwd: workspace %zu < %zu", ws_bytes, acimg_minmax_workspace(N, P, C));
    const int S = minmax_chunks(P, C), ppc = cdiv(P, S);
    float* part = static_cast<float*>(ws);
    hipLaunchKernelGGL(minmax_bwd_part_kernel, dim3(S, N), dim3(256), 0, (hipStream_t)stream, x, ldx, go, ldgo, mm,
                       part, P, C, ppc);
    hipLaunchKernelGGL(minmax_bwd_kernel, dim3(S, N), dim3(256), 0, (hipStream_t)stream, x, ldx, go, ldgo,
                       mm, part, gx, ldgx, P, C, ppc, accumulate, mask_relu);
    return check_launch("minmax_bwd");
}

int acimg_grad_slice(const float* src, int ldsrc, float* dst, int lddst, const float* mask, int ldmask,
                     long pixels, int C, int accumulate, void* stream) {
    hipLaunchKernelGGL(grad_slice_kernel, dim3(ew_grid(pixels * C)), dim3(256), 0, (hipStream_t)stream, src,
                       ldsrc, dst, lddst, mask, ldmask, pixels, C, accumulate);
    return check_launch("grad_slice");
}

int acimg_maxpool_fwd(const float* x, int ldx, float* y, int ldy, int N, int H, int W, int C, int k, void* stream) {
    if (k <= 0 || H < k || W < k) return fail(ACIMG_EINVAL, "maxpool_fwd: window %d does not fit %dx%d", k, H, W);
    const int OH = H / k, OW = W / k;
    const long total = (long)N * OH * OW * C;
    hipLaunchKernelGGL(maxpool_fwd_kernel, dim3(ew_grid(total)), dim3(256), 0, (hipStream_t)stream, x, ldx, y, ldy, H, W,
                       C, OH, OW, k, total);
    return check_launch("maxpool_fwd");
}

int acimg_maxpool_relu_bwd(const float* x, int ldx, const float* gy, int ldgy, float* gx, int ldgx, int N, int H,
                           int W, int C, int k, void* stream) {
    if (k <= 0 || H < k || W < k) return fail(ACIMG_EINVAL, "maxpool_relu_bwd: window %d does not fit %dx%d", k, H, W);
    const long total = (long)N * H * W * C;
    hipLaunchKernelGGL(maxpool_relu_bwd_kernel, dim3(ew_grid(total)), dim3(256), 0, (hipStream_t)stream, x, ldx, gy, ldgy,
                       gx, ldgx, H, W, C, H / k, W / k, k, total);
    return check_launch("maxpool_relu_bwd");
}

int acimg_spatial_sum(const float* x, int ldx, float* y, int N, int P, int C, void* stream) {
    hipLaunchKernelGGL(spatial_sum_kernel, dim3(N, cdiv(C, 64)), dim3(256), 0, (hipStream_t)stream, x, ldx, y, P, C);
    return check_launch("spatial_sum");
}

int acimg_spatial_sum_relu_bwd(const float* x, int ldx, const float* gy, float* gx, int ldgx, int N, int P, int C,
                               void* stream) {
    const long total = (long)N * P * C;
    hipLaunchKernelGGL(spatial_sum_relu_bwd_kernel, dim3(ew_grid(total)), dim3(256), 0, (hipStream_t)stream, x, ldx, gy,
                       gx, ldgx, P, C, total);
    return check_launch("spatial_sum_relu_bwd");
}

}  // extern "C"
