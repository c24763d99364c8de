// Batch norm of the acoustic-image train step for gfx950 (MI355X): the HBM-bound passes between the convolutions.  Each is a
// single pass with 16-byte accesses where the layout allows, wave-64 shuffle reductions and fp32 (or fp64 where noted)
// accumulation.  This file owns
//   bn_finalize_kernel<8 | 32>                          acimg_bn_finalize     statistics partials -> scale / shift, moving averages
//   bn_relu_kernel, bn_add_relu_kernel,                 acimg_bn_relu, acimg_bn_add_relu, acimg_bn_relu_maxpool
//   bn_relu_maxpool_kernel                                                    the apply passes, fp32 out
//   bn_relu_split_kernel, bn_add_relu_split_kernel,     acimg_bn_relu_split, acimg_bn_add_relu_split, acimg_bn_relu_maxpool_split,
//   bn_relu_maxpool_split_kernel                        acimg_split_plane_bytes    the same passes storing split planes (bricks)
//   bn_relu_bwd_kernel                                  acimg_bn_relu_bwd     one block per channel
//   bn_bwd_reduce / _finalize / _apply_kernel           acimg_bn_bwd, acimg_bn_bwd_workspace    the three-pass U-Net backward
// Callers: acimg/ops.py; conv_trunk.hip and gram.hip size planes with acimg_split_plane_bytes.  The brick layout the
// producers write: split_planes.hpp.
#include "split_planes.hpp"

namespace acimg {

// relu(a*s+t + shortcut), 4 channels: the tail of a residual unit
__device__ __forceinline__ float4 affine_add_relu4(const float4 va, const float4 s, const float4 t, const float4 vb) {
    return make_float4(fmaxf(va.x * s.x + t.x + vb.x, 0.f), fmaxf(va.y * s.y + t.y + vb.y, 0.f),
                       fmaxf(va.z * s.z + t.z + vb.z, 0.f), fmaxf(va.w * s.w + t.w + vb.w, 0.f));
}

// relu(max over the 3x3 / stride-2 window of output pixel (oh, ow) of x*s+sh): channels c .. c+3 of image n of x [.][H][W][C]
__device__ __forceinline__ float4 pooled_affine_max4(const float* x, long n, int oh, int ow, int c, int H, int W, int C,
                                                     int pad_t, int pad_l, const float4 s, const float4 sh) {
    float4 m = make_float4(0.f, 0.f, 0.f, 0.f);  // post-ReLU values are >= 0
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        const int ih = oh * 2 - pad_t + r;
        if ((unsigned)ih >= (unsigned)H) continue;
#pragma unroll
        for (int q = 0; q < 3; ++q) {
            const int iw = ow * 2 - pad_l + q;
            if ((unsigned)iw >= (unsigned)W) continue;
            const float4 v = *reinterpret_cast<const float4*>(x + ((n * H + ih) * W + iw) * C + c);
            m = max4(m, affine4(v, s, sh));
        }
    }
    return m;
}

// ------------------------------------------------------------------------------------------
// batch-norm statistics -> scale/shift (+ moving averages)
// block = 1024 threads = (1024 / CPB) row groups x CPB channels; 4 independent partial sums per thread keep
// several loads in flight (the partials are tiny, the kernel is pure load latency)
// ------------------------------------------------------------------------------------------
// CPB channels per workgroup (32, or 8 when there are thousands of partial rows and few channels: the stem, the
// full-resolution U-Net layers), 1024 / CPB row groups
template <int CPB>
__global__ __launch_bounds__(1024) void bn_finalize_kernel(
    const float* stats, int rows, int C, int ld, double count, const float* gamma, const float* beta,
    float* moving_mean, float* moving_var, float decay, float eps, int training, float* scale,
    float* shift, float* save_mean, float* save_invstd) {
    // Latency-bound kernel (54 launches per step): (1) the per-channel constants are requested FIRST so that their
    // global-load latency overlaps the partial-sum loads; (2) the row groups are combined by a 4-way split of the
    // final loop instead of one thread walking all NRG partials of a channel through dependent LDS reads (that loop
    // alone was ~3 us of the 6 us a launch took).
    constexpr int NRG = 1024 / CPB;
    constexpr int Q = 4;                       // threads per channel in the final combine
    static_assert(NRG % Q == 0, "row groups per combining thread");
    __shared__ double red[2][NRG][CPB];
    __shared__ double red2[2][Q][CPB];
    const int cl = threadIdx.x % CPB, rg = threadIdx.x / CPB;
    const int c = blockIdx.x * CPB + cl;
    float g = 1.f, b = 0.f, mm = 0.f, mv = 1.f;
    if (rg == 0 && c < C) {
        if (gamma) g = gamma[c];
        if (beta) b = beta[c];
        if (moving_mean) {
            mm = moving_mean[c];
            mv = moving_var[c];
        }
    }
    double s1 = 0.0, s2 = 0.0;
    if (training && c < C) {
        float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f, b0 = 0.f, b1 = 0.f, b2 = 0.f, b3 = 0.f;
        int r = rg;
        for (; r + 3 * NRG < rows; r += 4 * NRG) {
            a0 += stats[((long)r * 2 + 0) * ld + c];
            b0 += stats[((long)r * 2 + 1) * ld + c];
            a1 += stats[((long)(r + NRG) * 2 + 0) * ld + c];
            b1 += stats[((long)(r + NRG) * 2 + 1) * ld + c];
            a2 += stats[((long)(r + 2 * NRG) * 2 + 0) * ld + c];
            b2 += stats[((long)(r + 2 * NRG) * 2 + 1) * ld + c];
            a3 += stats[((long)(r + 3 * NRG) * 2 + 0) * ld + c];
            b3 += stats[((long)(r + 3 * NRG) * 2 + 1) * ld + c];
        }
        for (; r < rows; r += NRG) {
            a0 += stats[((long)r * 2 + 0) * ld + c];
            b0 += stats[((long)r * 2 + 1) * ld + c];
        }
        s1 = ((double)a0 + (double)a1) + ((double)a2 + (double)a3);
        s2 = ((double)b0 + (double)b1) + ((double)b2 + (double)b3);
    }
    float mean, var;
    if (training) {
        red[0][rg][cl] = s1;
        red[1][rg][cl] = s2;
        __syncthreads();
        if (rg < Q) {                          // Q threads per channel, NRG / Q partials each, in row-group order
            double t1 = 0.0, t2 = 0.0;
#pragma unroll
            for (int i = 0; i < NRG / Q; ++i) {
                t1 += red[0][rg * (NRG / Q) + i][cl];
                t2 += red[1][rg * (NRG / Q) + i][cl];
            }
            red2[0][rg][cl] = t1;
            red2[1][rg][cl] = t2;
        }
        __syncthreads();
        if (rg != 0 || c >= C) return;
        s1 = (red2[0][0][cl] + red2[0][1][cl]) + (red2[0][2][cl] + red2[0][3][cl]);
        s2 = (red2[1][0][cl] + red2[1][1][cl]) + (red2[1][2][cl] + red2[1][3][cl]);
        const double m = s1 / count;
        double v = s2 / count - m * m;
        if (v < 0.0) v = 0.0;
        mean = (float)m;
        var = (float)v;
        if (moving_mean) {
            const double unbiased = count > 1.0 ? v * (count / (count - 1.0)) : v;
            moving_mean[c] = decay * mm + (1.f - decay) * mean;
            moving_var[c] = decay * mv + (1.f - decay) * (float)unbiased;
        }
    } else {
        if (rg != 0 || c >= C) return;
        mean = mm;
        var = mv;
    }
    const float invstd = 1.f / sqrtf(var + eps);
    const float sc = g * invstd;
    scale[c] = sc;
    shift[c] = b - mean * sc;
    if (save_mean) save_mean[c] = mean;
    if (save_invstd) save_invstd[c] = invstd;
}

__global__ __launch_bounds__(256) void bn_relu_kernel(const float* x, const float* scale,
                                                      const float* shift, float* y, long rows, int C,
                                                      int ldx, int ldy) {
    const long total = rows * C;
    for (long idx = (long)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (long)gridDim.x * 256) {
        const long r = idx / C;
        const int c = (int)(idx - r * C);
        y[r * ldy + c] = fmaxf(x[r * ldx + c] * scale[c] + shift[c], 0.f);
    }
}

// out = relu(a*sa+ta + (b*sb+tb | b))
__global__ __launch_bounds__(256) void bn_add_relu_kernel(const float* a, const float* sa,
                                                          const float* ta, const float* b,
                                                          const float* sb, const float* tb,
                                                          float* out, long total4, int OH, int OW,
                                                          int C4, int BH, int BW, int bstride) {
    for (long idx = (long)blockIdx.x * 256 + threadIdx.x; idx < total4; idx += (long)gridDim.x * 256) {
        const int c4 = (int)(idx % C4);
        const long pix = idx / C4;
        const int c = c4 * 4;
        float4 va = *reinterpret_cast<const float4*>(a + pix * (C4 * 4) + c);
        const float4 s = *reinterpret_cast<const float4*>(sa + c);
        const float4 t = *reinterpret_cast<const float4*>(ta + c);
        long bpix = pix;
        if (bstride != 1) {
            const int ow = (int)(pix % OW);
            const long t2 = pix / OW;
            const int oh = (int)(t2 % OH);
            const long n = t2 / OH;
            bpix = (n * BH + (long)oh * bstride) * BW + (long)ow * bstride;
        }
        float4 vb = *reinterpret_cast<const float4*>(b + bpix * (C4 * 4) + c);
        if (sb) vb = affine4(vb, *reinterpret_cast<const float4*>(sb + c), *reinterpret_cast<const float4*>(tb + c));
        *reinterpret_cast<float4*>(out + pix * (C4 * 4) + c) = affine_add_relu4(va, s, t, vb);
    }
}

__global__ __launch_bounds__(256) void bn_relu_maxpool_kernel(const float* x, const float* scale,
                                                              const float* shift, float* out,
                                                              long total4, int H, int W, int C4,
                                                              int OH, int OW, int pad_t, int pad_l) {
    for (long idx = (long)blockIdx.x * 256 + threadIdx.x; idx < total4; idx += (long)gridDim.x * 256) {
        const int c = (int)(idx % C4) * 4;
        long t = idx / C4;
        const int ow = (int)(t % OW);
        t /= OW;
        const int oh = (int)(t % OH);
        const long n = t / OH;
        const float4 s = *reinterpret_cast<const float4*>(scale + c);
        const float4 sh = *reinterpret_cast<const float4*>(shift + c);
        *reinterpret_cast<float4*>(out + idx * 4) = pooled_affine_max4(x, n, oh, ow, c, H, W, C4 * 4, pad_t, pad_l, s, sh);
    }
}

// ------------------------------------------------------------------------------------------
// the same passes storing the split-plane format of the trunk kernels (split_planes.hpp: the layout, the brick-order work
// items, store_split4)
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void bn_relu_split_kernel(const float* x, const float* scale, const float* shift,
                                                            int relu, char* out, long lo_off, unsigned items, unsigned P,
                                                            int C) {
    const unsigned CQ = (unsigned)C >> 5;
    const bool pow2 = (CQ & (CQ - 1)) == 0;
    const int sh = 31 - __builtin_clz(CQ);
    for (unsigned u = blockIdx.x * 256u + threadIdx.x; u < items; u += gridDim.x * 256u) {
        const BrickItem it = brick_item(u, CQ, pow2, sh);
        if (it.pix >= P) continue;
        float4 v = *reinterpret_cast<const float4*>(x + (long)it.pix * C + it.c);
        if (scale) v = affine4(v, *reinterpret_cast<const float4*>(scale + it.c), *reinterpret_cast<const float4*>(shift + it.c));
        if (relu) v = relu4(v);
        store_split4(v, out, lo_off, it.off);
    }
}

// out = relu(a*sa+ta + shortcut) -> split planes (+ optional fp32 copy); shortcut = b32*sb+tb (projection,
// raw fp32) or the previous unit output read back from ITS split planes (identity, optional subsampling)
__global__ __launch_bounds__(256) void bn_add_relu_split_kernel(
    const float* a, const float* sa, const float* ta, const float* b32, const float* sb, const float* tb,
    const char* bsp, long b_lo_off, char* out, long out_lo_off, float* out32, unsigned items, unsigned P, int OH, int OW,
    int C, int BH, int BW, int bstride) {
    const unsigned CQ = (unsigned)C >> 5;
    const bool pow2 = (CQ & (CQ - 1)) == 0;
    const int sh = 31 - __builtin_clz(CQ);
    for (unsigned u = blockIdx.x * 256u + threadIdx.x; u < items; u += gridDim.x * 256u) {
        const BrickItem it = brick_item(u, CQ, pow2, sh);
        if (it.pix >= P) continue;
        const long idx = (long)it.pix * C + it.c;
        const float4 va = *reinterpret_cast<const float4*>(a + idx);
        const float4 s = *reinterpret_cast<const float4*>(sa + it.c);
        const float4 t = *reinterpret_cast<const float4*>(ta + it.c);
        unsigned bpix = it.pix;
        if (bstride != 1) {
            const unsigned ow = it.pix % (unsigned)OW;
            const unsigned t2 = it.pix / (unsigned)OW;
            const unsigned oh = t2 % (unsigned)OH;
            const unsigned n = t2 / (unsigned)OH;
            bpix = (n * (unsigned)BH + oh * (unsigned)bstride) * (unsigned)BW + ow * (unsigned)bstride;
        }
        float4 vb;
        if (b32) {
            vb = affine4(*reinterpret_cast<const float4*>(b32 + (long)bpix * C + it.c),
                         *reinterpret_cast<const float4*>(sb + it.c), *reinterpret_cast<const float4*>(tb + it.c));
        } else {
            const unsigned e = bstride != 1 ? plane_off(bpix, it.c, CQ) : it.off;
            vb = unsplit4(*reinterpret_cast<const uint2*>(bsp + e), *reinterpret_cast<const uint2*>(bsp + b_lo_off + e),
                          1.f / SPLIT3_ASCALE);
        }
        const float4 o = affine_add_relu4(va, s, t, vb);
        if (out32) *reinterpret_cast<float4*>(out32 + idx) = o;
        if (out) store_split4(o, out, out_lo_off, it.off);
    }
}

__global__ __launch_bounds__(256) void bn_relu_maxpool_split_kernel(const float* x, const float* scale,
                                                                    const float* shift, char* out, long lo_off,
                                                                    unsigned items, unsigned P, int H, int W, int C, int OH,
                                                                    int OW, int pad_t, int pad_l) {
    const unsigned CQ = (unsigned)C >> 5;
    const bool pow2 = (CQ & (CQ - 1)) == 0;
    const int shq = 31 - __builtin_clz(CQ);
    for (unsigned u = blockIdx.x * 256u + threadIdx.x; u < items; u += gridDim.x * 256u) {
        const BrickItem it = brick_item(u, CQ, pow2, shq);
        if (it.pix >= P) continue;
        const int c = (int)it.c;
        const int ow = (int)(it.pix % (unsigned)OW);
        const unsigned t = it.pix / (unsigned)OW;
        const int oh = (int)(t % (unsigned)OH);
        const long n = t / (unsigned)OH;
        const float4 s = *reinterpret_cast<const float4*>(scale + c);
        const float4 sh = *reinterpret_cast<const float4*>(shift + c);
        store_split4(pooled_affine_max4(x, n, oh, ow, c, H, W, C, pad_t, pad_l, s, sh), out, lo_off, it.off);
    }
}

// one block per channel
__global__ __launch_bounds__(1024) void bn_relu_bwd_kernel(const float* x, const float* y,
                                                          const float* gy, const float* gamma,
                                                          const float* mean, const float* invstd,
                                                          float* gx, float* dgamma, float* dbeta,
                                                          long rows, int C) {
    __shared__ float sm[32];
    const int c = blockIdx.x;
    const float mu = mean[c], is = invstd[c];
    float s1 = 0.f, s2 = 0.f;
    for (long r = threadIdx.x; r < rows; r += blockDim.x) {
        const float g = y[r * C + c] > 0.f ? gy[r * C + c] : 0.f;
        s1 += g;
        s2 += g * (x[r * C + c] - mu) * is;
    }
    s1 = block_sum(s1, sm);
    s2 = block_sum(s2, sm);
    if (threadIdx.x == 0) {
        dbeta[c] = s1;
        dgamma[c] = s2;
    }
    const float k = gamma[c] * is;
    const float inv_n = 1.f / (float)rows;
    for (long r = threadIdx.x; r < rows; r += blockDim.x) {
        const float g = y[r * C + c] > 0.f ? gy[r * C + c] : 0.f;
        const float xh = (x[r * C + c] - mu) * is;
        gx[r * C + c] = k * (g - s1 * inv_n - xh * s2 * inv_n);
    }
}

// ------------------------------------------------------------------------------------------
// Training-mode batch-norm backward for the conv-BN-ReLU stacks of the RGB / spectrogram U-Nets
// (models/unet_architecture.py:161-166): many row blocks per launch, float4 over channels.
//   g   = gy * [raw*scale + shift > 0]                    (ReLU mask recomputed, y is not re-read)
//   s1  = sum_rows g = dbeta,   s2 = sum_rows g * xhat = dgamma,   xhat = (raw - mean) * invstd
//   gx  = gamma * invstd * (g - s1/n - xhat * s2/n)
// pass 1 leaves per-block partials [blocks][2][C]; pass 2 (one block) adds them in block order
// (deterministic) and writes dgamma/dbeta; pass 3 is elementwise.
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void bn_bwd_reduce_kernel(const float* x, int ldx, const float* gy, int ldgy,
                                                            const float* scale, const float* shift,
                                                            const float* mean, const float* invstd, long rows,
                                                            int C, long rows_per_block, float* partial) {
    extern __shared__ float sm[];                 // [256][8]
    const int c4n = C >> 2;
    const int tc = threadIdx.x % c4n, tr = threadIdx.x / c4n;
    const int rstep = 256 / c4n;                  // rows covered per sweep (threads beyond rstep*c4n idle)
    const int c = tc * 4;
    float s1[4] = {0.f, 0.f, 0.f, 0.f}, s2[4] = {0.f, 0.f, 0.f, 0.f};
    if (tr < rstep) {
        const float4 sc = *reinterpret_cast<const float4*>(scale + c), sh = *reinterpret_cast<const float4*>(shift + c);
        const float4 mu = *reinterpret_cast<const float4*>(mean + c), is = *reinterpret_cast<const float4*>(invstd + c);
        const float scs[4] = {sc.x, sc.y, sc.z, sc.w}, shs[4] = {sh.x, sh.y, sh.z, sh.w};
        const float mus[4] = {mu.x, mu.y, mu.z, mu.w}, iss[4] = {is.x, is.y, is.z, is.w};
        const long r0 = (long)blockIdx.x * rows_per_block;
        const long r1 = min(rows, r0 + rows_per_block);
        // four rows per trip with sums of their own: eight 16-byte loads in flight per thread (one row per trip streamed the
        // two largest U-Net shapes at 2.5 TB/s - 54 us for 137 MB - while the apply pass, more bytes, took 33 us)
        float t1[4][4], t2[4][4];
#pragma unroll
        for (int u = 0; u < 4; ++u)
#pragma unroll
            for (int k = 0; k < 4; ++k) t1[u][k] = t2[u][k] = 0.f;
        long r = r0 + tr;
        for (; r + 3L * rstep < r1; r += 4L * rstep) {
            float4 xv[4], gv[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                xv[u] = *reinterpret_cast<const float4*>(x + (r + (long)u * rstep) * ldx + c);
                gv[u] = *reinterpret_cast<const float4*>(gy + (r + (long)u * rstep) * ldgy + c);
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const float xs[4] = {xv[u].x, xv[u].y, xv[u].z, xv[u].w}, gs[4] = {gv[u].x, gv[u].y, gv[u].z, gv[u].w};
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const float g = xs[k] * scs[k] + shs[k] > 0.f ? gs[k] : 0.f;
                    t1[u][k] += g;
                    t2[u][k] += g * (xs[k] - mus[k]) * iss[k];
                }
            }
        }
        for (; r < r1; r += rstep) {
            const float4 xv = *reinterpret_cast<const float4*>(x + r * ldx + c);
            const float4 gv = *reinterpret_cast<const float4*>(gy + r * ldgy + c);
            const float xs[4] = {xv.x, xv.y, xv.z, xv.w}, gs[4] = {gv.x, gv.y, gv.z, gv.w};
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const float g = xs[k] * scs[k] + shs[k] > 0.f ? gs[k] : 0.f;
                t1[0][k] += g;
                t2[0][k] += g * (xs[k] - mus[k]) * iss[k];
            }
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            s1[k] = (t1[0][k] + t1[1][k]) + (t1[2][k] + t1[3][k]);
            s2[k] = (t2[0][k] + t2[1][k]) + (t2[2][k] + t2[3][k]);
        }
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        sm[threadIdx.x * 8 + k] = s1[k];
        sm[threadIdx.x * 8 + 4 + k] = s2[k];
    }
    __syncthreads();
    if (threadIdx.x < c4n) {                      // thread tc sums its column group over the row slots, in order
        float a[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        for (int j = 0; j < rstep; ++j)
#pragma unroll
            for (int k = 0; k < 8; ++k) a[k] += sm[(j * c4n + threadIdx.x) * 8 + k];
        float* dst = partial + (long)blockIdx.x * 2 * C;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            dst[c + k] = a[k];
            dst[C + c + k] = a[4 + k];
        }
    }
}

// one workgroup per 32 channels x {dbeta, dgamma}: 8 row groups of 32 lanes walk the blocks, fixed-order tree
__global__ __launch_bounds__(256) void bn_bwd_finalize_kernel(const float* partial, int blocks, int C,
                                                              float* dgamma, float* dbeta, float* sums, int cw) {
    // 256 threads = cw channels x 256 / cw partial-row groups (cw = 8 / 16 / 32 by the channel count: with few channels more
    // groups walk the <= 256 partial rows - 8 dependent loads per thread instead of 32; the kernel is pure latency, 22 launches
    // per U-Net step); two sums in flight per thread; groups combined in order
    __shared__ float red[32][32];
    const int ng = 256 / cw;
    const int cl = threadIdx.x % cw, rg = threadIdx.x / cw;
    const int which = blockIdx.y;                       // 0: sum g (dbeta), 1: sum g*xhat (dgamma)
    const int c = blockIdx.x * cw + cl;
    float a0 = 0.f, a1 = 0.f;
    if (c < C) {
        int j = rg;
        for (; j + ng < blocks; j += 2 * ng) {
            a0 += partial[(long)j * 2 * C + which * C + c];
            a1 += partial[(long)(j + ng) * 2 * C + which * C + c];
        }
        if (j < blocks) a0 += partial[(long)j * 2 * C + which * C + c];
    }
    red[rg][cl] = a0 + a1;
    __syncthreads();
    if (rg == 0 && c < C) {
        float t = 0.f;
        for (int i = 0; i < ng; ++i) t += red[i][cl];
        (which ? dgamma : dbeta)[c] = t;
        sums[which * C + c] = t;
    }
}

__global__ __launch_bounds__(256) void bn_bwd_apply_kernel(const float* x, int ldx, const float* gy, int ldgy,
                                                           const float* scale, const float* shift,
                                                           const float* mean, const float* invstd,
                                                           const float* gamma, const float* sums, long rows, int C,
                                                           float* gx, int ldgx) {
    const int c4n = C >> 2;
    const float inv_n = 1.f / (float)rows;
    for (long idx = (long)blockIdx.x * 256 + threadIdx.x; idx < rows * c4n; idx += (long)gridDim.x * 256) {
        const long r = idx / c4n;
        const int c = (int)(idx - r * c4n) * 4;
        const float4 xv = *reinterpret_cast<const float4*>(x + r * ldx + c);
        const float4 gv = *reinterpret_cast<const float4*>(gy + r * ldgy + c);
        const float xs[4] = {xv.x, xv.y, xv.z, xv.w}, gs[4] = {gv.x, gv.y, gv.z, gv.w};
        float o[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const float g = xs[k] * scale[c + k] + shift[c + k] > 0.f ? gs[k] : 0.f;
            const float xh = (xs[k] - mean[c + k]) * invstd[c + k];
            o[k] = gamma[c + k] * invstd[c + k] * (g - sums[c + k] * inv_n - xh * sums[C + c + k] * inv_n);
        }
        *reinterpret_cast<float4*>(gx + r * ldgx + c) = make_float4(o[0], o[1], o[2], o[3]);
    }
}

// partial-sum workgroups of the reduce pass: one per CU (round 4 measured four per CU: 22 launches 1133 -> 1223 us, the
// finalize walks four times the partials)
static constexpr long BN_BWD_BLOCKS = 256;
// the ONE block count of bn_bwd: the workspace the caller sizes and the partials the passes write and walk
static inline int bn_bwd_blocks(long rows) { return clamped_blocks(rows, BN_BWD_BLOCKS); }   // the finalize pass walks the partials 8 at a time

}  // namespace acimg

using namespace acimg;

extern "C" {

int acimg_bn_finalize(const float* stats, int rows, int C, int ldstats, double count,
                      const float* gamma, const float* beta, float* moving_mean,
                      float* moving_var, float decay, float eps, int training, float* scale,
                      float* shift, float* save_mean, float* save_invstd, void* stream) {
    if (C <= 0 || (training && (!stats || rows <= 0 || count <= 0)) || (!training && (!moving_mean || !moving_var)))
        return fail(ACIMG_EINVAL, "bn_finalize: bad arguments");
    // (8 channels x 128 row groups for every layer was measured in round 2: 7.6 us per launch against 6.2 us)
    if (training && rows > 1024 && C <= 64)
        hipLaunchKernelGGL(bn_finalize_kernel<8>, dim3(cdiv(C, 8)), dim3(1024), 0, (hipStream_t)stream, stats,
                           rows, C, ldstats, count, gamma, beta, moving_mean, moving_var, decay, eps,
                           training, scale, shift, save_mean, save_invstd);
    else
        hipLaunchKernelGGL(bn_finalize_kernel<32>, dim3(cdiv(C, 32)), dim3(1024), 0, (hipStream_t)stream, stats,
                           rows, C, ldstats, count, gamma, beta, moving_mean, moving_var, decay, eps,
                           training, scale, shift, save_mean, save_invstd);
    return check_launch("bn_finalize");
}

int acimg_bn_relu(const float* x, const float* scale, const float* shift, float* y, long rows,
                  int C, int ldx, int ldy, void* stream) {
    hipLaunchKernelGGL(bn_relu_kernel, dim3(ew_grid(rows * C)), dim3(256), 0, (hipStream_t)stream, x,
                       scale, shift, y, rows, C, ldx, ldy);
    return check_launch("bn_relu");
}

int acimg_bn_add_relu(const float* a, const float* sa, const float* ta, const float* b,
                      const float* sb, const float* tb, float* out, int N, int OH, int OW, int C,
                      int BH, int BW, int bstride, void* stream) {
    if (C & 3) return fail(ACIMG_EINVAL, "bn_add_relu: C must be a multiple of 4");
    const long total4 = (long)N * OH * OW * (C / 4);
    hipLaunchKernelGGL(bn_add_relu_kernel, dim3(ew_grid(total4)), dim3(256), 0, (hipStream_t)stream, a,
                       sa, ta, b, sb, tb, out, total4, OH, OW, C / 4, BH, BW, bstride);
    return check_launch("bn_add_relu");
}

int acimg_bn_relu_maxpool(const float* x, const float* scale, const float* shift, float* out,
                          int N, int H, int W, int C, int OH, int OW, int pad_t, int pad_l,
                          void* stream) {
    if (C & 3) return fail(ACIMG_EINVAL, "bn_relu_maxpool: C must be a multiple of 4");
    const long total4 = (long)N * OH * OW * (C / 4);
    hipLaunchKernelGGL(bn_relu_maxpool_kernel, dim3(ew_grid(total4)), dim3(256), 0, (hipStream_t)stream,
                       x, scale, shift, out, total4, H, W, C / 4, OH, OW, pad_t, pad_l);
    return check_launch("bn_relu_maxpool");
}

size_t acimg_split_plane_bytes(long rows, int C) { return split_plane_bytes(rows, C); }

int acimg_bn_relu_split(const float* x, const float* scale, const float* shift, int relu, void* out,
                        size_t lo_off, long rows, int C, void* stream) {
    const unsigned items = split_items(rows, C);
    if (!items || (lo_off & 15) || lo_off < split_plane_bytes(rows, C) || !aligned16(x) || !aligned16(out))
        return fail(ACIMG_EINVAL, "bn_relu_split: C must be a multiple of 32, at most 2^32 elements, buffers aligned, "
                                  "lo_off >= acimg_split_plane_bytes(rows, C)");
    hipLaunchKernelGGL(bn_relu_split_kernel, dim3(ew_grid(items)), dim3(256), 0, (hipStream_t)stream, x, scale,
                       shift, relu, static_cast<char*>(out), (long)lo_off, items, (unsigned)rows, C);
    return check_launch("bn_relu_split");
}

int acimg_bn_add_relu_split(const float* a, const float* sa, const float* ta, const float* b32,
                            const float* sb, const float* tb, const void* b_planes, size_t b_lo_off,
                            void* out_planes, size_t out_lo_off, float* out32, int N, int OH, int OW, int C,
                            int BH, int BW, int bstride, void* stream) {
    const long rows = (long)N * OH * OW;
    const unsigned items = split_items(rows, C);
    if (!items) return fail(ACIMG_EINVAL, "bn_add_relu_split: C must be a multiple of 32, at most 2^32 elements");
    if ((b32 == nullptr) == (b_planes == nullptr))
        return fail(ACIMG_EINVAL, "bn_add_relu_split: exactly one of b32 / b_planes");
    if (b32 && (!sb || !tb)) return fail(ACIMG_EINVAL, "bn_add_relu_split: projection shortcut needs scale/shift");
    if (out_planes && out_lo_off < split_plane_bytes(rows, C))
        return fail(ACIMG_EINVAL, "bn_add_relu_split: out_lo_off < acimg_split_plane_bytes(rows, C)");
    if (b_planes && b_lo_off < split_plane_bytes((long)N * BH * BW, C))
        return fail(ACIMG_EINVAL, "bn_add_relu_split: b_lo_off < acimg_split_plane_bytes of the shortcut tensor");
    // one float4 per thread (no grid-stride loop): measured 4 % faster than 4096 persistent workgroups on this
    // three-stream pass (16 M float4 at the 56x75x512 stage)
    hipLaunchKernelGGL(bn_add_relu_split_kernel, dim3(clamped_blocks(items, 1L << 22)), dim3(256), 0, (hipStream_t)stream, a, sa,
                       ta, b32, sb, tb, static_cast<const char*>(b_planes), (long)b_lo_off,
                       static_cast<char*>(out_planes), (long)out_lo_off, out32, items, (unsigned)rows, OH, OW, C, BH, BW,
                       bstride);
    return check_launch("bn_add_relu_split");
}

int acimg_bn_relu_maxpool_split(const float* x, const float* scale, const float* shift, void* out,
                                size_t lo_off, int N, int H, int W, int C, int OH, int OW, int pad_t, int pad_l,
                                void* stream) {
    const long rows = (long)N * OH * OW;
    const unsigned items = split_items(rows, C);
    if (!items || lo_off < split_plane_bytes(rows, C))
        return fail(ACIMG_EINVAL, "bn_relu_maxpool_split: C must be a multiple of 32, lo_off >= acimg_split_plane_bytes");
    hipLaunchKernelGGL(bn_relu_maxpool_split_kernel, dim3(ew_grid(items)), dim3(256), 0, (hipStream_t)stream, x,
                       scale, shift, static_cast<char*>(out), (long)lo_off, items, (unsigned)rows, H, W, C, OH, OW, pad_t,
                       pad_l);
    return check_launch("bn_relu_maxpool_split");
}

int acimg_bn_relu_bwd(const float* x, const float* y, const float* gy, const float* gamma,
                      const float* save_mean, const float* save_invstd, float* gx, float* dgamma,
                      float* dbeta, long rows, int C, void* stream) {
    hipLaunchKernelGGL(bn_relu_bwd_kernel, dim3(C), dim3(1024), 0, (hipStream_t)stream, x, y, gy, gamma,
                       save_mean, save_invstd, gx, dgamma, dbeta, rows, C);
    return check_launch("bn_relu_bwd");
}

size_t acimg_bn_bwd_workspace(long rows, int C) { return (size_t)(bn_bwd_blocks(rows) + 1) * 2 * C * sizeof(float); }

int acimg_bn_bwd(const float* x, int ldx, const float* gy, int ldgy, const float* scale, const float* shift,
                 const float* save_mean, const float* save_invstd, const float* gamma, long rows, int C,
                 float* gx, int ldgx, float* dgamma, float* dbeta, void* ws, size_t ws_bytes, void* stream) {
    if ((C & 3) || C > 1024 || (ldx & 3) || (ldgy & 3) || (ldgx & 3) || !aligned16(x) || !aligned16(gy) ||
        !aligned16(gx))
        return fail(ACIMG_EINVAL, "bn_bwd: C=%d must be a multiple of 4 (<= 1024), buffers 16-byte aligned", C);
    if (ws_bytes < acimg_bn_bwd_workspace(rows, C) || !ws) return fail(ACIMG_EWORKSPACE, "bn_bwd: workspace too small");
    const long blocks = bn_bwd_blocks(rows);
    const long rpb = (rows + blocks - 1) / blocks;
    float* partial = static_cast<float*>(ws);
    float* sums = partial + blocks * 2 * C;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(bn_bwd_reduce_kernel, dim3((int)blocks), dim3(256), 256 * 8 * sizeof(float), st, x, ldx, gy, ldgy,
                       scale, shift, save_mean, save_invstd, rows, C, rpb, partial);
    const int cw = C <= 8 ? 8 : (C <= 16 ? 16 : 32);
    hipLaunchKernelGGL(bn_bwd_finalize_kernel, dim3(cdiv(C, cw), 2), dim3(256), 0, st, partial, (int)blocks, C, dgamma, dbeta, sums, cw);
    hipLaunchKernelGGL(bn_bwd_apply_kernel, dim3(ew_grid(rows * (C / 4))), dim3(256), 0, st, x, ldx, gy, ldgy, scale, shift,
                       save_mean, save_invstd, gamma, sums, rows, C, gx, ldgx);
    return check_launch("bn_bwd");
}

}  // extern "C"
