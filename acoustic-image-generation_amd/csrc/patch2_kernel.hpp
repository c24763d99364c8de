// The 2x2 / stride-2 transposed conv with 32 input and 8 output channels for gfx950: forward / data gradient and the
// weight gradient, operands loaded from global memory directly in MFMA layout.
#pragma once
#include "igemm_split3_kernel.hpp"

namespace acimg {

// ------------------------------------------------------------------------------------------
// 2x2 / stride-2 transposed conv with 32 input and 8 output channels (models/unet_architecture.py upsample_9 at 112x149 ->
// 224x298; round 4): patches do not overlap, so per INPUT pixel it is one 32 x 32 product - y'[(tap, k)] = W[(tap, k)][c] x[c],
// dx[c] = W^T[c][(tap, k)] gy'[(tap, k)] - and both operands can be loaded from global memory directly in MFMA layout: a
// lane's 8 k-values are 8 consecutive channels of one pixel (forward) or the 8 channels of one of the pixel's four output
// positions (data gradient).  No LDS, no scatter pass: forward stores are 64 contiguous bytes per pixel and output row (1 KiB
// runs per wave), data-gradient stores 128.  Weights (the 32 x 32 matrix, hi / lo) live in registers.  3-term split product:
// f16 hi / lo forward, bf16 hi / lo for the gradient.  The implicit GEMM with a scatter epilogue these replace ran at 90 /
// 65 us for 136 MB each way.
// MODE 0: y[n][2i + r][2j + s][k] = bias[k] + sum_c x[n][i][j][c] w[r][s][k][c]
// MODE 1: dx[n][i][j][c] = sum_{r,s,k} gy[n][2i + r][2j + s][k] w[r][s][k][c]   (optional ReLU mask on dx)
// ------------------------------------------------------------------------------------------
struct Patch2Params {
    const float* X; int ldx;       // MODE 0: x [N][H][W] pixels of ldx floats; MODE 1: gy [N][2H][2W] pixels of ldx floats
    float* Y; int ldy;             // MODE 0: y [N][2H][2W]; MODE 1: dx [N][H][W]
    const float* w; int ldw;       // [2][2][8][ldw >= 32]
    const float* bias; const float* mask; int ldmask; int act;
    int H, W; long pixels;         // the low-resolution grid
};

template <typename TR, int MODE>
__global__ __launch_bounds__(256) void patch2_32x8_kernel(const Patch2Params p) {
    typedef typename TR::V8 V8;
    typedef typename TR::T T;
    const int lane = threadIdx.x & 63, li = lane & 15, g = lane >> 4;
    // the weight matrix in the A slot, rows 16 n + li: MODE 0 rows are (tap, k) and the lane's 8 k-values channels 8 g ..;
    // MODE 1 rows are channels c and the lane's 8 k-values are (tap g, k 0 .. 7)
    V8 wh[2], wl[2];
#pragma unroll
    for (int n = 0; n < 2; ++n) {
        float v[8];
        if (MODE == 0) {
            const float* src = p.w + (long)(16 * n + li) * p.ldw + 8 * g;
            const float4 a = *reinterpret_cast<const float4*>(src), b = *reinterpret_cast<const float4*>(src + 4);
            v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w; v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
        } else {
#pragma unroll
            for (int k = 0; k < 8; ++k) v[k] = p.w[(long)(g * 8 + k) * p.ldw + 16 * n + li];
        }
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const float s_ = v[k] * TR::WSCALE;
            const T h = (T)s_;
            wh[n][k] = h;
            wl[n][k] = (T)(s_ - (float)h);
        }
    }
    f32x4 bv[2];
#pragma unroll
    for (int n = 0; n < 2; ++n)
        bv[n] = (MODE == 0 && p.bias) ? *reinterpret_cast<const f32x4*>(p.bias + 4 * (g & 1)) : f32x4{0.f, 0.f, 0.f, 0.f};
    const long groups = (p.pixels + 15) >> 4;
    const long nwaves = (long)gridDim.x * 4;
    for (long grp = (long)blockIdx.x * 4 + (threadIdx.x >> 6); grp < groups; grp += nwaves) {
        const long pix_raw = grp * 16 + li;
        const bool live = pix_raw < p.pixels;
        const long pix = live ? pix_raw : p.pixels - 1;
        const int j = (int)(pix % p.W);
        const long t = pix / p.W;
        const int i = (int)(t % p.H);
        const long img = t / p.H;
        // this lane's 8 values of the pixel operand
        const float* src = MODE == 0 ? p.X + pix * p.ldx + 8 * g
                                     : p.X + ((img * 2 * p.H + 2 * i + (g >> 1)) * (2L * p.W) + 2 * j + (g & 1)) * p.ldx;
        const float4 a = *reinterpret_cast<const float4*>(src), b = *reinterpret_cast<const float4*>(src + 4);
        uint2 h0, l0, h1, l1;
        split4<TR>(a, h0, l0);
        split4<TR>(b, h1, l1);
        const V8 xh = __builtin_bit_cast(V8, make_uint4(h0.x, h0.y, h1.x, h1.y));
        const V8 xl = __builtin_bit_cast(V8, make_uint4(l0.x, l0.y, l1.x, l1.y));
#pragma unroll
        for (int n = 0; n < 2; ++n) {
            f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
            acc = TR::mfma(wl[n], xh, acc);
            acc = TR::mfma(wh[n], xl, acc);
            acc = TR::mfma(wh[n], xh, acc);
            f32x4 v = acc * TR::OUTSCALE + bv[n];
            if (!live) continue;
            if (MODE == 0) {
                // rows 16 n + 4 g .. + 3 = tap 2 n + (g >> 1), channels 4 (g & 1) .. + 3: output pixel (2 i + n, 2 j + (g >> 1))
#pragma unroll
                for (int c = 0; c < 4; ++c) v[c] = apply_act(v[c], p.act);
                float* dst = p.Y + ((img * 2 * p.H + 2 * i + n) * (2L * p.W) + 2 * j + (g >> 1)) * p.ldy + 4 * (g & 1);
                *reinterpret_cast<f32x4*>(dst) = v;
            } else {
                if (p.mask) {
                    const f32x4 m = *reinterpret_cast<const f32x4*>(p.mask + pix * p.ldmask + 16 * n + 4 * g);
#pragma unroll
                    for (int c = 0; c < 4; ++c) v[c] = m[c] > 0.f ? v[c] : 0.f;
                }
                *reinterpret_cast<f32x4*>(p.Y + pix * p.ldy + 16 * n + 4 * g) = v;
            }
        }
    }
}

// Weight gradient of the same layer: dW[(tap, k)][c] = sum over input pixels of gy[n][2i + r][2j + s][k] x[n][i][j][c], a
// 32 x 32 matrix reduced over all pixels.  The pixels are the MFMA's K axis here, so a lane's 8 k-values are the SAME
// element of 8 consecutive pixels: 4-byte loads (16 lanes cover 64 contiguous bytes of a pixel, the texture addresser
// coalesces them), bf16 hi / lo on the way, 12 MFMAs per 32 pixels, the 32 x 32 tile in 16 accumulators per wave; the
// workgroup's sixteen waves are added through LDS in wave order into one slab per workgroup (slab_reduce_wide_kernel adds
// those in slab order: deterministic).  No LDS staging, no transposing reads.  136 MB in 127 us before (gather GEMM).
struct Patch2WgradParams {
    const float* X; int ldx;       // x [N][H][W][32]
    const float* G; int ldg;       // gy [N][2H][2W][8]
    float* out; int ldo;           // slabs [gridDim.x][32][ldo]
    float* db_part;                // [gridDim.x][8] partial bias gradients (sum of gy per channel) or null
    int H, W; long pixels;
};

__global__ __launch_bounds__(1024) void patch2_wgrad_32x8_kernel(const Patch2WgradParams p) {
    typedef SplitBF16 TR;
    typedef TR::V8 V8;
    typedef TR::T T;
    constexpr int NW = 16;             // waves per workgroup: one workgroup per CU, few slabs for the reduce launch to walk
    __shared__ float red[NW][32][33];
    __shared__ float redb[NW][64];
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6, li = lane & 15, g = lane >> 4;
    float sdb = 0.f;               // this lane's share of the bias gradient: every gy value it loads has channel li & 7
    f32x4 acc[2][2];
#pragma unroll
    for (int mt = 0; mt < 2; ++mt)
#pragma unroll
        for (int nt = 0; nt < 2; ++nt) acc[mt][nt] = f32x4{0.f, 0.f, 0.f, 0.f};
    // row m = 16 mt + li of gy' is (tap, k) = (2 mt + (li >> 3), li & 7): its offset from the pixel's top-left output position
    long offa[2];
#pragma unroll
    for (int mt = 0; mt < 2; ++mt) offa[mt] = ((long)mt * 2 * p.W + (li >> 3)) * p.ldg + (li & 7);
    const long blocks = (p.pixels + 31) >> 5;
    const long nwaves = (long)gridDim.x * NW;
    for (long blk = (long)blockIdx.x * NW + wid; blk < blocks; blk += nwaves) {
        // this lane's eight pixels: blk * 32 + 8 g + t
        const long pix0 = blk * 32 + 8 * g;
        long pc = pix0 < p.pixels ? pix0 : p.pixels - 1;
        int j = (int)(pc % p.W);
        long t_ = pc / p.W;
        int i = (int)(t_ % p.H);
        long img = t_ / p.H;
        float av[2][8], bvv[2][8];
#pragma unroll
        for (int t = 0; t < 8; ++t) {
            const bool live = pix0 + t < p.pixels;
            const float* gb = p.G + ((img * 2 * p.H + 2 * i) * (2L * p.W) + 2 * j) * p.ldg;
            const float* xb = p.X + ((img * p.H + i) * (long)p.W + j) * p.ldx;
#pragma unroll
            for (int mt = 0; mt < 2; ++mt) av[mt][t] = live ? gb[offa[mt]] : 0.f;
#pragma unroll
            for (int nt = 0; nt < 2; ++nt) bvv[nt][t] = live ? xb[16 * nt + li] : 0.f;
            if (live && pix0 + t + 1 < p.pixels) {       // the next pixel, by carry (no division)
                if (++j == p.W) {
                    j = 0;
                    if (++i == p.H) { i = 0; ++img; }
                }
            }
        }
        V8 ah[2], al[2], bh[2], bl[2];
#pragma unroll
        for (int q = 0; q < 2; ++q)
#pragma unroll
            for (int t = 0; t < 8; ++t) {
                sdb += av[q][t];
                const T h = (T)av[q][t];
                ah[q][t] = h;
                al[q][t] = (T)(av[q][t] - (float)h);
                const T hb = (T)bvv[q][t];
                bh[q][t] = hb;
                bl[q][t] = (T)(bvv[q][t] - (float)hb);
            }
#pragma unroll
        for (int mt = 0; mt < 2; ++mt)
#pragma unroll
            for (int nt = 0; nt < 2; ++nt) {
                acc[mt][nt] = TR::mfma(al[mt], bh[nt], acc[mt][nt]);
                acc[mt][nt] = TR::mfma(ah[mt], bl[nt], acc[mt][nt]);
                acc[mt][nt] = TR::mfma(ah[mt], bh[nt], acc[mt][nt]);
            }
    }
    // lane (li, g) of acc[mt][nt] holds rows 16 mt + 4 g .. + 3, column 16 nt + li
#pragma unroll
    for (int mt = 0; mt < 2; ++mt)
#pragma unroll
        for (int nt = 0; nt < 2; ++nt)
#pragma unroll
            for (int r = 0; r < 4; ++r) red[wid][16 * mt + 4 * g + r][16 * nt + li] = acc[mt][nt][r];
    redb[wid][lane] = sdb;
    __syncthreads();
    if (p.db_part && threadIdx.x < 8) {          // channel k: lanes k and k + 8 of every 16-lane row, every wave, in a fixed order
        float t = 0.f;
#pragma unroll
        for (int w = 0; w < NW; ++w)
#pragma unroll
            for (int gg = 0; gg < 4; ++gg) t += redb[w][16 * gg + threadIdx.x] + redb[w][16 * gg + 8 + threadIdx.x];
        p.db_part[(long)blockIdx.x * 8 + threadIdx.x] = t;
    }
    float* slab = p.out + (long)blockIdx.x * 32 * p.ldo;
    {
        const int row = threadIdx.x >> 5, col = threadIdx.x & 31;      // 1024 threads = the 32 x 32 tile, waves added in order
        float t = 0.f;
#pragma unroll
        for (int w = 0; w < NW; ++w) t += red[w][row][col];
        slab[row * p.ldo + col] = t;
    }
}

}  // namespace acimg
