// Column sums for gfx950 (the bias gradients of the weight-gradient entry points): partial sums per row block, then a
// fixed-order combine.
#pragma once
#include "common.hpp"

namespace acimg {

// column sums of G[rows][ld] (cols < ncols) -> out[ncols]; one block per 64 columns, 256 threads
// = 4 row-groups x 64 columns.
__global__ __launch_bounds__(256) void colsum_partial_kernel(const float* G, long rows, int ncols,
                                                             int ld, long rows_per_block,
                                                             float* partial /*[gridDim.y][ncols]*/) {
    __shared__ float red[4][64];
    const int col = blockIdx.x * 64 + (threadIdx.x & 63);
    const int rg = threadIdx.x >> 6;
    const long rb = (long)blockIdx.y * rows_per_block;
    const long re = min(rows, rb + rows_per_block);
    float s = 0.f;
    if (col < ncols)
        for (long r = rb + rg; r < re; r += 4) s += G[r * ld + col];
    red[rg][threadIdx.x & 63] = s;
    __syncthreads();
    if (rg == 0 && col < ncols)
        partial[(long)blockIdx.y * ncols + col] = red[0][threadIdx.x] + red[1][threadIdx.x] +
                                                  red[2][threadIdx.x] + red[3][threadIdx.x];
}
// narrow variant (ncols <= 64, multiple of 4, ld % 4 == 0): a workgroup sweeps rows_per_block rows with float4
// loads, (ncols/4) lanes per row; partial sums are combined in lane order -> deterministic
__global__ __launch_bounds__(256) void colsum_narrow_kernel(const float* G, long rows, int ncols, int ld,
                                                            long rows_per_block, float* partial) {
    __shared__ float sm[256 * 4];
    const int c4n = ncols >> 2;
    const int tc = threadIdx.x % c4n, tr = threadIdx.x / c4n;
    const int rstep = 256 / c4n;
    float a[4] = {0.f, 0.f, 0.f, 0.f};
    if (tr < rstep) {
        const long r0 = (long)blockIdx.x * rows_per_block;
        const long r1 = min(rows, r0 + rows_per_block);
        // four rows in flight per thread, sums of their own, combined in a fixed order
        float b[3][4] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
        long r = r0 + tr;
        for (; r + 3L * rstep < r1; r += 4L * rstep) {
            const float4 v0 = *reinterpret_cast<const float4*>(G + r * ld + tc * 4);
            const float4 v1 = *reinterpret_cast<const float4*>(G + (r + rstep) * ld + tc * 4);
            const float4 v2 = *reinterpret_cast<const float4*>(G + (r + 2L * rstep) * ld + tc * 4);
            const float4 v3 = *reinterpret_cast<const float4*>(G + (r + 3L * rstep) * ld + tc * 4);
            a[0] += v0.x; a[1] += v0.y; a[2] += v0.z; a[3] += v0.w;
            b[0][0] += v1.x; b[0][1] += v1.y; b[0][2] += v1.z; b[0][3] += v1.w;
            b[1][0] += v2.x; b[1][1] += v2.y; b[1][2] += v2.z; b[1][3] += v2.w;
            b[2][0] += v3.x; b[2][1] += v3.y; b[2][2] += v3.z; b[2][3] += v3.w;
        }
        for (; r < r1; r += rstep) {
            const float4 v = *reinterpret_cast<const float4*>(G + r * ld + tc * 4);
            a[0] += v.x; a[1] += v.y; a[2] += v.z; a[3] += v.w;
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) a[k] = (a[k] + b[0][k]) + (b[1][k] + b[2][k]);
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) sm[threadIdx.x * 4 + k] = a[k];
    __syncthreads();
    if (threadIdx.x < c4n) {
        float t[4] = {0.f, 0.f, 0.f, 0.f};
        for (int j = 0; j < rstep; ++j)
#pragma unroll
            for (int k = 0; k < 4; ++k) t[k] += sm[(j * c4n + threadIdx.x) * 4 + k];
#pragma unroll
        for (int k = 0; k < 4; ++k) partial[(long)blockIdx.x * ncols + threadIdx.x * 4 + k] = t[k];
    }
}
// 256 threads = 4 part groups x 64 columns - or, for up to 16 columns (where the 4-group form is 64 dependent loads per
// thread, ~13 us of latency for a kilobyte of result), 16 part groups x 16 columns; fixed-order combine
__global__ __launch_bounds__(256) void colsum_final_kernel(const float* partial, int parts, int ncols, float* out) {
    __shared__ float red[16][64];
    const bool narrow = ncols <= 16;
    const int cw = narrow ? 16 : 64, ng = 256 / cw;
    const int cl = threadIdx.x % cw, pg = threadIdx.x / cw;
    const int col = blockIdx.x * cw + cl;
    float s0 = 0.f, s1 = 0.f;
    if (col < ncols) {
        int i = pg;
        for (; i + ng < parts; i += 2 * ng) {
            s0 += partial[(long)i * ncols + col];
            s1 += partial[(long)(i + ng) * ncols + col];
        }
        if (i < parts) s0 += partial[(long)i * ncols + col];
    }
    red[pg][cl] = s0 + s1;
    __syncthreads();
    if (pg == 0 && col < ncols) {
        float t = 0.f;
        for (int g = 0; g < ng; ++g) t += red[g][cl];
        out[col] = t;
    }
}

}  // namespace acimg
