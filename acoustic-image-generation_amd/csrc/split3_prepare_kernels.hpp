// Weight preparation for the split 16-bit convolutions on gfx950: fp32 kernels -> hi / lo planes (one kernel or a job table
// per launch), and the same planes once more in LDS-tile order for the pre-split trunk kernels.
#pragma once
#include "igemm_split3_kernel.hpp"

namespace acimg {

// Weight preparation: fp32 HWIO kernel w[tap][c][ldw] -> split + transposed planes out[2][Nrows][Ktot]
// (out[0] = hi, out[1] = lo of w * WSCALE, k contiguous).
//   FWD  : rows n = output channel,  k = tap*C + c            value W[tap][c][n]
//   DGRAD: rows n = input channel c, k = tap'*K + ko          value W[ntaps-1-tap'][n][ko]   (flipped taps)
template <typename TR, bool DGRAD>
__device__ __forceinline__ void split3_prepare_body(const float* w, int ntaps, int C, int K, int ldw, int Nrows,
                                                    typename TR::T* out, int bx, int by, float (*tile)[33]) {
    typedef typename TR::T T;
    const int Ktot = DGRAD ? ntaps * K : ntaps * C;
    const int k0 = bx * 32, n0 = by * 32;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;  // 32 x 8
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        float v = 0.f;
        if constexpr (!DGRAD) {
            const int k = k0 + ty + 8 * i, n = n0 + tx;      // coalesced along n
            if (k < Ktot && n < ldw) v = w[(long)k * ldw + n];
            tile[ty + 8 * i][tx] = v;                        // tile[k][n]
        } else {
            const int n = n0 + ty + 8 * i, k = k0 + tx;      // coalesced along ko
            if (k < Ktot && n < C) {
                const int tp = k / K, ko = k - tp * K;
                v = w[((long)(ntaps - 1 - tp) * C + n) * ldw + ko];
            }
            tile[tx][ty + 8 * i] = v;                        // tile[k][n]
        }
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int n = n0 + ty + 8 * i, k = k0 + tx;
        if (n < Nrows && k < Ktot) {
            const float v = tile[tx][ty + 8 * i] * TR::WSCALE;
            const T h = (T)v;
            out[(long)n * Ktot + k] = h;
            out[((long)Nrows + n) * Ktot + k] = (T)(v - (float)h);
        }
    }
}

template <typename TR, bool DGRAD>
__global__ __launch_bounds__(256) void split3_prepare_kernel(const float* w, int ntaps, int C, int K, int ldw,
                                                             int Nrows, typename TR::T* out) {
    __shared__ float tile[32][33];
    split3_prepare_body<TR, DGRAD>(w, ntaps, C, K, ldw, Nrows, out, blockIdx.x, blockIdx.y, tile);
}

// several kernels in ONE launch (the generator re-splits its trainable kernels every step: forward f16 images and
// flipped / transposed bf16 images for the data gradients): job table by value, workgroup -> job by block ranges
struct PrepJob {
    const float* w;
    void* out;
    int ntaps, C, K, ldw, Nrows, dgrad, tiles_k, block0;   // dgrad: 0 forward f16, 1 data-gradient bf16, 2 forward bf16
};
struct PrepJobs {
    PrepJob j[16];
    int n;
};
__global__ __launch_bounds__(256) void split3_prepare_multi_kernel(const PrepJobs jobs) {
    __shared__ float tile[32][33];
    int ji = 0;
#pragma unroll 1
    for (int i = 1; i < jobs.n; ++i)
        if ((int)blockIdx.x >= jobs.j[i].block0) ji = i;
    const PrepJob& J = jobs.j[ji];
    const int lb = blockIdx.x - J.block0;
    const int bx = lb % J.tiles_k, by = lb / J.tiles_k;
    if (J.dgrad == 1)
        split3_prepare_body<SplitBF16, true>(J.w, J.ntaps, J.C, J.K, J.ldw, J.Nrows, static_cast<__bf16*>(J.out), bx, by, tile);
    else if (J.dgrad == 2)
        split3_prepare_body<SplitBF16, false>(J.w, J.ntaps, J.C, J.K, J.ldw, J.Nrows, static_cast<__bf16*>(J.out), bx, by, tile);
    else
        split3_prepare_body<SplitF16, false>(J.w, J.ntaps, J.C, J.K, J.ldw, J.Nrows, static_cast<_Float16*>(J.out), bx, by, tile);
}

// one thread per 16-byte chunk of the tile-ordered image: brick (nt, q, plane), row, physical chunk
__global__ void split3_brick_kernel(const char* __restrict__ planes, char* __restrict__ bricks, const int Nrows,
                                    const int Ktot, const long total) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int pch = (int)(i & 3), row = (int)((i >> 2) & 127), plane = (int)((i >> 9) & 1);
    const long bq = i >> 10;
    const int kit = Ktot / 32;
    const int nt = (int)(bq / kit), q = (int)(bq - (long)nt * kit);
    const int n = nt * 128 + row;
    uint4 v = make_uint4(0, 0, 0, 0);
    if (n < Nrows)
        v = *reinterpret_cast<const uint4*>(planes + (((long)plane * Nrows + n) * Ktot + q * 32 + ((pch ^ swz(row)) << 3)) * 2);
    *reinterpret_cast<uint4*>(bricks + i * 16) = v;
}

}  // namespace acimg
