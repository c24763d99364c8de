// The small kernels around the exact-f32 convolutions for gfx950: split-K reduce, sub-pixel weight gather, the tap-GEMM pack /
// unpack / gather / scatter, batch-norm partials after split-K, gap fill, zero insertion.  (Column sums: colsum_kernels.hpp;
// weight bricks: split3_prepare_kernels.hpp.)
#pragma once
#include "igemm_kernel.hpp"

namespace acimg {

// split-K reducer: sums the slabs and runs the epilogue
__global__ __launch_bounds__(256) void igemm_splitk_reduce_kernel(const float* slab, int splits,
                                                                  int M, int Ngemm, int slab_ld,
                                                                  const EpiParams e) {
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    const long total = (long)M * Ngemm;
    if (idx >= total) return;
    const int m = (int)(idx / Ngemm);
    const int n = (int)(idx - (long)m * Ngemm);
    float v = 0.f;
    for (int z = 0; z < splits; ++z) v += slab[((long)z * M + m) * slab_ld + n];
    if (n >= e.Nstore) return;
    int cn, pixoff, r, q, oh, ow;
    epi_col(e, n, cn, pixoff, r, q);
    const long rp = epi_row_pix(e, m, oh, ow);
    if (epi_lands(e, oh, ow, r, q)) epi_store(e, rp + pixoff, cn, v);
}

// ------------------------------------------------------------------------------------------
// SUB-PIXEL form of the stride-2 transposed convolutions with overlapping taps (round 4): the transposed conv
// `conv2d_transpose(k > 2, s = 2)` (models/unet_architecture.py:192-206: upconv_2D with (2,3) kernels) and the data
// gradient of a stride-2 conv (the strided "pool" convs, :168-176).  Both compute
//     Y[s i + a + oy0][s j + b + ox0][ko] = sum_{u, v, kin} A[i - u][j - v][kin] * w[a + 2 u][b + 2 v][ko][kin]
// i.e. an output pixel of parity class (a, b) only sees the kernel taps of its class: ceil(R/2) x ceil(S/2) of them.
// Round 1 ran these as a stride-1 correlation over a ZERO-INSERTED copy of A (4x the pixels, 3 of 4 products against
// zeros, plus the copy's 4x write and read).  Here the four classes are the column groups of ONE implicit GEMM over A's own
// grid - rows (i, j), K = (u', v', kin) with a ceil(R/2) x ceil(S/2) gather, columns (a, b, ko) - whose epilogue scatters
// element (i, j, a, b, ko) to pixel (2 i + a + oy0, 2 j + b + ox0): the k <= s scatter of the non-overlapping transposed
// convs, bounds-checked (EpiParams::scatter = 2).  The combined weight matrix is gathered from the layer's kernel by
// `subpixel_weights_kernel` (the kernels change every step).
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void subpixel_weights_kernel(const float* w, int R, int S, int Ko, int Kin, int ldw, int U,
                                                               int V, float* wc, int total) {
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= total) return;
    const int ncol = 4 * Ko;
    const int row = idx / ncol, col = idx - row * ncol;
    const int kin = row % Kin, tap = row / Kin;
    const int up = tap / V, vp = tap - up * V;
    const int cls = col / Ko, ko = col - cls * Ko;
    const int a = cls >> 1, b = cls & 1;
    const int r = a + 2 * (U - 1 - up), q = b + 2 * (V - 1 - vp);
    wc[idx] = (r < R && q < S) ? w[((long)(r * S + q) * Ko + ko) * ldw + kin] : 0.f;
}

// ------------------------------------------------------------------------------------------
// "tap GEMM" form of a stride-1 VALID convolution with FEW output channels (conv_map: 3x4, 2048 -> 12):
// as an implicit GEMM its N is one MFMA column and every output row gathers R*S*C inputs (no reuse across N:
// L2-bound); instead Z[input pixel][tap*K + k] = X[input pixel][:] . W[tap][:][k] is ONE plain GEMM with
// N = R*S*K columns that reads X once, and y[oh][ow][k] = sum_taps Z[oh+r][ow+s][tap*K + k] is a tiny gather.
// The weight gradient is the same GEMM transposed: dWt = X^T . GZ with GZ the tap-scattered output gradient.
// ------------------------------------------------------------------------------------------
// wt[c][tap*K + k] = w[tap][c][k]
__global__ __launch_bounds__(256) void tapconv_pack_kernel(const float* w, int taps, int C, int K, int ldw,
                                                           float* wt, int ldwt) {
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    const int TK = taps * K;
    if (idx >= (long)C * TK) return;
    const int c = (int)(idx / TK), n = (int)(idx - (long)c * TK);
    const int tap = n / K, k = n - tap * K;
    wt[(long)c * ldwt + n] = w[((long)tap * C + c) * ldw + k];
}

// dw[tap][c][k] = dwt[c][tap*K + k] + decay * w[tap][c][k]
__global__ __launch_bounds__(256) void tapconv_unpack_kernel(const float* dwt, int ldwt, int taps, int C, int K,
                                                             int ldw, const float* w, float decay, float* dw) {
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (long)taps * C * K) return;
    const int k = (int)(idx % K);
    const long tc = idx / K;
    const int c = (int)(tc % C), tap = (int)(tc / C);
    float v = dwt[(long)c * ldwt + tap * K + k];
    if (w) v = fmaf(decay, w[tc * ldw + k], v);
    dw[tc * ldw + k] = v;
}

constexpr int TG_PPB = 32;     // output pixels per workgroup of the gather (= rows per batch-norm partial)
// y[(n,oh,ow)][k] = sum_{r,s} z[(n,oh+r,ow+s)][(r*S+s)*K + k]; TG_PPB output pixels per workgroup, one thread per
// (pixel, k); optional batch-norm partials stats[block][2][stats_ld] (rows past the end count as zeros)
__global__ __launch_bounds__(256) void tapconv_gather_kernel(const float* z, int ldz, int H, int W, int R, int S,
                                                             int K, int OH, int OW, long Mout, float* y, int ldy,
                                                             float* stats, int stats_ld) {
    extern __shared__ __attribute__((aligned(16))) float tg_smem[];     // [128][K] tile of outputs
    const int ppb = TG_PPB;
    const long m0 = (long)blockIdx.x * ppb;
    for (int e = threadIdx.x; e < ppb * K; e += 256) {
        const int pl = e / K, k = e - pl * K;
        const long m = m0 + pl;
        float acc = 0.f;
        if (m < Mout) {
            const int ow = (int)(m % OW);
            const long t = m / OW;
            const int oh = (int)(t % OH);
            const long img = t / OH;
            for (int r = 0; r < R; ++r)
                for (int q = 0; q < S; ++q)
                    acc += z[((img * H + oh + r) * W + ow + q) * ldz + (r * S + q) * K + k];
            y[m * ldy + k] = acc;
        }
        tg_smem[e] = acc;
    }
    if (!stats) return;
    __syncthreads();
    if ((int)threadIdx.x < 2 * K) {
        const int which = threadIdx.x / K, k = threadIdx.x - which * K;
        float sum = 0.f;
        for (int pl = 0; pl < ppb; ++pl) {
            const float v = tg_smem[pl * K + k];
            sum += which ? v * v : v;
        }
        stats[((long)blockIdx.x * 2 + which) * stats_ld + k] = sum;
    }
}

// gz[(n,ih,iw)][(r*S+s)*K + k] = gy[(n,ih-r,iw-s)][k] (0 outside the output)
__global__ __launch_bounds__(256) void tapconv_scatter_kernel(const float* gy, int ldgy, int H, int W, int R, int S,
                                                              int K, int OH, int OW, long Min, float* gz, int ldgz) {
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    const int TK = R * S * K;
    if (idx >= Min * TK) return;
    const long pix = idx / TK;
    const int n = (int)(idx - pix * TK);
    const int tap = n / K, k = n - tap * K;
    const int r = tap / S, q = tap - r * S;
    const int iw = (int)(pix % W);
    const long t = pix / W;
    const int ih = (int)(t % H);
    const long img = t / H;
    const int oh = ih - r, ow = iw - q;
    float v = 0.f;
    if ((unsigned)oh < (unsigned)OH && (unsigned)ow < (unsigned)OW) v = gy[((img * OH + oh) * OW + ow) * ldgy + k];
    gz[pix * ldgz + n] = v;
}

// per-256-row-block column sums / sums of squares of y[M][K] (pixel stride ldy) -> stats[blk][2][ld]:
// the batch-norm partials for convs that ran split-K (their epilogue never sees a full accumulator)
__global__ __launch_bounds__(256) void partial_stats_kernel(const float* y, int ldy, int M, int K,
                                                            float* stats, int ld, int rows_per_block) {
    __shared__ float red[2][8][32];
    const int cl = threadIdx.x & 31, rg = threadIdx.x >> 5;
    const int r0 = blockIdx.x * rows_per_block;
    const int r1 = min(M, r0 + rows_per_block);
    for (int cb = 0; cb < K; cb += 32) {
        const int c = cb + cl;
        float s1 = 0.f, s2 = 0.f;
        if (c < K) {
            // four rows in flight per thread (one at a time this pass streamed 17 MB in 33 us)
            float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f, b0 = 0.f, b1 = 0.f, b2 = 0.f, b3 = 0.f;
            int r = r0 + rg;
            for (; r + 24 < r1; r += 32) {
                const float v0 = y[(long)r * ldy + c], v1 = y[(long)(r + 8) * ldy + c];
                const float v2 = y[(long)(r + 16) * ldy + c], v3 = y[(long)(r + 24) * ldy + c];
                a0 += v0; b0 += v0 * v0;
                a1 += v1; b1 += v1 * v1;
                a2 += v2; b2 += v2 * v2;
                a3 += v3; b3 += v3 * v3;
            }
            for (; r < r1; r += 8) {
                const float v = y[(long)r * ldy + c];
                a0 += v;
                b0 += v * v;
            }
            s1 = (a0 + a1) + (a2 + a3);
            s2 = (b0 + b1) + (b2 + b3);
        }
        red[0][rg][cl] = s1;
        red[1][rg][cl] = s2;
        __syncthreads();
        if (rg == 0 && c < K) {
            float a = 0.f, b = 0.f;
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                a += red[0][i][cl];
                b += red[1][i][cl];
            }
            stats[((long)blockIdx.x * 2 + 0) * ld + c] = a;
            stats[((long)blockIdx.x * 2 + 1) * ld + c] = b;
        }
        __syncthreads();
    }
}

// writes bias to the output positions of a kernel<stride transposed conv that no patch covers
__global__ __launch_bounds__(256) void deconv_gap_fill_kernel(float* y, int ldy, const float* bias,
                                                              long pixels, int OH, int OW, int K,
                                                              int R, int S, int stride, int vec) {
    const int k4 = K / 4;
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= pixels * k4) return;
    const long pix = idx / k4;
    const int c = (int)(idx - pix * k4) * 4;
    const int ox = (int)(pix % OW);
    const int oy = (int)((pix / OW) % OH);
    if ((oy % stride) < R && (ox % stride) < S) return;
    if (vec) {      // y, ldy and bias allow 16-byte accesses (epi_vec_flag, as the GEMM's epilogue before this kernel)
        float4 b = make_float4(0.f, 0.f, 0.f, 0.f);
        if (bias) b = *reinterpret_cast<const float4*>(bias + c);
        *reinterpret_cast<float4*>(y + pix * ldy + c) = b;
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) y[pix * ldy + c + k] = bias ? bias[c + k] : 0.f;
    }
}

// zero insertion: out[n, h*s, w*s, :] = in[n, h, w, :], zeros elsewhere; out is [N][(H-1)s+1][(W-1)s+1][C].
// Turns the data gradient of a stride-s conv (and the forward of a transposed conv whose kernel exceeds
// its stride) into a stride-1 correlation over a 4x larger, mostly-zero tensor: used only for the small
// stride-2 layers of the RGB / spectrogram U-Nets.
__global__ __launch_bounds__(256) void dilate2d_kernel(const float* in, int ldin, float* out, long opixels,
                                                       int H, int W, int OH, int OW, int C, int s) {
    const int c4 = C / 4;
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= opixels * c4) return;
    const long pix = idx / c4;
    const int c = (int)(idx - pix * c4) * 4;
    const int ow = (int)(pix % OW);
    const int oh = (int)((pix / OW) % OH);
    const long n = pix / ((long)OW * OH);
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (oh % s == 0 && ow % s == 0)
        v = *reinterpret_cast<const float4*>(in + ((n * H + oh / s) * W + ow / s) * ldin + c);
    *reinterpret_cast<float4*>(out + pix * C + c) = v;
}


}  // namespace acimg
