// Exact-f32 weight gradient dW = im2col(x)^T * gy for gfx950 (v_mfma_f32_16x16x4_f32: bit-for-bit an fmaf chain), split
// over pixels into slabs, and the two deterministic slab reducers that every split weight gradient ends with.
#pragma once
#include "igemm.hpp"

namespace acimg {

// ------------------------------------------------------------------------------------------
// weight gradient kernel: dW[kk][n] = sum_m A(m,kk) G[m][n]
// ------------------------------------------------------------------------------------------
// WGM x WGN = 4 waves: 2 x 2, or 4 x 1 for the 16-column tile of the few-column problems (N <= 16: conv_map's 12
// outputs, the 8-channel layers of the RGB / spectrogram U-Nets) where a 32-wide tile would be mostly padding
template <int BMO, int BN, int WGM = 2>
__global__ __launch_bounds__(256) void wgrad_f32_kernel(const WgradParams p) {
    constexpr int BKR = 16;  // pixels per step
    constexpr int LDA_S = BMO + 4;
    constexpr int LDB_S = BN + 4;
    constexpr int WGN = 4 / WGM;
    constexpr int WTM = BMO / WGM, WTN = BN / WGN;
    static_assert(WTM % 16 == 0 && WTN % 16 == 0, "wave tile");
    constexpr int TM = WTM / 16, TN = WTN / 16;
    constexpr int AQ = BMO / 4;               // float4 per A row
    constexpr int ARPP = 256 / AQ;            // A rows per pass
    constexpr int NA = (BKR + ARPP - 1) / ARPP;
    constexpr int BQ = BN / 4;
    constexpr int BRPP = 256 / BQ;
    constexpr int NB = (BKR + BRPP - 1) / BRPP;

    __shared__ __attribute__((aligned(16))) float As[BKR * LDA_S];
    __shared__ __attribute__((aligned(16))) float Bs[BKR * LDB_S];

    const int tid = threadIdx.x;
    const int lane = tid & 63, wid = tid >> 6;
    const int wm = wid / WGN, wn = wid % WGN;
    const int li = lane & 15, g = lane >> 4;
    const int kk0 = blockIdx.x * BMO, n0 = blockIdx.y * BN;

    const int m_begin = blockIdx.z * p.rows_per_split;
    const int m_end = min(p.M, m_begin + p.rows_per_split);

    // this thread's fixed A column (kk -> tap, c)
    const int aq = tid % AQ;
    const int arow0 = tid / AQ;
    const int kk = kk0 + aq * 4;
    const bool kk_ok = kk < p.KK;
    const bool kk_ones = p.db_out != nullptr && kk == p.KK;   // the all-ones column (bias gradient)
    int r = 0, s = 0, c = 0;
    if (kk_ok) {
        const int tap = kk / p.C;
        c = kk - tap * p.C;
        r = tap / p.S;
        s = tap - r * p.S;
    }
    const int bq = tid % BQ;
    const int brow0 = tid / BQ;
    const int nb = n0 + bq * 4;
    const bool nb_ok = nb < p.Nld;
    const int ohw = p.OH * p.OW;

    // pixel coordinates of this thread's A rows, advanced incrementally by BKR pixels per step (two integer
    // divisions per load were the bulk of this kernel's time on the few-channel layers: no hardware divider)
    int x_img[NA], x_oh[NA], x_ow[NA];
#pragma unroll
    for (int j = 0; j < NA; ++j) {
        const int m = m_begin + arow0 + j * ARPP;
        x_img[j] = m / ohw;
        const int rem = m - x_img[j] * ohw;
        x_oh[j] = rem / p.OW;
        x_ow[j] = rem - x_oh[j] * p.OW;
    }

    float4 ra[NA], rb[NB];
    auto load_tiles = [&](int mb) {
#pragma unroll
        for (int j = 0; j < NA; ++j) {
            const int row = arow0 + j * ARPP;
            const int m = mb + row;
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (row < BKR && kk_ones && m < m_end) v.x = 1.f;
            if (row < BKR && kk_ok && m < m_end) {
                const int ih = x_oh[j] * p.stride - p.pad_t + r;
                const int iw = x_ow[j] * p.stride - p.pad_l + s;
                if ((unsigned)ih < (unsigned)p.H && (unsigned)iw < (unsigned)p.W)
                    v = *reinterpret_cast<const float4*>(
                        p.X + ((long)(x_img[j] * p.H + ih) * p.W + iw) * p.ldx + c);
            }
            ra[j] = v;
            x_ow[j] += BKR;                    // this row slot moves BKR pixels ahead for the next call
            while (x_ow[j] >= p.OW) {
                x_ow[j] -= p.OW;
                if (++x_oh[j] == p.OH) {
                    x_oh[j] = 0;
                    ++x_img[j];
                }
            }
        }
#pragma unroll
        for (int j = 0; j < NB; ++j) {
            const int row = brow0 + j * BRPP;
            const int m = mb + row;
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (row < BKR && nb_ok && m < m_end)
                v = *reinterpret_cast<const float4*>(p.G + (long)m * p.ldg + nb);
            rb[j] = v;
        }
    };
    auto store_tiles = [&]() {
#pragma unroll
        for (int j = 0; j < NA; ++j) {
            const int row = arow0 + j * ARPP;
            if (row < BKR) *reinterpret_cast<float4*>(&As[row * LDA_S + aq * 4]) = ra[j];
        }
#pragma unroll
        for (int j = 0; j < NB; ++j) {
            const int row = brow0 + j * BRPP;
            if (row < BKR) *reinterpret_cast<float4*>(&Bs[row * LDB_S + bq * 4]) = rb[j];
        }
    };

    f32x4 acc[TM][TN];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

    if (m_begin < m_end) {
        load_tiles(m_begin);
        store_tiles();
    }
    __syncthreads();
    for (int mb = m_begin; mb < m_end; mb += BKR) {
        const bool more = (mb + BKR) < m_end;
        if (more) load_tiles(mb + BKR);
        float af[TM][4], bf[TN][4];
#pragma unroll
        for (int t = 0; t < 4; ++t) {
#pragma unroll
            for (int i = 0; i < TM; ++i) af[i][t] = As[(4 * g + t) * LDA_S + wm * WTM + i * 16 + li];
#pragma unroll
            for (int j = 0; j < TN; ++j) bf[j][t] = Bs[(4 * g + t) * LDB_S + wn * WTN + j * 16 + li];
        }
#pragma unroll
        for (int t = 0; t < 4; ++t)
#pragma unroll
            for (int i = 0; i < TM; ++i)
#pragma unroll
                for (int j = 0; j < TN; ++j)
                    acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(af[i][t], bf[j][t], acc[i][j], 0, 0, 0);
        __syncthreads();
        if (more) {
            store_tiles();
            __syncthreads();
        }
    }

    float* out = p.out + (long)blockIdx.z * p.KK * p.ldo;
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int rg = 0; rg < 4; ++rg) {
            const int row = kk0 + wm * WTM + i * 16 + g * 4 + rg;
            if (row > p.KK || (row == p.KK && p.db_out == nullptr)) continue;
            float* dst = row < p.KK ? out + (long)row * p.ldo : p.db_out + (long)blockIdx.z * p.ldo;
#pragma unroll
            for (int j = 0; j < TN; ++j) {
                const int n = n0 + wn * WTN + j * 16 + li;
                if (n < p.Ngemm) dst[n] = acc[i][j][rg];
            }
        }
}

// sums `splits` slabs of [rows][ld] (only cols < ncols) into out[rows][ld]; workgroups >= nb1 do the same for a
// second, one-row job (the bias gradient of the same launch: one reduce launch per weight gradient, not two)
__global__ __launch_bounds__(256) void slab_reduce_kernel(const float* slab, int splits, long rows,
                                                          int ncols, int ld, float* out, int nb1,
                                                          const float* slab2, float* out2) {
    long bid = blockIdx.x;
    if (bid >= nb1) {
        bid -= nb1;
        slab = slab2;
        out = out2;
        rows = 1;
    }
    const long idx = bid * 256 + threadIdx.x;
    if (idx >= rows * ncols) return;
    const long row = idx / ncols;
    const int col = (int)(idx - row * ncols);
    float v = 0.f;
    for (int z = 0; z < splits; ++z) v += slab[((long)z * rows + row) * ld + col];
    out[row * ld + col] = v;
}

// the same for many slabs (few-channel weight gradients use up to 2048 pixel splits): OUTS outputs per workgroup, 256 / OUTS
// lane groups walk the slabs with four loads in flight each, fixed-order combine -> deterministic.  OUTS = 32 for large
// gradients; 8 when there are few outputs (a 9 x 8 x 8 kernel is 576 numbers: 18 workgroups of 32 outputs each walked 512
// slabs in 16 dependent rounds - 8 to 20 us of pure latency per launch; 72 workgroups with 32 lane groups need 4 rounds)
template <int OUTS>
__global__ __launch_bounds__(256) void slab_reduce_wide_kernel(const float* slab, int splits, long rows,
                                                               int ncols, int ld, float* out, int nb1,
                                                               const float* slab2, float* out2) {
    constexpr int NG = 256 / OUTS;
    __shared__ float red[NG][OUTS];
    const int ol = threadIdx.x % OUTS, rg = threadIdx.x / OUTS;
    long bid = blockIdx.x;
    if (bid >= nb1) {                  // second job: the one-row bias gradient
        bid -= nb1;
        slab = slab2;
        out = out2;
        rows = 1;
    }
    const long idx = bid * OUTS + ol;
    const bool ok = idx < rows * ncols;
    const long row = ok ? idx / ncols : 0;
    const int col = ok ? (int)(idx - row * ncols) : 0;
    const float* src = slab + row * ld + col;
    const long zs = rows * ld;
    float v0 = 0.f, v1 = 0.f, v2 = 0.f, v3 = 0.f;
    if (ok) {
        int z = rg;
        for (; z + 3 * NG < splits; z += 4 * NG) {
            v0 += src[(long)z * zs];
            v1 += src[(long)(z + NG) * zs];
            v2 += src[(long)(z + 2 * NG) * zs];
            v3 += src[(long)(z + 3 * NG) * zs];
        }
        for (; z < splits; z += NG) v0 += src[(long)z * zs];
    }
    red[rg][ol] = (v0 + v1) + (v2 + v3);
    __syncthreads();
    if (rg == 0 && ok) {
        float t = 0.f;
#pragma unroll
        for (int i = 0; i < NG; ++i) t += red[i][ol];
        out[row * ld + col] = t;
    }
}

}  // namespace acimg
