// Tap-sharing bf16x3 weight gradient of the 3x3 / stride-1 / SAME layers with WIDE channels (the generator's 36x48 layers:
// 256->128, 128->128, 128->64, 64->64) for gfx950:  dW[tap][c][n] = sum_pixels x(pixel + tap)[c] * gy[pixel][n].
//
// As a per-tap implicit GEMM (wgrad_split3_kernel) every 128-row block of dW is one tap and one channel block, and each of
// them loads and splits its own fp32 x and gy tiles: for 256->128, gy is read and split 18 times and x 9 times, 995 MB of
// operands through L2 per launch for 85 MB of tensors.  Here a workgroup owns ALL NINE TAPS of CB = 32 input channels x NB
// output columns of one pixel split and walks tiles of TH = 2 output rows x the image width W:
//   - the gy tile (2 W pixels x NB) is loaded and split once into hi / lo planes laid out exactly as wgrad_split3_kernel's
//     ([pixel][256 B], 32-byte chunk index XOR (pixel & 3 | (pixel >> 3 & 1) << 2)), so `tr_frag` reads it unchanged;
//   - the x patch (4 rows x (W + 2) pixels x 32 channels, zeros outside the image and past the layer's channels) is loaded
//     and split once into hi / lo planes [patch pixel][64 B]; its 16-byte chunk index is XORed with 2 * (patch column >> 3 & 1).
//     A transposing read takes 4 consecutive pixels x 32 B per 16-lane group: consecutive pixels are 64 B apart, so the four
//     sit in different 16-bank quarters at any column, and the partner group of the same half-wave is 8 pixels = 512 B on,
//     where the XOR moves it to the other 32 B of the quarter - conflict free at every tap shift (W % 16 == 0 keeps both
//     groups in one patch row);
//   - a K step is 32 consecutive pixels of the tile; the tap only moves the lane's x address by (r (W + 2) + s) pixels.
// Per 16x16x32 product the three terms stay gl.xh, gh.xl, gh.xh with gy^T in the A slot: a lane's four accumulators are four
// consecutive n of one dW row, stored with 16 bytes.  The bias gradient is an MFMA against a ones fragment in the waves of
// channel tile 0 of channel block 0.
//
// Choices and their arithmetic:
//   CB = 32, NB = 128 (64 for <= 64 columns): with the slabs pick_wgrad_splits grants (29 / 57 / 57 / 103) the grid is
//     8 x 29 = 232, 4 x 57 = 228, 4 x 57 = 228, 2 x 103 = 206 workgroups on 256 CUs; CB = 64 would halve that.  Operand stream
//     for 256->128: (4 x 50 x 32 + 96 x 128) x 4 B = 74.8 KB per tile x 576 tiles x 8 channel blocks = 345 MB (2.9x less).
//   TH = 2: 576 tiles over 57 / 103 splits is 11 / 6 tiles at most per workgroup against 10.1 / 5.6 on average; TH = 4 would
//     read a third less of x but leaves 6-against-5.05 and 3-against-2.8.
//   waves: 8 (512 threads), wave = channel tile (wid & 1) x NB / 64 column tiles; per K step 4 (2) gy fragments, 18 x
//     fragments and 54 (27) MFMAs: 44 transposing reads at 2 LDS cycles against 54 MFMAs at 16 - the LDS is not the bound.
//     Accumulators: 9 x NB / 64 x 4 = 72 (36) floats, + 8 (4) for the bias.
//   staging: one LDS image (512 (W + 2) + 1024 W bytes = 73 KiB at W = 48) and the NEXT tile's 4 + 6 float4 held in registers
//     while this one is multiplied, as wgrad_halo16_kernel does; two barriers per tile (162 MFMAs per wave between them).
// A plain grid (channel block, column block, pixel split): no tickets, no hand-off.  Every workgroup stores its whole block
// of its slab, tiles or not, so the reduce never reads what nobody wrote.
#pragma once
#include "wgrad_split3_kernel.hpp"

namespace acimg {

struct WgradTapParams {
    const float* X; int H, W, C, ldx;
    const float* G; int ldg;
    int Ngemm, Nld;              // columns, valid floats per gy row
    int tiles_y; long tiles;     // row tiles per image (TH rows each), tiles of all images
    int KK;                      // 9 C
    float* out; float* db_out; int ldo;   // slabs [gridDim.z][KK][ldo], [gridDim.z][ldo]  (dW / db themselves when gridDim.z == 1)
};

constexpr int WT_TH = 2, WT_CB = 32, WT_MAXW = 48;
static inline size_t wgrad_tap_lds(int W) { return (size_t)512 * (W + 2) + (size_t)1024 * W; }

template <int NB>
__global__ __launch_bounds__(512) void wgrad_tap_kernel(const WgradTapParams p) {
    constexpr int TH = WT_TH, XH = TH + 2, CB = WT_CB;
    constexpr int TNW = NB / 64;                       // 16-column tiles per wave
    constexpr int GQ = NB / 4;                         // float4 per gy row
    constexpr int NXL = (XH * (WT_MAXW + 2) * (CB / 4) + 511) / 512;    // x float4 per thread and tile (4)
    constexpr int NGL = TH * WT_MAXW * GQ / 512;                        // gy float4 per thread and tile (6 / 3)
    static_assert(NB == 128 || NB == 64, "column block");
    extern __shared__ __attribute__((aligned(16))) float wt_smem[];
    char* const lds = reinterpret_cast<char*>(wt_smem);
    const int XW = p.W + 2, npix = TH * p.W;
    const int XPL = XH * XW * 64;                      // one x plane
    const int GPL = npix * 256;                        // one gy plane
    char* const xh_pl = lds;
    char* const xl_pl = lds + XPL;
    char* const gh_pl = lds + 2 * XPL;
    char* const gl_pl = gh_pl + GPL;

    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int li = lane & 15, g = lane >> 4, q = li >> 2, pp = li & 3;
    const int ct = wid & 1, ng = wid >> 1;
    const int c0 = blockIdx.x * CB, n0 = blockIdx.y * NB;
    const long t_begin = (long)blockIdx.z * p.tiles / gridDim.z, t_end = (long)(blockIdx.z + 1) * p.tiles / gridDim.z;

    // ---- this thread's items of a tile (the same patch pixels and channels for every tile) -------------------------------
    int x_row[NXL], x_goff[NXL], x_lds[NXL];
#pragma unroll
    for (int k = 0; k < NXL; ++k) {
        const int i = tid + 512 * k;
        const int c4 = i & 7, pix = i >> 3;
        const int row = pix / XW, col = pix - row * XW;
        const bool ok = row < XH && col >= 1 && col <= p.W && c0 + c4 * 4 < p.C;
        x_row[k] = row < XH ? (ok ? row - 1 : 1 << 20) : -(1 << 20);       // image row relative to the tile; never inside / no item
        x_goff[k] = ((row - 1) * p.W + col - 1) * p.ldx + c0 + c4 * 4;
        x_lds[k] = (row * XW + col) * 64 + (((c4 >> 1) ^ (2 * ((col >> 3) & 1))) << 4) + 8 * (c4 & 1);
    }
    const int gq = tid % GQ, gpix0 = tid / GQ;         // gy items: pixel gpix0 + k * (512 / GQ), columns n0 + 4 gq ..
    const bool gn_ok = n0 + gq * 4 < p.Nld;

    float4 rx[NXL], rg[NGL];
    auto load_tile = [&](long tile) {
        const long img = tile / p.tiles_y;
        const int y0 = (int)(tile - img * p.tiles_y) * TH;
        const float* xi = p.X + (img * p.H + y0) * (long)p.W * p.ldx;
        const float* gi = p.G + (img * p.H + y0) * (long)p.W * p.ldg + n0 + gq * 4;
        const int left = (p.H - y0) * p.W;             // pixels of the image from the tile's first on
#pragma unroll
        for (int k = 0; k < NXL; ++k) {
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if ((unsigned)(y0 + x_row[k]) < (unsigned)p.H) v = *reinterpret_cast<const float4*>(xi + x_goff[k]);
            rx[k] = v;
        }
#pragma unroll
        for (int k = 0; k < NGL; ++k) {
            const int pix = gpix0 + k * (512 / GQ);
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (gn_ok && pix < npix && pix < left) v = *reinterpret_cast<const float4*>(gi + (long)pix * p.ldg);
            rg[k] = v;
        }
    };
    auto store_tile = [&]() {
#pragma unroll
        for (int k = 0; k < NXL; ++k) {
            if (x_row[k] > -(1 << 20)) {
                uint2 hi, lo;
                split4<SplitBF16>(rx[k], hi, lo);
                *reinterpret_cast<uint2*>(xh_pl + x_lds[k]) = hi;
                *reinterpret_cast<uint2*>(xl_pl + x_lds[k]) = lo;
            }
        }
#pragma unroll
        for (int k = 0; k < NGL; ++k) {
            const int pix = gpix0 + k * (512 / GQ);
            if (pix < npix) {
                const int f = (pix & 3) | (((pix >> 3) & 1) << 2);
                const int off = pix * 256 + (((gq >> 2) ^ f) << 5) + ((gq & 3) << 3);
                uint2 hi, lo;
                split4<SplitBF16>(rg[k], hi, lo);
                *reinterpret_cast<uint2*>(gh_pl + off) = hi;
                *reinterpret_cast<uint2*>(gl_pl + off) = lo;
            }
        }
    };

    f32x4 acc[9][TNW], accb[TNW];
#pragma unroll
    for (int i = 0; i < TNW; ++i) {
        accb[i] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int t = 0; t < 9; ++t) acc[t][i] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
    const __bf16 one = (__bf16)1.f;
    const b16x8 ones = {one, one, one, one, one, one, one, one};
    const bool bias_wave = p.db_out != nullptr && blockIdx.x == 0 && ct == 0;     // wave-uniform
    const int nks = npix >> 5;
    const int xcb = 2 * ct + (pp >> 1), xsub = 8 * (pp & 1);
    const int rowb = XW * 64;

    long tile = t_begin;
    if (tile < t_end) load_tile(tile);
    for (; tile < t_end; ++tile) {
        __syncthreads();                               // everyone has finished reading the previous tile
        store_tile();
        __syncthreads();
        if (tile + 1 < t_end) load_tile(tile + 1);     // in flight while this tile is multiplied
        // this lane's pixels of a K step: 32 ks + 8 g + 4 h + q, h = 0, 1 -> (orow, ocol + 4 h) of the tile
        int orow = 0, ocol = 8 * g + q;
        for (int ks = 0; ks < nks; ++ks) {
            while (ocol >= p.W) { ocol -= p.W; ++orow; }
            int xa[3][2];
#pragma unroll
            for (int s_ = 0; s_ < 3; ++s_)
#pragma unroll
                for (int h = 0; h < 2; ++h) {
                    const int cx = ocol + 4 * h + s_;
                    xa[s_][h] = (orow * XW + cx) * 64 + ((xcb ^ (2 * ((cx >> 3) & 1))) << 4) + xsub;
                }
            b16x8 gh[TNW], gl[TNW];
#pragma unroll
            for (int i = 0; i < TNW; ++i) {
                const int colbyte = ((ng * TNW + i) * 16) * 2;
                gh[i] = tr_frag(gh_pl + ks * 8192, 8 * g, colbyte, lane);
                gl[i] = tr_frag(gl_pl + ks * 8192, 8 * g, colbyte, lane);
            }
#pragma unroll
            for (int r = 0; r < 3; ++r)
#pragma unroll
                for (int s_ = 0; s_ < 3; ++s_) {
                    const b16x8 xh = tr16_frag<b16x8>(xh_pl + r * rowb + xa[s_][0], xh_pl + r * rowb + xa[s_][1]);
                    const b16x8 xl = tr16_frag<b16x8>(xl_pl + r * rowb + xa[s_][0], xl_pl + r * rowb + xa[s_][1]);
#pragma unroll
                    for (int i = 0; i < TNW; ++i) {
                        acc[r * 3 + s_][i] = SplitBF16::mfma(gl[i], xh, acc[r * 3 + s_][i]);
                        acc[r * 3 + s_][i] = SplitBF16::mfma(gh[i], xl, acc[r * 3 + s_][i]);
                        acc[r * 3 + s_][i] = SplitBF16::mfma(gh[i], xh, acc[r * 3 + s_][i]);
                    }
                }
            if (bias_wave) {
#pragma unroll
                for (int i = 0; i < TNW; ++i) {
                    accb[i] = SplitBF16::mfma(gl[i], ones, accb[i]);
                    accb[i] = SplitBF16::mfma(gh[i], ones, accb[i]);
                }
            }
            ocol += 32;
        }
    }

    // ---- store: lane (li, g) of acc[tap][i] holds dW[tap][c0 + 16 ct + li][n .. n + 3], n = n0 + 16 (ng TNW + i) + 4 g ----
    float* out = p.out + (long)blockIdx.z * p.KK * p.ldo;
    const int c = c0 + ct * 16 + li;
#pragma unroll
    for (int i = 0; i < TNW; ++i) {
        const int n = n0 + (ng * TNW + i) * 16 + 4 * g;
        if (n >= p.Ngemm) continue;
        const bool whole = n + 3 < p.Ngemm;
        if (c < p.C) {
#pragma unroll
            for (int t = 0; t < 9; ++t) {
                float* dst = out + (long)(t * p.C + c) * p.ldo + n;
                if (whole) *reinterpret_cast<f32x4*>(dst) = acc[t][i];
                else
                    for (int k = 0; k < 4; ++k)
                        if (n + k < p.Ngemm) dst[k] = acc[t][i][k];
            }
        }
        if (bias_wave && li == 0) {
            float* dst = p.db_out + (long)blockIdx.z * p.ldo + n;
            if (whole) *reinterpret_cast<f32x4*>(dst) = accb[i];
            else
                for (int k = 0; k < 4; ++k)
                    if (n + k < p.Ngemm) dst[k] = accb[i][k];
        }
    }
}

}  // namespace acimg
