// Halo forms of the weight gradient for gfx950: a workgroup stages an output-pixel tile of gy and the x tile with its halo
// once and builds every tap from LDS.  wgrad_halo_kernel: exact f32, few channels; wgrad_halo16_kernel: bf16 / bf16x3,
// up to 64 input channels into at most 32 columns.
#pragma once
#include "igemm_split3_kernel.hpp"

namespace acimg {

// ------------------------------------------------------------------------------------------
// few-channel weight gradient (C <= 16 input channels, <= 32 output channels; the full-resolution layers of the
// RGB / spectrogram U-Nets: 72 x 8 ... 288 x 32 weights, millions of pixels).  As an implicit GEMM the im2col
// gather re-reads x once per tap through L2 (9x for 3x3); here a workgroup stages an 8 x 32 output-pixel tile of
// gy and the matching x tile WITH ITS HALO in LDS once and builds every tap from there:
//   dW[kk][n] += x_patch(pixel, kk) * gy[pixel][n]   on exact-f32 MFMA (16x16x4: 16 kk rows x 16 columns x 4
//   pixels), operands read from LDS per lane (ds_read_b32), the bias gradient as an all-ones row kk = KK.
// Workgroups walk tiles grid-stride and keep their sums in registers; one partial slab per workgroup, then the
// ordinary deterministic slab reduce.
// ------------------------------------------------------------------------------------------
struct WgradHaloParams {
    const float* X; int H, W, C, ldx;
    const float* G; int OH, OW, Kp, ldg;
    int R, S, stride, pad_t, pad_l;
    int XH, XW;                 // x tile extent incl. halo
    int tiles_x, tiles_y; long tiles;
    int KK;                     // R*S*C
    float* out; float* db_out; int ldo;   // slabs [gridDim.x][KK][ldo], [gridDim.x][ldo]
};
constexpr int WH_TH = 8, WH_TW = 32, WH_MAXT = 10;

// NT: 16-column tiles (1 or 2); NKT: 16-row tiles of (R*S*C + 1) the instance has accumulators for
template <int NT, int NKT>
__global__ __launch_bounds__(256, 3) void wgrad_halo_kernel(const WgradHaloParams p) {
    extern __shared__ __attribute__((aligned(16))) float wh_smem[];
    const int xsz = p.XH * p.XW * p.C;
    float* xs = wh_smem;                       // [XH][XW][C], then {1.0f, 0.0f, 0, 0}
    float* gs = wh_smem + xsz + 4;             // [8][32][Kp]
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int row16 = lane & 15, quad = lane >> 4;
    // LDS offset of this lane's x element for row tile t, relative to the pixel's window origin; the bias row reads
    // the constant 1, rows past it the constant 0 (absolute addresses: their pixel offset is masked away)
    int xoff[NKT], xmask[NKT];
#pragma unroll
    for (int t = 0; t < NKT; ++t) {
        const int kk = 16 * t + row16;
        if (kk < p.KK) {
            const int tap = kk / p.C, c = kk - tap * p.C;
            const int r = tap / p.S, q = tap - r * p.S;
            xoff[t] = (r * p.XW + q) * p.C + c;
            xmask[t] = -1;
        } else {
            xoff[t] = xsz + (kk == p.KK ? 0 : 1);      // the constants 1 (bias row) and 0
            xmask[t] = 0;
        }
    }
    int bcol[NT];
    float bscale[NT];               // columns past Kp multiply a valid (finite) element by 0
#pragma unroll
    for (int j = 0; j < NT; ++j) {
        bscale[j] = row16 + 16 * j < p.Kp ? 1.f : 0.f;
        bcol[j] = min(row16 + 16 * j, p.Kp - 1);
    }
    f32x4 acc[NKT][NT];
#pragma unroll
    for (int t = 0; t < NKT; ++t)
#pragma unroll
        for (int j = 0; j < NT; ++j) acc[t][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    if (tid == 0) {
        xs[xsz] = 1.f;
        xs[xsz + 1] = 0.f;
    }
    const int c4n = p.C >> 2, k4n = p.Kp >> 2;
    const int c4sh = c4n == 1 ? 0 : (c4n == 2 ? 1 : 2);
    // Software pipeline: the global loads of tile i+1 are issued (into registers) before tile i is multiplied, so
    // every workgroup keeps a tile's worth of HBM requests in flight all the time.
    // Staging is division-free and branch-free (stride 1, R, S <= 3: at most 10 x 34 x pixels): wave w takes x rows
    // w, w+4, w+8, its lanes the row's float4s lane, lane+64, lane+128; every load goes to a clamped (valid) address
    // and is zeroed by select, so all 9 + 4 loads of a thread are in flight together.
    float4 xv[3][3], gv[2][2];
    const int rowlen = p.XW << c4sh;
    auto issue = [&](long tile) {
        const int tx = (int)(tile % p.tiles_x);
        const long t2 = tile / p.tiles_x;
        const int ty = (int)(t2 % p.tiles_y);
        const long img = t2 / p.tiles_y;
        const int oh0 = ty * WH_TH, ow0 = tx * WH_TW;
        const int ih0 = oh0 * p.stride - p.pad_t, iw0 = ow0 * p.stride - p.pad_l;
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const int iy = wid + 4 * a;
            const int ih = ih0 + iy;
            const int ihc = min(max(ih, 0), p.H - 1);
            const float* grow = p.X + ((img * p.H + ihc) * p.W) * p.ldx;
#pragma unroll
            for (int bq = 0; bq < 3; ++bq) {
                const int e = lane + 64 * bq;
                const int ix = e >> c4sh, c4 = e & (c4n - 1);
                const int iw = iw0 + ix;
                const bool ok = iy < p.XH && e < rowlen && (unsigned)ih < (unsigned)p.H && (unsigned)iw < (unsigned)p.W;
                const float4 v = *reinterpret_cast<const float4*>(grow + (long)min(max(iw, 0), p.W - 1) * p.ldx + 4 * c4);
                xv[a][bq] = ok ? v : make_float4(0.f, 0.f, 0.f, 0.f);
            }
        }
#pragma unroll
        for (int half = 0; half < 2; ++half) {
            const int py = 2 * wid + half, px = lane & 31;
            const int oh = oh0 + py, ow = ow0 + px;
            const bool ok = oh < p.OH && ow < p.OW;
            const float* gsrc = p.G + ((img * p.OH + min(oh, p.OH - 1)) * p.OW + min(ow, p.OW - 1)) * p.ldg;
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const int k4 = (lane >> 5) + 2 * j;
                const float4 v = *reinterpret_cast<const float4*>(gsrc + 4 * min(k4, k4n - 1));
                gv[half][j] = ok && k4 < k4n ? v : make_float4(0.f, 0.f, 0.f, 0.f);
            }
        }
    };
    auto commit = [&]() {
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const int iy = wid + 4 * a;
#pragma unroll
            for (int bq = 0; bq < 3; ++bq) {
                const int e = lane + 64 * bq;
                if (iy < p.XH && e < rowlen)
                    *reinterpret_cast<float4*>(xs + iy * p.XW * p.C + (e >> c4sh) * p.C + 4 * (e & (c4n - 1))) = xv[a][bq];
            }
        }
#pragma unroll
        for (int half = 0; half < 2; ++half)
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const int k4 = (lane >> 5) + 2 * j;
                if (k4 < k4n)
                    *reinterpret_cast<float4*>(gs + ((2 * wid + half) * WH_TW + (lane & 31)) * p.Kp + 4 * k4) = gv[half][j];
            }
    };
    issue(blockIdx.x);
    for (long tile = blockIdx.x; tile < p.tiles; tile += gridDim.x) {
        __syncthreads();                                   // the previous tile has been consumed
        commit();
        __syncthreads();
        if (tile + gridDim.x < p.tiles) issue(tile + gridDim.x);
        // this wave: tile rows 2*wid, 2*wid+1 = 64 pixels, 4 at a time (quad = which of the 4); all addresses
        // advance incrementally (4 pixels per step, one row jump half way)
        {
            // register double buffer: the LDS reads of step g+1 are issued before the MFMAs of step g (all NKT row
            // tiles unconditionally - rows past KK + 1 read the constant 0 - so the loop has no branch)
            int xb = ((2 * wid) * p.XW + quad) * p.C;
            const float* gp = gs + ((2 * wid) * WH_TW + quad) * p.Kp;
            float a[2][NKT], b[2][NT];
#pragma unroll
            for (int t = 0; t < NKT; ++t) a[0][t] = xs[xoff[t] + (xb & xmask[t])];
#pragma unroll
            for (int j = 0; j < NT; ++j) b[0][j] = gp[bcol[j]] * bscale[j];
#pragma unroll 1
            for (int g2 = 0; g2 < 8; ++g2) {            // two steps per trip: buffers 0 -> 1 -> 0
#pragma unroll
                for (int cur = 0; cur < 2; ++cur) {
                    const int nxt = cur ^ 1;
                    const int gq = 2 * g2 + cur;
                    if (gq < 15) {
                        gp += 4 * p.Kp;
                        xb += 4 * p.C + (gq == 7 ? (p.XW - WH_TW) * p.C : 0);
#pragma unroll
                        for (int t = 0; t < NKT; ++t) a[nxt][t] = xs[xoff[t] + (xb & xmask[t])];
#pragma unroll
                        for (int j = 0; j < NT; ++j) b[nxt][j] = gp[bcol[j]] * bscale[j];
                    }
#pragma unroll
                    for (int t = 0; t < NKT; ++t)
#pragma unroll
                        for (int j = 0; j < NT; ++j)
                            acc[t][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[cur][t], b[cur][j], acc[t][j], 0, 0, 0);
                }
            }
        }
    }
    // the 4 waves add their sums in wave order (deterministic) in LDS: red[kk][NT*16]
    __syncthreads();
    float* red = wh_smem;
    const int rw = NT * 16;
    for (int w = 0; w < 4; ++w) {
        if (wid == w) {
#pragma unroll
            for (int t = 0; t < NKT; ++t) {
#pragma unroll
                for (int j = 0; j < NT; ++j)
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        float* dst = red + (16 * t + 4 * quad + i) * rw + 16 * j + row16;
                        *dst = (w == 0 ? 0.f : *dst) + acc[t][j][i];
                    }
            }
        }
        __syncthreads();
    }
    float* out = p.out + (long)blockIdx.x * p.KK * p.ldo;
    for (int e = tid; e < (p.KK + 1) * p.Kp; e += 256) {
        const int kk = e / p.Kp, n = e - kk * p.Kp;
        const float v = red[kk * rw + n];
        if (kk < p.KK) out[(long)kk * p.ldo + n] = v;
        else if (p.db_out) p.db_out[(long)blockIdx.x * p.ldo + n] = v;
    }
}

static size_t wgrad_halo_lds(int R, int S, int C, int Kp, int stride) {
    const int XH = (WH_TH - 1) * stride + R, XW = (WH_TW - 1) * stride + S;
    const size_t stage = ((size_t)XH * XW * C + 4 + (size_t)WH_TH * WH_TW * Kp) * sizeof(float);
    const size_t red = (size_t)WH_MAXT * 16 * (Kp > 16 ? 32 : 16) * sizeof(float);   // any instance's [16*NKT][16*NT]
    return stage > red ? stage : red;
}

// ------------------------------------------------------------------------------------------
// HALO form of the bf16 / bf16x3 weight gradient of the 3x3 / stride-1 layers with 32 or 64 input channels and 32 output
// channels (round 4; the 112x149 and 56x74 stages of the RGB / spectrogram U-Nets, models/unet_architecture.py:161-166,
// configs[1]).  As an implicit GEMM (wgrad_split3_kernel) these layers re-gather x once per tap through L2 - nine times the
// tensor for 2 x 576 x 32 MACs per pixel: 112x149 64->32 took 225 us against 41 us of HBM time for x and gy.  Here a
// workgroup stages a TH x 32 output-pixel tile of gy and the x tile WITH ITS HALO once, as bf16 (hi [, lo]) planes in LDS
// ([pixel][channel], 16-byte chunks swizzled by the pixel's COLUMN so that the transposing fragment reads - 4 pixels x 16
// channels per 16-lane group - are conflict free at every tap shift, and row offsets stay compile-time immediates), and
// forms all nine taps from there: K = the tile's pixels, one 32-pixel row per step, no barrier inside a tile.  gy^T sits in
// the A slot (a lane's 4 accumulators are 4 consecutive output channels of one dW row: 16-byte slab stores); the bias
// gradient rides as an MFMA against a constant ones fragment.  One workgroup per CU with the NEXT tile's global loads held in
// registers while the current one is multiplied (2 waves per SIMD: the 256-register budget pays for that); workgroups walk
// tiles grid-stride and keep their sums in registers: one partial slab each, then the deterministic slab reduce.
// Waves: C = 64: 4 channel tiles x 2 column tiles; C = 32: 2 x 2 x the tile's even / odd rows (summed through LDS at the end).
// ------------------------------------------------------------------------------------------
struct WgradHalo16Params {
    const float* X; int H, W, ldx;
    const float* G; int ldg;
    int tiles_x, tiles_y; long tiles;
    float* out; float* db_out; int ldo;      // slabs [gridDim.x][9 creal][ldo], [gridDim.x][ldo]
    int creal, nreal;                        // channels really there (multiples of 4; the rest of the C x 32 tile is zeros)
    // the producer's deferred batch norm on load: x' = relu(x * a_scale[c] + a_shift[c]) for pixels INSIDE the image (the
    // conv's zero padding applies after the affine); null = x as stored
    const float* a_scale; const float* a_shift; int a_relu;
};

// C: channel width of the x image (64, 32, or 16 for the few-channel layers: fewer real channels are zero padded);
// NNT: 16-column tiles of gy (2, or 1 for <= 16 output channels: the waves that would multiply padding take tile rows instead)
template <int C, int TERMS, int NNT = 2>
__global__ __launch_bounds__(512, C == 16 ? 4 : 1) void wgrad_halo16_kernel(const WgradHalo16Params p) {
    constexpr int TH = (TERMS == 1 || C == 16) ? 8 : 4, TW = 32, XH = TH + 2, XWV = TW + 2, XW = 36;
    constexpr int PITCH = C * 2;                      // bytes per pixel and plane
    constexpr int XPL = XH * XW * PITCH;              // one x plane
    constexpr int GPL = TH * TW * 64;                 // one gy plane (32 columns of bf16)
    constexpr int NCT = C / 16;                       // 16-channel tiles
    constexpr int NJ = 8 / (NCT * NNT);               // row groups: waves with the same (channel tile, column tile)
    constexpr int NXL = (XH * XWV * (C / 4) + 511) / 512, NGL = TH * TW * 8 / 512;     // float4 loads per thread and tile
    static_assert((C == 64 || C == 32 || C == 16) && TH % NJ == 0 && TH * TW * 8 % 512 == 0, "shape");
    extern __shared__ __attribute__((aligned(16))) float wh16_smem[];
    char* const lds = reinterpret_cast<char*>(wh16_smem);
    char* const gl = lds + (TERMS == 3 ? 2 : 1) * XPL;
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int li = lane & 15, g = lane >> 4, q = li >> 2, pp = li & 3;
    const int ct = wid % NCT, nt = (wid / NCT) % NNT, jh = wid / (NCT * NNT);
    // (C = 16: 32-byte pixels, no room to swizzle: pixels 8 apart share banks, a 2-way conflict the HBM-bound kernel absorbs)
    auto swx = [](int col) {
        return C == 64 ? 2 * (((col >> 1) & 1) | (((col >> 3) & 1) << 1)) : (C == 32 ? 2 * ((col >> 3) & 1) : 0);
    };
    auto swg = [](int col) { return 2 * ((col >> 3) & 1); };

    // fragment read addresses: lane (q, pp) of group g supplies pixel column s + 8 g + 4 h + q, channels 4 pp .. + 3 of its
    // 16-channel tile; the tile row is a compile-time distance
    int xb[3][2], gb[2];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const int col = 8 * g + 4 * h + q;
        gb[h] = (jh * TW + col) * 64 + (((2 * nt + (pp >> 1)) ^ swg(col)) << 4) + 8 * (pp & 1);
#pragma unroll
        for (int s_ = 0; s_ < 3; ++s_) {
            const int cx = col + s_;
            xb[s_][h] = (jh * XW + cx) * PITCH + (((2 * ct + (pp >> 1)) ^ swx(cx)) << 4) + 8 * (pp & 1);
        }
    }

    // this thread's items of a tile: x float4 (pixel of the XH x 34 window, 4 channels), gy float4 (pixel, 4 columns)
    float4 rx[NXL], rg[NGL];
    unsigned okm = 0;                          // which of rx[] came from inside the image (the affine applies to those only)
    // (a thread's x items are always the same four channels: 512 is a multiple of C / 4)
    const bool aff_ch = p.a_scale != nullptr && (tid % (C / 4)) * 4 < p.creal;
    const float4 asc = aff_ch ? *reinterpret_cast<const float4*>(p.a_scale + (tid % (C / 4)) * 4) : make_float4(1.f, 1.f, 1.f, 1.f);
    const float4 ash = aff_ch ? *reinterpret_cast<const float4*>(p.a_shift + (tid % (C / 4)) * 4) : make_float4(0.f, 0.f, 0.f, 0.f);
    auto load_tile = [&](long tile) {
        okm = 0;
        const int tx = (int)(tile % p.tiles_x);
        const long t2 = tile / p.tiles_x;
        const int ty = (int)(t2 % p.tiles_y);
        const long img = t2 / p.tiles_y;
        const float* xi = p.X + img * p.H * p.W * p.ldx;
        const float* gi = p.G + img * p.H * p.W * p.ldg;
#pragma unroll
        for (int k = 0; k < NXL; ++k) {
            const int i = tid + 512 * k;
            const int c4 = i % (C / 4), pix = i / (C / 4);
            const int row = pix / XWV, col = pix - row * XWV;
            const int iy = ty * TH + row - 1, ix = tx * TW + col - 1;
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (row < XH && c4 * 4 < p.creal && (unsigned)iy < (unsigned)p.H && (unsigned)ix < (unsigned)p.W) {
                v = *reinterpret_cast<const float4*>(xi + ((long)iy * p.W + ix) * p.ldx + c4 * 4);
                okm |= 1u << k;
            }
            rx[k] = v;
        }
#pragma unroll
        for (int k = 0; k < NGL; ++k) {
            const int i = tid + 512 * k;
            const int c4 = i & 7, pix = i >> 3;
            const int row = pix / TW, col = pix - row * TW;
            const int oy = ty * TH + row, ox = tx * TW + col;
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (oy < p.H && ox < p.W && c4 * 4 < p.nreal) v = *reinterpret_cast<const float4*>(gi + ((long)oy * p.W + ox) * p.ldg + c4 * 4);
            rg[k] = v;
        }
    };
    auto store_tile = [&]() {
#pragma unroll
        for (int k = 0; k < NXL; ++k) {
            const int i = tid + 512 * k;
            const int c4 = i % (C / 4), pix = i / (C / 4);
            const int row = pix / XWV, col = pix - row * XWV;
            if (row < XH) {
                const int off = (row * XW + col) * PITCH + (((c4 >> 1) ^ swx(col)) << 4) + 8 * (c4 & 1);
                uint2 hi, lo;
                split4<SplitBF16>(p.a_scale && ((okm >> k) & 1u) ? affine_relu4(rx[k], asc, ash, p.a_relu != 0) : rx[k], hi, lo);
                *reinterpret_cast<uint2*>(lds + off) = hi;
                if (TERMS == 3) *reinterpret_cast<uint2*>(lds + XPL + off) = lo;
            }
        }
#pragma unroll
        for (int k = 0; k < NGL; ++k) {
            const int i = tid + 512 * k;
            const int c4 = i & 7, pix = i >> 3;
            const int col = pix & (TW - 1);
            const int off = pix * 64 + (((c4 >> 1) ^ swg(col)) << 4) + 8 * (c4 & 1);
            uint2 hi, lo;
            split4<SplitBF16>(rg[k], hi, lo);
            *reinterpret_cast<uint2*>(gl + off) = hi;
            if (TERMS == 3) *reinterpret_cast<uint2*>(gl + GPL + off) = lo;
        }
    };

    f32x4 acc[9], accb = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int t = 0; t < 9; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
    const __bf16 one = (__bf16)1.f;
    const b16x8 ones = {one, one, one, one, one, one, one, one};

    long tile = blockIdx.x;
    if (tile < p.tiles) load_tile(tile);
    for (; tile < p.tiles; tile += gridDim.x) {
        __syncthreads();                               // everyone has finished reading the previous tile
        store_tile();
        __syncthreads();
        if (tile + gridDim.x < p.tiles) load_tile(tile + gridDim.x);     // in flight while this tile is multiplied
#pragma unroll
        for (int jj = 0; jj < TH / NJ; ++jj) {
            const int j = jj * NJ;                     // (+ jh: in the lane bases)
            const b16x8 gh = tr16_frag<b16x8>(gl + j * TW * 64 + gb[0], gl + j * TW * 64 + gb[1]);
            b16x8 glo;
            if (TERMS == 3) glo = tr16_frag<b16x8>(gl + GPL + j * TW * 64 + gb[0], gl + GPL + j * TW * 64 + gb[1]);
#pragma unroll
            for (int r = 0; r < 3; ++r)
#pragma unroll
                for (int s_ = 0; s_ < 3; ++s_) {
                    const char* xrow = lds + (j + r) * XW * PITCH;
                    const b16x8 xh = tr16_frag<b16x8>(xrow + xb[s_][0], xrow + xb[s_][1]);
                    if (TERMS == 3) {
                        const b16x8 xl = tr16_frag<b16x8>(xrow + XPL + xb[s_][0], xrow + XPL + xb[s_][1]);
                        acc[r * 3 + s_] = SplitBF16::mfma(glo, xh, acc[r * 3 + s_]);
                        acc[r * 3 + s_] = SplitBF16::mfma(gh, xl, acc[r * 3 + s_]);
                    }
                    acc[r * 3 + s_] = SplitBF16::mfma(gh, xh, acc[r * 3 + s_]);
                }
            if (ct == 0) {
                if (TERMS == 3) accb = SplitBF16::mfma(glo, ones, accb);
                accb = SplitBF16::mfma(gh, ones, accb);
            }
        }
    }
    // the row groups of one (channel tile, column tile) meet through LDS (C = 32), then lane (li, g) of acc[tap] holds
    // dW[tap * C + 16 ct + li][16 nt + 4 g .. + 3]
    if (NJ > 1) {
        // one round per row group (in group order: deterministic): its waves park their sums, group 0 adds them
        f32x4* red = reinterpret_cast<f32x4*>(lds);
        const int w0 = wid % (NCT * NNT);            // this wave's (channel tile, column tile) slot
        for (int r = 1; r < NJ; ++r) {
            __syncthreads();
            if (jh == r) {
#pragma unroll
                for (int t = 0; t < 9; ++t) red[(w0 * 10 + t) * 64 + lane] = acc[t];
                red[(w0 * 10 + 9) * 64 + lane] = accb;
            }
            __syncthreads();
            if (jh == 0) {
#pragma unroll
                for (int t = 0; t < 9; ++t) acc[t] += red[(w0 * 10 + t) * 64 + lane];
                accb += red[(w0 * 10 + 9) * 64 + lane];
            }
        }
        if (jh != 0) return;
    }
    float* out = p.out + (long)blockIdx.x * (9 * p.creal) * p.ldo;
    const bool nok = nt * 16 + 4 * g < p.nreal;
    if (nok && ct * 16 + li < p.creal) {
#pragma unroll
        for (int t = 0; t < 9; ++t)
            *reinterpret_cast<f32x4*>(out + (long)(t * p.creal + ct * 16 + li) * p.ldo + nt * 16 + 4 * g) = acc[t];
    }
    if (p.db_out && ct == 0 && li == 0 && nok)
        *reinterpret_cast<f32x4*>(p.db_out + (long)blockIdx.x * p.ldo + nt * 16 + 4 * g) = accb;
}

}  // namespace acimg
