// Few-channel 3x3 convolution (forward / data gradient) on split 16-bit MFMAs for gfx950 and its weight image.
#pragma once
#include "igemm_split3_kernel.hpp"

namespace acimg {

// ------------------------------------------------------------------------------------------
// MFMA form of the FEW-CHANNEL 3x3 / stride-1 / SAME layers (8 or 16 channels in, up to 32 out: the full-resolution
// layers of the RGB / spectrogram U-Nets; round 4).  The direct kernel does these with packed fp32 FMAs at ~2x its
// VALU bound (224x298 8->8: 61 us for 27 us of bytes), every input value fetched nine times through the L1.  Here the taps
// are the GEMM's K axis: a pixel's CIN channels are one 16- or 32-byte run of a 16-bit plane, so the 8 k-values a lane
// holds of a 16x16x32 MFMA operand are ONE tap's channels of ONE pixel - a single ds_read_b128 at the tap's shift, four
// (two) taps per MFMA, 9 taps in 3 (5) MFMAs per term with the spare tap slots multiplied by zero weights.  A workgroup
// stages a 16 x 32 pixel tile WITH ITS HALO once (fp32 -> hi / lo planes on the way), keeps the whole weight image in
// registers (weights in the A slot: a lane's 4 accumulators are 4 consecutive output channels of one pixel, 16-byte
// stores), 3-term split product (fp32-class: f16 hi/lo forward, bf16 hi/lo for gradients).  MODE 0: forward - bias, raw
// output, batch-norm partials of conv + bias: one statistics row per workgroup; MODE 1: data gradient as a forward conv of
// gy with the flipped / transposed image, residual added.  Persistent workgroups, two per CU; XCD j walks the contiguous
// tile range [j * per, (j + 1) * per) so that neighbouring tiles share an L2; the next tile's loads are held in registers
// while the current one is multiplied.
// ------------------------------------------------------------------------------------------
struct FewParams {
    const float* X; int H, W, ldx;               // H, W: the OUTPUT grid (tiles); the tensor that is convolved:
    int Hin, Win, SH, SW, dil, pad_t, pad_l;     //   Hin x Win pixels, stored SH x SW (dil 2: zero-inserted view of a stride-2 gy)
    const char* Wimg; unsigned w_lo_off;         // 16-bit image [NOUTP][KTOT] (k = tap slot * CIN + c), hi plane; lo plane w_lo_off bytes on
    float* Y; int ldy, nout;                     // nout: real output channels (multiple of 4)
    const float* bias; const float* res; int ldres;
    float* stats; int stats_ld;                  // [gridDim.x][2][stats_ld] or null
    int tiles_x, tiles_y; long tiles, per;
    // the producer's deferred batch norm on load: x' = relu(x * a_scale[c] + a_shift[c]) for pixels INSIDE the image (the
    // conv's zero padding applies after the affine); null = x as stored
    const float* a_scale; const float* a_shift; int a_relu;
    // weight preparation
    const float* w; int ldw, wrows, cin, mode;
};
constexpr int FEW16_WGS = 512;
constexpr int few16_ktot(int cin) { return ((9 + 32 / cin - 1) / (32 / cin)) * 32; }

// w (fp32 HWIO, possibly the flipped / transposed view of a data gradient) -> the [NOUTP][KTOT] hi / lo image
template <typename TR>
__global__ __launch_bounds__(256) void few16_prepare_kernel(const FewParams p, int CIN, int NOUTP, typename TR::T* img) {
    typedef typename TR::T T;
    const int KTOT = few16_ktot(CIN);
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= NOUTP * KTOT) return;
    const int row = i / KTOT, k = i - row * KTOT;
    const int slot = k / CIN, c = k - slot * CIN;
    float v = 0.f;
    if (slot < 9 && row < p.nout && c < p.cin)
        v = p.mode == 0 ? p.w[((long)slot * p.wrows + c) * p.ldw + row] : p.w[((long)(8 - slot) * p.wrows + row) * p.ldw + c];
    v *= TR::WSCALE;
    const T h = (T)v;
    img[i] = h;
    img[(size_t)NOUTP * KTOT + i] = (T)(v - (float)h);
}

template <typename TR, int CIN, int NOUTP, int MODE, int CLOAD = CIN>
__global__ __launch_bounds__(512, (NOUTP == 32 && MODE == 0) ? 2 : 4) void conv_few16_kernel(const FewParams p) {
    typedef typename TR::V8 V8;
    constexpr int TH = 16, TW = 32, XH = TH + 2, XWV = TW + 2, XW = 36;
    constexpr int PB = CIN * 2;                        // bytes per pixel and plane
    constexpr int XPL = XH * XW * PB;
    constexpr int TPK = 32 / CIN;                      // taps per 32-deep MFMA
    constexpr int NKB = (9 + TPK - 1) / TPK;           // MFMAs per term and tile
    constexpr int KTOT = NKB * 32;
    constexpr int NT = NOUTP / 16;
    constexpr int NXL = (XH * XWV * (CLOAD / 4) + 511) / 512;
    static_assert((CIN == 8 || CIN == 16) && (CLOAD == CIN || (CIN == 8 && CLOAD == 4)), "few-channel instance");
    static_assert(2 * XPL >= 8 * 2 * NOUTP * 4, "statistics scratch");
    __shared__ __attribute__((aligned(16))) char xl[2 * XPL];
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int li = lane & 15, g = lane >> 4;

    // the weight image -> registers (once per workgroup): lane (li, g) of (n, kb) holds row 16 n + li, k = 32 kb + 8 g .. + 7
    V8 wh[NT][NKB], wlo[NT][NKB];
#pragma unroll
    for (int n = 0; n < NT; ++n)
#pragma unroll
        for (int kb = 0; kb < NKB; ++kb) {
            const size_t off = ((size_t)(n * 16 + li) * KTOT + kb * 32 + g * 8) * 2;
            wh[n][kb] = *reinterpret_cast<const V8*>(p.Wimg + off);
            wlo[n][kb] = *reinterpret_cast<const V8*>(p.Wimg + p.w_lo_off + off);
        }
    // this lane's tap shift of each MFMA: slot = kb * TPK + g / (4 / TPK); spare slots read tap 0 (their weights are zero)
    int boff[NKB];
#pragma unroll
    for (int kb = 0; kb < NKB; ++kb) {
        int slot = kb * TPK + (CIN == 8 ? g : g >> 1);
        if (slot > 8) slot = 0;
        const int r = slot / 3, q = slot - 3 * r;
        boff[kb] = (r * XW + q) * PB + (CIN == 8 ? 0 : (g & 1) * 16);
    }

    float4 rx[NXL];
    unsigned okm = 0;                          // which of rx[] came from inside the image (the affine applies to those only)
    // (a thread's items are always the same four channels: 512 is a multiple of CLOAD / 4)
    const float4 asc = p.a_scale ? *reinterpret_cast<const float4*>(p.a_scale + (tid % (CLOAD / 4)) * 4) : make_float4(1.f, 1.f, 1.f, 1.f);
    const float4 ash = p.a_scale ? *reinterpret_cast<const float4*>(p.a_shift + (tid % (CLOAD / 4)) * 4) : make_float4(0.f, 0.f, 0.f, 0.f);
    auto load_tile = [&](long tile) {
        okm = 0;
        const int tx = (int)(tile % p.tiles_x);
        const long t2 = tile / p.tiles_x;
        const int ty = (int)(t2 % p.tiles_y);
        const long img = t2 / p.tiles_y;
        const float* xi = p.X + img * p.SH * p.SW * p.ldx;
#pragma unroll
        for (int k = 0; k < NXL; ++k) {
            const int i = tid + 512 * k;
            const int c4 = i % (CLOAD / 4), pix = i / (CLOAD / 4);
            const int row = pix / XWV, col = pix - row * XWV;
            const int iy = ty * TH + row - p.pad_t, ix = tx * TW + col - p.pad_l;
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            bool ok = row < XH && (unsigned)iy < (unsigned)p.Hin && (unsigned)ix < (unsigned)p.Win;
            int sy = iy, sx = ix;
            if (p.dil == 2) {               // the zero-inserted view: only the even positions hold data
                ok = ok && !((iy | ix) & 1);
                sy >>= 1; sx >>= 1;
            }
            if (ok) {
                v = *reinterpret_cast<const float4*>(xi + ((long)sy * p.SW + sx) * p.ldx + c4 * 4);
                okm |= 1u << k;
            }
            rx[k] = v;
        }
    };
    auto store_tile = [&]() {
#pragma unroll
        for (int k = 0; k < NXL; ++k) {
            const int i = tid + 512 * k;
            const int c4 = i % (CLOAD / 4), pix = i / (CLOAD / 4);
            const int row = pix / XWV, col = pix - row * XWV;
            if (row < XH) {
                const int off = (row * XW + col) * PB + c4 * 8;
                uint2 hi, lo;
                split4<TR>(p.a_scale && ((okm >> k) & 1u) ? affine_relu4(rx[k], asc, ash, p.a_relu != 0) : rx[k], hi, lo);
                *reinterpret_cast<uint2*>(xl + off) = hi;
                *reinterpret_cast<uint2*>(xl + XPL + off) = lo;
            }
        }
    };
    if (CLOAD < CIN) {                      // 4 real channels in an 8-channel image: the upper half stays zero
        for (int i = tid; i < 2 * XH * XW; i += 512)
            *reinterpret_cast<uint2*>(xl + (i / (XH * XW)) * XPL + (i % (XH * XW)) * PB + 8) = make_uint2(0u, 0u);
    }

    f32x4 s1[NT], s2[NT], bv[NT];
#pragma unroll
    for (int n = 0; n < NT; ++n) {
        s1[n] = s2[n] = f32x4{0.f, 0.f, 0.f, 0.f};
        bv[n] = (MODE == 0 && p.bias && n * 16 + 4 * g < p.nout) ? *reinterpret_cast<const f32x4*>(p.bias + n * 16 + 4 * g)
                                                                 : f32x4{0.f, 0.f, 0.f, 0.f};
    }

    // XCD j = blockIdx.x % 8 walks tiles [j * per, (j + 1) * per), its gridDim.x / 8 workgroups interleaved
    const int xcd = blockIdx.x & 7, nslot = gridDim.x >> 3;
    const long t_end = min((long)(xcd + 1) * p.per, p.tiles);
    long tile = (long)xcd * p.per + (blockIdx.x >> 3);
    if (tile < t_end) load_tile(tile);
    for (; tile < t_end; tile += nslot) {
        __syncthreads();                               // everyone has finished reading the previous tile
        store_tile();
        __syncthreads();
        const int tx = (int)(tile % p.tiles_x);
        const long t2 = tile / p.tiles_x;
        const int ty = (int)(t2 % p.tiles_y);
        const long img = t2 / p.tiles_y;
        if (tile + nslot < t_end) load_tile(tile + nslot);     // in flight while this tile is multiplied
        // wave wid: tile rows 2 wid, 2 wid + 1, both 16-pixel halves
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int urow = 2 * wid + (u >> 1), ucol = (u & 1) * 16;
            const int base = (urow * XW + ucol + li) * PB;
            f32x4 acc[NT];
#pragma unroll
            for (int n = 0; n < NT; ++n) acc[n] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int kb = 0; kb < NKB; ++kb) {
                const V8 xh = *reinterpret_cast<const V8*>(xl + base + boff[kb]);
                const V8 xlo = *reinterpret_cast<const V8*>(xl + XPL + base + boff[kb]);
#pragma unroll
                for (int n = 0; n < NT; ++n) {
                    acc[n] = TR::mfma(wlo[n][kb], xh, acc[n]);
                    acc[n] = TR::mfma(wh[n][kb], xlo, acc[n]);
                    acc[n] = TR::mfma(wh[n][kb], xh, acc[n]);
                }
            }
            // lane (li, g) of acc[n] holds output pixel (row urow, column ucol + li), channels 16 n + 4 g .. + 3
            const int oy = ty * TH + urow, ox = tx * TW + ucol + li;
            if (oy < p.H && ox < p.W) {
                const long pix = (img * p.H + oy) * p.W + ox;
#pragma unroll
                for (int n = 0; n < NT; ++n) {
                    if (n * 16 + 4 * g < p.nout) {
                        f32x4 v = acc[n] * TR::OUTSCALE + bv[n];
                        if (MODE == 1) {
                            if (p.res) v += *reinterpret_cast<const f32x4*>(p.res + pix * p.ldres + n * 16 + 4 * g);
                        } else {
                            s1[n] += v;
                            s2[n] += v * v;
                        }
                        *reinterpret_cast<f32x4*>(p.Y + pix * p.ldy + n * 16 + 4 * g) = v;
                    }
                }
            }
        }
    }
    if (MODE == 0 && p.stats) {
        // the workgroup's statistics row: 16 pixel lanes by DPP, 8 waves through LDS, in wave order
        __syncthreads();
        float* red = reinterpret_cast<float*>(xl);     // [8][2][NOUTP]
#pragma unroll
        for (int n = 0; n < NT; ++n)
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const float a = row16_sum(s1[n][c]), b = row16_sum(s2[n][c]);
                if (li == 0) {
                    red[(wid * 2 + 0) * NOUTP + n * 16 + 4 * g + c] = a;
                    red[(wid * 2 + 1) * NOUTP + n * 16 + 4 * g + c] = b;
                }
            }
        __syncthreads();
        if (tid < 2 * NOUTP) {
            const int which = tid / NOUTP, n = tid % NOUTP;
            float t = 0.f;
#pragma unroll
            for (int w = 0; w < 8; ++w) t += red[(w * 2 + which) * NOUTP + n];
            if (n < p.nout) p.stats[((long)blockIdx.x * 2 + which) * p.stats_ld + n] = t;
        }
    }
}

}  // namespace acimg
