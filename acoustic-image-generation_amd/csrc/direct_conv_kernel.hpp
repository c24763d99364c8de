// Direct (no MFMA) fp32 convolution of the few-channel layers for gfx950 and its weight re-layout.
#pragma once
#include "common.hpp"

namespace acimg {

// ------------------------------------------------------------------------------------------
// Direct convolution for FEW-CHANNEL layers (C*K <= 512: the 4/8/16-channel full-resolution layers of the RGB /
// spectrogram U-Nets, models/unet_architecture.py:55-60,78-85).  There the implicit GEMM is a bad fit: a
// workgroup runs 3 K steps on tiles that are mostly padding and never amortises its prologue.  Here a lane owns
// one output pixel and 8 output channels, walks the taps with 16-byte loads (neighbouring lanes hit the same
// lines) and takes the weights as wave-uniform LDS broadcasts: 8 FMAs per input value, the work is VALU- and
// HBM-shaped.  mode 0: forward, weights HWIO w[tap][c][k]; mode 1: stride-1 data gradient read as a forward
// conv over gy with flipped taps, weights w[ntaps-1-tap][kout][cin].
// ------------------------------------------------------------------------------------------
struct DirectParams {
    const float* x; int ldx, H, W, C;
    float* y; int ldy, OH, OW, K;
    int R, S, stride, pad_t, pad_l;
    const float* w; int ldw, mode, wrows;   // wrows: rows per tap of the weight tensor (C fwd, Kout dgrad)
    const float* bias; int act;
    const float* res; int ldres;
    float* stats; int stats_ld;   // optional: per-256-pixel-block (sum, sum^2) of conv + bias, [blocks][2][stats_ld]
    long M;
};

// weights -> [K/8][ntaps][C][8] (8 consecutive output channels innermost), zero beyond K
__global__ __launch_bounds__(256) void direct_prepare_kernel(const DirectParams p, float* wprep, int total) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int ntaps = p.R * p.S;
    const int k = i & 7, c = (i >> 3) % p.C, tap = ((i >> 3) / p.C) % ntaps, kg = ((i >> 3) / p.C) / ntaps;
    const int ko = kg * 8 + k;
    float v = 0.f;
    if (ko < p.K)
        v = p.mode == 0 ? p.w[((long)tap * p.wrows + c) * p.ldw + ko]
                        : p.w[((long)(ntaps - 1 - tap) * p.wrows + ko) * p.ldw + c];
    wprep[i] = v;
}

// TR, TS, TC > 0: compile-time kernel extent / channel count (the tap and channel loops unroll completely: all the
// pixel loads of a thread are in flight together and the weights arrive as batched scalar loads); 0: run-time
template <int TR, int TS, int TC>
__global__ __launch_bounds__(256) void direct_conv_kernel(const DirectParams p, const float* __restrict__ wprep) {
    // the weight addresses below are wave-uniform: they become scalar loads (s_load_dwordx8), the FMAs take the
    // weights from SGPRs, no LDS and no vector-memory traffic for them
    const int R = TR ? TR : p.R, S = TS ? TS : p.S, C = TC ? TC : p.C;
    const int ntaps = R * S;
    // XCD-aware order: the dispatcher deals workgroups to the 8 XCDs round-robin, and a 256-pixel block shares its input
    // rows with the blocks one image row above and below (and with the other output-channel groups of its own pixels).
    // Dealt out in launch order those neighbours sit behind three different L2s and every input row is fetched three
    // times (counters: 243 MB read per launch for a 68 MB input); here XCD j walks the contiguous range
    // [j * per, (j + 1) * per) of (pixel block, channel group) pairs, channel groups innermost.
    const int ny = (p.K + 7) >> 3;
    const long total = ((p.M + 255) >> 8) * ny, per = (total + 7) >> 3;
    const long unit = (long)(blockIdx.x & 7) * per + (blockIdx.x >> 3);
    if (unit >= total) return;
    const long bx = unit / ny;
    const int by = (int)(unit - bx * ny);
    const int kg = by * 8;
    const float* __restrict__ wl = wprep + (long)by * ntaps * C * 8;
    const long m_raw = bx * 256 + threadIdx.x;
    const bool live = m_raw < p.M;
    const long m = live ? m_raw : p.M - 1;         // dead lanes recompute the last pixel and contribute nothing
    const int ow = (int)(m % p.OW);
    const long t = m / p.OW;
    const int oh = (int)(t % p.OH);
    const long n = t / p.OH;
    typedef float f32x2 __attribute__((ext_vector_type(2)));
    f32x2 acc2[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) acc2[k] = f32x2{0.f, 0.f};
    const int ih0 = oh * p.stride - p.pad_t, iw0 = ow * p.stride - p.pad_l;
    const float* const img = p.x + n * p.H * p.W * p.ldx;
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const int ih = ih0 + r;
        const int ihc = min(max(ih, 0), p.H - 1);
#pragma unroll
        for (int q = 0; q < S; ++q) {
            const int iw = iw0 + q;
            const bool ok = (unsigned)ih < (unsigned)p.H && (unsigned)iw < (unsigned)p.W;
            // clamped address: the load is unconditional (and can be hoisted), padding taps are zeroed by select
            const float* src = img + ((long)ihc * p.W + min(max(iw, 0), p.W - 1)) * p.ldx;
            const float* __restrict__ wt = wl + (r * S + q) * C * 8;
#pragma unroll
            for (int c = 0; c < C; c += 4) {
                float4 xv = *reinterpret_cast<const float4*>(src + c);
                const float xs[4] = {ok ? xv.x : 0.f, ok ? xv.y : 0.f, ok ? xv.z : 0.f, ok ? xv.w : 0.f};
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    // packed fp32 FMAs (v_pk_fma_f32: two accumulators per instruction, same rounding as fmaf)
                    const f32x2 xx = {xs[i], xs[i]};
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const f32x2 ww = *reinterpret_cast<const f32x2*>(wt + (c + i) * 8 + 2 * j);
                        acc2[j] = __builtin_elementwise_fma(xx, ww, acc2[j]);
                    }
                }
            }
        }
    }
    float acc[8];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        acc[2 * k] = acc2[k][0];
        acc[2 * k + 1] = acc2[k][1];
    }
    if (p.stats) {
        // batch-norm partials of this 256-pixel row block (conv + bias, before any activation): lanes -> waves -> LDS
        __shared__ float sred[4][16];
        const int wid = threadIdx.x >> 6, lane = threadIdx.x & 63;
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const float v = live ? acc[k] + (p.bias && kg + k < p.K ? p.bias[kg + k] : 0.f) : 0.f;
            const float s1 = wave_sum(v), s2 = wave_sum(v * v);
            if (lane == 0) {
                sred[wid][k] = s1;
                sred[wid][8 + k] = s2;
            }
        }
        __syncthreads();
        if (threadIdx.x < 16 && kg + (threadIdx.x & 7) < p.K) {
            const int k = threadIdx.x & 7, which = threadIdx.x >> 3;
            p.stats[(bx * 2 + which) * p.stats_ld + kg + k] =
                (sred[0][threadIdx.x] + sred[1][threadIdx.x]) + (sred[2][threadIdx.x] + sred[3][threadIdx.x]);
        }
    }
    if (!live) return;
    float* dst = p.y + m * p.ldy + kg;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        if (kg + 4 * h >= p.K) break;
        float4 o = make_float4(acc[4 * h], acc[4 * h + 1], acc[4 * h + 2], acc[4 * h + 3]);
        if (p.bias) {
            const float4 b = *reinterpret_cast<const float4*>(p.bias + kg + 4 * h);
            o.x += b.x; o.y += b.y; o.z += b.z; o.w += b.w;
        }
        if (p.res) {
            const float4 rr = *reinterpret_cast<const float4*>(p.res + m * p.ldres + kg + 4 * h);
            o.x += rr.x; o.y += rr.y; o.z += rr.z; o.w += rr.w;
        }
        o.x = apply_act(o.x, p.act); o.y = apply_act(o.y, p.act);
        o.z = apply_act(o.z, p.act); o.w = apply_act(o.w, p.act);
        const int left = p.K - (kg + 4 * h);          // pad columns (K % 4 != 0) are written as zeros
        if (left < 4) {
            o.w = 0.f;
            if (left < 3) o.z = 0.f;
            if (left < 2) o.y = 0.f;
        }
        *reinterpret_cast<float4*>(dst + 4 * h) = o;
    }
}

}  // namespace acimg
