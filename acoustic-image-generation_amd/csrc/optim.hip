// Parameter updates and random numbers of the acoustic-image train step for gfx950 (MI355X).  This file owns
//   adam_kernel      acimg_adam_step    one fused Adam update over a flat parameter buffer
//   axpy_kernel      acimg_axpy         y += a * x (gradient accumulation)
//   randn_kernel     acimg_randn        stateless standard normal samples (Philox4x32-10 + Box-Muller)
// Callers: acimg/ops.py and acimg/trainer.py.  tests/randn_ref.py restates randn_kernel.
#include "common.hpp"

namespace acimg {

__global__ __launch_bounds__(256) void axpy_kernel(float a, const float* x, float* y, long n) {
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) y[i] += a * x[i];
}

__global__ __launch_bounds__(256) void adam_kernel(float* p, const float* g, float* m, float* v, long n,
                                                   float lr_t, float b1, float b2, float eps, float gs) {
    const long n4 = n >> 2;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n4; i += (long)gridDim.x * 256) {
        float4 pv = reinterpret_cast<float4*>(p)[i];
        const float4 gv = reinterpret_cast<const float4*>(g)[i];
        float4 mv = reinterpret_cast<float4*>(m)[i];
        float4 vv = reinterpret_cast<float4*>(v)[i];
        float* pp = &pv.x;
        const float* gp = &gv.x;
        float* mp = &mv.x;
        float* vp = &vv.x;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const float gg = gp[k] * gs;
            mp[k] = b1 * mp[k] + (1.f - b1) * gg;
            vp[k] = b2 * vp[k] + (1.f - b2) * gg * gg;
            pp[k] -= lr_t * mp[k] / (sqrtf(vp[k]) + eps);
        }
        reinterpret_cast<float4*>(p)[i] = pv;
        reinterpret_cast<float4*>(m)[i] = mv;
        reinterpret_cast<float4*>(v)[i] = vv;
    }
    for (long i = (n4 << 2) + (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
        const float gg = g[i] * gs;
        m[i] = b1 * m[i] + (1.f - b1) * gg;
        v[i] = b2 * v[i] + (1.f - b2) * gg * gg;
        p[i] -= lr_t * m[i] / (sqrtf(v[i]) + eps);
    }
}

// ------------------------------------------------------------------------------------------
// standard normal samples, Philox4x32-10 counter RNG + Box-Muller (stands where the reference
// calls tf.random_normal, models/unet_acresnet.py:77): 4 samples per counter, stateless.
// ------------------------------------------------------------------------------------------
__device__ __forceinline__ void philox_round(uint32_t& c0, uint32_t& c1, uint32_t& c2, uint32_t& c3,
                                             uint32_t k0, uint32_t k1) {
    const uint64_t p0 = (uint64_t)0xD2511F53u * c0;
    const uint64_t p1 = (uint64_t)0xCD9E8D57u * c2;
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0;
    const uint32_t n1 = (uint32_t)p1;
    const uint32_t n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
    const uint32_t n3 = (uint32_t)p0;
    c0 = n0; c1 = n1; c2 = n2; c3 = n3;
}

__global__ __launch_bounds__(256) void randn_kernel(float* out, long n, uint64_t seed, uint64_t offset) {
    const long quads = (n + 3) >> 2;
    for (long q = (long)blockIdx.x * 256 + threadIdx.x; q < quads; q += (long)gridDim.x * 256) {
        const uint64_t ctr = (uint64_t)q + offset;
        uint32_t c0 = (uint32_t)ctr, c1 = (uint32_t)(ctr >> 32), c2 = 0x9E3779B9u, c3 = 0xBB67AE85u;
        uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
#pragma unroll
        for (int r = 0; r < 10; ++r) {
            philox_round(c0, c1, c2, c3, k0, k1);
            k0 += 0x9E3779B9u;
            k1 += 0xBB67AE85u;
        }
        const float u0 = ((float)(c0 >> 8) + 0.5f) * (1.0f / 16777216.0f);
        const float u1 = ((float)(c1 >> 8) + 0.5f) * (1.0f / 16777216.0f);
        const float u2 = ((float)(c2 >> 8) + 0.5f) * (1.0f / 16777216.0f);
        const float u3 = ((float)(c3 >> 8) + 0.5f) * (1.0f / 16777216.0f);
        const float r0 = sqrtf(-2.f * logf(u0)), r1 = sqrtf(-2.f * logf(u2));
        float s0, cs0, s1, cs1;
        sincospif(2.f * u1, &s0, &cs0);
        sincospif(2.f * u3, &s1, &cs1);
        const float v[4] = {r0 * cs0, r0 * s0, r1 * cs1, r1 * s1};
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (q * 4 + k < n) out[q * 4 + k] = v[k];
    }
}

}  // namespace acimg

using namespace acimg;

extern "C" {

int acimg_axpy(float a, const float* x, float* y, long n, void* stream) {
    hipLaunchKernelGGL(axpy_kernel, dim3(ew_grid(n)), dim3(256), 0, (hipStream_t)stream, a, x, y, n);
    return check_launch("axpy");
}

int acimg_adam_step(float* p, const float* g, float* m, float* v, long n, float lr_t, float beta1,
                    float beta2, float eps, float grad_scale, void* stream) {
    if (!aligned16(p) || !aligned16(g) || !aligned16(m) || !aligned16(v))
        return fail(ACIMG_EINVAL, "adam_step: buffers must be 16-byte aligned");
    hipLaunchKernelGGL(adam_kernel, dim3(ew_grid(n / 4 + 1)), dim3(256), 0, (hipStream_t)stream, p, g, m,
                       v, n, lr_t, beta1, beta2, eps, grad_scale);
    return check_launch("adam_step");
}

int acimg_randn(float* out, long n, uint64_t seed, uint64_t offset, void* stream) {
    if (n <= 0) return fail(ACIMG_EINVAL, "randn: n must be positive");
    hipLaunchKernelGGL(randn_kernel, dim3(ew_grid((n + 3) / 4)), dim3(256), 0, (hipStream_t)stream, out, n,
                       seed, offset);
    return check_launch("randn");
}

}  // extern "C"
