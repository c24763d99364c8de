// Shared host/device helpers for libacimg (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstring>

#include "../../include/acimg.h"

namespace acimg {

// ---- per-thread error text -------------------------------------------------------------
inline char* err_buf() {
    static thread_local char buf[512] = {0};
    return buf;
}
inline int fail(int code, const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(err_buf(), 512, fmt, ap);
    va_end(ap);
    return code;
}
inline int check_launch(const char* what) {
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(ACIMG_ELAUNCH, "%s: %s", what, hipGetErrorString(e));
    return ACIMG_OK;
}
inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }
inline int cdiv(long a, long b) { return (int)((a + b - 1) / b); }
// workgroups of 256 threads for `work` items: ceil(work / 256), clamped to [1, cap]
inline int clamped_blocks(long work, long cap) {
    long b = (work + 255) / 256;
    if (b > cap) b = cap;
    if (b < 1) b = 1;
    return (int)b;
}
// grid of the grid-stride elementwise kernels
inline int ew_grid(long work_items) { return clamped_blocks(work_items, 4096); }

// ---- device helpers ---------------------------------------------------------------------
using f32x4 = __attribute__((ext_vector_type(4))) float;

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
    return v;
}
__device__ __forceinline__ float wave_min(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fminf(v, __shfl_xor(v, o, 64));
    return v;
}
__device__ __forceinline__ double wave_sum_d(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// block-wide sum for blockDim.x <= 1024 (multiple of 64); result valid in every thread
__device__ __forceinline__ float block_sum(float v, float* smem /* >= 17 floats */) {
    v = wave_sum(v);
    const int wid = threadIdx.x >> 6, lane = threadIdx.x & 63, nw = blockDim.x >> 6;
    __syncthreads();
    if (lane == 0) smem[wid] = v;
    __syncthreads();
    float r = 0.f;
    for (int i = 0; i < nw; ++i) r += smem[i];
    return r;
}

// per-component float4 arithmetic of the 16-byte elementwise passes
__device__ __forceinline__ float4 affine4(const float4 v, const float4 s, const float4 t) {
    return make_float4(v.x * s.x + t.x, v.y * s.y + t.y, v.z * s.z + t.z, v.w * s.w + t.w);
}
__device__ __forceinline__ float4 relu4(const float4 v) {
    return make_float4(fmaxf(v.x, 0.f), fmaxf(v.y, 0.f), fmaxf(v.z, 0.f), fmaxf(v.w, 0.f));
}
__device__ __forceinline__ float4 scale4(const float4 v, const float k) {
    return make_float4(v.x * k, v.y * k, v.z * k, v.w * k);
}
__device__ __forceinline__ float4 max4(const float4 a, const float4 b) {
    return make_float4(fmaxf(a.x, b.x), fmaxf(a.y, b.y), fmaxf(a.z, b.z), fmaxf(a.w, b.w));
}

// ---- split-fp16 ("f16x3") operand format ------------------------------------------------------
// A value v is kept as hi = f16(v*SCALE), lo = f16(v*SCALE - hi): 22 mantissa bits in 4 bytes.  The
// power-of-two scales keep fp16 in range: activations x2^-2 (finite up to 2.6e5), weights x2^10.
// (Where the halves of a pre-split activation tensor lie in memory - the brick planes - is split_planes.hpp's.)
constexpr float SPLIT3_WSCALE = 1024.f;
constexpr float SPLIT3_ASCALE = 0.25f;
constexpr float SPLIT3_OUTSCALE = 1.f / 256.f;   // undoes both on the fp32 accumulators
typedef _Float16 h16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 h16x4 __attribute__((ext_vector_type(4)));

// v (already scaled) -> packed hi / lo halves
__device__ __forceinline__ void split4_scaled(const float4 v, uint2& hi, uint2& lo) {
    const h16x4 h = {(_Float16)v.x, (_Float16)v.y, (_Float16)v.z, (_Float16)v.w};
    const h16x4 l = {(_Float16)(v.x - (float)h[0]), (_Float16)(v.y - (float)h[1]), (_Float16)(v.z - (float)h[2]),
                     (_Float16)(v.w - (float)h[3])};
    hi = __builtin_bit_cast(uint2, h);
    lo = __builtin_bit_cast(uint2, l);
}
// packed hi / lo halves -> fp32 values (unscaled)
__device__ __forceinline__ float4 unsplit4(const uint2 hi, const uint2 lo, float inv_scale) {
    const h16x4 h = __builtin_bit_cast(h16x4, hi), l = __builtin_bit_cast(h16x4, lo);
    return make_float4(((float)h[0] + (float)l[0]) * inv_scale, ((float)h[1] + (float)l[1]) * inv_scale,
                       ((float)h[2] + (float)l[2]) * inv_scale, ((float)h[3] + (float)l[3]) * inv_scale);
}

// ---- what every LDS-DMA / MFMA kernel needs (trunk and weight-gradient kernel headers, gram.hip) ------------------
using u32x4 = __attribute__((__vector_size__(4 * sizeof(unsigned int)))) unsigned int;    // a buffer store's 16 bytes
typedef __attribute__((address_space(3))) void* lds_ptr_t;                                // an LDS-DMA destination
// a buffer offset >= num_records of every descriptor (tensors < 2 GiB): the load returns zeros, an LDS-DMA writes zeros
constexpr unsigned OOB = 0x80000000u;
typedef short s16x4 __attribute__((ext_vector_type(4)));
typedef short s16x8 __attribute__((ext_vector_type(8)));

// `s_waitcnt vmcnt(N)` with a compile-time N.  An `asm volatile` with a memory clobber: nothing moves across it, and the
// compiler's own counter bookkeeping does not see it (where that matters - a pipelined loop whose fragment registers were
// loaded one iteration earlier - igemm_split3r_kernel.hpp waits through the builtin instead).
template <int N>
__device__ __forceinline__ void wait_vmcnt() {
    static_assert(N >= 0 && N < 64, "vmcnt immediate");
    asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
}

// The transposing fragment read of gfx950: `ds_read_b64_tr_b16` returns, per 16-lane group and column-major, a
// 4 (k) x 16 (column) block of 16-bit elements out of a tile kept [k][column] in LDS - exactly the layout of a 16x16x32
// MFMA operand, whose lane group g owns k = 8 g .. 8 g + 7.  So a fragment is TWO reads, of the k rows 8 g + (0 .. 3) at
// r0 and 8 g + (4 .. 7) at r1 (the caller's tile image decides the two addresses), packed into one operand V8 (h16x8 or
// b16x8).
template <typename V8>
__device__ __forceinline__ V8 tr16_frag(const char* r0, const char* r1) {
    const s16x4 v0 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)r0);
    const s16x4 v1 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)r1);
    const s16x8 v = {v0[0], v0[1], v0[2], v0[3], v1[0], v1[1], v1[2], v1[3]};
    return __builtin_bit_cast(V8, v);
}

__device__ __forceinline__ float apply_act(float v, int act) {
    if (act == ACIMG_ACT_RELU) return fmaxf(v, 0.f);
    if (act == ACIMG_ACT_SIGMOID) return 1.f / (1.f + __expf(-v));
    return v;
}

}  // namespace acimg
