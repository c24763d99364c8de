// What the split-MFMA implicit-GEMM kernels share on the device, stated once: the three-term sweep of one K step and the
// balanced K ranges of a tail tile.  (The K-range hand-off is igemm_kernel.hpp's - the exact-f32 kernel's split-K uses it
// too; the counted wait, the transposing fragment read and the vector types every LDS-DMA / MFMA kernel needs are
// common.hpp's.)
// Device-inline only (conv_host.hpp's rule for kernel headers): no kernel, no launch, no read of g_cfg.  Included by
// igemm_split3_kernel.hpp, and through it by every split-operand kernel header.
// Every function here is inlined into kernels whose instruction streams are held fixed (tools/codeobj_diff.py,
// profiles/gemm_core/): a parameter keeps the type and value category its callers had in place, and a kernel whose code
// would change with the shared form keeps its own, with a pointer to the statement here.
#pragma once
#include "igemm_kernel.hpp"

namespace acimg {

// ---- the split product of one K step ---------------------------------------------------------------------------------
// x * w ~= xh*wh + xh*wl + xl*wh per 16x16x32 product, three MFMAs accumulated in fp32 (TR::mfma: SplitF16 / SplitBF16 of
// igemm_split3_kernel.hpp).  Weights sit in the A slot (b*), activations in the B slot (a*): rows of D = output channels.
// TERM ORDER per accumulator: 0: bl*ah, 1: bh*al, 2: bh*ah - the small terms first, so that they are not rounded away
// against the large one.  The order is part of the result's bits: every trunk kernel form (one-tile, persistent, ring;
// halo up to its K order) and the tap-sharing kernels add the same three products in this order, which is what the tests
// that compare them bit for bit rest on.  It is written here and nowhere else.
// One term of one accumulator row i (the granule the ring kernel interleaves its reads and requests with):
template <typename TR, int T, int TN>
__device__ __forceinline__ void split_term_row(f32x4 (&acc)[TN], const typename TR::V8& ah, const typename TR::V8& al,
                                               const typename TR::V8 (&bh)[TN], const typename TR::V8 (&bl)[TN]) {
    static_assert(T >= 0 && T < 3, "term");
#pragma unroll
    for (int j = 0; j < TN; ++j) acc[j] = TR::mfma(T == 0 ? bl[j] : bh[j], T == 1 ? al : ah, acc[j]);
}
// One term over the whole wave tile (the persistent kernel puts its requests between the terms):
template <typename TR, int T, int TM, int TN>
__device__ __forceinline__ void split_term(f32x4 (&acc)[TM][TN], const typename TR::V8 (&ah)[TM],
                                           const typename TR::V8 (&al)[TM], const typename TR::V8 (&bh)[TN],
                                           const typename TR::V8 (&bl)[TN]) {
#pragma unroll
    for (int i = 0; i < TM; ++i) split_term_row<TR, T>(acc[i], ah[i], al[i], bh, bl);
}
// The sweep: TERM-MAJOR.  The three terms of a product are a whole sweep (TM x TN MFMAs) apart, so no MFMA waits on its
// predecessor's accumulator; the per-accumulator order above is unchanged.  The caller has issued ALL fragment reads of
// the step before it (one exposed LDS latency per step instead of one per fragment pair) and keeps them there with a
// __builtin_amdgcn_sched_barrier(0) of its own.  TERMS == 1 (16-bit operand arithmetic / storage: the hi halves multiplied
// once) keeps only the last term; al / bl are then never read.
template <typename TR, int TERMS, int TM, int TN>
__device__ __forceinline__ void split_sweep(f32x4 (&acc)[TM][TN], const typename TR::V8 (&ah)[TM],
                                            const typename TR::V8 (&al)[TM], const typename TR::V8 (&bh)[TN],
                                            const typename TR::V8 (&bl)[TN]) {
    static_assert(TERMS == 1 || TERMS == 3, "1 = rounded operands, 3 = split product");
    if (TERMS == 3) {
        split_term<TR, 0>(acc, ah, al, bh, bl);
        split_term<TR, 1>(acc, ah, al, bh, bl);
    }
    split_term<TR, 2>(acc, ah, al, bh, bl);
}

// ---- balanced K ranges of a tail tile --------------------------------------------------------------------------------
// `kiters` K steps cut into `s` ranges whose lengths differ by at most one: base = kiters / s, the first kiters % s ranges
// one step longer.  Range r is [begin, end).
struct KRange {
    int begin, end;
};
__device__ __forceinline__ KRange balanced_krange(const int kiters, const int s, const int r) {
    const int base = kiters / s, extra = kiters - base * s;
    KRange k;
    k.begin = r * base + min(r, extra);
    k.end = k.begin + base + (r < extra ? 1 : 0);
    return k;
}

}  // namespace acimg
