// Tap-sharing split-operand forward conv of the 3x3 / stride-1 / SAME layers with WIDE channels (the generator's 36x48 layers:
// 256->128, 128->128, 128->64, 64->64) for gfx950, instantiated for SplitF16 (forward: bias + activation) and SplitBF16 (data
// gradient: a forward conv of gy with the flipped / transposed image; residual + ReLU mask).
//
// As a per-tap implicit GEMM (igemm_split3_kernel) every one of the 9 taps x C / 32 K steps gathers its 128 x 32 fp32
// activation tile from L2 again, splits it again in VALU and writes the halves to LDS again: each activation element is
// fetched and split nine times per column tile.  Here a workgroup owns TH = 2 whole image rows (2 W consecutive GEMM rows,
// W = 32 or 48: a 16-pixel MFMA tile never straddles an image row) x NB output columns and walks K chunk-major:
//   - per 32-channel chunk the patch of (TH + 2) x (W + 2) pixels is loaded ONCE (zeros outside the image) and split once
//     into hi / lo planes [patch pixel][64 B] whose 16-byte chunk index is XORed with 2 * (patch pixel >> 2 & 1).  The
//     hardware serves a ds_read_b128 in lane groups that hold fragment rows 0-3 / 12-15 with k chunk g and rows 4-11 with
//     g ^ 1; rows 4 apart share a 64-byte quarter of the 256-byte bank window, and with this XOR the four of them land on
//     four different chunks WHEREVER the fragment's 16 consecutive pixels start - conflict free at every tap shift (the
//     eight XOR patterns of period 4 that do so are (0,2,0,2) and its like; the row-aligned swz() of the per-tap kernel
//     is not among them).  The 64 + 16 byte pitch of conv_halo16_kernel was built first: two-way conflicts on 3 of 16
//     slots of every activation fragment, 8 KB more LDS, the ten launches 664 us against 636 with the XOR;
//   - a tap only moves the fragment address by (r (W + 2) + s) pixels;
//   - the weights are the unchanged [hi | lo][n][tap C + c] image, read per (chunk, tap) - only the byte offset differs
//     from the per-tap kernel - through registers into the same double-buffered, swizzled LDS stage, two steps ahead;
//   - the next chunk's patch loads are issued when this chunk is stored and stay in registers while its nine taps are
//     multiplied; all loads of a chunk are issued before any conversion, and the conversion happens at the store.
// Per 16x16x32 product the three terms stay bl.ah, bh.al, bh.ah (weights in the A slot) and the accumulators go through
// igemm_epilogue unchanged (2^-8 output scale of the f16 form first).  K is summed chunk-major instead of tap-major: the
// same products, in another order.
//
// Choices and their arithmetic:
//   TH = 2: at W = 48 a 96 x 128 tile, 576 tiles at batch 32; 8 waves = 2 tile rows x 4 column groups, a wave owns 3 x 2
//     (3 x 1 at NB = 64) MFMA tiles: 18 MFMAs and 10 fragment reads per step, 24 accumulator registers.  TH = 4 would read a
//     third less of x and give 36 MFMAs per 16 reads but leaves 288 tiles for 256 CUs.
//   activation bytes per nine steps: 4 x 50 x 32 x 4 B = 25.6 KB of fp32 instead of 9 x 12.3 KB; split VALU one ninth.
//   LDS: patch 2 x 4 x 50 x 64 B = 25600 B + weight stages 2 x 16 KiB = 58368 B at W = 48, NB = 128 (41984 B at NB = 64):
//     two workgroups per CU, and below the per-tap kernel's 64 KiB next to the trunk lanes' 68 KiB workgroups.
//   registers: the chunk's channel offset and the weight step's K offset ride in the buffer loads' scalar offset, and the
//     items' LDS offsets are one base plus constants: with 64-bit pointers per item the bf16 instance needed 138 VGPRs
//     (one workgroup per CU) or spilled at 128.  __launch_bounds__(512, 4) asks for the two workgroups.
//   a plain grid (row tile, column block): no atomics, no tickets, no workspace; one barrier per step, two at a chunk's end.
//   an odd height's last tile holds one image row: its second row loads zeros and its waves store nothing.
//   not built: TH = 3 / 4 (more accumulators than 128 VGPRs hold beside the fragments), the weight image in LDS-tile order
//     fetched by LDS-DMA (the next increment: the kernel is at ~3x its MFMA bound on 256->128).
// Resource usage (-Rpass-analysis=kernel-resource-usage; VGPRs, scratch, waves / SIMD), W = 48: f16 NB = 128: 112, 0, 4;
// f16 NB = 64: 82, 0, 5; bf16 NB = 128: 128, 0, 4; bf16 NB = 64: 90, 0, 5.  W = 32: 90 / 66 / 98 / 70 VGPRs, no scratch.
#pragma once
#include "igemm_split3_kernel.hpp"

namespace acimg {

constexpr int CT_TH = 2, CT_PITCH = 64;
static constexpr int conv_tap_lds(int W, int NB) { return 2 * (CT_TH + 2) * (W + 2) * CT_PITCH + 2 * 2 * NB * 64; }

template <typename TR, int W, int NB>
__global__ __launch_bounds__(512, 4) void conv_tap_kernel(const IgemmParams p) {
    typedef typename TR::V8 V8;
    constexpr int TH = CT_TH, XH = TH + 2, XW = W + 2, PITCH = CT_PITCH;
    constexpr int XPL = XH * XW * PITCH;               // one patch plane
    constexpr int BM = TH * W, WGM = TH, WGN = 8 / WGM, WTM = BM / WGM, WTN = NB / WGN, TM = WTM / 16, TN = WTN / 16;
    constexpr int B_BYTES = NB * 64, WSTAGE = 2 * B_BYTES;
    constexpr int NXL = (XH * XW * 8 + 511) / 512;     // patch float4 per thread and chunk (4 / 3)
    constexpr int NBL = 2 * NB * 4 / 512;              // weight 16-byte chunks per thread and step (2 / 1)
    static_assert((NB == 128 || NB == 64) && W % 16 == 0 && WTM == W && XPL % 16 == 0, "tile / thread mapping");

    extern __shared__ __attribute__((aligned(16))) float smem[];
    char* const lds = reinterpret_cast<char*>(smem);
    char* const wst = lds + 2 * XPL;

    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int wm = wid / WGN, wn = wid % WGN;          // wm = tile row
    const int li = lane & 15, g = lane >> 4;
    const int tiles_y = (p.H + TH - 1) / TH;
    const int img = blockIdx.x / tiles_y, y0 = (blockIdx.x - img * tiles_y) * TH;
    const int m0 = (img * p.H + y0) * W, n0 = blockIdx.y * NB;
    const int Ktot = 9 * p.C;

    const __amdgpu_buffer_rsrc_t rsA =
        __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(p.A), 0, p.a_bytes, 0x00020000);
    const __amdgpu_buffer_rsrc_t rsB =
        __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(p.B), 0, p.b_bytes, 0x00020000);

    // ---- this thread's patch items: (patch pixel, four channels), the same for every chunk ----------------------------------
    // item k is patch pixel (tid >> 3) + 64 k, channels 4 (tid & 7) ..: its LDS offset is item 0's plus a constant; its byte
    // offset in x is out of the descriptor's range when the pixel lies outside the image (the load then returns zeros), and
    // the chunk's channel offset rides in the load's scalar offset
    const int x_lds0 = (tid >> 3) * PITCH + (((tid >> 1) & 3) ^ (2 * ((tid >> 5) & 1))) * 16 + (tid & 1) * 8;   // (64 k pixels on: same XOR)
    unsigned x_voff[NXL];
#pragma unroll
    for (int k = 0; k < NXL; ++k) {
        const int pix = (tid >> 3) + 64 * k;
        const int row = pix / XW, col = pix - row * XW;
        const bool ok = row < XH && col >= 1 && col <= W && (unsigned)(y0 + row - 1) < (unsigned)p.H;
        x_voff[k] = ok ? (unsigned)(((m0 + (row - 1) * W + col - 1) * p.lda + (tid & 7) * 4) * 4) : OOB;
    }
    // ---- weight chunks of this thread: (hi / lo, row, 16-byte k chunk) as in igemm_split3_kernel ---------------------------
    // chunk j of NBL is item 0's 512 / (4 NB) planes further (NB = 128: j = hi / lo; NB = 64: one chunk per thread)
    const int b_which = tid / (NB * 4), b_row = (tid & (NB * 4 - 1)) >> 2, b_kc = tid & 3;
    const unsigned b_plane = (unsigned)((long)p.Nld * Ktot * 2);
    const unsigned b_goff0 = n0 + b_row < p.Nld ? (unsigned)((((long)b_which * p.Nld + n0 + b_row) * Ktot + b_kc * 8) * 2) : OOB;
    const int b_lds0 = b_which * B_BYTES + b_row * 64 + ((b_kc ^ swz(b_row)) << 4);

    float4 rx[NXL];
    uint4 rb0[NBL], rb1[NBL];
    const int n_it = 9 * (p.C >> 5);
    int nit = 0, ld_tap = 0, ld_c0 = 0;                // next weight step to load: its tap and chunk
    int xc0 = 0;                                       // next chunk of x to load

    auto load_x = [&]() {
#pragma unroll
        for (int k = 0; k < NXL; ++k)
            rx[k] = __builtin_bit_cast(float4, __builtin_amdgcn_raw_buffer_load_b128(rsA, x_voff[k], xc0 * 4, 0));
        xc0 += 32;
    };
    auto store_x = [&]() {
#pragma unroll
        for (int k = 0; k < NXL; ++k) {
            if ((tid >> 3) + 64 * k < XH * XW) {
                uint2 hi, lo;
                split4<TR>(rx[k], hi, lo);
                *reinterpret_cast<uint2*>(lds + x_lds0 + 64 * k * PITCH) = hi;
                *reinterpret_cast<uint2*>(lds + XPL + x_lds0 + 64 * k * PITCH) = lo;
            }
        }
    };
    auto load_w = [&](uint4 (&rb)[NBL]) {
        const int kbyte = (ld_tap * p.C + ld_c0) * 2;  // the scalar offset: an out-of-range row stays out of range
#pragma unroll
        for (int j = 0; j < NBL; ++j)
            rb[j] = __builtin_bit_cast(uint4, __builtin_amdgcn_raw_buffer_load_b128(
                                                  rsB, b_goff0 == OOB ? OOB : b_goff0 + j * b_plane, kbyte, 0));
        ++nit;
        if (++ld_tap == 9) {
            ld_tap = 0;
            ld_c0 += 32;
        }
    };
    auto store_w = [&](int buf, const uint4 (&rb)[NBL]) {
#pragma unroll
        for (int j = 0; j < NBL; ++j) *reinterpret_cast<uint4*>(wst + buf * WSTAGE + b_lds0 + j * B_BYTES) = rb[j];
    };

    f32x4 acc[TM][TN];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

    const int a_pix = wm * XW + li;                    // patch pixel of tap (0, 0), fragment 0; + 16 i + r XW + s
    const int b_off = (wn * WTN + li) * 64 + ((g ^ swz(li)) << 4);   // + 16 j rows (swz has period 16)
    auto compute = [&](int buf, int tap) {
        const int r = (tap * 11) >> 5, s = tap - 3 * r;
        const int px = a_pix + r * XW + s;             // (16 pixels on the XOR is the same: fragment i is 16 i PITCH further)
        const char* xa = lds + px * PITCH + ((g ^ (2 * ((px >> 2) & 1))) << 4);
        const char* wb = wst + buf * WSTAGE;
        V8 ah[TM], al[TM], bh[TN], bl[TN];
#pragma unroll
        for (int i = 0; i < TM; ++i) {
            ah[i] = *reinterpret_cast<const V8*>(xa + i * 16 * PITCH);
            al[i] = *reinterpret_cast<const V8*>(xa + XPL + i * 16 * PITCH);
        }
#pragma unroll
        for (int j = 0; j < TN; ++j) {
            bh[j] = *reinterpret_cast<const V8*>(wb + b_off + j * 16 * 64);
            bl[j] = *reinterpret_cast<const V8*>(wb + B_BYTES + b_off + j * 16 * 64);
        }
        __builtin_amdgcn_sched_barrier(0);
        split_sweep<TR, 3>(acc, ah, al, bh, bl);
    };

    int tp = 0;                                        // tap of the step being multiplied
    // after step `it` (tap tp) has been multiplied: stage step it + 1 into weight buffer `buf`, and its chunk if it opens one
    auto advance = [&](int buf, uint4 (&rb)[NBL], int it) {
        if (it + 1 < n_it) {
            if (tp == 8) {
                __syncthreads();                       // everyone has finished reading this chunk's patch
                store_x();
                if (xc0 < p.C) load_x();               // in flight while the chunk's nine taps are multiplied
            }
            store_w(buf, rb);
            if (nit < n_it) load_w(rb);
        }
        __syncthreads();
        tp = tp == 8 ? 0 : tp + 1;
    };

    load_x();                                          // chunk 0
    load_w(rb0);                                       // step 0
    store_x();
    store_w(0, rb0);
    if (xc0 < p.C) load_x();                           // chunk 1
    if (nit < n_it) load_w(rb0);                       // step 1
    if (nit < n_it) load_w(rb1);                       // step 2
    __syncthreads();
    // loop top (it even): weight buffer 0 = step it, rb0 = step it + 1, rb1 = step it + 2
    for (int it = 0; it < n_it; it += 2) {
        compute(0, tp);
        advance(1, rb0, it);
        if (it + 1 >= n_it) break;
        compute(1, tp);
        advance(0, rb1, it + 1);
    }

#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
            if (TR::OUTSCALE != 1.f) acc[i][j] *= TR::OUTSCALE;   // exact: undo the power-of-two operand scaling
    // a wave's rows are one image row: the second row of an odd height's last tile belongs to the next image (no statistics
    // here, so the epilogue has no barrier)
    if (y0 + wm < p.H) igemm_epilogue<BM, NB, WGM, WGN, 512, TM, TN>(p, acc, smem, m0, n0, wm, wn, li, g, tid);
}

}  // namespace acimg
