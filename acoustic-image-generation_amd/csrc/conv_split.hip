// Host side of the on-the-fly split 16-bit convolutions for gfx950 (MI355X): the tile choice (pick_split3), the
// conv_halo16_*_shape / conv_tap_ok predicates with the measurements that justify each route, fwd_split_onthefly /
// dgrad_split_onthefly behind acimg_conv2d_fwd_split3 / _bf16 and _dgrad_split3 / _bf16, the weight-preparation entries and the
// weight-byte queries.  Shared with the other families: conv_host.hpp.
// Kernel headers (their rule: conv_host.hpp) this file owns, and alone includes: igemm_split3_kernel.hpp (split 16-bit implicit
// GEMM on the fly; its 128x128 / 128x64 tiles are compiled in conv_tiles.hip: conv_tiles.hpp says why), conv_tap_kernel.hpp,
// conv_halo16_kernel.hpp (halo form of the 32- / 64-channel 3x3 forward conv and data gradient), split3_prepare_kernels.hpp.
#include "conv_host.hpp"
#include "conv_tiles.hpp"
#include "conv_tap_kernel.hpp"
#include "conv_halo16_kernel.hpp"
#include "split3_prepare_kernels.hpp"

namespace acimg {

// ---- f16x3 (split fp16) forward convolution (frozen ResNet trunk) ----
// Tile choice, measured per trunk conv shape at batch 32 (tools/tune_dma.py): the 8-wave 128x128 tile
// (2 workgroups/CU) wins on every shape with at least ~1 tile per CU; below that (the stride-2 3x3 conv into
// the 14x19 stage: 134 tiles) 64x128 fills more CUs; Cout = 64 uses 128x64.
Split3Cfg pick_split3(int M, int K, bool allow32) {
    if (K <= 32 && allow32) return {128, 32};     // on-the-fly kernel only (32-channel U-Net layers)
    if (K <= 64) return {128, 64};
    if (g_cfg.split3_tile_bm) {   // experiments only (acimg_configure validated the pair)
        return {g_cfg.split3_tile_bm, g_cfg.split3_tile_bn};
    }
    if ((long)cdiv(M, 128) * cdiv(K, 128) < 200) return {64, 128};
    return {128, 128};
}

// shapes the halo forward / data-gradient kernel takes: 3x3, stride 1, one pixel of padding, (reduction, output) channels
// (32 | 64, 32) forward and (32, 32 | 64) backward, from 65536 pixels on
static bool conv_halo16_dgrad_shape(const AcimgConvDesc* d) {
    return d->R == 3 && d->S == 3 && d->stride == 1 && d->pad_t == 1 && d->pad_l == 1 && d->OH == d->H && d->OW == d->W &&
           (d->C == 32 || d->C == 64) && d->K == 32 && (long)d->N * d->H * d->W >= 65536 && g_cfg.wgrad_halo;
}
bool conv_halo16_fwd_shape(const AcimgConvDesc* d) { return conv_halo16_dgrad_shape(d) && d->act == ACIMG_ACT_NONE; }

template <typename TR, int TERMS, int CIN, int NOUT, int MODE>
static int launch_conv_halo16(ConvHaloParams q, int N, hipStream_t st) {
    constexpr int TH = TERMS == 1 ? 8 : 4, NPL = TERMS == 3 ? 2 : 1;
    constexpr int lds = NPL * ((TH + 2) * 36 * (CIN * 2 + 16) + NOUT * (9 * CIN * 2 + 16));
    static_assert(lds <= 160 * 1024 && 8 * 2 * NOUT * 4 <= lds, "LDS budget");
    q.tiles_x = cdiv(q.W, 32); q.tiles_y = cdiv(q.H, TH);
    q.tiles = (long)N * q.tiles_x * q.tiles_y;
    if (!q.nout) q.nout = NOUT;
    static bool attr_set = false;
    if (!attr_set) {
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(conv_halo16_kernel<TR, TERMS, CIN, NOUT, MODE>),
                                  hipFuncAttributeMaxDynamicSharedMemorySize, lds);
        attr_set = true;
    }
    hipLaunchKernelGGL((conv_halo16_kernel<TR, TERMS, CIN, NOUT, MODE>), dim3(CONV_HALO16_WGS), dim3(512), lds, st, q);
    return check_launch("conv_halo16");
}

// the 16-row instance behind acimg_conv2d_dgrad (conv_f32.hip, which prepares wimg)
int launch_dgrad_halo16_narrow(const AcimgConvDesc* d, const float* gy, int ldgy, const void* wimg, float* dx, int lddx,
                               const float* residual, int ldres, const float* mask, int ldmask, hipStream_t st) {
    ConvHaloParams q{};
    q.X = gy; q.H = d->H; q.W = d->W; q.ldx = ldgy; q.Wimg = static_cast<const char*>(wimg); q.w_lo_off = 16 * 288 * 2;
    q.Y = dx; q.ldy = lddx; q.nout = d->C; q.res = residual; q.ldres = ldres; q.mask = mask; q.ldmask = ldmask;
    return launch_conv_halo16<SplitBF16, 3, 32, 16, 1>(q, d->N, st);
}

// Row-major planes [hi | lo][ldw][R*S*C], then (C % 32 == 0) the same weights once more in LDS-TILE ORDER: for every
// (128-column tile nt, K step q of 32) the two 8 KiB plane images exactly as the trunk kernels keep them in LDS
// (64-byte rows, logical chunk kc of row r at chunk kc ^ swz(r)), so a wave's LDS-DMA request for a weight piece is one
// contiguous KiB = eight whole 128-byte lines instead of sixteen 64-byte pieces of rows 2*R*S*C bytes apart.
size_t split3_rowmajor_bytes(const AcimgConvDesc* d) { return (size_t)2 * d->ldw * d->R * d->S * d->C * 2; }
static size_t split3_brick_bytes(const AcimgConvDesc* d) {
    return d->C % 32 ? 0 : (size_t)cdiv(d->ldw, 128) * (d->R * d->S * d->C / 32) * 2 * 8192;
}

template <typename TR, int TERMS = 3>
static int launch_split3(IgemmParams& p, hipStream_t st) {
    Split3Cfg c = pick_split3(p.M, p.Ngemm, true);
    dim3 grid(cdiv(p.M, c.bm), cdiv(p.Ngemm, c.bn), 1);
    if (c.bm == 128 && c.bn == 32)
        hipLaunchKernelGGL((igemm_split3_kernel<128, 32, 4, 1, 256, TR, TERMS>), grid, dim3(256), 2 * (2 * 128 * 64 + 2 * 32 * 64), st, p);
    else if (c.bm == 128 && c.bn == 128)
        hipLaunchKernelGGL((igemm_split3_kernel<128, 128, 2, 4, 512, TR, TERMS>), grid, dim3(512), 65536, st, p);
    else if (c.bm == 64 && c.bn == 128)
        hipLaunchKernelGGL((igemm_split3_kernel<64, 128, 1, 4, 256, TR, TERMS>), grid, dim3(256), 2 * (2 * 64 * 64 + 2 * 128 * 64), st, p);
    else if (c.bm == 128 && c.bn == 64)
        hipLaunchKernelGGL((igemm_split3_kernel<128, 64, 2, 2, 256, TR, TERMS>), grid, dim3(256), 2 * (2 * 128 * 64 + 2 * 64 * 64), st, p);
    else
        return fail(ACIMG_EINVAL, "split3: unsupported tile %dx%d", c.bm, c.bn);
    return check_launch("igemm_split3");
}

// the tap-sharing form of the on-the-fly split convs (conv_tap_kernel.hpp): 3x3 / stride 1 / SAME, image rows of 32 or 48 pixels
// (whole two-row tiles, the last of an odd height half empty), at least 64 reduction channels in whole 32-channel chunks, more than 32 output
// columns stored with 16-byte accesses, the three-term product, no input affine and no statistics.  Everything else (the
// one-term bf16 modes, in_scale / stats calls, the 12x16 layers, wide images) stays on igemm_split3_kernel.
// Measured per shape at batch 32 (profiles/conv_tap/, tools/op_report.py, three reports each, per-tap kernel -> this form, us):
// forward 128->128 87.1-88.4 -> 68.4-68.5 and 82.2-82.8 -> 67.0-68.4, 256->128 148.5-149.1 -> 123.0-123.3, 128->64 54.3-55.0 ->
// 48.8-49.2, 64->64 33.3-34.4 -> 29.4-30.5; data gradient 64->64 34.8-35.3 -> 31.5-32.4, 128->64 55.8-56.7 -> 48.0-50.4, 128->128
// 79.2-79.9 -> 64.8-65.1 and 86.5-87.5 -> 67.3-68.6, 256->128 145.2-146.6 -> 99.4-100.1: all ten beat the per-tap kernel's lowest
// by more than its spread (the narrowest: 64->64, 2.4 and 2.8 us against spreads of 0.5 and 1.1), so none is routed back.
static bool conv_tap_ok(const IgemmParams& p, int terms) {
    return terms == 3 && p.R == 3 && p.S == 3 && p.stride == 1 && p.pad_t == 1 && p.pad_l == 1 && p.OH == p.H && p.OW == p.W &&
           (p.W == 32 || p.W == 48) && p.C >= 64 && p.C % 32 == 0 && p.Ngemm > 32 && p.e.vec && (p.lda & 3) == 0 &&
           aligned16(p.A) && aligned16(p.B) && p.M % (p.H * p.W) == 0 && !p.a_scale && !p.e.stats && p.splits == 1 && g_cfg.wgrad_halo;
}
template <typename TR>
static int launch_conv_tap(const IgemmParams& p, hipStream_t st) {
    const dim3 grid(p.M / (p.H * p.W) * cdiv(p.H, CT_TH), cdiv(p.Ngemm, p.Ngemm <= 64 ? 64 : 128), 1);
#define ACIMG_CT(Wv, NBv) hipLaunchKernelGGL((conv_tap_kernel<TR, Wv, NBv>), grid, dim3(512), conv_tap_lds(Wv, NBv), st, p)
    if (p.W == 48) { if (p.Ngemm <= 64) ACIMG_CT(48, 64); else ACIMG_CT(48, 128); }
    else           { if (p.Ngemm <= 64) ACIMG_CT(32, 64); else ACIMG_CT(32, 128); }
#undef ACIMG_CT
    return check_launch("conv_tap");
}

// both operands are addressed through 32-bit buffer descriptors
static int split_extents(IgemmParams& p, long a_bytes, long b_bytes, const char* who) {
    if (a_bytes >= (1L << 31) || b_bytes >= (1L << 31)) return fail(ACIMG_EINVAL, "%s: operand >= 2 GiB", who);
    p.a_bytes = (unsigned)a_bytes; p.b_bytes = (unsigned)b_bytes;
    return ACIMG_OK;
}

static int fwd_split_onthefly(const AcimgConvDesc* d, const float* x, const void* wsplit, const float* bias, float* y,
                              const float* in_scale, const float* in_shift, int in_relu, float* stats, void* stream,
                              bool bf16) {
    int rc = check_desc(d, "conv2d_fwd_split3", true);
    if (rc) return rc;
    if (d->C % 32) return fail(ACIMG_EINVAL, "conv2d_fwd_split3: C=%d must be a multiple of 32", d->C);
    if (d->ldw < d->K) return fail(ACIMG_EINVAL, "conv2d_fwd_split3: ldw<K");
    if ((rc = check_wide("conv2d_fwd_split3", {{"x", x}, {"wsplit", wsplit}, {"in_scale", in_scale}, {"in_shift", in_shift}}))) return rc;
    if (conv_halo16_fwd_shape(d)) {
        // (acimg_conv2d_fwd_split3_stats_rows already told the caller this shape leaves CONV_HALO16_WGS rows: no fallback)
        if ((in_scale != nullptr) != (in_shift != nullptr) || (in_relu && !in_scale))
            return fail(ACIMG_EINVAL, "conv2d_fwd_split3: the halo form of this shape needs scale AND shift of an input affine");
        if ((rc = check_route("conv2d_fwd_split3", "halo-16 forward", {{"y", y, d->ldy}, {"bias", bias, 0}}))) return rc;
        ConvHaloParams q{};
        q.a_scale = in_scale; q.a_shift = in_shift; q.a_relu = in_relu;
        q.X = x; q.H = d->H; q.W = d->W; q.ldx = d->ldx; q.Wimg = static_cast<const char*>(wsplit);
        q.w_lo_off = (unsigned)((size_t)d->ldw * d->R * d->S * d->C * 2);
        q.Y = y; q.ldy = d->ldy; q.bias = bias; q.stats = stats; q.stats_ld = d->ldw;
        hipStream_t st = (hipStream_t)stream;
        if (bf16) return d->C == 64 ? launch_conv_halo16<SplitBF16, 1, 64, 32, 0>(q, d->N, st)
                                    : launch_conv_halo16<SplitBF16, 1, 32, 32, 0>(q, d->N, st);
        return d->C == 64 ? launch_conv_halo16<SplitF16, 3, 64, 32, 0>(q, d->N, st)
                          : launch_conv_halo16<SplitF16, 3, 32, 32, 0>(q, d->N, st);
    }
    IgemmParams p = fwd_view(d);
    split_ksteps(p);
    p.A = x; p.a_scale = in_scale; p.a_shift = in_shift; p.a_relu = in_relu;
    p.B = static_cast<const float*>(wsplit);
    rc = split_extents(p, (((long)d->N * d->H * d->W - 1) * d->ldx + d->C) * 4, (long)acimg_conv2d_split3_weight_bytes(d),
                       "conv2d_fwd_split3");
    if (rc) return rc;
    p.e.Y = y; p.e.bias = bias; p.e.stats = stats;
    epi_vec_flag(p.e);
    if (conv_tap_ok(p, bf16 ? 1 : 3)) return launch_conv_tap<SplitF16>(p, (hipStream_t)stream);
    if (bf16) return launch_split3<SplitBF16, 1>(p, (hipStream_t)stream);
    return launch_split3<SplitF16>(p, (hipStream_t)stream);
}

/* data gradient on the bf16x3 path (stride-1 convs): a forward conv of gy with the flipped/transposed kernel */
static int dgrad_split_onthefly(const AcimgConvDesc* d, const float* gy, int ldgy, const void* wsplit_t, float* dx,
                                int lddx, const float* residual, int ldres, const float* mask, int ldmask,
                                void* stream, int terms) {
    int rc = check_desc(d, "conv2d_dgrad_split3");
    if (rc) return rc;
    if (d->stride != 1 || d->K % 32 || d->K > ldgy)
        return fail(ACIMG_EINVAL, "conv2d_dgrad_split3: needs stride 1 and K %% 32 == 0 (K=%d) <= ldgy", d->K);
    if ((rc = check_wide_ld("conv2d_dgrad_split3", {{"ldgy", ldgy}})) ||
        (rc = check_wide("conv2d_dgrad_split3", {{"gy", gy}, {"wsplit_t", wsplit_t}})))
        return rc;
    if (lddx <= 0) lddx = d->ldx;
    if (lddx < d->C) return fail(ACIMG_EINVAL, "conv2d_dgrad_split3: lddx < C");
    if (conv_halo16_dgrad_shape(d) && aligned16(dx) && (lddx & 3) == 0 &&
        (!residual || (aligned16(residual) && (ldres & 3) == 0)) && (!mask || (aligned16(mask) && (ldmask & 3) == 0))) {
        // a forward SAME conv of gy (32 channels) with the flipped / transposed image: rows = the layer's input channels
        ConvHaloParams q{};
        q.X = gy; q.H = d->H; q.W = d->W; q.ldx = ldgy; q.Wimg = static_cast<const char*>(wsplit_t);
        q.w_lo_off = (unsigned)((size_t)d->C * d->R * d->S * d->K * 2);
        q.Y = dx; q.ldy = lddx; q.res = residual; q.ldres = ldres; q.mask = mask; q.ldmask = ldmask;
        hipStream_t st = (hipStream_t)stream;
        if (terms == 1) return d->C == 64 ? launch_conv_halo16<SplitBF16, 1, 32, 64, 1>(q, d->N, st)
                                          : launch_conv_halo16<SplitBF16, 1, 32, 32, 1>(q, d->N, st);
        return d->C == 64 ? launch_conv_halo16<SplitBF16, 3, 32, 64, 1>(q, d->N, st)
                          : launch_conv_halo16<SplitBF16, 3, 32, 32, 1>(q, d->N, st);
    }
    IgemmParams p = flipped_view(d, d->K, ldgy);
    split_ksteps(p);
    p.A = gy; p.B = static_cast<const float*>(wsplit_t); p.Nld = d->C;
    rc = split_extents(p, (((long)d->N * d->OH * d->OW - 1) * ldgy + d->K) * 4, (long)acimg_conv2d_split3_dgrad_weight_bytes(d),
                       "conv2d_dgrad_split3");
    if (rc) return rc;
    EpiParams& e = p.e;
    e.Y = dx; e.ldy = lddx; e.res = residual; e.ldres = ldres; e.mask = mask; e.ldmask = ldmask;
    epi_vec_flag(e);
    if (conv_tap_ok(p, terms)) return launch_conv_tap<SplitBF16>(p, (hipStream_t)stream);
    if (terms == 1) return launch_split3<SplitBF16, 1>(p, (hipStream_t)stream);
    return launch_split3<SplitBF16>(p, (hipStream_t)stream);
}

}  // namespace acimg

using namespace acimg;

extern "C" {      // ---- C ABI ----

int acimg_conv2d_fwd_split3_stats_rows(const AcimgConvDesc* d) {
    const int M = d->N * d->OH * d->OW;
    if (conv_halo16_fwd_shape(d)) return CONV_HALO16_WGS;      // the halo form leaves one row per workgroup
    return cdiv(M, pick_split3(M, d->K).bm);
}

size_t acimg_conv2d_split3_weight_bytes(const AcimgConvDesc* d) {
    return split3_rowmajor_bytes(d) + split3_brick_bytes(d);
}

int acimg_conv2d_split3_prepare(const AcimgConvDesc* d, const float* w, void* wsplit, void* stream) {
    int rc = check_desc(d, "conv2d_split3_prepare", true);
    if (rc || (rc = check_wide("conv2d_split3_prepare", {{"w", w}, {"wsplit", wsplit}}))) return rc;
    const int Ktot = d->R * d->S * d->C;
    hipLaunchKernelGGL((split3_prepare_kernel<SplitF16, false>), dim3(cdiv(Ktot, 32), cdiv(d->ldw, 32)), dim3(256), 0,
                       (hipStream_t)stream, w, d->R * d->S, d->C, d->K, d->ldw, d->ldw, static_cast<_Float16*>(wsplit));
    rc = check_launch("split3_prepare");
    if (rc || !split3_brick_bytes(d)) return rc;
    const long total = (long)(split3_brick_bytes(d) / 16);
    hipLaunchKernelGGL(split3_brick_kernel, dim3((unsigned)cdiv(total, 256L)), dim3(256), 0, (hipStream_t)stream,
                       static_cast<const char*>(wsplit), static_cast<char*>(wsplit) + split3_rowmajor_bytes(d), d->ldw, Ktot,
                       total);
    return check_launch("split3_prepare (tile order)");
}

int acimg_conv2d_bf16_prepare(const AcimgConvDesc* d, const float* w, void* wsplit, void* stream) {
    int rc = check_desc(d, "conv2d_bf16_prepare", true);
    if (rc || (rc = check_wide("conv2d_bf16_prepare", {{"w", w}, {"wsplit", wsplit}}))) return rc;
    const int Ktot = d->R * d->S * d->C;
    hipLaunchKernelGGL((split3_prepare_kernel<SplitBF16, false>), dim3(cdiv(Ktot, 32), cdiv(d->ldw, 32)), dim3(256), 0,
                       (hipStream_t)stream, w, d->R * d->S, d->C, d->K, d->ldw, d->ldw, static_cast<__bf16*>(wsplit));
    return check_launch("conv2d_bf16_prepare");
}

size_t acimg_conv2d_split3_dgrad_weight_bytes(const AcimgConvDesc* d) {
    return (size_t)2 * d->C * d->R * d->S * up4(d->K) * 2;
}

int acimg_conv2d_split3_prepare_dgrad(const AcimgConvDesc* d, const float* w, void* wsplit, void* stream) {
    int rc = check_desc(d, "conv2d_split3_prepare_dgrad");
    if (rc || (rc = check_wide("conv2d_split3_prepare_dgrad", {{"w", w}, {"wsplit", wsplit}}))) return rc;
    if (d->K % 32 || d->K > d->ldw) return fail(ACIMG_EINVAL, "conv2d_split3_prepare_dgrad: K must be a multiple of 32");
    const int Ktot = d->R * d->S * d->K;
    hipLaunchKernelGGL((split3_prepare_kernel<SplitBF16, true>), dim3(cdiv(Ktot, 32), cdiv(d->C, 32)), dim3(256), 0,
                       (hipStream_t)stream, w, d->R * d->S, d->C, d->K, d->ldw, d->C, static_cast<__bf16*>(wsplit));
    return check_launch("split3_prepare_dgrad");
}

/* all of a model's trainable kernels in one launch: mode[i] = 0 forward image (acimg_conv2d_split3_prepare), 1 data-
 * gradient image (acimg_conv2d_split3_prepare_dgrad), 2 forward bf16 image (acimg_conv2d_bf16_prepare) */
int acimg_conv2d_split3_prepare_multi(int n, const AcimgConvDesc* const* descs, const float* const* w, void* const* out,
                                      const int* mode, void* stream) {
    if (n == 0) return ACIMG_OK;
    if (n < 0 || n > 16 || !descs || !w || !out || !mode)
        return fail(ACIMG_EINVAL, "conv2d_split3_prepare_multi: need 0..16 jobs and non-null tables");
    PrepJobs jobs{};
    jobs.n = n;
    int blocks = 0;
    for (int i = 0; i < n; ++i) {
        const AcimgConvDesc* d = descs[i];
        int rc = check_desc(d, "conv2d_split3_prepare_multi", true);
        if (rc) return rc;
        if (!w[i] || !out[i]) return fail(ACIMG_EINVAL, "conv2d_split3_prepare_multi: null pointer in job %d", i);
        if ((rc = check_wide("conv2d_split3_prepare_multi", {{"w", w[i]}, {"wsplit", out[i]}}))) return rc;
        PrepJob& J = jobs.j[i];
        J.w = w[i]; J.out = out[i]; J.ntaps = d->R * d->S; J.C = d->C; J.K = d->K; J.ldw = d->ldw;
        if (mode[i] < 0 || mode[i] > 2) return fail(ACIMG_EINVAL, "conv2d_split3_prepare_multi: job %d: mode is 0, 1 or 2", i);
        J.dgrad = mode[i];
        int tiles_n;
        if (J.dgrad == 1) {
            if (d->K % 32 || d->K > d->ldw)
                return fail(ACIMG_EINVAL, "conv2d_split3_prepare_multi: job %d: K must be a multiple of 32", i);
            J.Nrows = d->C;
            J.tiles_k = cdiv(d->R * d->S * d->K, 32);
            tiles_n = cdiv(d->C, 32);
        } else {
            J.Nrows = d->ldw;
            J.tiles_k = cdiv(d->R * d->S * d->C, 32);
            tiles_n = cdiv(d->ldw, 32);
        }
        J.block0 = blocks;
        blocks += J.tiles_k * tiles_n;
    }
    hipLaunchKernelGGL(split3_prepare_multi_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, jobs);
    return check_launch("split3_prepare_multi");
}

int acimg_conv2d_fwd_split3(const AcimgConvDesc* d, const float* x, const void* wsplit, const float* bias,
                            float* y, const float* in_scale, const float* in_shift, int in_relu, float* stats,
                            void* stream) {
    return fwd_split_onthefly(d, x, wsplit, bias, y, in_scale, in_shift, in_relu, stats, stream, false);
}

/* bf16 operands (activations and weights rounded to bf16, one MFMA per product, fp32 accumulation); weights from
 * acimg_conv2d_bf16_prepare */
int acimg_conv2d_fwd_bf16(const AcimgConvDesc* d, const float* x, const void* wsplit, const float* bias,
                          float* y, const float* in_scale, const float* in_shift, int in_relu, float* stats,
                          void* stream) {
    return fwd_split_onthefly(d, x, wsplit, bias, y, in_scale, in_shift, in_relu, stats, stream, true);
}

int acimg_conv2d_dgrad_split3(const AcimgConvDesc* d, const float* gy, int ldgy, const void* wsplit_t, float* dx,
                              int lddx, const float* residual, int ldres, const float* mask, int ldmask,
                              void* stream) {
    return dgrad_split_onthefly(d, gy, ldgy, wsplit_t, dx, lddx, residual, ldres, mask, ldmask, stream, 3);
}

/* the same with gy and the kernel rounded to bf16, one MFMA per product (weights: acimg_conv2d_split3_prepare_dgrad) */
int acimg_conv2d_dgrad_bf16(const AcimgConvDesc* d, const float* gy, int ldgy, const void* wsplit_t, float* dx,
                            int lddx, const float* residual, int ldres, const float* mask, int ldmask,
                            void* stream) {
    return dgrad_split_onthefly(d, gy, ldgy, wsplit_t, dx, lddx, residual, ldres, mask, ldmask, stream, 1);
}

}  // extern "C"
