// Host side of the convolutions for gfx950 (MI355X): this file decides which kernel a call runs and launches it.  It holds
// the tuning record (g_cfg), the *_shape / *_ok predicates with the measurements that justify each route, the workspace
// formulas, the kernel selections (pick_*, TrunkVariant), every launch_* / dispatch_*, and the C entry points.  The device
// code lives in one header per kernel family (kernels, their parameter structs, tile constants and design notes; no launch,
// no predicate that reads g_cfg, no entry point):
//   igemm_kernel.hpp          exact-f32 implicit GEMM (forward, data gradient, patch scatter) and its epilogue
//   wgrad_f32_kernel.hpp      exact-f32 weight gradient; the slab reducers of every split weight gradient
//   wgrad_halo_kernel.hpp     halo weight gradients: exact f32 (few channels) and bf16 / bf16x3 (<= 64 -> <= 32 channels)
//   direct_conv_kernel.hpp    direct few-channel conv
//   conv_few16_kernel.hpp     few-channel 3x3 conv on split 16-bit MFMAs
//   patch2_kernel.hpp         2x2 / stride-2 transposed conv 32 -> 8: forward / data gradient, weight gradient
//   conv_halo16_kernel.hpp    halo form of the 32- / 64-channel 3x3 forward conv and data gradient
//   conv_aux_kernels.hpp      split-K reduce, sub-pixel weights, tap-GEMM helpers, column sums, statistics, fills, bricks
//   igemm_split3*_kernel.hpp  split 16-bit implicit GEMM: on the fly (split3) and the pre-split trunk kernels (d, dp, r, h)
//   wgrad_split3_kernel.hpp, wgrad_tap_kernel.hpp, conv_tap_kernel.hpp, skinny_kernel.hpp
#include "wgrad_split3_kernel.hpp"
#include "wgrad_tap_kernel.hpp"
#include "conv_tap_kernel.hpp"
#include "igemm_split3d_kernel.hpp"
#include "igemm_split3dp_kernel.hpp"
#include "igemm_split3r_kernel.hpp"
#include "igemm_split3h_kernel.hpp"
#include "skinny_kernel.hpp"
#include "wgrad_f32_kernel.hpp"
#include "wgrad_halo_kernel.hpp"
#include "direct_conv_kernel.hpp"
#include "conv_few16_kernel.hpp"
#include "patch2_kernel.hpp"
#include "conv_halo16_kernel.hpp"
#include "conv_aux_kernels.hpp"
#include <cstdlib>
#include <algorithm>
#include <type_traits>

namespace acimg {

// slab [splits][rows][ld] -> out [rows][ld] (ncols of them); optionally slab2 [splits][ld] -> out2 [ncols] (bias gradient)
static void launch_slab_reduce_wide(const float* slab, int splits, long rows, int ncols, int ld, float* out, const float* slab2,
                                    float* out2, hipStream_t st) {
    const long total = rows * ncols;
    if (total <= 4096) {
        const int nb1 = (int)cdiv(total, 8), nb2 = out2 ? cdiv(ncols, 8) : 0;
        hipLaunchKernelGGL(slab_reduce_wide_kernel<8>, dim3(nb1 + nb2), dim3(256), 0, st, slab, splits, rows, ncols, ld, out, nb1,
                           slab2, out2);
    } else {
        const int nb1 = (int)cdiv(total, 32), nb2 = out2 ? cdiv(ncols, 32) : 0;
        hipLaunchKernelGGL(slab_reduce_wide_kernel<32>, dim3(nb1 + nb2), dim3(256), 0, st, slab, splits, rows, ncols, ld, out, nb1,
                           slab2, out2);
    }
}

// ------------------------------------------------------------------------------------------
// host side: configuration choice and launch
// ------------------------------------------------------------------------------------------
struct TileCfg {
    int bm, bn;
};

static TileCfg pick_cfg(int M, int Ngemm) {
    if (Ngemm <= 16) return {256, 16};
    if (Ngemm <= 64) return {128, 64};
    const long tiles128 = (long)cdiv(M, 128) * cdiv(Ngemm, 128);
    if (tiles128 < 192) return {64, 64};
    return {128, 128};
}

// Tuning record (acimg_configure): plain ints, defaults compiled in, written only by acimg_configure and never by a
// launch; the launch heuristics below read it instead of the process environment.
static constexpr AcimgConfig DEFAULT_CFG = {320, 768, 1, 128, 1, 0, 0, 1, 0, 1, 0, 0, 0, 1, 0, 0};     // acimg_config_default
static AcimgConfig g_cfg = DEFAULT_CFG;

static int pick_splits(int M, int Ngemm, TileCfg c, int kiters) {
    // measured on the generator's 12x16 layers (192-288 tiles of 64x64, 36+ K steps: tools/splitk_sweep.sh):
    // below ~1.25 workgroups per CU a K split towards ~3 per CU pays for its reduce pass
    const int cut = g_cfg.splitk_cut, target = g_cfg.splitk_target;
    const long tiles = (long)cdiv(M, c.bm) * cdiv(Ngemm, c.bn);
    if (tiles >= cut || kiters < 8) return 1;
    long s = (target + tiles - 1) / tiles;
    if (s > kiters / 4) s = kiters / 4;
    if (s > 64) s = 64;
    if (s < 1) s = 1;
    return (int)s;
}

static size_t igemm_ws_bytes(int M, int Ngemm, int kiters) {
    TileCfg c = pick_cfg(M, Ngemm);
    int s = pick_splits(M, Ngemm, c, kiters);
    if (s <= 1) return 0;
    const int ld = (Ngemm + 3) & ~3;
    const size_t rows = (size_t)s * M * ld * sizeof(float);                                   // reduce-launch layout
    const size_t tiled = (size_t)s * cdiv(M, c.bm) * cdiv(Ngemm, c.bn) * c.bm * c.bn * sizeof(float);   // hand-off layout
    return rows > tiled ? rows : tiled;
}

template <int BM, int BN, int WGM, int WGN, int NTHR>
static void launch_cfg(const IgemmParams& p, bool nt, bool cal, dim3 grid, hipStream_t st) {
    constexpr int BK = 32;
    constexpr int a_elems = BM * (BK + 4);
    constexpr int bnt = BN * (BK + 4), bnn = BK * (BN + 4);
    const int stage = a_elems + (nt ? bnt : bnn);
    const int stat_elems = WGM * 2 * BN;
    const int elems = 2 * stage > stat_elems ? 2 * stage : stat_elems;
    const size_t shm = (size_t)elems * sizeof(float);
    if (nt) {
        if (cal) hipLaunchKernelGGL((igemm_f32_kernel<BM, BN, WGM, WGN, NTHR, true, true>), grid, dim3(NTHR), shm, st, p);
        else hipLaunchKernelGGL((igemm_f32_kernel<BM, BN, WGM, WGN, NTHR, true, false>), grid, dim3(NTHR), shm, st, p);
    } else {
        if (cal) hipLaunchKernelGGL((igemm_f32_kernel<BM, BN, WGM, WGN, NTHR, false, true>), grid, dim3(NTHR), shm, st, p);
        else hipLaunchKernelGGL((igemm_f32_kernel<BM, BN, WGM, WGN, NTHR, false, false>), grid, dim3(NTHR), shm, st, p);
    }
}

// 16-byte epilogue accesses: every operand the epilogue touches allows them
static void epi_vec_flag(EpiParams& e) {
    e.vec = aligned16(e.Y) && (e.ldy & 3) == 0 && (!e.bias || aligned16(e.bias)) &&
            (!e.res || (aligned16(e.res) && (e.ldres & 3) == 0)) &&
            (!e.mask || (aligned16(e.mask) && (e.ldmask & 3) == 0)) && (!e.scatter || (e.Ko & 3) == 0);
}

// ---- descriptor -> implicit-GEMM views: the geometry fields of IgemmParams; operands, row runs and epilogue extras are the
// caller's ----
// forward conv: rows = output pixels, K = (tap, input channel), columns = output channels
static IgemmParams fwd_view(const AcimgConvDesc* d) {
    IgemmParams p{};
    p.H = d->H; p.W = d->W; p.C = d->C; p.lda = d->ldx;
    p.OH = d->OH; p.OW = d->OW; p.R = d->R; p.S = d->S; p.stride = d->stride;
    p.pad_t = d->pad_t; p.pad_l = d->pad_l;
    p.M = d->N * d->OH * d->OW;
    p.Nld = d->ldw; p.Ngemm = d->K;
    p.e.ldy = d->ldy; p.e.M = p.M; p.e.Nstore = d->K; p.e.act = d->act; p.e.stats_ld = d->ldw;
    return p;
}
// data gradient of a stride-1 conv: a forward conv of gy (ca channels, pixel stride ldgy) with the flipped kernel,
//   dx[h,w,c] = sum_{r',s',k} gy[h-(R-1-pt)+r', w-(S-1-pl)+s', k] * W[R-1-r'][S-1-s'][c][k]
// (gy: [N][GH][GW] pixels of ca channels; dx: [N][H][W] pixels of `cols` channels; pad_t / pad_l: the conv's own padding)
static IgemmParams flipped_view(int N, int GH, int GW, int ca, int ldgy, int H, int W, int R, int S, int pad_t, int pad_l,
                                int cols) {
    IgemmParams p{};
    p.H = GH; p.W = GW; p.C = ca; p.lda = ldgy;
    p.OH = H; p.OW = W; p.R = R; p.S = S; p.stride = 1;
    p.pad_t = R - 1 - pad_t; p.pad_l = S - 1 - pad_l;
    p.M = N * H * W;
    p.Ngemm = cols;
    p.e.M = p.M; p.e.Nstore = cols; p.e.act = ACIMG_ACT_NONE;
    return p;
}
static IgemmParams flipped_view(const AcimgConvDesc* d, int ca, int ldgy) {
    return flipped_view(d->N, d->OH, d->OW, ca, ldgy, d->H, d->W, d->R, d->S, d->pad_t, d->pad_l, d->C);
}
// the 16-bit MFMA kernels walk K as (tap, 32-channel chunk) in one pass
static void split_ksteps(IgemmParams& p) {
    p.ntaps = p.R * p.S;
    p.kiters = p.ntaps * (p.C / 32);
    p.splits = 1;
}

// tickets: ACIMG_TICKET_WORDS zeroed ints owned by the caller (or nullptr: split-K combines through a reduce launch)
static int launch_igemm(IgemmParams p, bool nt, void* ws, size_t ws_bytes, void* tickets, hipStream_t st) {
    if (p.M <= 0 || p.Ngemm <= 0) return fail(ACIMG_EINVAL, "igemm: empty problem");
    if ((p.C & 3) || (p.lda & 3) || (p.ldb & 3))
        return fail(ACIMG_EINVAL, "igemm: C=%d lda=%d ldb=%d must be multiples of 4", p.C, p.lda, p.ldb);
    if (!aligned16(p.A) || !aligned16(p.B)) return fail(ACIMG_EINVAL, "igemm: operands must be 16-byte aligned");
    const int nseg = p.rowrun ? p.R : p.R * p.S;
    p.L = p.rowrun ? p.S * p.C : p.C;
    p.cps = cdiv(p.L, 32);
    p.kiters = nseg * p.cps;
    p.ntaps = p.R * p.S;
    const bool cal = (p.C % 32) == 0;
    // buffer descriptors: extents of A (gathered NHWC tensor) and B
    const long nimg = p.M / ((long)p.OH * p.OW);
    const long a_bytes = ((nimg * p.H * p.W - 1) * p.lda + p.C) * 4;
    const long b_bytes = nt ? (((long)(p.ntaps - 1) * p.tap_stride + (long)(p.Ngemm - 1) * p.ldb + p.C) * 4)
                            : ((long)p.R * p.S * p.C * p.ldb * 4);
    if (a_bytes >= (1L << 31) || b_bytes >= (1L << 31) || a_bytes <= 0 || b_bytes <= 0)
        return fail(ACIMG_EINVAL, "igemm: operand extent %ld / %ld bytes outside (0, 2 GiB)", a_bytes, b_bytes);
    p.a_bytes = (unsigned)a_bytes;
    p.b_bytes = (unsigned)b_bytes;
    EpiParams& e = p.e;
    epi_vec_flag(e);
    TileCfg c = pick_cfg(p.M, p.Ngemm);
    p.splits = pick_splits(p.M, p.Ngemm, c, p.kiters);
    float* stats_after = nullptr;  // split-K + BN statistics: a small pass over y afterwards
    if (e.stats && p.splits > 1) {
        // (a bias is fine: the statistics pass reads y = acc + bias, which is what the batch norm normalises)
        if (e.scatter || e.res || e.mask || e.act != ACIMG_ACT_NONE)
            return fail(ACIMG_EINVAL, "igemm: statistics with split-K need a raw (conv + bias) output");
        stats_after = e.stats;
        e.stats = nullptr;
    }
    p.slab = nullptr;
    p.slab_ld = (p.Ngemm + 3) & ~3;
    p.ts_counters = nullptr;
    dim3 grid(cdiv(p.M, c.bm), cdiv(p.Ngemm, c.bn), p.splits);
    if (p.splits > 1) {
        size_t need = (size_t)p.splits * p.M * p.slab_ld * sizeof(float);
        const size_t tiles = (size_t)grid.x * grid.y;
        if (tickets && (reinterpret_cast<uintptr_t>(tickets) & 15))
            return fail(ACIMG_EINVAL, "igemm: ticket words must be 16-byte aligned");
        const bool handoff = tickets != nullptr && tiles <= ACIMG_TICKET_WORDS && g_cfg.splitk_handoff;
        if (handoff) need = (size_t)p.splits * tiles * c.bm * c.bn * sizeof(float);
        if (ws == nullptr || ws_bytes < need)
            return fail(ACIMG_EWORKSPACE, "igemm: workspace %zu < %zu", ws_bytes, need);
        p.slab = static_cast<float*>(ws);
        if (handoff) p.ts_counters = static_cast<int*>(tickets);
    }
    if (c.bm == 128 && c.bn == 128) launch_cfg<128, 128, 2, 4, 512>(p, nt, cal, grid, st);
    else if (c.bm == 128 && c.bn == 64) launch_cfg<128, 64, 2, 2, 256>(p, nt, cal, grid, st);
    else if (c.bm == 64 && c.bn == 64) launch_cfg<64, 64, 2, 2, 256>(p, nt, cal, grid, st);
    else launch_cfg<256, 16, 4, 1, 256>(p, nt, cal, grid, st);
    int rc = check_launch("igemm");
    if (rc) return rc;
    if (p.splits > 1) {
        if (p.ts_counters == nullptr) {
            const long total = (long)p.M * p.Ngemm;
            hipLaunchKernelGGL(igemm_splitk_reduce_kernel, dim3(cdiv(total, 256)), dim3(256), 0, st,
                               p.slab, p.splits, p.M, p.Ngemm, p.slab_ld, p.e);
            rc = check_launch("igemm_splitk_reduce");
        }
        if (!rc && stats_after) {
            hipLaunchKernelGGL(partial_stats_kernel, dim3(cdiv(p.M, 256)), dim3(256), 0, st, e.Y, e.ldy, p.M,
                               e.Nstore, stats_after, e.stats_ld, 256);
            rc = check_launch("partial_stats");
        }
    }
    return rc;
}

static int pick_wgrad_splits(int M, int KK, int Ngemm, int bmo, int bn) {
    const long tiles = (long)cdiv(KK, bmo) * cdiv(Ngemm, bn);
    long s = (512 + tiles - 1) / tiles;   // ~2 workgroups per CU; every split costs a KK x N slab round trip
    const int minpix = g_cfg.wgrad_minpix;
    const long maxs = (M + minpix - 1) / minpix;  // at least `minpix` pixels per split
    long cap = 128;
    if ((long)KK * Ngemm <= 8192) {       // few-channel layers (the RGB / spectrogram U-Nets: 72 x 8 ... 288 x 32
        s = (2048 + tiles - 1) / tiles;   // weights, millions of pixels): slabs are a few KB, the pixel stream is
        cap = 2048;                       // everything -> ~8 workgroups per CU
    }
    if (s > maxs) s = maxs;
    if (s > cap) s = cap;
    if (s < 1) s = 1;
    return (int)s;
}
static void wgrad_tile(int Ngemm, int& bmo, int& bn) {
    bmo = 128;
    bn = Ngemm <= 16 ? 16 : (Ngemm <= 32 ? 32 : (Ngemm <= 64 ? 64 : 128));
    // column counts just above a multiple of 128 (the generator's 133- and 144-column layers): 64-column tiles
    // cover them with fewer padded columns (136 -> 192 instead of 256)
    if (Ngemm > 64 && cdiv(Ngemm, 64) * 64 < cdiv(Ngemm, 128) * 128) bn = 64;
}
static int wgrad_split3_bn(int Ngemm) {      // column tile of the split-MFMA weight-gradient kernel
    return Ngemm > 64 ? 128 : (Ngemm > 32 ? 64 : 32);   // (64-column tiles for 144 columns: measured equal / slower)
}
// the part of wgrad_halo16_ok (below) that the sizing query knows: 3x3 taps of at most 64 channels into at
// most 32 columns, from 65536 pixels on
static bool wgrad_halo16_shape(long M, int KK, int Ngemm) { return Ngemm <= 32 && KK % 9 == 0 && KK <= 9 * 64 && M >= 65536; }
// the part of wgrad_tap_ok (below) that depends on the shape alone: 3x3 taps of at least 64 channels into more than 32 columns
// (wgrad_tap_kernel; it asks for no more slabs than pick_wgrad_splits grants, so the sizing query does not look at it)
static bool wgrad_tap_shape(int KK, int Ngemm) { return KK % 9 == 0 && KK >= 9 * 64 && Ngemm > 32; }
static size_t wgrad_ws_bytes(int M, int KK, int Ngemm, int ldo) {
    // one sizing query serves acimg_conv2d_wgrad and acimg_conv2d_wgrad_split3 / _bf16: the larger of their slab counts
    int bmo, bn;
    wgrad_tile(Ngemm, bmo, bn);
    int s = std::max(pick_wgrad_splits(M, KK, Ngemm, bmo, bn), pick_wgrad_splits(M, KK, Ngemm, bmo, wgrad_split3_bn(Ngemm)));
    // the halo form of the 3x3 32- / 64-channel -> 32-column layers (wgrad_halo16_kernel) leaves one slab per CU
    if (wgrad_halo16_shape(M, KK, Ngemm) && s < (KK <= 9 * 16 ? 512 : 256)) s = KK <= 9 * 16 ? 512 : 256;
    // (s + 1: one slab more than any launch below asks for - each needs splits x (KK + 1) rows, bias row included.  The guard-
    // band tests of every workspace pass without it; it stays because callers size their buffers by this answer)
    return s > 1 ? (size_t)(s + 1) * ((size_t)KK + 1) * ldo * sizeof(float) : 0;
}

// the exact-f32 halo form (wgrad_halo_kernel): 4 / 8 / 16 input channels into at most 16 columns, from 65536 pixels on
static bool wgrad_halo_ok(const WgradParams& p) {
    return (p.C == 4 || p.C == 8 || p.C == 16) && p.Nld <= 16 && p.Ngemm == p.Nld && p.stride == 1 && p.R <= 3 && p.S <= 3 && (long)p.M >= 65536 && (p.ldx & 3) == 0 && (p.ldg & 3) == 0 &&
           (p.KK + 1 + 15) / 16 <= WH_MAXT && wgrad_halo_lds(p.R, p.S, p.C, p.Nld, p.stride) <= 65536 &&
           g_cfg.wgrad_halo;
}

// split3: the caller asked for 16-bit matrix-core arithmetic (acimg_conv2d_wgrad_split3 / _bf16).  The FEW-CHANNEL layers
// (fewer than 32 input channels: the full-resolution layers of the RGB / spectrogram U-Nets, which arrive through the fp32
// entry acimg_conv2d_wgrad) take the same kernel in its three-term form - fp32-class results (5e-6) - on a zero-padded
// 32 x 32 channel tile: 224x298 16->8 189 -> ~60 us against the exact-f32 halo kernel (round 4)
static bool wgrad_halo16_ok(const WgradParams& p, bool split3) {
    const bool few = p.C < 32;
    return wgrad_halo16_shape(p.M, p.KK, p.Ngemm) && (split3 || few) && p.R == 3 && p.S == 3 && p.stride == 1 && p.pad_t == 1 &&
           p.pad_l == 1 && (p.C == 64 || (p.C <= 32 && p.C % 4 == 0)) && p.Ngemm % 4 == 0 && p.Nld == p.Ngemm && p.OH == p.H &&
           p.OW == p.W && p.ldo >= p.Ngemm && g_cfg.wgrad_halo;
}

// the tap-sharing form of the bf16x3 weight gradient (wgrad_tap_kernel.hpp): 3x3 / stride 1 / SAME, image rows of 32 or 48
// pixels (a multiple of 16 keeps a fragment's two 8-pixel groups in one row; 16-pixel rows are the latency-bound 12x16 layers,
// left on the per-tap kernel), no input affine.  Measured per shape at batch 32 (profiles/wgrad_tap/, tools/op_report.py, per-tap
// kernel -> this form): 36x48 256->128 181.3-183.8 -> 122.3 us, 128->128 110.6-112.6 -> 74.2, 128->64 80.8-81.3 -> 50.1, 64->64
// 35.1-35.5 -> 33.4: all four beat the per-tap kernel by more than its spread over three reports, so all four ship here
static bool wgrad_tap_ok(const WgradParams& p) {
    return wgrad_tap_shape(p.KK, p.Ngemm) && p.R == 3 && p.S == 3 && p.stride == 1 && p.pad_t == 1 && p.pad_l == 1 &&
           p.OH == p.H && p.OW == p.W && p.W % 16 == 0 && p.W >= 32 && p.W <= WT_MAXW && p.KK == 9 * p.C && p.Nld == p.Ngemm &&
           p.Ngemm % 4 == 0 && p.ldo >= p.Ngemm && p.M % (p.H * p.W) == 0 && !p.a_scale && g_cfg.wgrad_halo;
}

// The partial slabs of a split weight gradient in the caller's workspace: n slabs [KK][ldo], then the n bias rows [ldo].  The
// kernel is handed the bias rows (db_out) only when a bias gradient was asked for; fits: the workspace holds all of it.
struct WgradSlabs {
    size_t need;
    bool fits;
    float *out, *db_rows, *db_out;
};
static WgradSlabs wgrad_slabs(const WgradParams& p, int n, const float* db, void* ws, size_t ws_bytes) {
    WgradSlabs s{};
    s.need = (size_t)n * ((size_t)p.KK + 1) * p.ldo * sizeof(float);
    s.fits = ws != nullptr && ws_bytes >= s.need;
    if (s.fits) {
        s.out = static_cast<float*>(ws);
        s.db_rows = s.out + (size_t)n * p.KK * p.ldo;
        s.db_out = db ? s.db_rows : nullptr;
    }
    return s;
}
static int wgrad_ws_short(const WgradSlabs& s, size_t ws_bytes) {
    return fail(ACIMG_EWORKSPACE, "wgrad: workspace %zu < %zu", ws_bytes, s.need);
}
// sums the n slabs into dw and the bias rows into db, in slab order: the wide kernel above 32 slabs, and always for the
// halo forms (wide: one slab per workgroup, hundreds of them)
static int wgrad_reduce(const WgradSlabs& s, int n, const WgradParams& p, float* dw, float* db, bool wide, hipStream_t st) {
    if (wide || n > 32) {
        launch_slab_reduce_wide(s.out, n, (long)p.KK, p.Ngemm, p.ldo, dw, s.db_out, db, st);
    } else {
        const long total = (long)p.KK * p.Ngemm;
        const int nb1 = (int)cdiv(total, 256), nb2 = db ? cdiv(p.Ngemm, 256) : 0;
        hipLaunchKernelGGL(slab_reduce_kernel, dim3(nb1 + nb2), dim3(256), 0, st, s.out, n, (long)p.KK, p.Ngemm, p.ldo, dw, nb1,
                           s.db_rows, db);
    }
    return check_launch("wgrad_reduce");
}

// db (optional): fused bias gradient, db[n] = sum_m G[m][n] for n < Ngemm
static int launch_wgrad(WgradParams p, float* dw, float* db, void* ws, size_t ws_bytes, hipStream_t st,
                        bool split3 = false, int terms = 3) {
    if ((p.C & 3) || (p.ldx & 3) || (p.ldg & 3) || (p.ldo & 3))
        return fail(ACIMG_EINVAL, "wgrad: C=%d ldx=%d ldg=%d ldo=%d must be multiples of 4", p.C, p.ldx, p.ldg, p.ldo);
    if (!aligned16(p.X) || !aligned16(p.G) || !aligned16(dw))
        return fail(ACIMG_EINVAL, "wgrad: operands must be 16-byte aligned");
    if (p.a_scale && !wgrad_halo16_ok(p, split3))
        return fail(ACIMG_EINVAL, "wgrad: an input affine is only taken by the halo form (3x3 / stride 1 / SAME, <= 32 columns, >= 65536 pixels)");
    if (p.a_scale && (!p.a_shift || !aligned16(p.a_scale) || !aligned16(p.a_shift)))
        return fail(ACIMG_EINVAL, "wgrad: the input affine needs scale and shift, 16-byte aligned");
    int bmo, bn;
    wgrad_tile(p.Ngemm, bmo, bn);
    if (wgrad_halo16_ok(p, split3)) {
        WgradHalo16Params q{};
        q.X = p.X; q.H = p.H; q.W = p.W; q.ldx = p.ldx; q.G = p.G; q.ldg = p.ldg; q.ldo = p.ldo;
        q.creal = p.C; q.nreal = p.Ngemm;
        q.a_scale = p.a_scale; q.a_shift = p.a_shift; q.a_relu = p.a_relu;
        if (p.C < 32) terms = 3;                                       // few-channel layers: always the fp32-class form
        const int cpad = p.C == 64 ? 64 : (p.C > 16 ? 32 : 16);
        const int nnt = (cpad == 16 && p.Ngemm <= 16) ? 1 : 2;
        const int th = (terms == 1 || cpad == 16) ? 8 : 4;
        q.tiles_x = cdiv(p.W, 32); q.tiles_y = cdiv(p.H, th);
        q.tiles = (long)(p.M / (p.H * p.W)) * q.tiles_x * q.tiles_y;
        int nb = p.C <= 16 ? 512 : 256;     // one workgroup per CU; two for the few-channel instances (56 KiB of LDS, tiny slabs:
        if (nb > q.tiles) nb = (int)q.tiles;       // their load / store / multiply phases overlap across workgroups)
        const WgradSlabs sl = wgrad_slabs(p, nb, db, ws, ws_bytes);
        if (sl.fits) {      // (the sizing query covers it: pick_wgrad_splits gives these shapes >= 256 slabs)
            q.out = sl.out;
            q.db_out = sl.db_out;
            const int xh = th + 2, planes = terms == 3 ? 2 : 1;
            int lds = planes * (xh * 36 * cpad * 2 + th * 32 * 64);
            if (lds < 4 * 10 * 64 * 16) lds = 4 * 10 * 64 * 16;                   // the row groups' final sums through LDS
#define ACIMG_WH16(Cv, Tv)                                                                                              \
    do {                                                                                                                \
        static bool attr_set = false;                                                                                   \
        if (!attr_set) {                                                                                                \
            (void)hipFuncSetAttribute(reinterpret_cast<const void*>(wgrad_halo16_kernel<Cv, Tv>),                       \
                                      hipFuncAttributeMaxDynamicSharedMemorySize, 2 * (10 * 36 * 64 * 2 + 8 * 32 * 64)); \
            attr_set = true;                                                                                            \
        }                                                                                                               \
        hipLaunchKernelGGL((wgrad_halo16_kernel<Cv, Tv>), dim3(nb), dim3(512), lds, st, q);                             \
    } while (0)
            if (cpad == 64 && terms == 1) ACIMG_WH16(64, 1);
            else if (cpad == 64) ACIMG_WH16(64, 3);
            else if (cpad == 32 && terms == 1) ACIMG_WH16(32, 1);
            else if (cpad == 32) ACIMG_WH16(32, 3);
            else if (nnt == 2) ACIMG_WH16(16, 3);
            else {
                static bool attr16 = false;
                if (!attr16) {
                    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(wgrad_halo16_kernel<16, 3, 1>),
                                              hipFuncAttributeMaxDynamicSharedMemorySize, 65536);
                    attr16 = true;
                }
                hipLaunchKernelGGL((wgrad_halo16_kernel<16, 3, 1>), dim3(nb), dim3(512), lds, st, q);
            }
#undef ACIMG_WH16
            int rc = check_launch("wgrad_halo16");
            return rc ? rc : wgrad_reduce(sl, nb, p, dw, db, true, st);
        }
    }
    if (p.a_scale) return fail(ACIMG_EWORKSPACE, "wgrad: workspace too small for the halo form, which the input affine needs");
    if (wgrad_halo_ok(p)) {
        WgradHaloParams q{};
        q.X = p.X; q.H = p.H; q.W = p.W; q.C = p.C; q.ldx = p.ldx;
        q.G = p.G; q.OH = p.OH; q.OW = p.OW; q.Kp = p.Nld; q.ldg = p.ldg;
        q.R = p.R; q.S = p.S; q.stride = p.stride; q.pad_t = p.pad_t; q.pad_l = p.pad_l;
        q.XH = (WH_TH - 1) * p.stride + p.R; q.XW = (WH_TW - 1) * p.stride + p.S;
        q.tiles_x = cdiv(p.OW, WH_TW); q.tiles_y = cdiv(p.OH, WH_TH);
        q.tiles = (long)(p.M / (p.OH * p.OW)) * q.tiles_x * q.tiles_y;
        q.KK = p.KK; q.ldo = p.ldo;
        int nb = pick_wgrad_splits(p.M, p.KK, p.Ngemm, bmo, bn);     // = what the workspace was sized for
        if (nb > 768) nb = 768;                                      // 3 resident workgroups per CU, each pipelined
        if (nb > q.tiles) nb = (int)q.tiles;
        if (nb < 2) nb = 2;
        const WgradSlabs sl = wgrad_slabs(p, nb, db, ws, ws_bytes);
        if (!sl.fits) return wgrad_ws_short(sl, ws_bytes);
        q.out = sl.out;
        q.db_out = sl.db_out;
        const size_t lds = wgrad_halo_lds(p.R, p.S, p.C, p.Nld, p.stride);
        const int nkt = (p.KK + 1 + 15) / 16;
#define ACIMG_WH(NTv, NKTv) hipLaunchKernelGGL((wgrad_halo_kernel<NTv, NKTv>), dim3(nb), dim3(256), lds, st, q)
        if (nkt <= 1) ACIMG_WH(1, 1);
        else if (nkt <= 2) ACIMG_WH(1, 2);
        else if (nkt <= 3) ACIMG_WH(1, 3);
        else if (nkt <= 5) ACIMG_WH(1, 5);
        else ACIMG_WH(1, 10);
#undef ACIMG_WH
        int rc = check_launch("wgrad_halo");
        return rc ? rc : wgrad_reduce(sl, nb, p, dw, db, true, st);
    }
    if (split3) bn = wgrad_split3_bn(p.Ngemm);
    if (split3 && terms == 3 && wgrad_tap_ok(p)) {
        WgradTapParams q{};
        q.X = p.X; q.H = p.H; q.W = p.W; q.C = p.C; q.ldx = p.ldx; q.G = p.G; q.ldg = p.ldg;
        q.Ngemm = p.Ngemm; q.Nld = p.Nld; q.KK = p.KK; q.ldo = p.ldo;
        q.tiles_y = cdiv(p.H, WT_TH);
        q.tiles = (long)(p.M / (p.H * p.W)) * q.tiles_y;
        // pixel splits: what the generic path is granted for this shape (the workspace is sized for it), one tile each at least
        int ns = pick_wgrad_splits(p.M, p.KK, p.Ngemm, bmo, bn);
        if (ns > q.tiles) ns = (int)q.tiles;
        const WgradSlabs sl = wgrad_slabs(p, ns, db, ws, ws_bytes);
        if (ns > 1) {
            if (!sl.fits) return wgrad_ws_short(sl, ws_bytes);
            q.out = sl.out;
            q.db_out = sl.db_out;
        } else {                // one slab: the kernel writes dW / db themselves, no reduce
            q.out = dw;
            q.db_out = db;
        }
        const size_t lds = wgrad_tap_lds(p.W);
        static bool attr_set = false;
        if (!attr_set) {
            (void)hipFuncSetAttribute(reinterpret_cast<const void*>(wgrad_tap_kernel<128>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                      (int)wgrad_tap_lds(WT_MAXW));
            (void)hipFuncSetAttribute(reinterpret_cast<const void*>(wgrad_tap_kernel<64>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                      (int)wgrad_tap_lds(WT_MAXW));
            attr_set = true;
        }
        const dim3 grid(cdiv(p.C, WT_CB), cdiv(p.Ngemm, bn), ns);
        if (bn == 128) hipLaunchKernelGGL((wgrad_tap_kernel<128>), grid, dim3(512), lds, st, q);
        else hipLaunchKernelGGL((wgrad_tap_kernel<64>), grid, dim3(512), lds, st, q);
        int rc = check_launch("wgrad_tap");
        return (rc || ns == 1) ? rc : wgrad_reduce(sl, ns, p, dw, db, false, st);
    }
    p.splits = pick_wgrad_splits(p.M, p.KK, p.Ngemm, bmo, bn);
    int rps = cdiv(p.M, p.splits);
    rps = ((rps + 31) / 32) * 32;
    p.rows_per_split = rps;
    p.splits = cdiv(p.M, rps);
    const WgradSlabs sl = wgrad_slabs(p, p.splits, db, ws, ws_bytes);
    if (p.splits > 1) {
        if (!sl.fits) return wgrad_ws_short(sl, ws_bytes);
        p.out = sl.out;
        p.db_out = sl.db_out;
    } else {
        p.out = dw;
        p.db_out = db;
    }
    const int rows = p.KK + (db ? 1 : 0);
    dim3 grid(cdiv(rows, bmo), cdiv(p.Ngemm, bn), p.splits);
    if (split3 && terms == 1 && bn == 128) hipLaunchKernelGGL((wgrad_split3_kernel<128, 1, 512>), grid, dim3(512), 65536, st, p);
    else if (split3 && terms == 1 && bn == 64) hipLaunchKernelGGL((wgrad_split3_kernel<64, 1, 512>), grid, dim3(512), 65536, st, p);
    else if (split3 && terms == 1) hipLaunchKernelGGL((wgrad_split3_kernel<32, 1>), grid, dim3(256), 65536, st, p);
    else if (split3 && bn == 128) hipLaunchKernelGGL((wgrad_split3_kernel<128, 3, 512>), grid, dim3(512), 65536, st, p);
    else if (split3 && bn == 64) hipLaunchKernelGGL((wgrad_split3_kernel<64, 3, 512>), grid, dim3(512), 65536, st, p);
    else if (split3) hipLaunchKernelGGL((wgrad_split3_kernel<32>), grid, dim3(256), 65536, st, p);
    else if (bn == 128) hipLaunchKernelGGL((wgrad_f32_kernel<128, 128>), grid, dim3(256), 0, st, p);
    else if (bn == 64) hipLaunchKernelGGL((wgrad_f32_kernel<128, 64>), grid, dim3(256), 0, st, p);
    else if (bn == 32) hipLaunchKernelGGL((wgrad_f32_kernel<128, 32>), grid, dim3(256), 0, st, p);
    else hipLaunchKernelGGL((wgrad_f32_kernel<128, 16, 4>), grid, dim3(256), 0, st, p);
    int rc = check_launch("wgrad");
    return (rc || p.splits <= 1) ? rc : wgrad_reduce(sl, p.splits, p, dw, db, false, st);
}

// column sums; workspace: parts*ncols floats
static int colsum_parts(long rows) {
    int parts = (int)((rows + 255) / 256);
    if (parts > 256) parts = 256;
    if (parts < 1) parts = 1;
    return parts;
}
static int launch_colsum(const float* G, long rows, int ncols, int ld, float* out, void* ws,
                         size_t ws_bytes, hipStream_t st) {
    const int parts = colsum_parts(rows);
    const long rpb = (rows + parts - 1) / parts;
    const size_t need = (size_t)parts * ncols * sizeof(float);
    if (ws == nullptr || ws_bytes < need) return fail(ACIMG_EWORKSPACE, "colsum: workspace %zu < %zu", ws_bytes, need);
    float* partial = static_cast<float*>(ws);
    if (ncols <= 64 && (ncols & 3) == 0 && (ld & 3) == 0 && aligned16(G))
        hipLaunchKernelGGL(colsum_narrow_kernel, dim3(parts), dim3(256), 0, st, G, rows, ncols, ld, rpb, partial);
    else
        hipLaunchKernelGGL(colsum_partial_kernel, dim3(cdiv(ncols, 64), parts), dim3(256), 0, st, G, rows,
                           ncols, ld, rpb, partial);
    hipLaunchKernelGGL(colsum_final_kernel, dim3(cdiv(ncols, 64)), dim3(256), 0, st, partial, parts, ncols, out);
    return check_launch("colsum");
}
static size_t colsum_ws_bytes(int ncols) { return (size_t)256 * ncols * sizeof(float); }

// row_run: the caller's kernel accepts ldx < C with S == 1: the C "channels" of a tap are then a run of C / ldx
// consecutive pixels of one input row (windows of neighbouring outputs overlap), see acimg_conv2d_fwd_split3
static int check_desc(const AcimgConvDesc* d, const char* who, bool row_run = false) {
    if (!d) return fail(ACIMG_EINVAL, "%s: null descriptor", who);
    if (d->N <= 0 || d->H <= 0 || d->W <= 0 || d->C <= 0 || d->K <= 0 || d->OH <= 0 || d->OW <= 0 ||
        d->R <= 0 || d->S <= 0 || d->stride <= 0)
        return fail(ACIMG_EINVAL, "%s: non-positive dimension", who);
    const bool run_view = row_run && d->S == 1 && d->pad_l == 0 && d->ldx > 0 && d->C % d->ldx == 0 &&
                          (d->OW - 1) * d->stride + d->C / d->ldx <= d->W;
    if ((d->C & 3) || (d->ldx & 3) || (d->ldw & 3) || (d->ldx < d->C && !run_view))
        return fail(ACIMG_EINVAL, "%s: C=%d ldx=%d ldw=%d must be multiples of 4 (ldx>=C)", who, d->C, d->ldx, d->ldw);
    if ((long)d->N * d->H * d->W * d->ldx >= (1L << 31) || (long)d->N * d->OH * d->OW * (long)d->ldy >= (1L << 31))
        return fail(ACIMG_EINVAL, "%s: tensor exceeds 2^31 elements", who);
    return ACIMG_OK;
}
static inline int up4(int v) { return (v + 3) & ~3; }

// few-channel direct path: C <= 16 (wider pixels stop coalescing across lanes), K <= 32 and a multiple of 8.
// direct_shape is what the sizing queries know (the few-channel MFMA form's shapes lie inside it); direct_ok adds the operands
static bool direct_shape(int C, int K) { return C <= 16 && K <= 32; }
static bool direct_ok(int C, int K, int ldy, int ldres, const float* y, const float* bias, const float* res,
                      bool affine, const float* mask) {
    return !affine && !mask && direct_shape(C, K) && ldy >= ((K + 3) & ~3) && (C & 3) == 0 && (ldy & 3) == 0 &&
           (!res || ((ldres & 3) == 0 && aligned16(res))) && aligned16(y) && (!bias || aligned16(bias));
}
static size_t direct_ws_bytes(int R, int S, int C, int K) { return ((size_t)R * S * C * K * sizeof(float) + 255) & ~(size_t)255; }
static int launch_direct(const DirectParams& q, void* ws, size_t ws_bytes, hipStream_t st) {
    if (!aligned16(q.x) || (q.ldx & 3)) return fail(ACIMG_EINVAL, "direct conv: input must be 16-byte aligned");
    const int total = q.R * q.S * q.C * ((q.K + 7) & ~7);
    if (!ws || ws_bytes < (size_t)total * sizeof(float)) return fail(ACIMG_EWORKSPACE, "direct conv: workspace too small");
    float* wprep = static_cast<float*>(ws);
    hipLaunchKernelGGL(direct_prepare_kernel, dim3(cdiv(total, 256)), dim3(256), 0, st, q, wprep, total);
    const long units = (long)cdiv(q.M, 256) * cdiv(q.K, 8);
    const dim3 grid((unsigned)(8 * ((units + 7) / 8)));          // 8 equal ranges, one per XCD (see the kernel)
#define ACIMG_DIRECT(RR, SS, CC) \
    hipLaunchKernelGGL((direct_conv_kernel<RR, SS, CC>), grid, dim3(256), 0, st, q, wprep)
    if (q.R == 3 && q.S == 3 && q.C == 4) ACIMG_DIRECT(3, 3, 4);
    else if (q.R == 3 && q.S == 3 && q.C == 8) ACIMG_DIRECT(3, 3, 8);
    else if (q.R == 3 && q.S == 3 && q.C == 16) ACIMG_DIRECT(3, 3, 16);
    else if (q.R == 1 && q.S == 1 && q.C == 8) ACIMG_DIRECT(1, 1, 8);
    else if (q.R == 2 && q.S == 2 && q.C == 8) ACIMG_DIRECT(2, 2, 8);
    else ACIMG_DIRECT(0, 0, 0);
#undef ACIMG_DIRECT
    return check_launch("direct_conv");
}

// shapes the few-channel MFMA kernel takes (cin = channels of the tensor that is convolved, nout = channels written)
// cin = channels of the tensor that is convolved (4 forward only: an 8-channel image with a zero upper half), nout = written
static bool few16_channels(int cin, int nout, long pixels) {
    return (cin == 4 || cin == 8 || cin == 16) && nout >= 4 && nout <= 32 && (nout & 3) == 0 && !(cin != 8 && nout > 16) &&
           pixels >= 65536 && g_cfg.wgrad_halo;
}
// (ldx a multiple of 4: the kernel stages x in float4 pieces - and the predicate is what acimg_conv2d_stats_rows and
// acimg_conv2d_affine_input_ok answer from, so it must not promise this form to a descriptor the entry point refuses)
static bool few16_fwd_shape(const AcimgConvDesc* d) {
    return d->R == 3 && d->S == 3 && d->stride == 1 && d->pad_t == 1 && d->pad_l == 1 && d->OH == d->H && d->OW == d->W &&
           few16_channels(d->C, d->K, (long)d->N * d->OH * d->OW) && d->act == ACIMG_ACT_NONE && d->ldx >= d->C &&
           (d->ldx & 3) == 0;
}
// the data gradient of a 3x3 conv is a 3x3 / stride-1 conv of gy (K channels, padded to 4) into C channels: of gy itself
// (stride 1) or of its zero-inserted view (stride 2: the view is formed while the tile is staged, no copy)
static bool few16_dgrad_shape(const AcimgConvDesc* d) {
    const int ca = (d->K + 3) & ~3;
    return d->R == 3 && d->S == 3 && (d->stride == 1 || d->stride == 2) && ca != 4 && d->pad_t <= 2 && d->pad_l <= 2 &&
           few16_channels(ca, d->C, (long)d->N * d->H * d->W);
}
static size_t few16_ws_bytes(int cin, int nout) {
    return ((size_t)2 * (nout <= 16 ? 16 : 32) * few16_ktot(cin == 4 ? 8 : cin) * 2 + 255) & ~(size_t)255;
}

template <typename TR, int CIN, int NOUTP, int MODE, int CLOAD = CIN>
static int launch_few16(FewParams q, int N, void* ws, hipStream_t st) {
    constexpr int KTOT = few16_ktot(CIN);
    q.tiles_x = cdiv(q.W, 32); q.tiles_y = cdiv(q.H, 16);
    q.tiles = (long)N * q.tiles_x * q.tiles_y;
    q.per = (q.tiles + 7) / 8;
    typename TR::T* img = static_cast<typename TR::T*>(ws);
    q.Wimg = static_cast<const char*>(ws); q.w_lo_off = NOUTP * KTOT * 2;
    hipLaunchKernelGGL((few16_prepare_kernel<TR>), dim3(cdiv(NOUTP * KTOT, 256)), dim3(256), 0, st, q, CIN, NOUTP, img);
    hipLaunchKernelGGL((conv_few16_kernel<TR, CIN, NOUTP, MODE, CLOAD>), dim3(FEW16_WGS), dim3(512), 0, st, q);
    return check_launch("conv_few16");
}
// forward (MODE 0, f16 hi / lo) or data gradient (MODE 1, bf16 hi / lo) on the few-channel MFMA kernel
template <int MODE>
static int dispatch_few16(const FewParams& q, int N, int cin, int nout, void* ws, size_t ws_bytes, hipStream_t st) {
    if (!ws || ws_bytes < few16_ws_bytes(cin, nout) || !aligned16(ws)) return fail(ACIMG_EWORKSPACE, "conv_few16: workspace too small");
    typedef typename std::conditional<MODE == 0, SplitF16, SplitBF16>::type TR;
    if (cin == 4) return launch_few16<TR, 8, 16, MODE, 4>(q, N, ws, st);
    if (cin == 8) return nout <= 16 ? launch_few16<TR, 8, 16, MODE>(q, N, ws, st) : launch_few16<TR, 8, 32, MODE>(q, N, ws, st);
    return launch_few16<TR, 16, 16, MODE>(q, N, ws, st);
}

static bool patch2_shape(const AcimgConvDesc* d) {
    return d->R == 2 && d->S == 2 && d->stride == 2 && d->C == 32 && d->K == 8 && d->OH == 2 * d->H && d->OW == 2 * d->W &&
           (long)d->N * d->H * d->W >= 65536 && g_cfg.wgrad_halo;
}
template <typename TR, int MODE>
static int launch_patch2(const Patch2Params& q, hipStream_t st) {
    const long groups = (q.pixels + 15) >> 4;
    long blocks = (groups + 3) / 4;
    if (blocks > 256 * 16) blocks = 256 * 16;          // sixteen 4-wave workgroups per CU, each wave walks its groups
    hipLaunchKernelGGL((patch2_32x8_kernel<TR, MODE>), dim3((unsigned)blocks), dim3(256), 0, st, q);
    return check_launch("patch2_32x8");
}

static int fwd_kiters(const AcimgConvDesc* d) {
    const bool rowrun = d->S > 1 && d->ldx == d->C;
    const int L = rowrun ? d->S * d->C : d->C;
    return (rowrun ? d->R : d->R * d->S) * cdiv(L, 32);
}

// rows of y covered by one statistics partial: the implicit-GEMM tile height, or 256 after split-K
static int stats_block_rows(const AcimgConvDesc* d) {
    const int M = d->N * d->OH * d->OW;
    TileCfg c = pick_cfg(M, d->K);
    return pick_splits(M, d->K, c, fwd_kiters(d)) > 1 ? 256 : c.bm;
}
// a dense layer over at most 64 batch rows with a large weight matrix (csrc/skinny_kernel.hpp)
static bool skinny_shape(const AcimgConvDesc* d) {
    return d->R == 1 && d->S == 1 && d->H == 1 && d->W == 1 && d->OH == 1 && d->OW == 1 && d->stride == 1 &&
           d->pad_t == 0 && d->pad_l == 0 && d->N <= 64 && d->C >= 4096 && (d->C & 3) == 0 && (d->K & 3) == 0 &&
           (long)d->C * d->ldw * 4 < (1L << 31) && (long)d->N * d->ldx * 4 < (1L << 31);
}
static size_t skinny_fwd_ws_bytes(const AcimgConvDesc* d) {
    return skinny_shape(d) ? (size_t)cdiv(d->C, SKINNY_KS) * d->N * d->K * 4 : 0;
}

// the sub-pixel form pays from 16 output channels on: with 8 (the full-resolution layers) its scatter writes 16-byte
// pieces of 32-byte pixels and the zero-inserted copy + the direct few-channel kernel is faster (224x298 8->8 3x3/2 data
// gradient: 99 us against 144 us; profiles/r04/op_report_unet_rgb_bf16_r04g_subpixel.txt)
static bool subpixel_ok(int stride, int Ko, int Kin) { return stride == 2 && (Ko & 3) == 0 && (Kin & 3) == 0 && Ko >= 16; }
static size_t subpixel_ws_bytes(int N, int YH, int YW, int oy0, int ox0, int R, int S, int Kin, int Ko) {
    const int U = (R + 1) / 2, V = (S + 1) / 2;
    const int AH = (YH - 1 - oy0) / 2 + 1, AW = (YW - 1 - ox0) / 2 + 1;
    const size_t wc = ((size_t)U * V * Kin * 4 * Ko * 4 + 255) & ~(size_t)255;
    const size_t a = igemm_ws_bytes(N * AH * AW, 4 * Ko, U * V * cdiv(Kin, 32));
    const size_t b = igemm_ws_bytes(N * AH * AW, 4 * Ko, U * cdiv(V * Kin, 32));
    return wc + (a > b ? a : b);
}
// A: [N][aH][aW][Kin] (pixel stride lda); w[r][s][ko][kin] with row pitch ldw; Y: [N][YH][YW] pixels of ldy floats
static int launch_subpixel(const float* A, int N, int aH, int aW, int Kin, int lda, const float* w, int R, int S, int ldw,
                           int Ko, float* Y, int ldy, int YH, int YW, int oy0, int ox0, const float* bias, const float* res,
                           int ldres, const float* mask, int ldmask, int act, void* ws, size_t ws_bytes, void* tickets,
                           hipStream_t st, const char* what) {
    const int U = (R + 1) / 2, V = (S + 1) / 2;
    const int AH = (YH - 1 - oy0) / 2 + 1, AW = (YW - 1 - ox0) / 2 + 1;
    const int rows = U * V * Kin, ncol = 4 * Ko;
    const size_t wcb = ((size_t)rows * ncol * 4 + 255) & ~(size_t)255;
    if (!ws || ws_bytes < wcb || !aligned16(ws)) return fail(ACIMG_EWORKSPACE, "%s: workspace too small for the sub-pixel weights", what);
    if ((Ko & 3) || (Kin & 3)) return fail(ACIMG_EINVAL, "%s: channel counts must be multiples of 4", what);
    float* wc = static_cast<float*>(ws);
    hipLaunchKernelGGL(subpixel_weights_kernel, dim3(cdiv((long)rows * ncol, 256)), dim3(256), 0, st, w, R, S, Ko, Kin, ldw, U, V, wc,
                       rows * ncol);
    int rc = check_launch("subpixel_weights");
    if (rc) return rc;
    IgemmParams p{};
    p.A = A; p.H = aH; p.W = aW; p.C = Kin; p.lda = lda; p.OH = AH; p.OW = AW;
    p.R = U; p.S = V; p.stride = 1; p.pad_t = U - 1; p.pad_l = V - 1;
    p.M = N * AH * AW;
    p.rowrun = (V > 1 && lda == Kin) ? 1 : 0;
    p.B = wc; p.ldb = ncol; p.Nld = ncol; p.Ngemm = ncol; p.tap_stride = 0; p.flip = 0;
    p.e.Y = Y; p.e.ldy = ldy; p.e.M = p.M; p.e.Nstore = ncol; p.e.bias = bias; p.e.act = act;
    p.e.res = res; p.e.ldres = ldres; p.e.mask = mask; p.e.ldmask = ldmask;
    p.e.scatter = 2; p.e.Ko = Ko; p.e.Sq = 2; p.e.sc = 2; p.e.YH = YH; p.e.YW = YW; p.e.AH = AH; p.e.AW = AW;
    p.e.oy0 = oy0; p.e.ox0 = ox0;
    return launch_igemm(p, false, static_cast<char*>(ws) + wcb, ws_bytes - wcb, tickets, st);
}

static bool dgrad_is_patch(const AcimgConvDesc* d) {
    return d->stride > 1 && d->stride == d->R && d->stride == d->S && !d->pad_t && !d->pad_l &&
           d->OH * d->stride == d->H && d->OW * d->stride == d->W;
}
static size_t dilated_bytes(int N, int H, int W, int C, int s) {
    return ((size_t)N * ((H - 1) * s + 1) * ((W - 1) * s + 1) * C * 4 + 255) & ~(size_t)255;
}

// data gradient of a 3x3 / stride-1 / SAME layer with 32 output and 4 - 16 input channels (configs[1]: 112x149 8 -> 32) through
// the fp32 entry: a conv of the 32-channel gy on the 16-row instance of the halo kernel (conv_halo16_kernel.hpp)
static bool dgrad_halo16_narrow_shape(const AcimgConvDesc* d) {
    return d->R == 3 && d->S == 3 && d->stride == 1 && d->pad_t == 1 && d->pad_l == 1 && d->OH == d->H && d->OW == d->W &&
           d->K == 32 && d->C <= 16 && (d->C & 3) == 0 && (long)d->N * d->H * d->W >= 65536 && g_cfg.wgrad_halo;
}
static constexpr size_t DGRAD_HALO16_NARROW_WS = 2 * 16 * 288 * 2;
// ------------------------------------------------------------------------------------------
// f16x3 (split fp16) forward convolution (frozen ResNet trunk)
// ------------------------------------------------------------------------------------------
struct Split3Cfg { int bm, bn; };
// Tile choice, measured per trunk conv shape at batch 32 (tools/tune_dma.py): the 8-wave 128x128 tile
// (2 workgroups/CU) wins on every shape with at least ~1 tile per CU; below that (the stride-2 3x3 conv into
// the 14x19 stage: 134 tiles) 64x128 fills more CUs; Cout = 64 uses 128x64.
static Split3Cfg pick_split3(int M, int K, bool allow32 = false) {
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
static bool conv_halo16_fwd_shape(const AcimgConvDesc* d) {
    return d->R == 3 && d->S == 3 && d->stride == 1 && d->pad_t == 1 && d->pad_l == 1 && d->OH == d->H && d->OW == d->W &&
           (d->C == 32 || d->C == 64) && d->K == 32 && (long)d->N * d->H * d->W >= 65536 && d->act == ACIMG_ACT_NONE &&
           g_cfg.wgrad_halo;
}
static bool conv_halo16_dgrad_shape(const AcimgConvDesc* d) {
    return d->R == 3 && d->S == 3 && d->stride == 1 && d->pad_t == 1 && d->pad_l == 1 && d->OH == d->H && d->OW == d->W &&
           (d->C == 32 || d->C == 64) && d->K == 32 && (long)d->N * d->H * d->W >= 65536 && g_cfg.wgrad_halo;
}

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

static int dgrad_halo16_narrow(const AcimgConvDesc* d, const float* gy, int ldgy, const float* w, float* dx, int lddx,
                               const float* residual, int ldres, const float* mask, int ldmask, void* ws, hipStream_t st) {
    // the flipped / transposed image [16 rows = input channels, zero beyond C][k = tap * 32 + gy channel], bf16 hi / lo
    FewParams f{};
    f.w = w; f.ldw = d->ldw; f.wrows = d->C; f.cin = d->K; f.mode = 1; f.nout = d->C;
    hipLaunchKernelGGL((few16_prepare_kernel<SplitBF16>), dim3(cdiv(16 * 288, 256)), dim3(256), 0, st, f, 32, 16,
                       static_cast<__bf16*>(ws));
    ConvHaloParams q{};
    q.X = gy; q.H = d->H; q.W = d->W; q.ldx = ldgy; q.Wimg = static_cast<const char*>(ws); q.w_lo_off = 16 * 288 * 2;
    q.Y = dx; q.ldy = lddx; q.nout = d->C; q.res = residual; q.ldres = ldres; q.mask = mask; q.ldmask = ldmask;
    return launch_conv_halo16<SplitBF16, 3, 32, 16, 1>(q, d->N, st);
}

// ---- which kernel a pre-split (trunk) forward conv runs on: the ONE place that decides it.  fwd_presplit launches what
// pick_trunk says; acimg_conv2d_fwd_split3p_stats_rows and acimg_conv2d_fwd_split3_tiling report it ----
enum TrunkKind { TRUNK_ONE_TILE = 0, TRUNK_PERSISTENT = 1, TRUNK_RING = 2, TRUNK_HALO = 3 };   // = the tiling query's third word
struct TrunkPick {
    TrunkKind kind;
    int bm, bn;          // row and column tile
    int stats_rows;      // statistics partials the kernel leaves: one per row tile
    bool big_out;        // the output exceeds a 32-bit buffer descriptor
};

// Halo kernel (igemm_split3h_kernel.hpp) for a pre-split trunk conv: 3x3 / stride 1 / SAME on 128x128 tiles, image rows
// short enough for an 18-brick patch.  trunk_halo = 1 takes it where it was measured to pay, 2 wherever it applies.
static constexpr int HALO_NB = 18;
static bool halo_applies(const AcimgConvDesc* d, int terms, const Split3Cfg& c) {
    if (terms != 3 || d->R != 3 || d->S != 3 || d->stride != 1 || d->pad_t != 1 || d->pad_l != 1 || d->OH != d->H ||
        d->OW != d->W || d->C % 32)
        return false;
    if (c.bm != 128 || c.bn != 128) return false;
    return ((d->W + 16) >> 4) + 8 + (d->W >> 4) + 1 <= HALO_NB;
}

static TrunkPick pick_trunk(const AcimgConvDesc* d, int terms, bool two_pass) {
    const int M = d->N * d->OH * d->OW;
    const Split3Cfg c = pick_split3(M, d->K);
    const bool t128 = c.bm == 128 && c.bn == 128;
    // the persistent and the ring kernel address the output through a 32-bit buffer descriptor; a larger output (per-GPU
    // batches around 512 on the first trunk units) falls back to the one-tile kernel's 64-bit pointer stores
    TrunkPick t{TRUNK_ONE_TILE, c.bm, c.bn, 0, (long)M * d->ldy * 4 >= (1L << 31)};
    // statistics-only / fused-tail passes: always the persistent kernel (whole tiles, then K ranges of the tail tiles);
    // fwd_presplit refuses the shapes that kernel does not take
    if (two_pass) t.kind = TRUNK_PERSISTENT;
    // trunk_halo = 1 ("where it was measured to pay") selects nothing yet: at batch 32 the halo form is at parity with the
    // per-tap kernels on the 56x75 / 28x38 layers and behind the ring kernel on 14x19; 2 = wherever it applies
    else if (g_cfg.trunk_halo == 2 && halo_applies(d, terms, c)) t.kind = TRUNK_HALO;
    // Ring kernel (igemm_split3r_kernel.hpp) for a pre-split trunk conv, and with how many tile rows (ring_rows; 0 = not on it).
    // Measured per shape at batch 32 and 30 (tools/trunk_shapes.py, profiles/r03/trunk_shapes_r03*.txt): in its steady state
    // the ring kernel's K loop is 8-14 % faster than the two-workgroups-per-CU kernels' (long-K layers whose tiles fill one
    // round of the 256 CUs), but with ONE workgroup per CU it pays more for tile quantisation (a 1.04-round layer leaves
    // 246 CUs idle for a round, where 512 slots leave a quarter of the chip) and for short-K tiles (the output tile's stores
    // and the deferred stage at every unit boundary).  trunk_ring = 1 therefore takes it where it won: layers of at most
    // ~1.2 rounds of 128x128 tiles over the CUs (the 14x19 stage) with at least 64 K steps, on 128-row tiles with the tail
    // cut into K ranges; trunk_ring = 2 forces it (experiments, tests).
    int ring_rows = 0;
    if (!two_pass && t.kind != TRUNK_HALO && !t.big_out && g_cfg.trunk_ring && terms == 3 && t128) {
        const long t128s = (long)cdiv(M, 128) * cdiv(d->K, 128);
        const int kiters = d->R * d->S * (d->C / 32);
        const long t256 = (long)cdiv(M, 256) * cdiv(d->K, 128);
        if (g_cfg.trunk_ring == 1) ring_rows = (t128s > 256 && t128s <= 300 && kiters >= 64) ? 128 : 0;
        else if (g_cfg.trunk_ring_bm) ring_rows = g_cfg.trunk_ring_bm;
        else ring_rows = t256 >= 500 ? 256 : 128;
    }
    if (ring_rows) {
        t.kind = TRUNK_RING;
        t.bm = ring_rows;
    }
    // Persistent kernel or one tile per workgroup for the pre-split (trunk) forward conv (tools/trunk_shapes.py,
    // profiles/r02/trunk_shapes_*.txt): walking a tile list wins 2-9 % wherever there is at least one full round of whole
    // 128x128 tiles (most on short-K multi-round layers); when every tile belongs to the split tail (fewer tiles than
    // resident workgroups) the one-tile kernel's leaner code is 3-7 % faster.
    const long tiles = (long)cdiv(M, c.bm) * cdiv(d->K, c.bn);
    if (t.kind == TRUNK_ONE_TILE && !t.big_out && t128 && (g_cfg.trunk_persistent == 2 || (g_cfg.trunk_persistent == 1 && tiles >= 512)))
        t.kind = TRUNK_PERSISTENT;
    t.stats_rows = cdiv(M, t.bm);
    return t;
}

// Row-major planes [hi | lo][ldw][R*S*C], then (C % 32 == 0) the same weights once more in LDS-TILE ORDER: for every
// (128-column tile nt, K step q of 32) the two 8 KiB plane images exactly as the trunk kernels keep them in LDS
// (64-byte rows, logical chunk kc of row r at chunk kc ^ swz(r)), so a wave's LDS-DMA request for a weight piece is one
// contiguous KiB = eight whole 128-byte lines instead of sixteen 64-byte pieces of rows 2*R*S*C bytes apart.
static size_t split3_rowmajor_bytes(const AcimgConvDesc* d) { return (size_t)2 * d->ldw * d->R * d->S * d->C * 2; }
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

static int fwd_split_onthefly(const AcimgConvDesc* d, const float* x, const void* wsplit, const float* bias, float* y,
                              const float* in_scale, const float* in_shift, int in_relu, float* stats, void* stream,
                              bool bf16) {
    int rc = check_desc(d, "conv2d_fwd_split3", true);
    if (rc) return rc;
    if (d->C % 32) return fail(ACIMG_EINVAL, "conv2d_fwd_split3: C=%d must be a multiple of 32", d->C);
    if (d->ldw < d->K || !aligned16(x) || !aligned16(wsplit))
        return fail(ACIMG_EINVAL, "conv2d_fwd_split3: ldw<K or unaligned operands");
    if (conv_halo16_fwd_shape(d)) {
        // (acimg_conv2d_fwd_split3_stats_rows already told the caller this shape leaves CONV_HALO16_WGS rows: no fallback)
        if ((in_scale != nullptr) != (in_shift != nullptr) || (in_relu && !in_scale) || !aligned16(y) || (d->ldy & 3) || (d->ldx & 3) ||
            (bias && !aligned16(bias)) || (in_scale && (!aligned16(in_scale) || !aligned16(in_shift))))
            return fail(ACIMG_EINVAL, "conv2d_fwd_split3: the halo form of this shape needs scale AND shift of an input affine, "
                                      "16-byte aligned y / bias / affine and ldx, ldy multiples of 4");
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
    const long a_bytes = (((long)d->N * d->H * d->W - 1) * d->ldx + d->C) * 4;
    const long b_bytes = (long)acimg_conv2d_split3_weight_bytes(d);
    if (a_bytes >= (1L << 31) || b_bytes >= (1L << 31)) return fail(ACIMG_EINVAL, "conv2d_fwd_split3: operand >= 2 GiB");
    p.a_bytes = (unsigned)a_bytes; p.b_bytes = (unsigned)b_bytes;
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
    if (d->stride != 1 || d->K % 32 || d->K > ldgy || (ldgy & 3))
        return fail(ACIMG_EINVAL, "conv2d_dgrad_split3: needs stride 1 and K %% 32 == 0 (K=%d)", d->K);
    if (lddx <= 0) lddx = d->ldx;
    if (conv_halo16_dgrad_shape(d) && aligned16(gy) && aligned16(wsplit_t) && aligned16(dx) && (lddx & 3) == 0 &&
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
    const long a_bytes = (((long)d->N * d->OH * d->OW - 1) * ldgy + d->K) * 4;
    const long b_bytes = (long)acimg_conv2d_split3_dgrad_weight_bytes(d);
    if (a_bytes >= (1L << 31) || b_bytes >= (1L << 31)) return fail(ACIMG_EINVAL, "conv2d_dgrad_split3: operand >= 2 GiB");
    p.a_bytes = (unsigned)a_bytes; p.b_bytes = (unsigned)b_bytes;
    EpiParams& e = p.e;
    e.Y = dx; e.ldy = lddx; e.res = residual; e.ldres = ldres; e.mask = mask; e.ldmask = ldmask;
    epi_vec_flag(e);
    if (conv_tap_ok(p, terms)) return launch_conv_tap<SplitBF16>(p, (hipStream_t)stream);
    if (terms == 1) return launch_split3<SplitBF16, 1>(p, (hipStream_t)stream);
    return launch_split3<SplitBF16>(p, (hipStream_t)stream);
}

// ---- tail split of the trunk kernel: which tiles to cut, and into how many K ranges ------------------------
struct TailPlan { int whole, s, rem; };

// One record per trunk kernel that is launched: what a launch and the occupancy question need to know about it, and what
// was learnt about it in this process (both once per process).
struct TrunkVariant {
    const void* fn;
    int threads;
    size_t lds;                  // dynamic LDS bytes of a launch
    int wgs_per_cu;              // resident workgroups per CU assumed when no device answers
    bool lds_opt_in;             // its dynamic LDS exceeds 64 KiB: needs the opt-in once per process
    TrunkVariant* slots_of;      // the sibling whose occupancy stands for this kernel's (nullptr: its own)
    int slots;                   // resident workgroups on the device, 0 = not asked yet
    bool opted_in;
};
// one-tile kernels: 2 stages x (hi, lo) x 64-byte rows; the epilogue restages the fp32 output tile there (+ 2 x WGM x BN
// floats of statistics scratch behind it)
static constexpr size_t tile_lds(size_t bm, size_t bn) { return std::max(2 * 2 * (bm + bn) * 64, bm * bn * 4) + 4 * 2 * bn * 4; }
// (a 64-deep K step - whole 128-byte operand rows, one workgroup per CU - was measured slower on every trunk shape in
//  round 2 and removed when the operands moved to LDS-tile order, which gives whole-line requests at two per CU)
static constexpr size_t PERSISTENT_LDS = (size_t)2 * 4 * 128 * 64 + 4 * 2 * 128 * 4;    // 2 stages + statistics scratch
static constexpr size_t ring_lds(size_t rows) { return 3 * 2 * (rows + 128) * 64 + 4 * 2 * 128 * 4; }
static constexpr size_t HALO_LDS = (size_t)2 * (HALO_NB * 1024 + 64) + 2 * 2 * 128 * 64;
#define ACIMG_KFN(...) reinterpret_cast<const void*>(__VA_ARGS__)
static TrunkVariant TILE_128x128 = {ACIMG_KFN(igemm_split3d_kernel<128, 128, 2, 4, 512, 2, 2>), 512, tile_lds(128, 128), 2, false, nullptr};
static TrunkVariant TILE_64x128 = {ACIMG_KFN(igemm_split3d_kernel<64, 128, 1, 4, 256, 2, 2>), 256, tile_lds(64, 128), 3, false, nullptr};
static TrunkVariant TILE_128x64 = {ACIMG_KFN(igemm_split3d_kernel<128, 64, 2, 2, 256, 2, 2>), 256, tile_lds(128, 64), 3, false, nullptr};
static TrunkVariant TILE1_128x128 = {ACIMG_KFN(igemm_split3d_kernel<128, 128, 2, 4, 512, 2, 2, 1>), 512, tile_lds(128, 128), 2, false, &TILE_128x128};
static TrunkVariant TILE1_64x128 = {ACIMG_KFN(igemm_split3d_kernel<64, 128, 1, 4, 256, 2, 2, 1>), 256, tile_lds(64, 128), 3, false, &TILE_64x128};
static TrunkVariant TILE1_128x64 = {ACIMG_KFN(igemm_split3d_kernel<128, 64, 2, 2, 256, 2, 2, 1>), 256, tile_lds(128, 64), 3, false, &TILE_128x64};
static TrunkVariant PERSISTENT = {ACIMG_KFN(igemm_split3dp_kernel<32, 0>), 512, PERSISTENT_LDS, 2, false, nullptr};
static TrunkVariant PERSISTENT_SPREAD = {ACIMG_KFN(igemm_split3dp_kernel<32, 1>), 512, PERSISTENT_LDS, 2, false, &PERSISTENT};
static TrunkVariant PERSISTENT1 = {ACIMG_KFN(igemm_split3dp_kernel<32, 0, 1>), 512, PERSISTENT_LDS, 2, false, &PERSISTENT};
static TrunkVariant PASS_STATS = {ACIMG_KFN(igemm_split3dp_kernel<32, 0, 3, 1>), 512, PERSISTENT_LDS, 2, false, nullptr};
static TrunkVariant PASS_TAIL = {ACIMG_KFN(igemm_split3dp_kernel<32, 0, 3, 2>), 512, PERSISTENT_LDS, 2, false, nullptr};
static TrunkVariant PASS_TAIL_PROJ = {ACIMG_KFN(igemm_split3dp_kernel<32, 0, 3, 3>), 512, PERSISTENT_LDS, 2, false, nullptr};
static TrunkVariant RING_256 = {ACIMG_KFN(igemm_split3r_kernel<4>), 512, ring_lds(256), 1, true, nullptr};
static TrunkVariant RING_128 = {ACIMG_KFN(igemm_split3r_kernel<2>), 512, ring_lds(128), 1, true, nullptr};
static TrunkVariant HALO = {ACIMG_KFN(igemm_split3h_kernel<HALO_NB>), 512, HALO_LDS, 2, true, nullptr};
#undef ACIMG_KFN

static void opt_in_lds(TrunkVariant& v) {
    if (!v.lds_opt_in || v.opted_in) return;
    (void)hipFuncSetAttribute(v.fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)v.lds);
    v.opted_in = true;
}
// workgroups of `v` the device holds at once (the occupancy question is only answered for a kernel that may use its LDS:
// it is opted in first)
static int resident_slots(TrunkVariant& v) {
    opt_in_lds(v);
    TrunkVariant& o = v.slots_of ? *v.slots_of : v;
    if (!o.slots) {
        int dev = 0, ncu = 0, per = 0;
        if (hipGetDevice(&dev) != hipSuccess ||
            hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess ||
            hipOccupancyMaxActiveBlocksPerMultiprocessor(&per, o.fn, o.threads, v.lds) != hipSuccess || ncu <= 0 || per <= 0) {
            (void)hipGetLastError();
            ncu = 256;                    // MI355X; no device (CPU-side sizing queries): same answer
            per = o.wgs_per_cu;
        }
        o.slots = ncu * per;
    }
    return o.slots;
}
// `units` and `cap` reach the kernels that walk a unit list (persistent, ring).  The one-tile and halo kernels take p alone:
// the runtime reads as many argument pointers as the kernel's metadata declares, so the two spare ones are never touched.
// The launch's status is left to the caller's check_launch (hipGetLastError), as after hipLaunchKernelGGL.
static void launch_trunk(const TrunkVariant& v, int nwg, hipStream_t st, IgemmParams& p, int units = 0, int cap = 0) {
    void* args[] = {&p, &units, &cap};
    (void)hipLaunchKernel(v.fn, dim3(nwg), dim3(v.threads), args, v.lds, st);
}
static TailPlan pick_tail(int T, int P, int KI, int max_units) {
    const int rem = T % P;
    TailPlan best{T, 1, 0};
    if (rem == 0 || !g_cfg.tail_split) return best;
    if (g_cfg.tail_s) {   // experiments only: force the number of K ranges
        const int s = g_cfg.tail_s;
        if (s > 1 && KI / s >= 1 && (long)rem * s <= max_units) return TailPlan{T - rem, s, rem};
        return best;
    }
    // cost in K steps of the last round: whole tiles = KI; s ranges = rounds(rem*s) * ceil(KI/s) + hand-off
    double best_cost = KI;
    static const int cand[] = {2, 3, 4, 6, 8, 12, 16};
    for (int s : cand) {
        if (KI / s < 2 || (long)rem * s > max_units) break;
        // hand-off calibrated on the trunk shapes (tools/tune_dma.py): partial store + ticket + the last arriver's
        // s x 64 KiB of sc1 loads cost about 8 + s K steps, so 1x1 layers with few K steps are left whole
        const double cost = (double)cdiv((long)rem * s, P) * cdiv(KI, s) + 8.0 + 1.0 * s;
        if (cost < 0.9 * best_cost) {
            best_cost = cost;
            best = TailPlan{T - rem, s, rem};
        }
    }
    return best;
}
static constexpr int TS_MAX_UNITS = 1024;      // partial slots (64 KiB each for a 128x128 tile; a 256x128 tile takes two)
static constexpr size_t TS_COUNTER_BYTES = 4096;
static constexpr size_t TS_WS_BYTES = TS_COUNTER_BYTES + (size_t)TS_MAX_UNITS * 128 * 128 * sizeof(float);   // acimg_conv2d_fwd_split3p_workspace

// Tail wiring of a trunk launch: with the caller's workspace (and a kernel that takes the split: `allow`) the tiles of the
// last, partial round over `slots` workgroups are cut into K ranges; the ticket counters and partial slots are wired either
// way.  Returns the number of work units: whole tiles + K ranges.
static int wire_tail(IgemmParams& p, void* ws, size_t ws_bytes, int tiles, int slots, int max_units, bool allow) {
    TailPlan t{tiles, 1, 0};
    if (allow && ws && ws_bytes >= TS_WS_BYTES) t = pick_tail(tiles, slots, p.kiters, max_units);
    p.ts_whole = t.whole; p.ts_s = t.s;
    p.ts_counters = static_cast<int*>(ws);
    p.ts_partial = ws ? reinterpret_cast<float*>(static_cast<char*>(ws) + TS_COUNTER_BYTES) : nullptr;
    return t.whole + t.rem * t.s;
}

#if defined(ACIMG_STAMP) || defined(ACIMG_ABLATE)
static float* g_stamp_buf = nullptr;      // diagnostic build only (tools/build_stamp.sh): never in libacimg.so
static int g_stamp_nostore = 0;           // ablation: the persistent kernel's output stores go out of range (dropped)
#endif

// the two passes of a conv whose raw output never reaches memory (igemm_split3dp_kernel, EPI 1 / 2)
struct Split3pTail {
    int mode;                      // 1: statistics only; 2: relu(acc * scale + shift + shortcut) -> split planes;
                                   // 3: the same with a projection shortcut (raw fp32 + its own scale / shift)
    const float* scale;
    const float* shift;
    const void* sc_planes;         // mode 3: the fp32 [M][K] output of the shortcut conv
    size_t sc_lo_off;
    void* out_planes;
    size_t out_lo_off;
    const float* scale2;
    const float* shift2;
};

static int fwd_presplit(const AcimgConvDesc* d, const void* x_planes, size_t x_lo_off, const void* wsplit, float* y,
                        float* stats, void* ws, size_t ws_bytes, void* stream, const int terms,
                        const Split3pTail* tail = nullptr) {
    int rc = check_desc(d, "conv2d_fwd_split3p");
    if (rc) return rc;
    if (d->C % 32) return fail(ACIMG_EINVAL, "conv2d_fwd_split3p: C=%d must be a multiple of 32", d->C);
    if (d->ldw < d->K || !aligned16(x_planes) || !aligned16(wsplit) || !aligned16(y) || (d->ldy & 3) || d->ldx != d->C ||
        (x_lo_off & 15))
        return fail(ACIMG_EINVAL, "conv2d_fwd_split3p: ldw<K, ldx != C (split-format tensors are dense) or unaligned operands");
    IgemmParams p = fwd_view(d);
    split_ksteps(p);
    p.A = static_cast<const float*>(x_planes); p.B = static_cast<const float*>(wsplit);
    const long plane = (long)acimg_split_plane_bytes((long)d->N * d->H * d->W, d->C);
    const long a_bytes = (long)x_lo_off + plane;
    const long b_bytes = (long)acimg_conv2d_split3_weight_bytes(d);
    if (a_bytes >= (1L << 31) || b_bytes >= (1L << 31) || (long)x_lo_off < plane)
        return fail(ACIMG_EINVAL, "conv2d_fwd_split3p: operand >= 2 GiB or overlapping planes");
    p.a_bytes = (unsigned)a_bytes; p.b_bytes = (unsigned)b_bytes; p.a_lo_off = (unsigned)x_lo_off;
    p.b_brick = (unsigned)split3_rowmajor_bytes(d);
    EpiParams& e = p.e;
    e.Y = y; e.stats = stats; e.vec = 1;
    const TrunkPick t = pick_trunk(d, terms, tail != nullptr);
    hipStream_t st = (hipStream_t)stream;
    // XCD-aware rasterisation: the ~64 tiles resident on one XCD (32 of the ring kernel's, one workgroup per CU) form a
    // (64/gn) x gn rectangle of the tile grid
    p.ras_tiles_m = cdiv(p.M, t.bm);
    p.ras_tiles_n = cdiv(d->K, t.bn);
    p.ras_gn = std::min(p.ras_tiles_n, 8);
    p.ras_gm = std::max(1, (t.kind == TRUNK_RING ? 32 : 64) / p.ras_gn);
    const int T = p.ras_tiles_m * p.ras_tiles_n;
    const bool t128 = t.bm == 128 && t.bn == 128;
    if (tail) {
        if (terms != 3 || !t128 || t.big_out || d->K % 128 || d->ldy != d->K || d->ldw != d->K)
            return fail(ACIMG_EINVAL, "conv2d_fwd_split3p (two-pass): needs 128x128 tiles, K %% 128 == 0, dense output < 2 GiB");
        TrunkVariant& v = tail->mode == 1 ? PASS_STATS : tail->mode == 2 ? PASS_TAIL : PASS_TAIL_PROJ;
        const int slots = resident_slots(v);
        const int units = wire_tail(p, ws, ws_bytes, T, slots, TS_MAX_UNITS, true);
        const int nwg = std::min(units, slots);
        const char* what = "conv2d_fwd_split3p_stats";
        e.Y = nullptr;
        if (tail->mode != 1) {
            const long oplane = (long)acimg_split_plane_bytes((long)p.M, d->K);
            if (!aligned16(tail->sc_planes) || !aligned16(tail->out_planes) || (tail->out_lo_off & 15) ||
                (long)tail->out_lo_off < oplane || (long)tail->out_lo_off + oplane >= (1L << 31))
                return fail(ACIMG_EINVAL, "conv2d_fwd_split3p_tail: unaligned / overlapping / >= 2 GiB split-format operands");
            e.stats = nullptr;
            e.f_scale = tail->scale; e.f_shift = tail->shift;
            e.f_sc = static_cast<const char*>(tail->sc_planes);
            e.f_out = static_cast<char*>(tail->out_planes); e.f_out_lo = (unsigned)tail->out_lo_off;
            e.f_out_bytes = (unsigned)(tail->out_lo_off + oplane);
            if (tail->mode == 3) {
                e.f_scale2 = tail->scale2; e.f_shift2 = tail->shift2;
                e.f_sc_lo = 0; e.f_sc_bytes = (unsigned)((long)p.M * d->K * 4);      // < 2 GiB: big_out was refused above
                what = "conv2d_fwd_split3p_tail_proj";
            } else {
                if ((tail->sc_lo_off & 15) || (long)tail->sc_lo_off < oplane || (long)tail->sc_lo_off + oplane >= (1L << 31))
                    return fail(ACIMG_EINVAL, "conv2d_fwd_split3p_tail: unaligned / overlapping / >= 2 GiB shortcut planes");
                e.f_sc_lo = (unsigned)tail->sc_lo_off;
                e.f_sc_bytes = (unsigned)(tail->sc_lo_off + oplane);
                what = "conv2d_fwd_split3p_tail";
            }
        }
        launch_trunk(v, nwg, st, p, units, nwg);
        return check_launch(what);
    }
    if (t.kind == TRUNK_HALO) {
        // one tile per workgroup, K walked as (channel chunk, tap) over one staged patch per chunk; tail tiles in K ranges
        const int units = wire_tail(p, ws, ws_bytes, T, resident_slots(HALO), TS_MAX_UNITS, true);
        launch_trunk(HALO, units, st, p);
        return check_launch("conv2d_fwd_split3p (halo)");
    }
#if defined(ACIMG_STAMP) || defined(ACIMG_ABLATE)
    p.slab = g_stamp_buf;
    p.flip = g_stamp_nostore;
#endif
    if (t.kind == TRUNK_RING) {
        // one workgroup per CU walks units blockIdx.x, blockIdx.x + P, ... (whole tiles, then K ranges of the tail tiles)
        TrunkVariant& v = t.bm == 256 ? RING_256 : RING_128;
        const int slots = resident_slots(v);
        const int units = wire_tail(p, ws, ws_bytes, T, slots, TS_MAX_UNITS * 128 / t.bm, true);
        const int nwg = std::min(units, slots);
        p.splits = g_cfg.trunk_stagger > 0 ? 2 : 1;   // ring kernel: waves 4-7 do a step's scalar work before their first MFMA group
        launch_trunk(v, nwg, st, p, units, nwg);
        return check_launch("conv2d_fwd_split3p (ring)");
    }
    if (t.kind == TRUNK_PERSISTENT) {
        TrunkVariant& v = terms == 1 ? PERSISTENT1 : g_cfg.trunk_dma_pos == 1 ? PERSISTENT_SPREAD : PERSISTENT;
        const int slots = resident_slots(v);
        const int units = wire_tail(p, ws, ws_bytes, T, slots, TS_MAX_UNITS, true);
        p.splits = g_cfg.trunk_stagger > 0 ? g_cfg.trunk_stagger * (p.kiters * 2500 + 8000) / 100 : 1;
        // a workgroup per resident slot walks units blockIdx.x, blockIdx.x + P, ...: whole tiles first (with the
        // next tile's first operand stage and addresses prepared under the current tile's last K step and output
        // stores), then the K ranges of the tail tiles
        const int nwg = std::min(units, slots);
        launch_trunk(v, nwg, st, p, units, nwg);
        return check_launch("conv2d_fwd_split3p");
    }
    // one tile (or K range of a tail tile) per workgroup
    TrunkVariant& v = t128 ? (terms == 1 ? TILE1_128x128 : TILE_128x128)
                    : t.bm == 64 ? (terms == 1 ? TILE1_64x128 : TILE_64x128) : (terms == 1 ? TILE1_128x64 : TILE_128x64);
    const int units = wire_tail(p, ws, ws_bytes, T, resident_slots(v), TS_MAX_UNITS, t128);
    launch_trunk(v, units, st, p);
    return check_launch("conv2d_fwd_split3p");
}

/* ---- tap-GEMM helpers (see the kernels above) ---- */
static int tapconv_check(const AcimgConvDesc* d, const char* who) {
    int rc = check_desc(d, who);
    if (rc) return rc;
    if (d->stride != 1 || d->pad_t || d->pad_l || d->OH != d->H - d->R + 1 || d->OW != d->W - d->S + 1)
        return fail(ACIMG_EINVAL, "%s: stride-1 VALID convolutions only", who);
    if (d->K > 64) return fail(ACIMG_EINVAL, "%s: K=%d > 64 (this form is for few output channels)", who, d->K);
    return ACIMG_OK;
}

/* weight + bias gradient on the bf16x3 MFMA path (same contract as acimg_conv2d_wgrad) */
static int wgrad_split_onthefly(const AcimgConvDesc* d, const float* x, const float* gy, int ldgy, float* dw, float* db,
                                void* ws, size_t ws_bytes, void* stream, int terms) {
    int rc = check_desc(d, "conv2d_wgrad_split3");
    if (rc) return rc;
    const int kp = up4(d->K);
    if (kp > ldgy || kp > d->ldw) return fail(ACIMG_EINVAL, "conv2d_wgrad_split3: padded K exceeds ldgy/ldw");
    WgradParams p{};
    p.X = x; p.H = d->H; p.W = d->W; p.C = d->C; p.ldx = d->ldx;
    p.OH = d->OH; p.OW = d->OW; p.R = d->R; p.S = d->S; p.stride = d->stride; p.pad_t = d->pad_t; p.pad_l = d->pad_l;
    p.M = d->N * d->OH * d->OW; p.KK = d->R * d->S * d->C;
    p.G = gy; p.ldg = ldgy; p.Ngemm = kp; p.Nld = kp; p.ldo = d->ldw;
    return launch_wgrad(p, dw, db, ws, ws_bytes, (hipStream_t)stream, true, terms);
}

}  // namespace acimg

using namespace acimg;

// ==========================================================================================
// C ABI
// ==========================================================================================
extern "C" {

int acimg_conv2d_stats_rows(const AcimgConvDesc* d) {
    if (few16_fwd_shape(d)) return FEW16_WGS;        // the few-channel MFMA kernel leaves one row per workgroup
    return cdiv((long)d->N * d->OH * d->OW, stats_block_rows(d));
}

int acimg_conv2d_fwd_tiling(const AcimgConvDesc* d, int* out) {
    if (!d || !out) return fail(ACIMG_EINVAL, "conv2d_fwd_tiling: null argument");
    const int M = d->N * d->OH * d->OW;
    TileCfg c = pick_cfg(M, d->K);
    out[0] = c.bm;
    out[1] = c.bn;
    out[2] = pick_splits(M, d->K, c, fwd_kiters(d));
    return ACIMG_OK;
}

int acimg_config_default(AcimgConfig* c) {
    if (!c) return fail(ACIMG_EINVAL, "config_default: null");
    *c = DEFAULT_CFG;
    return ACIMG_OK;
}

int acimg_configure(const AcimgConfig* c) {
    if (!c) return fail(ACIMG_EINVAL, "configure: null");
    if (c->splitk_cut < 0 || c->splitk_target < 1 || c->wgrad_minpix < 1 || c->tail_s < 0)
        return fail(ACIMG_EINVAL, "configure: negative / zero tuning value");
    if (c->trunk_persistent < 0 || c->trunk_persistent > 2) return fail(ACIMG_EINVAL, "configure: trunk_persistent is 0, 1 or 2");
    if (c->trunk_dma_pos < 0 || c->trunk_dma_pos > 1) return fail(ACIMG_EINVAL, "configure: trunk_dma_pos is 0 or 1");
    if (c->trunk_stagger < 0 || c->trunk_stagger > 100) return fail(ACIMG_EINVAL, "configure: trunk_stagger is a percentage");
    if (c->trunk_bk != 0 && c->trunk_bk != 32)
        return fail(ACIMG_EINVAL, "configure: trunk_bk must be 0 or 32 (the 64-deep K step was measured slower and removed)");
    if (c->trunk_ring < 0 || c->trunk_ring > 2) return fail(ACIMG_EINVAL, "configure: trunk_ring is 0, 1 or 2");
    if (c->trunk_ring_bm != 0 && c->trunk_ring_bm != 128 && c->trunk_ring_bm != 256)
        return fail(ACIMG_EINVAL, "configure: trunk_ring_bm must be 0 (per shape), 128 or 256");
    if (c->trunk_halo < 0 || c->trunk_halo > 2) return fail(ACIMG_EINVAL, "configure: trunk_halo is 0, 1 or 2");
    if (c->split3_tile_bm || c->split3_tile_bn) {
        const int bm = c->split3_tile_bm, bn = c->split3_tile_bn;
        if (!((bm == 128 && bn == 128) || (bm == 64 && bn == 128) || (bm == 128 && bn == 64)))
            return fail(ACIMG_EINVAL, "configure: split3 tile %dx%d is not an instantiated tile", bm, bn);
    }
    g_cfg = *c;
    return ACIMG_OK;
}

size_t acimg_conv2d_fwd_workspace(const AcimgConvDesc* d) {
    const size_t a = igemm_ws_bytes(d->N * d->OH * d->OW, d->K, fwd_kiters(d));
    const size_t b = direct_shape(d->C, d->K) ? direct_ws_bytes(d->R, d->S, d->C, (d->K + 7) & ~7) : 0;
    const size_t c = skinny_fwd_ws_bytes(d);
    const size_t f = few16_fwd_shape(d) ? few16_ws_bytes(d->C, d->K) : 0;
    return std::max(std::max(a, f), std::max(b, c));
}

int acimg_conv2d_fwd(const AcimgConvDesc* d, const float* x, const float* w, const float* bias,
                     float* y, const float* in_scale, const float* in_shift, int in_relu,
                     float* stats, void* ws, size_t ws_bytes, void* tickets, void* stream) {
    int rc = check_desc(d, "conv2d_fwd");
    if (rc) return rc;
    if (d->ldw < d->K) return fail(ACIMG_EINVAL, "conv2d_fwd: ldw < K");
    if (skinny_shape(d) && !in_scale && !in_shift && !in_relu && !stats && ws && ws_bytes >= skinny_fwd_ws_bytes(d) && aligned16(x) &&
        aligned16(w) && aligned16(y) && aligned16(ws) && (!bias || aligned16(bias)) && (d->ldw & 3) == 0 && (d->ldx & 3) == 0 &&
        (d->ldy & 3) == 0) {
        // the VAE heads' dense layer: weight rows read once in whole lines, K slabs combined in slab order
        SkinnyParams q{};
        q.W = w; q.X = x; q.out = y; q.bias = bias; q.act = d->act; q.part = static_cast<float*>(ws);
        q.M = d->N; q.C = d->C; q.N = d->K; q.ldw = d->ldw; q.ldx = d->ldx; q.ldo = d->ldy;
        q.slabs = cdiv(d->C, SKINNY_KS);
        const dim3 grid(q.slabs, cdiv(d->K, 64));
        const int mb = cdiv(d->N, 16);
        if (mb == 1) hipLaunchKernelGGL(skinny_fwd_kernel<1>, grid, dim3(64), 0, (hipStream_t)stream, q);
        else if (mb == 2) hipLaunchKernelGGL(skinny_fwd_kernel<2>, grid, dim3(64), 0, (hipStream_t)stream, q);
        else if (mb == 3) hipLaunchKernelGGL(skinny_fwd_kernel<3>, grid, dim3(64), 0, (hipStream_t)stream, q);
        else hipLaunchKernelGGL(skinny_fwd_kernel<4>, grid, dim3(64), 0, (hipStream_t)stream, q);
        rc = check_launch("conv2d_fwd (skinny)");
        if (rc) return rc;
        hipLaunchKernelGGL(skinny_fwd_reduce_kernel, dim3(cdiv(d->N * (d->K / 4), 256)), dim3(256), 0, (hipStream_t)stream, q);
        return check_launch("conv2d_fwd (skinny reduce)");
    }
    if (few16_fwd_shape(d)) {
        // acimg_conv2d_stats_rows(d) promised one statistics row per workgroup of this kernel: no silent fallback
        if ((in_scale != nullptr) != (in_shift != nullptr) || (in_relu && !in_scale) || !aligned16(x) || !aligned16(y) || (d->ldy & 3) ||
            d->ldy < d->K || (bias && !aligned16(bias)) || (in_scale && (!aligned16(in_scale) || !aligned16(in_shift))))
            return fail(ACIMG_EINVAL, "conv2d_fwd: few-channel MFMA shape with half an input affine or unaligned operands");
        FewParams q{};
        q.a_scale = in_scale; q.a_shift = in_shift; q.a_relu = in_relu;
        q.X = x; q.H = d->H; q.W = d->W; q.ldx = d->ldx; q.Y = y; q.ldy = d->ldy; q.nout = d->K; q.bias = bias;
        q.Hin = q.SH = d->H; q.Win = q.SW = d->W; q.dil = 1; q.pad_t = 1; q.pad_l = 1;
        q.stats = stats; q.stats_ld = d->ldw;
        q.w = w; q.ldw = d->ldw; q.wrows = d->C; q.cin = d->C; q.mode = 0;
        return dispatch_few16<0>(q, d->N, d->C, d->K, ws, ws_bytes, (hipStream_t)stream);
    }
    if (direct_ok(d->C, d->K, d->ldy, 0, y, bias, nullptr, in_scale != nullptr, nullptr) &&
        (long)d->N * d->OH * d->OW >= 65536) {
        DirectParams q{};
        q.x = x; q.ldx = d->ldx; q.H = d->H; q.W = d->W; q.C = d->C;
        q.y = y; q.ldy = d->ldy; q.OH = d->OH; q.OW = d->OW; q.K = d->K;
        q.R = d->R; q.S = d->S; q.stride = d->stride; q.pad_t = d->pad_t; q.pad_l = d->pad_l;
        q.w = w; q.ldw = d->ldw; q.mode = 0; q.wrows = d->C; q.bias = bias; q.act = d->act;
        q.M = (long)d->N * d->OH * d->OW;
        const bool fuse_stats = stats && stats_block_rows(d) == 256 && d->act == ACIMG_ACT_NONE;
        if (fuse_stats) { q.stats = stats; q.stats_ld = d->ldw; }
        rc = launch_direct(q, ws, ws_bytes, (hipStream_t)stream);
        if (!rc && stats && !fuse_stats) {   // batch-norm partials of y = conv + bias, in acimg_conv2d_stats_rows(d) row blocks
            hipLaunchKernelGGL(partial_stats_kernel, dim3(acimg_conv2d_stats_rows(d)), dim3(256), 0, (hipStream_t)stream,
                               y, d->ldy, (int)q.M, d->K, stats, d->ldw, stats_block_rows(d));
            rc = check_launch("partial_stats");
        }
        return rc;
    }
    IgemmParams p = fwd_view(d);
    p.A = x; p.rowrun = (d->S > 1 && d->ldx == d->C) ? 1 : 0;
    p.a_scale = in_scale; p.a_shift = in_shift; p.a_relu = in_relu;
    p.B = w; p.ldb = d->ldw;
    p.e.Y = y; p.e.bias = bias; p.e.stats = stats;
    return launch_igemm(p, false, ws, ws_bytes, tickets, (hipStream_t)stream);
}

size_t acimg_conv2d_dgrad_workspace(const AcimgConvDesc* d) {
    if (dgrad_halo16_narrow_shape(d)) return DGRAD_HALO16_NARROW_WS + 256;
    if (dgrad_is_patch(d)) return igemm_ws_bytes(d->N * d->OH * d->OW, d->R * d->S * d->C, cdiv(up4(d->K), 32));
    const int ca = up4(d->K);
    if (subpixel_ok(d->stride, d->C, ca))   // sub-pixel form: combined weights + the GEMM's own split-K slabs
        return subpixel_ws_bytes(d->N, d->H, d->W, -d->pad_t, -d->pad_l, d->R, d->S, ca, d->C);
    if (d->stride > 1)   // zero-inserted copy of gy, then the stride-1 path
        return dilated_bytes(d->N, d->OH, d->OW, ca, d->stride) +
               igemm_ws_bytes(d->N * d->H * d->W, d->C, d->R * d->S * cdiv(ca, 32)) +
               igemm_ws_bytes(d->N * d->H * d->W, d->C, d->R * cdiv(d->S * ca, 32)) +
               (direct_shape(ca, d->C) ? std::max(direct_ws_bytes(d->R, d->S, ca, (d->C + 7) & ~7), few16_ws_bytes(ca, d->C)) : 0);
    // rowrun depends on ldgy, unknown here: per-tap kiters is the larger bound for splits
    return igemm_ws_bytes(d->N * d->H * d->W, d->C, d->R * d->S * cdiv(ca, 32)) +
           igemm_ws_bytes(d->N * d->H * d->W, d->C, d->R * cdiv(d->S * ca, 32)) +
           (direct_shape(ca, d->C) ? std::max(direct_ws_bytes(d->R, d->S, ca, (d->C + 7) & ~7), few16_ws_bytes(ca, d->C)) : 0);
}

int acimg_conv2d_dgrad(const AcimgConvDesc* d, const float* gy, int ldgy, const float* w,
                       float* dx, int lddx, const float* residual, int ldres, const float* mask,
                       int ldmask, void* ws, size_t ws_bytes, void* tickets, void* stream) {
    int rc = check_desc(d, "conv2d_dgrad");
    if (rc) return rc;
    const int ca = up4(d->K);
    if (ca > ldgy || ca > d->ldw || (ldgy & 3)) return fail(ACIMG_EINVAL, "conv2d_dgrad: padded K=%d exceeds ldgy=%d/ldw=%d", ca, ldgy, d->ldw);
    if (skinny_shape(d) && aligned16(gy) && aligned16(w) && (d->ldw & 3) == 0) {
        // a dense layer over a few batch rows (the 28 416 -> 300 VAE heads): the weight matrix is read once, in rows
        SkinnyParams q{};
        q.W = w; q.G = gy; q.out = dx; q.res = residual; q.mask = mask;
        q.M = d->N; q.C = d->C; q.N = ca;
        q.ldw = d->ldw; q.ldg = ldgy; q.ldo = lddx > 0 ? lddx : d->ldx; q.ldres = ldres; q.ldmask = ldmask;
        if (q.ldo < d->C) return fail(ACIMG_EINVAL, "conv2d_dgrad: lddx < C");
        const dim3 grid(cdiv(cdiv(d->C, 16), 4));
        const int mb = cdiv(d->N, 16);
        if (mb == 1) hipLaunchKernelGGL(skinny_dgrad_kernel<1>, grid, dim3(256), 0, (hipStream_t)stream, q);
        else if (mb == 2) hipLaunchKernelGGL(skinny_dgrad_kernel<2>, grid, dim3(256), 0, (hipStream_t)stream, q);
        else if (mb == 3) hipLaunchKernelGGL(skinny_dgrad_kernel<3>, grid, dim3(256), 0, (hipStream_t)stream, q);
        else hipLaunchKernelGGL(skinny_dgrad_kernel<4>, grid, dim3(256), 0, (hipStream_t)stream, q);
        return check_launch("conv2d_dgrad (skinny)");
    }
    if (lddx <= 0) lddx = d->ldx;
    if (lddx < d->C) return fail(ACIMG_EINVAL, "conv2d_dgrad: lddx < C");
    if (subpixel_ok(d->stride, d->C, ca) && !dgrad_is_patch(d))
        // dx[2 oy - pad_t + r][2 ox - pad_l + s][c] += gy[oy][ox][k] w[r][s][c][k]: the sub-pixel form over gy's own grid
        return launch_subpixel(gy, d->N, d->OH, d->OW, ca, ldgy, w, d->R, d->S, d->ldw, d->C, dx, lddx, d->H, d->W, -d->pad_t,
                               -d->pad_l, nullptr, residual, ldres, mask, ldmask, ACIMG_ACT_NONE, ws, ws_bytes, tickets,
                               (hipStream_t)stream, "conv2d_dgrad");
    if (dgrad_halo16_narrow_shape(d) && aligned16(gy) && aligned16(dx) && (lddx & 3) == 0 && ws && aligned16(ws) &&
        ws_bytes >= DGRAD_HALO16_NARROW_WS && (!residual || ((ldres & 3) == 0 && aligned16(residual))) &&
        (!mask || ((ldmask & 3) == 0 && aligned16(mask))))
        return dgrad_halo16_narrow(d, gy, ldgy, w, dx, lddx, residual, ldres, mask, ldmask, ws, (hipStream_t)stream);
    if (few16_dgrad_shape(d) && !subpixel_ok(d->stride, d->C, ca) && !mask && aligned16(gy) && aligned16(dx) && (lddx & 3) == 0 &&
        ws && aligned16(ws) && ws_bytes >= few16_ws_bytes(ca, d->C) && (!residual || ((ldres & 3) == 0 && aligned16(residual)))) {
        // dx[h][w][c] = sum gy1[h - (2 - pad_t) + r'][w - (2 - pad_l) + s'][k] W[2 - r'][2 - s'][c][k], gy1 = gy (stride 1) or
        // its zero-inserted view (stride 2), zero outside
        FewParams q{};
        q.X = gy; q.ldx = ldgy; q.SH = d->OH; q.SW = d->OW; q.dil = d->stride;
        q.Hin = (d->OH - 1) * d->stride + 1; q.Win = (d->OW - 1) * d->stride + 1;
        q.pad_t = 2 - d->pad_t; q.pad_l = 2 - d->pad_l;
        q.H = d->H; q.W = d->W; q.Y = dx; q.ldy = lddx; q.nout = d->C;
        q.res = residual; q.ldres = ldres;
        q.w = w; q.ldw = d->ldw; q.wrows = d->C; q.cin = d->K; q.mode = 1;
        return dispatch_few16<1>(q, d->N, ca, d->C, ws, ws_bytes, (hipStream_t)stream);
    }
    if (d->stride > 1 && !dgrad_is_patch(d)) {
        // general stride: the strided conv is a subsampled stride-1 conv, so its data gradient is the stride-1
        // data gradient of the zero-inserted gy
        const size_t db = dilated_bytes(d->N, d->OH, d->OW, ca, d->stride);
        if (ws_bytes < db || !ws) return fail(ACIMG_EWORKSPACE, "conv2d_dgrad: workspace too small for the dilated gradient");
        const int OH1 = (d->OH - 1) * d->stride + 1, OW1 = (d->OW - 1) * d->stride + 1;
        const long opix = (long)d->N * OH1 * OW1;
        if (opix * ca >= (1L << 31)) return fail(ACIMG_EINVAL, "conv2d_dgrad: dilated gradient exceeds 2^31 elements");
        hipLaunchKernelGGL(dilate2d_kernel, dim3(cdiv(opix * (ca / 4), 256)), dim3(256), 0, (hipStream_t)stream, gy, ldgy,
                           static_cast<float*>(ws), opix, d->OH, d->OW, OH1, OW1, ca, d->stride);
        rc = check_launch("dilate2d");
        if (rc) return rc;
        AcimgConvDesc d1 = *d;
        d1.stride = 1; d1.OH = OH1; d1.OW = OW1;
        return acimg_conv2d_dgrad(&d1, static_cast<const float*>(ws), ca, w, dx, lddx, residual, ldres, mask, ldmask,
                                  static_cast<char*>(ws) + db, ws_bytes - db, tickets, stream);
    }
    if (d->stride == 1 && direct_ok(ca, d->C, lddx, ldres, dx, nullptr, residual, false, mask) &&
        (long)d->N * d->H * d->W >= 65536) {
        DirectParams q{};
        q.x = gy; q.ldx = ldgy; q.H = d->OH; q.W = d->OW; q.C = ca;
        q.y = dx; q.ldy = lddx; q.OH = d->H; q.OW = d->W; q.K = d->C;
        q.R = d->R; q.S = d->S; q.stride = 1; q.pad_t = d->R - 1 - d->pad_t; q.pad_l = d->S - 1 - d->pad_l;
        q.w = w; q.ldw = d->ldw; q.mode = 1; q.wrows = d->C; q.act = ACIMG_ACT_NONE;
        q.res = residual; q.ldres = ldres;
        q.M = (long)d->N * d->H * d->W;
        return launch_direct(q, ws, ws_bytes, (hipStream_t)stream);
    }
    IgemmParams p{};
    if (d->stride == 1) {
        p = flipped_view(d, ca, ldgy);
        p.rowrun = (d->S > 1 && ldgy == ca) ? 1 : 0;
        p.tap_stride = (long)d->C * d->ldw; p.flip = 1;
    } else {
        // patch scatter: rows = output pixels, columns = (tap, c)
        p.H = d->OH; p.W = d->OW; p.C = ca; p.lda = ldgy; p.OH = d->OH; p.OW = d->OW;
        p.R = 1; p.S = 1; p.stride = 1;
        p.M = d->N * d->OH * d->OW;
        p.Ngemm = d->R * d->S * d->C;
        p.e.M = p.M; p.e.Nstore = p.Ngemm; p.e.act = ACIMG_ACT_NONE;
        p.e.scatter = 1; p.e.Ko = d->C; p.e.Sq = d->S; p.e.sc = d->stride;
        p.e.YH = d->H; p.e.YW = d->W; p.e.AH = d->OH; p.e.AW = d->OW;
    }
    p.A = gy; p.B = w; p.ldb = d->ldw;
    p.e.Y = dx; p.e.ldy = lddx; p.e.res = residual; p.e.ldres = ldres; p.e.mask = mask; p.e.ldmask = ldmask;
    return launch_igemm(p, true, ws, ws_bytes, tickets, (hipStream_t)stream);
}

size_t acimg_conv2d_wgrad_workspace(const AcimgConvDesc* d) {
    return wgrad_ws_bytes(d->N * d->OH * d->OW, d->R * d->S * d->C, up4(d->K), d->ldw) + colsum_ws_bytes(up4(d->K));
}

int acimg_conv2d_wgrad(const AcimgConvDesc* d, const float* x, const float* gy, int ldgy,
                       float* dw, float* db, void* ws, size_t ws_bytes, void* stream) {
    int rc = check_desc(d, "conv2d_wgrad");
    if (rc) return rc;
    const int kp = up4(d->K);
    if (kp > ldgy || kp > d->ldw) return fail(ACIMG_EINVAL, "conv2d_wgrad: padded K exceeds ldgy/ldw");
    if (skinny_shape(d) && aligned16(x) && aligned16(gy) && aligned16(dw) && (!db || aligned16(db)) && (d->ldw & 3) == 0 &&
        (ldgy & 3) == 0 && (d->ldx & 3) == 0) {
        // the same dense layer's weight gradient: every weight row is written once, 256 contiguous bytes per wave
        SkinnyParams q{};
        q.X = x; q.G = gy; q.out = dw; q.db = db;
        q.M = d->N; q.C = d->C; q.N = kp;
        q.ldw = d->ldw; q.ldg = ldgy; q.ldx = d->ldx;
        const int ngroups = cdiv(kp, 64);
        const int tasks = cdiv(d->C, 64) * ngroups;
        hipLaunchKernelGGL(skinny_wgrad_kernel, dim3(cdiv(tasks, 4)), dim3(256), 0, (hipStream_t)stream, q, ngroups);
        return check_launch("conv2d_wgrad (skinny)");
    }
    WgradParams p{};
    p.X = x; p.H = d->H; p.W = d->W; p.C = d->C; p.ldx = d->ldx;
    p.OH = d->OH; p.OW = d->OW; p.R = d->R; p.S = d->S; p.stride = d->stride; p.pad_t = d->pad_t; p.pad_l = d->pad_l;
    p.M = d->N * d->OH * d->OW; p.KK = d->R * d->S * d->C;
    p.G = gy; p.ldg = ldgy; p.Ngemm = kp; p.Nld = kp; p.ldo = d->ldw;
    return launch_wgrad(p, dw, db, ws, ws_bytes, (hipStream_t)stream);
}

size_t acimg_deconv_workspace(const AcimgConvDesc* d) {
    size_t a = igemm_ws_bytes(d->N * d->H * d->W, d->R * d->S * d->K, cdiv(d->C, 32));
    size_t b = igemm_ws_bytes(d->N * d->H * d->W, d->C, d->R * d->S * cdiv(up4(d->K), 32));
    size_t c = wgrad_ws_bytes(d->N * d->H * d->W, d->R * d->S * up4(d->K), d->C, d->ldw) + colsum_ws_bytes(up4(d->K));
    size_t m = a > b ? a : b;
    m = m > c ? m : c;
    if (patch2_shape(d)) {                      // weight gradient of the pointwise form: one 32 x ldw slab per workgroup
        const size_t pw = (size_t)PATCH2_WGRAD_WGS * (32 * d->ldw + 8) * sizeof(float);
        m = m > pw ? m : pw;
    }
    if (direct_shape(up4(d->K), d->C)) {        // data gradient on the direct few-channel kernel
        const size_t dd = direct_ws_bytes(d->R, d->S, up4(d->K), (d->C + 7) & ~7);
        m = m > dd ? m : dd;
    }
    if ((d->R > d->stride || d->S > d->stride) && subpixel_ok(d->stride, d->K, d->C)) {   // forward in the sub-pixel form
        const size_t sp = subpixel_ws_bytes(d->N, d->OH, d->OW, 0, 0, d->R, d->S, d->C, d->K);
        return m > sp ? m : sp;
    }
    if (d->R > d->stride || d->S > d->stride)   // forward goes through a zero-inserted copy of x
        m += dilated_bytes(d->N, d->H, d->W, d->C, d->stride) +
             igemm_ws_bytes(d->N * d->OH * d->OW, d->K, d->R * d->S * cdiv(d->C, 32)) +
             igemm_ws_bytes(d->N * d->OH * d->OW, d->K, d->R * cdiv(d->S * d->C, 32));
    return m;
}

int acimg_deconv_fwd(const AcimgConvDesc* d, const float* x, const float* w, const float* bias,
                     float* y, void* ws, size_t ws_bytes, void* tickets, void* stream) {
    int rc = check_desc(d, "deconv_fwd");
    if (rc) return rc;
    if (d->ldw < d->C || (d->K & 3)) return fail(ACIMG_EINVAL, "deconv_fwd: ldw<C or K%%4");
    if (d->R > d->stride || d->S > d->stride) {
        // overlapping patches (tf conv2d_transpose VALID: OH = (H-1)*stride + R): y = stride-1 "full" correlation
        // of the zero-inserted x with the flipped kernel = the data gradient of the stride-1 VALID conv
        // [OH,OW,K] -> [(H-1)s+1, (W-1)s+1, C] whose HWIO kernel is this layer's [R][S][K][C]
        if (d->OH != (d->H - 1) * d->stride + d->R || d->OW != (d->W - 1) * d->stride + d->S)
            return fail(ACIMG_EINVAL, "deconv_fwd: kernel>stride needs OH=(H-1)*stride+R");
        if (subpixel_ok(d->stride, d->K, d->C))
            // y[2 h + r][2 w + s][k] += x[h][w][c] W[r][s][k][c]: the sub-pixel form over x's own grid (every output
            // pixel belongs to exactly one parity class: written once, bias included)
            return launch_subpixel(x, d->N, d->H, d->W, d->C, d->ldx, w, d->R, d->S, d->ldw, d->K, y, d->ldy, d->OH, d->OW, 0, 0,
                                   bias, nullptr, 0, nullptr, 0, d->act, ws, ws_bytes, tickets, (hipStream_t)stream,
                                   "deconv_fwd");
        const size_t db = dilated_bytes(d->N, d->H, d->W, d->C, d->stride);
        if (ws_bytes < db || !ws) return fail(ACIMG_EWORKSPACE, "deconv_fwd: workspace too small for the dilated input");
        const int H1 = (d->H - 1) * d->stride + 1, W1 = (d->W - 1) * d->stride + 1;
        const long opix = (long)d->N * H1 * W1;
        hipLaunchKernelGGL(dilate2d_kernel, dim3(cdiv(opix * (d->C / 4), 256)), dim3(256), 0, (hipStream_t)stream, x, d->ldx,
                           static_cast<float*>(ws), opix, d->H, d->W, H1, W1, d->C, d->stride);
        rc = check_launch("dilate2d");
        if (rc) return rc;
        IgemmParams p = flipped_view(d->N, H1, W1, d->C, d->C, d->OH, d->OW, d->R, d->S, 0, 0, d->K);
        p.A = static_cast<const float*>(ws); p.B = w; p.ldb = d->ldw;
        p.rowrun = d->S > 1 ? 1 : 0;
        p.tap_stride = (long)d->K * d->ldw; p.flip = 1;
        p.e.Y = y; p.e.ldy = d->ldy; p.e.bias = bias; p.e.act = d->act;
        return launch_igemm(p, true, static_cast<char*>(ws) + db, ws_bytes - db, tickets, (hipStream_t)stream);
    }
    if (d->OH != d->H * d->stride || d->OW != d->W * d->stride)
        return fail(ACIMG_EINVAL, "deconv_fwd: kernel<=stride needs OH=H*stride");
    if (patch2_shape(d) && aligned16(x) && aligned16(y) && aligned16(w) && (d->ldx & 3) == 0 && (d->ldy & 3) == 0 && (d->ldw & 3) == 0 &&
        (!bias || aligned16(bias))) {
        Patch2Params q{};
        q.X = x; q.ldx = d->ldx; q.Y = y; q.ldy = d->ldy; q.w = w; q.ldw = d->ldw; q.bias = bias; q.act = d->act;
        q.H = d->H; q.W = d->W; q.pixels = (long)d->N * d->H * d->W;
        return launch_patch2<SplitF16, 0>(q, (hipStream_t)stream);
    }
    IgemmParams p{};
    p.A = x; p.H = d->H; p.W = d->W; p.C = d->C; p.lda = d->ldx; p.OH = d->H; p.OW = d->W;
    p.R = 1; p.S = 1; p.stride = 1; p.M = d->N * d->H * d->W; p.rowrun = 0;
    p.B = w; p.ldb = d->ldw; p.tap_stride = 0; p.flip = 0; p.Ngemm = d->R * d->S * d->K;
    p.e.Y = y; p.e.ldy = d->ldy; p.e.M = p.M; p.e.Nstore = p.Ngemm; p.e.bias = bias; p.e.act = d->act;
    p.e.scatter = 1; p.e.Ko = d->K; p.e.Sq = d->S; p.e.sc = d->stride;
    p.e.YH = d->OH; p.e.YW = d->OW; p.e.AH = d->H; p.e.AW = d->W;
    rc = launch_igemm(p, true, ws, ws_bytes, tickets, (hipStream_t)stream);
    if (rc) return rc;
    if (d->R < d->stride || d->S < d->stride) {
        const long pixels = (long)d->N * d->OH * d->OW;
        hipLaunchKernelGGL(deconv_gap_fill_kernel, dim3(cdiv(pixels * (d->K / 4), 256)), dim3(256), 0,
                           (hipStream_t)stream, y, d->ldy, bias, pixels, d->OH, d->OW, d->K, d->R, d->S, d->stride);
        rc = check_launch("deconv_gap_fill");
    }
    return rc;
}

int acimg_deconv_dgrad(const AcimgConvDesc* d, const float* gy, int ldgy, const float* w,
                       float* dx, const float* mask, int ldmask, void* ws, size_t ws_bytes,
                       void* tickets, void* stream) {
    int rc = check_desc(d, "deconv_dgrad");
    if (rc) return rc;
    const int ca = up4(d->K);
    if (ca > ldgy || (ldgy & 3) || ca != d->K) return fail(ACIMG_EINVAL, "deconv_dgrad: K must be a multiple of 4 and <= ldgy");
    // dx[n,h,w,c] = sum_{r,s,k} gy[n, h*stride+r, w*stride+s, k] * W[r][s][k][c]  (a strided conv)
    if (patch2_shape(d) && aligned16(gy) && aligned16(dx) && aligned16(w) && (d->ldx & 3) == 0 && (d->ldw & 3) == 0 &&
        (!mask || (aligned16(mask) && (ldmask & 3) == 0))) {
        Patch2Params q{};
        q.X = gy; q.ldx = ldgy; q.Y = dx; q.ldy = d->ldx; q.w = w; q.ldw = d->ldw; q.mask = mask; q.ldmask = ldmask;
        q.H = d->H; q.W = d->W; q.pixels = (long)d->N * d->H * d->W;
        return launch_patch2<SplitBF16, 1>(q, (hipStream_t)stream);
    }
    if (!mask && direct_ok(ca, d->C, d->ldx, 0, dx, nullptr, nullptr, false, nullptr) &&
        (long)d->N * d->H * d->W >= 65536) {
        // few channels: the direct kernel, the [kh][kw][out][in] kernel read as the HWIO kernel of that conv
        DirectParams q{};
        q.x = gy; q.ldx = ldgy; q.H = d->OH; q.W = d->OW; q.C = ca;
        q.y = dx; q.ldy = d->ldx; q.OH = d->H; q.OW = d->W; q.K = d->C;
        q.R = d->R; q.S = d->S; q.stride = d->stride; q.pad_t = 0; q.pad_l = 0;
        q.w = w; q.ldw = d->ldw; q.mode = 0; q.wrows = d->K; q.act = ACIMG_ACT_NONE;
        q.M = (long)d->N * d->H * d->W;
        return launch_direct(q, ws, ws_bytes, (hipStream_t)stream);
    }
    IgemmParams p{};
    p.A = gy; p.H = d->OH; p.W = d->OW; p.C = ca; p.lda = ldgy; p.OH = d->H; p.OW = d->W;
    p.R = d->R; p.S = d->S; p.stride = d->stride; p.pad_t = 0; p.pad_l = 0;
    p.M = d->N * d->H * d->W;
    p.rowrun = (d->S > 1 && ldgy == ca) ? 1 : 0;
    p.B = w; p.ldb = d->ldw; p.Nld = d->ldw; p.Ngemm = d->C;
    p.e.Y = dx; p.e.ldy = d->ldx; p.e.M = p.M; p.e.Nstore = d->C; p.e.mask = mask; p.e.ldmask = ldmask;
    return launch_igemm(p, false, ws, ws_bytes, tickets, (hipStream_t)stream);
}

int acimg_deconv_wgrad(const AcimgConvDesc* d, const float* x, const float* gy, int ldgy,
                       float* dw, float* db, void* ws, size_t ws_bytes, void* stream) {
    int rc = check_desc(d, "deconv_wgrad");
    if (rc) return rc;
    const int ca = up4(d->K);
    if (ca > ldgy || (ldgy & 3) || ca != d->K) return fail(ACIMG_EINVAL, "deconv_wgrad: K must be a multiple of 4 and <= ldgy");
    // dW[(r,s,k)][c] = sum_{n,h,w} gy[n,h*stride+r,w*stride+s,k] * x[n,h,w,c]
    if (patch2_shape(d) && aligned16(dw) && (d->ldw & 3) == 0 && ws && aligned16(ws) &&
        ws_bytes >= (size_t)PATCH2_WGRAD_WGS * (32 * d->ldw + 8) * sizeof(float) && (!db || aligned16(db))) {
        Patch2WgradParams q{};
        q.X = x; q.ldx = d->ldx; q.G = gy; q.ldg = ldgy; q.out = static_cast<float*>(ws); q.ldo = d->ldw;
        q.db_part = db ? q.out + (size_t)PATCH2_WGRAD_WGS * 32 * d->ldw : nullptr;
        q.H = d->H; q.W = d->W; q.pixels = (long)d->N * d->H * d->W;
        hipLaunchKernelGGL(patch2_wgrad_32x8_kernel, dim3(PATCH2_WGRAD_WGS), dim3(1024), 0, (hipStream_t)stream, q);
        rc = check_launch("patch2_wgrad");
        if (rc) return rc;
        launch_slab_reduce_wide(q.out, PATCH2_WGRAD_WGS, 32L, 32, d->ldw, dw, nullptr, nullptr, (hipStream_t)stream);
        rc = check_launch("patch2_wgrad reduce");
        if (rc) return rc;
        // the transposed conv adds its bias at every output pixel, and every output pixel belongs to exactly one patch: the
        // bias gradient is the sum of all the gy values the kernel has just read
        if (db) {
            hipLaunchKernelGGL(colsum_final_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, q.db_part, PATCH2_WGRAD_WGS, 8, db);
            rc = check_launch("patch2_wgrad bias");
        }
        return rc;
    }
    WgradParams p{};
    p.X = gy; p.H = d->OH; p.W = d->OW; p.C = ca; p.ldx = ldgy;
    p.OH = d->H; p.OW = d->W; p.R = d->R; p.S = d->S; p.stride = d->stride; p.pad_t = 0; p.pad_l = 0;
    p.M = d->N * d->H * d->W; p.KK = d->R * d->S * ca;
    p.G = x; p.ldg = d->ldx; p.Ngemm = d->C; p.Nld = d->C; p.ldo = d->ldw;
    if (db) {       // refuse before dw is written: an unsplit weight gradient takes no workspace, the column sum always does
        const size_t need = (size_t)colsum_parts((long)d->N * d->OH * d->OW) * d->K * sizeof(float);
        if (ws == nullptr || ws_bytes < need) return fail(ACIMG_EWORKSPACE, "deconv_wgrad: workspace %zu < %zu (bias gradient)", ws_bytes, need);
    }
    rc = launch_wgrad(p, dw, nullptr, ws, ws_bytes, (hipStream_t)stream);
    if (rc) return rc;
    // the transposed conv adds its bias at EVERY output pixel (gaps included): plain column sum of gy
    if (db) rc = launch_colsum(gy, (long)d->N * d->OH * d->OW, d->K, ldgy, db, ws, ws_bytes, (hipStream_t)stream);
    return rc;
}

int acimg_conv2d_fwd_split3_stats_rows(const AcimgConvDesc* d) {
    const int M = d->N * d->OH * d->OW;
    if (conv_halo16_fwd_shape(d)) return CONV_HALO16_WGS;      // the halo form leaves one row per workgroup
    return cdiv(M, pick_split3(M, d->K).bm);
}

int acimg_conv2d_fwd_split3p_stats_rows(const AcimgConvDesc* d) { return pick_trunk(d, 3, false).stats_rows; }

int acimg_conv2d_fwd_split3_tiling(const AcimgConvDesc* d, int* out) {
    if (!d || !out) return fail(ACIMG_EINVAL, "conv2d_fwd_split3_tiling: null argument");
    const TrunkPick t = pick_trunk(d, 3, false);
    out[0] = t.bm;
    out[1] = t.bn;
    out[2] = t.kind;
    return ACIMG_OK;
}

size_t acimg_conv2d_split3_weight_bytes(const AcimgConvDesc* d) {
    return split3_rowmajor_bytes(d) + split3_brick_bytes(d);
}

int acimg_conv2d_split3_prepare(const AcimgConvDesc* d, const float* w, void* wsplit, void* stream) {
    int rc = check_desc(d, "conv2d_split3_prepare", true);
    if (rc) return rc;
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
    if (rc) return rc;
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
    if (rc) return rc;
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

size_t acimg_conv2d_fwd_split3p_workspace(const AcimgConvDesc* d) {
    (void)d;
    return TS_WS_BYTES;
}

#if defined(ACIMG_STAMP) || defined(ACIMG_ABLATE)
int acimg_debug_stamp_buffer(void* buf) {
    g_stamp_buf = static_cast<float*>(buf);
    return 0;
}
int acimg_debug_no_output_stores(int on) {
    g_stamp_nostore = on;
    return 0;
}
#endif

int acimg_conv2d_fwd_split3p(const AcimgConvDesc* d, const void* x_planes, size_t x_lo_off, const void* wsplit,
                             float* y, float* stats, void* ws, size_t ws_bytes, void* stream) {
    return fwd_presplit(d, x_planes, x_lo_off, wsplit, y, stats, ws, ws_bytes, stream, 3);
}

int acimg_conv2d_fwd_split1p(const AcimgConvDesc* d, const void* x_planes, size_t x_lo_off, const void* wsplit,
                             float* y, float* stats, void* ws, size_t ws_bytes, void* stream) {
    return fwd_presplit(d, x_planes, x_lo_off, wsplit, y, stats, ws, ws_bytes, stream, 1);
}

int acimg_conv2d_fwd_split3p_stats(const AcimgConvDesc* d, const void* x_planes, size_t x_lo_off, const void* wsplit,
                                   float* stats, void* ws, size_t ws_bytes, void* stream) {
    if (!stats) return fail(ACIMG_EINVAL, "conv2d_fwd_split3p_stats: null statistics buffer");
    const Split3pTail t{1, nullptr, nullptr, nullptr, 0, nullptr, 0, nullptr, nullptr};
    return fwd_presplit(d, x_planes, x_lo_off, wsplit, nullptr, stats, ws, ws_bytes, stream, 3, &t);
}

int acimg_conv2d_fwd_split3p_tail(const AcimgConvDesc* d, const void* x_planes, size_t x_lo_off, const void* wsplit,
                                  const float* scale, const float* shift, const void* sc_planes, size_t sc_lo_off,
                                  void* out_planes, size_t out_lo_off, void* ws, size_t ws_bytes, void* stream) {
    if (!scale || !shift || !sc_planes || !out_planes || !aligned16(scale) || !aligned16(shift))
        return fail(ACIMG_EINVAL, "conv2d_fwd_split3p_tail: null / unaligned scale, shift, shortcut or output");
    const Split3pTail t{2, scale, shift, sc_planes, sc_lo_off, out_planes, out_lo_off, nullptr, nullptr};
    return fwd_presplit(d, x_planes, x_lo_off, wsplit, nullptr, nullptr, ws, ws_bytes, stream, 3, &t);
}

int acimg_conv2d_fwd_split3p_tail_proj(const AcimgConvDesc* d, const void* x_planes, size_t x_lo_off, const void* wsplit,
                                       const float* scale, const float* shift, const float* sc32, const float* sc_scale,
                                       const float* sc_shift, void* out_planes, size_t out_lo_off, void* ws, size_t ws_bytes,
                                       void* stream) {
    if (!scale || !shift || !sc32 || !sc_scale || !sc_shift || !out_planes || !aligned16(scale) || !aligned16(shift) ||
        !aligned16(sc_scale) || !aligned16(sc_shift))
        return fail(ACIMG_EINVAL, "conv2d_fwd_split3p_tail_proj: null / unaligned scale, shift, shortcut or output");
    const Split3pTail t{3, scale, shift, sc32, 0, out_planes, out_lo_off, sc_scale, sc_shift};
    return fwd_presplit(d, x_planes, x_lo_off, wsplit, nullptr, nullptr, ws, ws_bytes, stream, 3, &t);
}

int acimg_tapconv_stats_rows(const AcimgConvDesc* d) { return cdiv(d->N * d->OH * d->OW, TG_PPB); }

int acimg_tapconv_pack(const AcimgConvDesc* d, const float* w, float* wt, int ldwt, void* stream) {
    int rc = tapconv_check(d, "tapconv_pack");
    if (rc) return rc;
    const int TK = d->R * d->S * d->K;
    if (!w || !wt || ldwt < TK) return fail(ACIMG_EINVAL, "tapconv_pack: null pointer or ldwt < R*S*K");
    hipLaunchKernelGGL(tapconv_pack_kernel, dim3(cdiv((long)d->C * TK, 256)), dim3(256), 0, (hipStream_t)stream, w,
                       d->R * d->S, d->C, d->K, d->ldw, wt, ldwt);
    return check_launch("tapconv_pack");
}

int acimg_tapconv_unpack(const AcimgConvDesc* d, const float* dwt, int ldwt, const float* w, float decay, float* dw,
                         void* stream) {
    int rc = tapconv_check(d, "tapconv_unpack");
    if (rc) return rc;
    const int TK = d->R * d->S * d->K;
    if (!dwt || !dw || ldwt < TK) return fail(ACIMG_EINVAL, "tapconv_unpack: null pointer or ldwt < R*S*K");
    hipLaunchKernelGGL(tapconv_unpack_kernel, dim3(cdiv((long)d->R * d->S * d->C * d->K, 256)), dim3(256), 0,
                       (hipStream_t)stream, dwt, ldwt, d->R * d->S, d->C, d->K, d->ldw, w, decay, dw);
    return check_launch("tapconv_unpack");
}

int acimg_tapconv_gather(const AcimgConvDesc* d, const float* z, int ldz, float* y, float* stats, void* stream) {
    int rc = tapconv_check(d, "tapconv_gather");
    if (rc) return rc;
    const int TK = d->R * d->S * d->K;
    if (!z || !y || ldz < TK || d->ldy < d->K) return fail(ACIMG_EINVAL, "tapconv_gather: null pointer or ldz < R*S*K");
    const long Mout = (long)d->N * d->OH * d->OW;
    hipLaunchKernelGGL(tapconv_gather_kernel, dim3(cdiv(Mout, TG_PPB)), dim3(256), (size_t)TG_PPB * d->K * 4,
                       (hipStream_t)stream, z, ldz, d->H, d->W, d->R, d->S, d->K, d->OH, d->OW, Mout, y, d->ldy, stats,
                       d->ldw);
    return check_launch("tapconv_gather");
}

int acimg_tapconv_scatter(const AcimgConvDesc* d, const float* gy, int ldgy, float* gz, int ldgz, void* stream) {
    int rc = tapconv_check(d, "tapconv_scatter");
    if (rc) return rc;
    const int TK = d->R * d->S * d->K;
    if (!gy || !gz || ldgz < TK || ldgy < d->K) return fail(ACIMG_EINVAL, "tapconv_scatter: null pointer or ldgz < R*S*K");
    const long Min = (long)d->N * d->H * d->W;
    hipLaunchKernelGGL(tapconv_scatter_kernel, dim3(cdiv(Min * TK, 256)), dim3(256), 0, (hipStream_t)stream, gy, ldgy,
                       d->H, d->W, d->R, d->S, d->K, d->OH, d->OW, Min, gz, ldgz);
    return check_launch("tapconv_scatter");
}

int acimg_conv2d_wgrad_split3(const AcimgConvDesc* d, const float* x, const float* gy, int ldgy,
                              float* dw, float* db, void* ws, size_t ws_bytes, void* stream) {
    return wgrad_split_onthefly(d, x, gy, ldgy, dw, db, ws, ws_bytes, stream, 3);
}

/* the same with x and gy rounded to bf16, one MFMA per product */
int acimg_conv2d_wgrad_bf16(const AcimgConvDesc* d, const float* x, const float* gy, int ldgy,
                            float* dw, float* db, void* ws, size_t ws_bytes, void* stream) {
    return wgrad_split_onthefly(d, x, gy, ldgy, dw, db, ws, ws_bytes, stream, 1);
}

/* precision of a conv layer's entry points: 0 = acimg_conv2d_fwd / _wgrad (fp32-class), 1 = _split3, 2 = _bf16 */
int acimg_conv2d_affine_input_ok(const AcimgConvDesc* d, int precision) {
    if (!d || precision < 0 || precision > 2 || check_desc(d, "conv2d_affine_input_ok")) return 0;
    WgradParams p{};
    p.H = d->H; p.W = d->W; p.C = d->C; p.ldx = d->ldx;
    p.OH = d->OH; p.OW = d->OW; p.R = d->R; p.S = d->S; p.stride = d->stride; p.pad_t = d->pad_t; p.pad_l = d->pad_l;
    p.M = d->N * d->OH * d->OW; p.KK = d->R * d->S * d->C;
    p.Ngemm = up4(d->K); p.Nld = p.Ngemm; p.ldo = d->ldw;
    const bool fwd = precision == 0 ? few16_fwd_shape(d) : conv_halo16_fwd_shape(d);
    return fwd && wgrad_halo16_ok(p, precision != 0) ? 1 : 0;
}

int acimg_conv2d_wgrad_affine(const AcimgConvDesc* d, int precision, const float* x, const float* in_scale, const float* in_shift,
                              int in_relu, const float* gy, int ldgy, float* dw, float* db, void* ws, size_t ws_bytes,
                              void* stream) {
    int rc = check_desc(d, "conv2d_wgrad_affine");
    if (rc) return rc;
    if (precision < 0 || precision > 2 || !in_scale || !in_shift)
        return fail(ACIMG_EINVAL, "conv2d_wgrad_affine: precision 0 / 1 / 2 and both halves of the affine");
    const int kp = up4(d->K);
    if (kp > ldgy || kp > d->ldw) return fail(ACIMG_EINVAL, "conv2d_wgrad_affine: padded K exceeds ldgy/ldw");
    WgradParams p{};
    p.X = x; p.H = d->H; p.W = d->W; p.C = d->C; p.ldx = d->ldx;
    p.OH = d->OH; p.OW = d->OW; p.R = d->R; p.S = d->S; p.stride = d->stride; p.pad_t = d->pad_t; p.pad_l = d->pad_l;
    p.M = d->N * d->OH * d->OW; p.KK = d->R * d->S * d->C;
    p.G = gy; p.ldg = ldgy; p.Ngemm = kp; p.Nld = kp; p.ldo = d->ldw;
    p.a_scale = in_scale; p.a_shift = in_shift; p.a_relu = in_relu;
    return launch_wgrad(p, dw, db, ws, ws_bytes, (hipStream_t)stream, precision != 0, precision == 2 ? 1 : 3);
}

}  // extern "C"
