// Host side of the weight gradients for gfx950 (MI355X): launch_wgrad with its wgrad_*_shape / *_ok predicates and the
// measurements that justify each route, the slab workspace and its reducers, the column sums, and every weight-gradient entry
// point (exact f32, bf16x3 / bf16, with an input affine, of the transposed conv).  Shared with the other families: conv_host.hpp.
// Kernel headers (their rule: conv_host.hpp) this file owns, and alone includes: wgrad_f32_kernel.hpp (exact-f32 weight gradient;
// the slab reducers of every split weight gradient), wgrad_halo_kernel.hpp (halo forms: exact f32 for few channels, bf16 /
// bf16x3 for <= 64 -> <= 32 channels), wgrad_split3_kernel.hpp, wgrad_tap_kernel.hpp, colsum_kernels.hpp.
#include "conv_host.hpp"
#include "wgrad_split3_kernel.hpp"
#include "wgrad_tap_kernel.hpp"
#include "wgrad_f32_kernel.hpp"
#include "wgrad_halo_kernel.hpp"
#include "colsum_kernels.hpp"
#include <algorithm>

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
size_t wgrad_ws_bytes(int M, int KK, int Ngemm, int ldo) {
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

static int colsum_parts(long rows);
static int launch_colsum(const float* G, long rows, int ncols, int ld, float* out, void* ws, size_t ws_bytes, hipStream_t st);

// db (optional): fused bias gradient, db[n] = sum_m G[m][n] for n < Ngemm
static int launch_wgrad(WgradParams p, float* dw, float* db, void* ws, size_t ws_bytes, hipStream_t st,
                        bool split3 = false, int terms = 3) {
    if ((p.C & 3) || (p.ldx & 3) || (p.ldg & 3) || (p.ldo & 3))
        return fail(ACIMG_EINVAL, "wgrad: C=%d ldx=%d ldg=%d ldo=%d must be multiples of 4", p.C, p.ldx, p.ldg, p.ldo);
    if (!aligned16(p.X) || !aligned16(p.G) || !aligned16(dw))
        return fail(ACIMG_EINVAL, "wgrad: operands must be 16-byte aligned");
    if (int wrc = check_ws_aligned("wgrad", ws)) return wrc;       // (wgrad_slabs: the kernels store slab rows in 16-byte pieces)
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
    // An unsplit launch writes dW and db themselves, and the split-MFMA kernels store a row in 16-byte pieces: right for dw and
    // the slabs, not for a db that is only float-aligned (include/acimg.h: any float*).  Such a db is left to the column sums
    // of G, whose partials the sizing query reserves; refused here, before dW is written, when they do not fit.
    const bool db_colsum = split3 && db && !aligned16(db);
    const auto colsum_fits = [&]() { return ws && ws_bytes >= (size_t)colsum_parts(p.M) * p.Ngemm * sizeof(float); };
    const auto colsum_short = [&]() { return fail(ACIMG_EWORKSPACE, "wgrad: workspace %zu too small for the bias gradient's column sums", ws_bytes); };
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
            if (db_colsum && !colsum_fits()) return colsum_short();
            q.out = dw;
            q.db_out = db_colsum ? nullptr : db;
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
        if (rc || ns > 1) return rc ? rc : wgrad_reduce(sl, ns, p, dw, db, false, st);
        return db_colsum ? launch_colsum(p.G, p.M, p.Ngemm, p.ldg, db, ws, ws_bytes, st) : rc;
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
        if (db_colsum && !colsum_fits()) return colsum_short();
        p.out = dw;
        p.db_out = db_colsum ? nullptr : db;
    }
    const int rows = p.KK + (p.db_out ? 1 : 0);
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
    if (rc || p.splits > 1) return rc ? rc : wgrad_reduce(sl, p.splits, p, dw, db, false, st);
    return db_colsum ? launch_colsum(p.G, p.M, p.Ngemm, p.ldg, db, ws, ws_bytes, st) : rc;
}

// column sums; workspace: parts*ncols floats
static int colsum_parts(long rows) { return clamped_blocks(rows, 256); }
static int launch_colsum(const float* G, long rows, int ncols, int ld, float* out, void* ws, size_t ws_bytes, hipStream_t st) {
    const int parts = colsum_parts(rows);
    const long rpb = (rows + parts - 1) / parts;
    const size_t need = (size_t)parts * ncols * sizeof(float);
    if (ws == nullptr || ws_bytes < need) return fail(ACIMG_EWORKSPACE, "colsum: workspace %zu < %zu", ws_bytes, need);
    if (int wrc = check_ws_aligned("colsum", ws)) return wrc;
    float* partial = static_cast<float*>(ws);
    if (ncols <= 64 && (ncols & 3) == 0 && (ld & 3) == 0 && aligned16(G))
        hipLaunchKernelGGL(colsum_narrow_kernel, dim3(parts), dim3(256), 0, st, G, rows, ncols, ld, rpb, partial);
    else
        hipLaunchKernelGGL(colsum_partial_kernel, dim3(cdiv(ncols, 64), parts), dim3(256), 0, st, G, rows,
                           ncols, ld, rpb, partial);
    hipLaunchKernelGGL(colsum_final_kernel, dim3(cdiv(ncols, 64)), dim3(256), 0, st, partial, parts, ncols, out);
    return check_launch("colsum");
}
size_t colsum_ws_bytes(int ncols) { return (size_t)256 * ncols * sizeof(float); }

// descriptor -> weight-gradient view: dW rows = (tap, input channel), columns = output channels padded to 4
static WgradParams wgrad_view(const AcimgConvDesc* d, const float* x, const float* gy, int ldgy) {
    WgradParams p{};
    p.X = x; p.H = d->H; p.W = d->W; p.C = d->C; p.ldx = d->ldx;
    p.OH = d->OH; p.OW = d->OW; p.R = d->R; p.S = d->S; p.stride = d->stride; p.pad_t = d->pad_t; p.pad_l = d->pad_l;
    p.M = d->N * d->OH * d->OW; p.KK = d->R * d->S * d->C;
    p.G = gy; p.ldg = ldgy; p.Ngemm = up4(d->K); p.Nld = p.Ngemm; p.ldo = d->ldw;
    return p;
}

/* weight + bias gradient of a conv: the one body of acimg_conv2d_wgrad (exact f32), _wgrad_split3 / _bf16 (the bf16x3 / bf16 MFMA
 * path: split3, terms = 3 / 1, same contract) and _wgrad_affine (in_scale / in_shift); who: the entry's name in the error texts */
static int wgrad_entry(const AcimgConvDesc* d, const char* who, const float* x, const float* gy, int ldgy, float* dw, float* db,
                       void* ws, size_t ws_bytes, void* stream, bool split3, int terms, const float* in_scale = nullptr,
                       const float* in_shift = nullptr, int in_relu = 0) {
    int rc = check_desc(d, who);
    if (rc) return rc;
    if (up4(d->K) > ldgy || up4(d->K) > d->ldw) return fail(ACIMG_EINVAL, "%s: padded K exceeds ldgy/ldw", who);
    if ((rc = check_wide_ld(who, {{"ldgy", ldgy}})) ||
        (rc = check_wide(who, {{"x", x}, {"gy", gy}, {"dw", dw}, {"in_scale", in_scale}, {"in_shift", in_shift}})) ||
        (rc = check_ws_aligned(who, ws)))
        return rc;
    if (!split3 && !in_scale && skinny_shape(d) && (!db || aligned16(db)))     // (acimg_conv2d_wgrad alone: the VAE heads' dense layer)
        return launch_skinny_wgrad(d, x, gy, ldgy, dw, db, (hipStream_t)stream);
    WgradParams p = wgrad_view(d, x, gy, ldgy);
    p.a_scale = in_scale; p.a_shift = in_shift; p.a_relu = in_relu;
    return launch_wgrad(p, dw, db, ws, ws_bytes, (hipStream_t)stream, split3, terms);
}

}  // namespace acimg

using namespace acimg;

extern "C" {      // ---- C ABI ----

size_t acimg_conv2d_wgrad_workspace(const AcimgConvDesc* d) {
    return wgrad_ws_bytes(d->N * d->OH * d->OW, d->R * d->S * d->C, up4(d->K), d->ldw) + colsum_ws_bytes(up4(d->K));
}

int acimg_conv2d_wgrad(const AcimgConvDesc* d, const float* x, const float* gy, int ldgy,
                       float* dw, float* db, void* ws, size_t ws_bytes, void* stream) {
    return wgrad_entry(d, "conv2d_wgrad", x, gy, ldgy, dw, db, ws, ws_bytes, stream, false, 3);
}

int acimg_deconv_wgrad(const AcimgConvDesc* d, const float* x, const float* gy, int ldgy,
                       float* dw, float* db, void* ws, size_t ws_bytes, void* stream) {
    int rc = check_desc(d, "deconv_wgrad");
    if (rc) return rc;
    const int ca = up4(d->K);
    if (ca > ldgy || (ldgy & 3) || ca != d->K) return fail(ACIMG_EINVAL, "deconv_wgrad: K must be a multiple of 4 and <= ldgy");
    if ((rc = check_wide("deconv_wgrad", {{"x", x}, {"gy", gy}, {"dw", dw}})) || (rc = check_ws_aligned("deconv_wgrad", ws))) return rc;
    // dW[(r,s,k)][c] = sum_{n,h,w} gy[n,h*stride+r,w*stride+s,k] * x[n,h,w,c]
    if (patch2_shape(d) && ws && ws_bytes >= patch2_wgrad_ws_bytes(d->ldw) && (!db || aligned16(db))) {
        float* slabs = static_cast<float*>(ws);
        float* db_part = db ? slabs + (size_t)PATCH2_WGRAD_WGS * 32 * d->ldw : nullptr;
        rc = launch_patch2_wgrad(d, x, gy, ldgy, slabs, db_part, (hipStream_t)stream);
        if (rc) return rc;
        launch_slab_reduce_wide(slabs, PATCH2_WGRAD_WGS, 32L, 32, d->ldw, dw, nullptr, nullptr, (hipStream_t)stream);
        rc = check_launch("patch2_wgrad reduce");
        if (rc) return rc;
        // the transposed conv adds its bias at every output pixel, and every output pixel belongs to exactly one patch: the
        // bias gradient is the sum of all the gy values the kernel has just read
        if (db) {
            hipLaunchKernelGGL(colsum_final_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, db_part, PATCH2_WGRAD_WGS, 8, db);
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

int acimg_conv2d_wgrad_split3(const AcimgConvDesc* d, const float* x, const float* gy, int ldgy,
                              float* dw, float* db, void* ws, size_t ws_bytes, void* stream) {
    return wgrad_entry(d, "conv2d_wgrad_split3", x, gy, ldgy, dw, db, ws, ws_bytes, stream, true, 3);
}

/* the same with x and gy rounded to bf16, one MFMA per product */
int acimg_conv2d_wgrad_bf16(const AcimgConvDesc* d, const float* x, const float* gy, int ldgy,
                            float* dw, float* db, void* ws, size_t ws_bytes, void* stream) {
    return wgrad_entry(d, "conv2d_wgrad_split3", x, gy, ldgy, dw, db, ws, ws_bytes, stream, true, 1);
}

/* precision of a conv layer's entry points: 0 = acimg_conv2d_fwd / _wgrad (fp32-class), 1 = _split3, 2 = _bf16 */
int acimg_conv2d_affine_input_ok(const AcimgConvDesc* d, int precision) {
    if (!d || precision < 0 || precision > 2 || check_desc(d, "conv2d_affine_input_ok")) return 0;
    const WgradParams p = wgrad_view(d, nullptr, nullptr, 0);
    const bool fwd = precision == 0 ? few16_fwd_shape(d) : conv_halo16_fwd_shape(d);
    return fwd && wgrad_halo16_ok(p, precision != 0) ? 1 : 0;
}

int acimg_conv2d_wgrad_affine(const AcimgConvDesc* d, int precision, const float* x, const float* in_scale, const float* in_shift,
                              int in_relu, const float* gy, int ldgy, float* dw, float* db, void* ws, size_t ws_bytes,
                              void* stream) {
    int rc = check_desc(d, "conv2d_wgrad_affine");     // (here too: a refused descriptor is reported before a refused precision)
    if (rc) return rc;
    if (precision < 0 || precision > 2 || !in_scale || !in_shift)
        return fail(ACIMG_EINVAL, "conv2d_wgrad_affine: precision 0 / 1 / 2 and both halves of the affine");
    return wgrad_entry(d, "conv2d_wgrad_affine", x, gy, ldgy, dw, db, ws, ws_bytes, stream, precision != 0, precision == 2 ? 1 : 3,
                       in_scale, in_shift, in_relu);
}

}  // extern "C"
