// Host side of the exact-f32 convolutions for gfx950 (MI355X): the tuning record (g_cfg) with acimg_configure, check_desc, and
// the routes of acimg_conv2d_fwd / _dgrad and acimg_deconv_fwd / _dgrad - their *_shape / *_ok predicates with the measurements
// that justify each route, the workspace, statistics-rows and tiling queries - and the acimg_tapconv_* entries.  (Weight
// gradients: conv_wgrad.hip; on-the-fly 16-bit convs: conv_split.hip; pre-split trunk: conv_trunk.hip; shared: conv_host.hpp.)
// Kernel headers (their rule: conv_host.hpp) this file owns, and alone includes: igemm_kernel.hpp (exact-f32 implicit GEMM and
// its epilogue; its 128-row tiles are compiled in conv_tiles.hip: conv_tiles.hpp says why), direct_conv_kernel.hpp,
// conv_few16_kernel.hpp (few-channel 3x3 conv on split 16-bit MFMAs), patch2_kernel.hpp (2x2 / stride-2 transposed conv 32 -> 8),
// skinny_kernel.hpp (dense layers, <= 64 rows), conv_aux_kernels.hpp (split-K reduce, small helpers).
#include "conv_host.hpp"
#include "conv_tiles.hpp"
#include "skinny_kernel.hpp"
#include "direct_conv_kernel.hpp"
#include "conv_few16_kernel.hpp"
#include "patch2_kernel.hpp"
#include "conv_aux_kernels.hpp"
#include <algorithm>
#include <type_traits>

namespace acimg {

struct TileCfg { int bm, bn; };

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
AcimgConfig g_cfg = DEFAULT_CFG;

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
        if (int wrc = check_ws_aligned("igemm", ws)) return wrc;       // the K ranges are stored in 16-byte pieces
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

// row_run: the caller's kernel accepts ldx < C with S == 1: the C "channels" of a tap are then a run of C / ldx
// consecutive pixels of one input row (windows of neighbouring outputs overlap), see acimg_conv2d_fwd_split3
int check_desc(const AcimgConvDesc* d, const char* who, bool row_run) {
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
    if (int wrc = check_ws_aligned("direct conv", ws)) return wrc;     // the kernel reads the prepared weights in 16-byte pieces
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

// shapes the few-channel MFMA kernel takes: cin = channels of the tensor that is convolved (4 forward only: an 8-channel image
// with a zero upper half), nout = channels written
static bool few16_channels(int cin, int nout, long pixels) {
    return (cin == 4 || cin == 8 || cin == 16) && nout >= 4 && nout <= 32 && (nout & 3) == 0 && !(cin != 8 && nout > 16) &&
           pixels >= 65536 && g_cfg.wgrad_halo;
}
// (ldx a multiple of 4: the kernel stages x in float4 pieces - and the predicate is what acimg_conv2d_stats_rows and
// acimg_conv2d_affine_input_ok answer from, so it must not promise this form to a descriptor the entry point refuses)
bool few16_fwd_shape(const AcimgConvDesc* d) {
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

bool patch2_shape(const AcimgConvDesc* d) {
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
int launch_patch2_wgrad(const AcimgConvDesc* d, const float* x, const float* gy, int ldgy, float* slabs, float* db_part,
                        hipStream_t st) {
    Patch2WgradParams q{};
    q.X = x; q.ldx = d->ldx; q.G = gy; q.ldg = ldgy; q.out = slabs; q.ldo = d->ldw; q.db_part = db_part;
    q.H = d->H; q.W = d->W; q.pixels = (long)d->N * d->H * d->W;
    hipLaunchKernelGGL(patch2_wgrad_32x8_kernel, dim3(PATCH2_WGRAD_WGS), dim3(1024), 0, st, q);
    return check_launch("patch2_wgrad");
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
bool skinny_shape(const AcimgConvDesc* d) {
    return d->R == 1 && d->S == 1 && d->H == 1 && d->W == 1 && d->OH == 1 && d->OW == 1 && d->stride == 1 &&
           d->pad_t == 0 && d->pad_l == 0 && d->N <= 64 && d->C >= 4096 && (d->C & 3) == 0 && (d->K & 3) == 0 &&
           (long)d->C * d->ldw * 4 < (1L << 31) && (long)d->N * d->ldx * 4 < (1L << 31);
}
static size_t skinny_fwd_ws_bytes(const AcimgConvDesc* d) {
    return skinny_shape(d) ? (size_t)cdiv(d->C, SKINNY_KS) * d->N * d->K * 4 : 0;
}
// the forward and data-gradient kernels are instantiated per number of 16-row blocks of the batch (N <= 64: 1..4)
#define ACIMG_SKINNY_MB(kernel, N, grid, threads, st, q)                          \
    switch (cdiv(N, 16)) {                                                        \
        case 1: hipLaunchKernelGGL(kernel<1>, grid, threads, 0, st, q); break;    \
        case 2: hipLaunchKernelGGL(kernel<2>, grid, threads, 0, st, q); break;    \
        case 3: hipLaunchKernelGGL(kernel<3>, grid, threads, 0, st, q); break;    \
        default: hipLaunchKernelGGL(kernel<4>, grid, threads, 0, st, q);          \
    }
// the same dense layer's weight gradient: every weight row is written once, 256 contiguous bytes per wave
int launch_skinny_wgrad(const AcimgConvDesc* d, const float* x, const float* gy, int ldgy, float* dw, float* db, hipStream_t st) {
    SkinnyParams q{};
    q.X = x; q.G = gy; q.out = dw; q.db = db;
    q.M = d->N; q.C = d->C; q.N = up4(d->K);
    q.ldw = d->ldw; q.ldg = ldgy; q.ldx = d->ldx;
    const int ngroups = cdiv(q.N, 64);
    const int tasks = cdiv(d->C, 64) * ngroups;
    hipLaunchKernelGGL(skinny_wgrad_kernel, dim3(cdiv(tasks, 4)), dim3(256), 0, st, q, ngroups);
    return check_launch("conv2d_wgrad (skinny)");
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
// zero insertion: in [N][H][W] pixels of C channels (pixel stride ldin) -> out [N][(H-1)s+1][(W-1)s+1][C], dilated_bytes of it
static int launch_dilate2d(const float* in, int ldin, float* out, int N, int H, int W, int C, int s, hipStream_t st) {
    const int H1 = (H - 1) * s + 1, W1 = (W - 1) * s + 1;
    const long opix = (long)N * H1 * W1;
    hipLaunchKernelGGL(dilate2d_kernel, dim3(cdiv(opix * (C / 4), 256)), dim3(256), 0, st, in, ldin, out, opix, H, W, H1, W1, C, s);
    return check_launch("dilate2d");
}

// data gradient of a 3x3 / stride-1 / SAME layer with 32 output and 4 - 16 input channels (configs[1]: 112x149 8 -> 32) through
// the fp32 entry: a conv of the 32-channel gy on the 16-row instance of the halo kernel (conv_halo16_kernel.hpp)
static bool dgrad_halo16_narrow_shape(const AcimgConvDesc* d) {
    return d->R == 3 && d->S == 3 && d->stride == 1 && d->pad_t == 1 && d->pad_l == 1 && d->OH == d->H && d->OW == d->W &&
           d->K == 32 && d->C <= 16 && (d->C & 3) == 0 && (long)d->N * d->H * d->W >= 65536 && g_cfg.wgrad_halo;
}
static constexpr size_t DGRAD_HALO16_NARROW_WS = 2 * 16 * 288 * 2;

/* ---- tap-GEMM helpers (see the kernels above) ---- */
static int tapconv_check(const AcimgConvDesc* d, const char* who) {
    int rc = check_desc(d, who);
    if (rc) return rc;
    if (d->stride != 1 || d->pad_t || d->pad_l || d->OH != d->H - d->R + 1 || d->OW != d->W - d->S + 1)
        return fail(ACIMG_EINVAL, "%s: stride-1 VALID convolutions only", who);
    if (d->K > 64) return fail(ACIMG_EINVAL, "%s: K=%d > 64 (this form is for few output channels)", who, d->K);
    return ACIMG_OK;
}

}  // namespace acimg

using namespace acimg;

extern "C" {      // ---- C ABI ----

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
    if ((rc = check_wide("conv2d_fwd", {{"x", x}, {"w", w}, {"in_scale", in_scale}, {"in_shift", in_shift}, {"tickets", tickets}})) ||
        (rc = check_ws_aligned("conv2d_fwd", ws)))
        return rc;
    if (skinny_shape(d) && !in_scale && !in_shift && !in_relu && !stats && ws && ws_bytes >= skinny_fwd_ws_bytes(d) &&
        aligned16(y) && (!bias || aligned16(bias)) && (d->ldy & 3) == 0) {
        // the VAE heads' dense layer: weight rows read once in whole lines, K slabs combined in slab order
        SkinnyParams q{};
        q.W = w; q.X = x; q.out = y; q.bias = bias; q.act = d->act; q.part = static_cast<float*>(ws);
        q.M = d->N; q.C = d->C; q.N = d->K; q.ldw = d->ldw; q.ldx = d->ldx; q.ldo = d->ldy;
        q.slabs = cdiv(d->C, SKINNY_KS);
        const dim3 grid(q.slabs, cdiv(d->K, 64));
        ACIMG_SKINNY_MB(skinny_fwd_kernel, d->N, grid, dim3(64), (hipStream_t)stream, q);
        rc = check_launch("conv2d_fwd (skinny)");
        if (rc) return rc;
        hipLaunchKernelGGL(skinny_fwd_reduce_kernel, dim3(cdiv(d->N * (d->K / 4), 256)), dim3(256), 0, (hipStream_t)stream, q);
        return check_launch("conv2d_fwd (skinny reduce)");
    }
    if (few16_fwd_shape(d)) {
        // acimg_conv2d_stats_rows(d) promised one statistics row per workgroup of this kernel: no silent fallback
        if ((in_scale != nullptr) != (in_shift != nullptr) || (in_relu && !in_scale) || d->ldy < d->K)
            return fail(ACIMG_EINVAL, "conv2d_fwd: few-channel MFMA shape with half an input affine or ldy < K");
        if ((rc = check_route("conv2d_fwd", "few-channel MFMA forward", {{"y", y, d->ldy}, {"bias", bias, 0}}))) return rc;
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

// (the narrow halo route's answer is for that kernel alone: acimg_conv2d_dgrad refuses, by name, a dx / residual / mask that
// would take the shape to a route below, which needs more)
size_t acimg_conv2d_dgrad_workspace(const AcimgConvDesc* d) {
    if (dgrad_halo16_narrow_shape(d)) return DGRAD_HALO16_NARROW_WS + 256;
    if (dgrad_is_patch(d)) return igemm_ws_bytes(d->N * d->OH * d->OW, d->R * d->S * d->C, cdiv(up4(d->K), 32));
    const int ca = up4(d->K);
    if (subpixel_ok(d->stride, d->C, ca))   // sub-pixel form: combined weights + the GEMM's own split-K slabs
        return subpixel_ws_bytes(d->N, d->H, d->W, -d->pad_t, -d->pad_l, d->R, d->S, ca, d->C);
    // zero-inserted copy of gy (stride > 1), then the stride-1 path
    // rowrun depends on ldgy, unknown here: per-tap kiters is the larger bound for splits
    return (d->stride > 1 ? dilated_bytes(d->N, d->OH, d->OW, ca, d->stride) : 0) +
           igemm_ws_bytes(d->N * d->H * d->W, d->C, d->R * d->S * cdiv(ca, 32)) +
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
    if ((rc = check_wide("conv2d_dgrad", {{"gy", gy}, {"w", w}, {"tickets", tickets}})) || (rc = check_ws_aligned("conv2d_dgrad", ws)))
        return rc;
    if (skinny_shape(d)) {
        // a dense layer over a few batch rows (the 28 416 -> 300 VAE heads): the weight matrix is read once, in rows
        SkinnyParams q{};
        q.W = w; q.G = gy; q.out = dx; q.res = residual; q.mask = mask;
        q.M = d->N; q.C = d->C; q.N = ca;
        q.ldw = d->ldw; q.ldg = ldgy; q.ldo = lddx > 0 ? lddx : d->ldx; q.ldres = ldres; q.ldmask = ldmask;
        if (q.ldo < d->C) return fail(ACIMG_EINVAL, "conv2d_dgrad: lddx < C");
        const dim3 grid(cdiv(cdiv(d->C, 16), 4));
        ACIMG_SKINNY_MB(skinny_dgrad_kernel, d->N, grid, dim3(256), (hipStream_t)stream, q);
        return check_launch("conv2d_dgrad (skinny)");
    }
    if (lddx <= 0) lddx = d->ldx;
    if (lddx < d->C) return fail(ACIMG_EINVAL, "conv2d_dgrad: lddx < C");
    if (subpixel_ok(d->stride, d->C, ca) && !dgrad_is_patch(d))
        // dx[2 oy - pad_t + r][2 ox - pad_l + s][c] += gy[oy][ox][k] w[r][s][c][k]: the sub-pixel form over gy's own grid
        return launch_subpixel(gy, d->N, d->OH, d->OW, ca, ldgy, w, d->R, d->S, d->ldw, d->C, dx, lddx, d->H, d->W, -d->pad_t,
                               -d->pad_l, nullptr, residual, ldres, mask, ldmask, ACIMG_ACT_NONE, ws, ws_bytes, tickets,
                               (hipStream_t)stream, "conv2d_dgrad");
    if (dgrad_halo16_narrow_shape(d)) {
        // acimg_conv2d_dgrad_workspace(d) answered for this kernel alone: no silent fall-through to a route that needs more
        if (!ws || ws_bytes < DGRAD_HALO16_NARROW_WS)
            return fail(ACIMG_EWORKSPACE, "conv2d_dgrad: workspace %zu < %zu", ws_bytes, DGRAD_HALO16_NARROW_WS);
        if ((rc = check_route("conv2d_dgrad", "narrow-halo data gradient",
                              {{"dx", dx, lddx}, {"residual", residual, ldres}, {"mask", mask, ldmask}})))
            return rc;
        // the flipped / transposed image [16 rows = input channels, zero beyond C][k = tap * 32 + gy channel], bf16 hi / lo
        FewParams f{};
        f.w = w; f.ldw = d->ldw; f.wrows = d->C; f.cin = d->K; f.mode = 1; f.nout = d->C;
        hipLaunchKernelGGL((few16_prepare_kernel<SplitBF16>), dim3(cdiv(16 * 288, 256)), dim3(256), 0, (hipStream_t)stream, f, 32, 16,
                           static_cast<__bf16*>(ws));
        return launch_dgrad_halo16_narrow(d, gy, ldgy, ws, dx, lddx, residual, ldres, mask, ldmask, (hipStream_t)stream);
    }
    if (few16_dgrad_shape(d) && !subpixel_ok(d->stride, d->C, ca) && !mask && aligned16(dx) && (lddx & 3) == 0 &&
        ws && ws_bytes >= few16_ws_bytes(ca, d->C) && (!residual || ((ldres & 3) == 0 && aligned16(residual)))) {
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
        if ((long)d->N * OH1 * OW1 * ca >= (1L << 31)) return fail(ACIMG_EINVAL, "conv2d_dgrad: dilated gradient exceeds 2^31 elements");
        rc = launch_dilate2d(gy, ldgy, static_cast<float*>(ws), d->N, d->OH, d->OW, ca, d->stride, (hipStream_t)stream);
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

size_t acimg_deconv_workspace(const AcimgConvDesc* d) {
    size_t a = igemm_ws_bytes(d->N * d->H * d->W, d->R * d->S * d->K, cdiv(d->C, 32));
    size_t b = igemm_ws_bytes(d->N * d->H * d->W, d->C, d->R * d->S * cdiv(up4(d->K), 32));
    size_t c = wgrad_ws_bytes(d->N * d->H * d->W, d->R * d->S * up4(d->K), d->C, d->ldw) + colsum_ws_bytes(up4(d->K));
    size_t m = a > b ? a : b;
    m = m > c ? m : c;
    if (patch2_shape(d)) {                      // weight gradient of the pointwise form: one 32 x ldw slab per workgroup
        const size_t pw = patch2_wgrad_ws_bytes(d->ldw);
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
    if ((rc = check_wide("deconv_fwd", {{"x", x}, {"w", w}, {"tickets", tickets}})) || (rc = check_ws_aligned("deconv_fwd", ws)))
        return rc;
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
        rc = launch_dilate2d(x, d->ldx, static_cast<float*>(ws), d->N, d->H, d->W, d->C, d->stride, (hipStream_t)stream);
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
    if (patch2_shape(d) && aligned16(y) && (d->ldy & 3) == 0 && (!bias || aligned16(bias))) {
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
    epi_vec_flag(p.e);      // (launch_igemm decides the same for its epilogue; the gap fill below follows it)
    rc = launch_igemm(p, true, ws, ws_bytes, tickets, (hipStream_t)stream);
    if (rc) return rc;
    if (d->R < d->stride || d->S < d->stride) {
        const long pixels = (long)d->N * d->OH * d->OW;
        hipLaunchKernelGGL(deconv_gap_fill_kernel, dim3(cdiv(pixels * (d->K / 4), 256)), dim3(256), 0,
                           (hipStream_t)stream, y, d->ldy, bias, pixels, d->OH, d->OW, d->K, d->R, d->S, d->stride, p.e.vec);
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
    if ((rc = check_wide("deconv_dgrad", {{"gy", gy}, {"w", w}, {"tickets", tickets}})) || (rc = check_ws_aligned("deconv_dgrad", ws)))
        return rc;
    // dx[n,h,w,c] = sum_{r,s,k} gy[n, h*stride+r, w*stride+s, k] * W[r][s][k][c]  (a strided conv)
    if (patch2_shape(d) && aligned16(dx) && (!mask || (aligned16(mask) && (ldmask & 3) == 0))) {
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

}  // extern "C"
