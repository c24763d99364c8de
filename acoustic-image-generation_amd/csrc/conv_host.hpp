// What the four host files of the convolutions share (conv_f32.hip, conv_wgrad.hip, conv_split.hip, conv_trunk.hip): the
// tuning record, the descriptor views, and the few predicates, byte formulas and launchers that one family's entry point or
// query needs from another's file.  Everything else is static in its own file.
// The device code lives in one header per kernel family (kernels, their parameter structs, tile constants and design notes; no
// launch, no predicate that reads g_cfg, no entry point).  No kernel is included from here: each kernel header belongs to
// exactly one of the four files, so every __global__ kernel is compiled into one object only (the instances that conv_tiles.hpp
// lists: into conv_tiles.o).
#pragma once
#include "igemm.hpp"
#include <initializer_list>

namespace acimg {

// ---- conv_f32.hip ----
// the ONE tuning record: acimg_configure writes it, the predicates and launch heuristics of all four files read it
extern AcimgConfig g_cfg;

int check_desc(const AcimgConvDesc* d, const char* who, bool row_run = false);
static inline int up4(int v) { return (v + 3) & ~3; }

// ---- operand forms (include/acimg.h, "Operand forms of the convolution family"): ONE rule, applied by every entry point
// before its first launch.  Operands the kernels touch with 16-byte accesses whatever the route (x, gy, w and weight images,
// split planes, in_scale / in_shift, dw, tickets) are refused by name; outputs and epilogue operands take any float* and
// only choose the epilogue (epi_vec_flag) or, on the shapes the header lists, are refused by the route that was promised.
struct WideOperand { const char* name; const void* ptr; };
static inline int check_wide(const char* who, std::initializer_list<WideOperand> ops) {
    for (const WideOperand& o : ops)
        if (!aligned16(o.ptr)) return fail(ACIMG_EINVAL, "%s: %s must be 16-byte aligned", who, o.name);
    return ACIMG_OK;
}
struct WideLd { const char* name; int ld; };
static inline int check_wide_ld(const char* who, std::initializer_list<WideLd> lds) {
    for (const WideLd& l : lds)
        if (l.ld & 3) return fail(ACIMG_EINVAL, "%s: %s=%d must be a multiple of 4 floats", who, l.name, l.ld);
    return ACIMG_OK;
}
// the workspace is written in 16-byte pieces (split-K slabs, weight-gradient slabs, prepared weights): code and wording of
// launch_subpixel's refusal
static inline int check_ws_aligned(const char* who, const void* ws) {
    return aligned16(ws) ? ACIMG_OK : fail(ACIMG_EWORKSPACE, "%s: workspace too small or not 16-byte aligned", who);
}
// a route that the sizing / statistics-rows query promised and that takes 16-byte accesses to its outputs: no silent
// fall-through to a kernel the reported workspace does not cover
struct RouteOperand { const char* name; const void* ptr; int ld; };
static inline int check_route(const char* who, const char* route, std::initializer_list<RouteOperand> ops) {
    for (const RouteOperand& o : ops)
        if (!aligned16(o.ptr) || (o.ptr && (o.ld & 3)))
            return fail(ACIMG_EINVAL, "%s: %s of the %s must be 16-byte aligned with a leading dimension in multiples of 4",
                        who, o.name, route);
    return ACIMG_OK;
}
// 16-byte epilogue accesses: every operand the epilogue touches allows them
static inline void epi_vec_flag(EpiParams& e) {
    e.vec = aligned16(e.Y) && (e.ldy & 3) == 0 && (!e.bias || aligned16(e.bias)) &&
            (!e.res || (aligned16(e.res) && (e.ldres & 3) == 0)) &&
            (!e.mask || (aligned16(e.mask) && (e.ldmask & 3) == 0)) && (!e.scatter || (e.Ko & 3) == 0);
}

// ---- descriptor -> implicit-GEMM views: the geometry fields of IgemmParams; operands, row runs and epilogue extras are the
// caller's ----
// forward conv: rows = output pixels, K = (tap, input channel), columns = output channels
static inline IgemmParams fwd_view(const AcimgConvDesc* d) {
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
static inline IgemmParams flipped_view(int N, int GH, int GW, int ca, int ldgy, int H, int W, int R, int S, int pad_t, int pad_l,
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
static inline IgemmParams flipped_view(const AcimgConvDesc* d, int ca, int ldgy) {
    return flipped_view(d->N, d->OH, d->OW, ca, ldgy, d->H, d->W, d->R, d->S, d->pad_t, d->pad_l, d->C);
}
// the 16-bit MFMA kernels walk K as (tap, 32-channel chunk) in one pass
static inline void split_ksteps(IgemmParams& p) {
    p.ntaps = p.R * p.S;
    p.kiters = p.ntaps * (p.C / 32);
    p.splits = 1;
}

// shapes whose answer another family's entry point or query reads
bool few16_fwd_shape(const AcimgConvDesc* d);      // acimg_conv2d_affine_input_ok
bool skinny_shape(const AcimgConvDesc* d);         // acimg_conv2d_wgrad
bool patch2_shape(const AcimgConvDesc* d);         // acimg_deconv_wgrad
// the weight-gradient kernels of the skinny and patch2 headers are launched for conv_wgrad.hip from the file that owns them;
// the patch2 one leaves PATCH2_WGRAD_WGS slabs [32][ldw], then as many 8-float partial bias sums
static constexpr int PATCH2_WGRAD_WGS = 256;
static inline size_t patch2_wgrad_ws_bytes(int ldw) { return (size_t)PATCH2_WGRAD_WGS * (32 * ldw + 8) * sizeof(float); }
int launch_skinny_wgrad(const AcimgConvDesc* d, const float* x, const float* gy, int ldgy, float* dw, float* db, hipStream_t st);
int launch_patch2_wgrad(const AcimgConvDesc* d, const float* x, const float* gy, int ldgy, float* slabs, float* db_part,
                        hipStream_t st);

// ---- conv_wgrad.hip ---- (acimg_deconv_workspace)
size_t wgrad_ws_bytes(int M, int KK, int Ngemm, int ldo);
size_t colsum_ws_bytes(int ncols);

// ---- conv_split.hip ----
struct Split3Cfg { int bm, bn; };
Split3Cfg pick_split3(int M, int K, bool allow32 = false);      // pick_trunk
size_t split3_rowmajor_bytes(const AcimgConvDesc* d);           // fwd_presplit
bool conv_halo16_fwd_shape(const AcimgConvDesc* d);             // acimg_conv2d_affine_input_ok
// acimg_conv2d_dgrad's narrow halo route: the one conv_halo16_kernel instance behind the fp32 entry
int launch_dgrad_halo16_narrow(const AcimgConvDesc* d, const float* gy, int ldgy, const void* wimg, float* dx, int lddx,
                               const float* residual, int ldres, const float* mask, int ldmask, hipStream_t st);

}  // namespace acimg
