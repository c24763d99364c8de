/*
 * acimg.h — C ABI of libacimg.so: the MI355X (gfx950) kernels behind the acoustic-image
 * generation train step of IIT-PAVIS/Acoustic-Image-Generation.
 *
 * The reference has no FFI layer: every arithmetic op on its hot path is a TensorFlow-1.x op
 * call inside models/<name>.py and trainer/mfcctrainer.py.  Each entry point
 * below replaces one family of those op calls and cites the call site(s) it stands in for.
 *
 * Conventions (all entry points):
 *   - return 0 on success, a negative ACIMG_E* code otherwise; acimg_last_error() holds text;
 *     nothing is thrown across the boundary;
 *   - the CALLER owns every buffer (device pointers, 16-byte aligned), including workspace and the
 *     ticket words of the in-kernel reductions (explicit `tickets` / scratch arguments); the library
 *     allocates nothing.  Its only process-wide state is the tuning record of acimg_configure() (thirteen
 *     plain ints with compiled-in defaults, written by that call alone, never by a launch, and never
 *     read from the process environment) and the per-thread text of acimg_last_error();
 *   - all work is enqueued on `stream` (a hipStream_t passed as void*), no host sync;
 *   - tensors are NHWC float32; a tensor is (ptr, C, ld): C logical channels per pixel and
 *     ld >= C the pixel stride in floats, so producers can write straight into channel slices
 *     of a concat buffer (tf.concat never materialises).  Channel counts seen by the GEMM
 *     kernels are multiples of 4 (the host pads 3->4, 133->136, 145->148, 150->152, 266->268
 *     with zeros; padded weights rows/cols are zero and provably stay zero under Adam).
 *   - OPERAND FORMS of the convolution family (every acimg_conv2d_* / acimg_deconv_* entry point, the prepare calls
 *     included); each refusal below precedes the first launch and leaves every output byte untouched:
 *       operands read with 16-byte accesses - x, gy, w, every prepared weight image, split planes, in_scale / in_shift
 *         (and the per-channel scale / shift vectors of the _tail entries), the ticket words - must be 16-byte aligned with
 *         leading dimensions (ldx, ldw, ldgy) in multiples of 4 floats: anything else is ACIMG_EINVAL with text that names
 *         the operand.  dw is written that way and counts among them.  So does the workspace, with its own code: a
 *         workspace that is NULL, short or not 16-byte aligned is ACIMG_EWORKSPACE;
 *       outputs and epilogue operands - y / dx, bias, residual, mask, db, stats - may be ANY 4-byte-aligned float* with
 *         any leading dimension at or above the channel count: the call succeeds with the same documented result on a
 *         general kernel, and the workspace the query reported is enough for it.  EXCEPT where the query already promised
 *         one kernel, which are refused with ACIMG_EINVAL naming the operand: the few-channel MFMA forward of
 *         acimg_conv2d_fwd (it promised FEW16 statistics rows: y, ldy, bias), the halo-16 forward of
 *         acimg_conv2d_fwd_split3 / _bf16 (3x3 / stride 1 / SAME, C = 32 or 64 into K = 32 from 65536 pixels on: y, ldy,
 *         bias), the narrow-halo data gradient of acimg_conv2d_dgrad (3x3 / stride 1 / SAME, K = 32 into C <= 16 from
 *         65536 pixels on, whose workspace query answers for that kernel alone: dx, lddx, residual, ldres, mask, ldmask),
 *         and the pre-split trunk entries (acimg_conv2d_fwd_split3p and siblings: y is dense and 16-byte aligned).
 *   - weights use TensorFlow's own layouts, padded as above:
 *       conv2d            HWIO  [R][S][Cin_p][Cout_p]
 *       conv2d_transpose        [R][S][Cout_p][Cin_p]
 *       dense                   [Kin_p][Nout_p]
 */
#ifndef ACIMG_H_
#define ACIMG_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ACIMG_VERSION 207

#define ACIMG_OK 0
#define ACIMG_EINVAL (-1)     /* bad descriptor / shape / alignment */
#define ACIMG_EWORKSPACE (-2) /* workspace too small */
#define ACIMG_ELAUNCH (-3)    /* hipLaunch / runtime error */

#define ACIMG_ACT_NONE 0
#define ACIMG_ACT_RELU 1
#define ACIMG_ACT_SIGMOID 2

int acimg_version(void);
/* copies the calling thread's last error text (NUL terminated) into buf */
int acimg_last_error(char* buf, size_t len);

/* ------------------------------------------------------------------------------------------
 * Convolution family.  One descriptor serves forward / data-gradient / weight-gradient.
 *   x : [N,H,W,C]   (pixel stride ldx)      y : [N,OH,OW,K] (pixel stride ldy)
 *   w : HWIO [R][S][C][ldw], ldw >= K
 * TF 'SAME' asymmetric padding is resolved by the host into pad_t/pad_l;
 * OH/OW are given explicitly.
 * ---------------------------------------------------------------------------------------- */
typedef struct AcimgConvDesc {
    int32_t N, H, W, C, ldx;
    int32_t K, ldy, OH, OW;
    int32_t R, S, stride, pad_t, pad_l;
    int32_t ldw;
    int32_t act; /* ACIMG_ACT_* applied by the forward epilogue */
} AcimgConvDesc;

/* Forward: y = act(conv(x', w) + bias), x' = relu(x*in_scale[c] + in_shift[c]) when in_scale
 * is given (deferred batch-norm of the producer, zero padding applied AFTER the affine), else x.
 * stats (optional, [grid_m][2][ldw] floats, grid_m = acimg_conv2d_stats_rows(d)) receives per
 * row-block partial sums / sums of squares of conv + bias BEFORE the activation for batch-norm statistics (the
 * few-channel direct kernel with an activation sums the stored, activated y instead; batch-norm layers use ACT_NONE).
 * With an activation the meaning of `stats` therefore follows the KERNEL THAT RUNS, not the shape alone: a y / bias that is
 * not 16-byte aligned, or an ldy that is no multiple of 4, moves a direct-kernel shape onto the implicit GEMM and its
 * pre-activation sums (operand forms, above).  Nothing in this project asks for statistics of an activated layer.
 * The row count belongs to THIS descriptor, `act` included (the few-channel 3x3 / stride-1 layers from 65536
 * pixels on run on an MFMA kernel that leaves one row per workgroup - 512 - when act is ACIMG_ACT_NONE, and on
 * the direct kernel with one row per 256 pixels otherwise): size the buffer from the descriptor that is launched.
 * ARITHMETIC: exact fp32 products (fp32 matrix cores / packed FMAs) EXCEPT, from 65536 output pixels on (wgrad_halo = 1, the
 * default), the few-channel layers: 3x3 / stride 1 / SAME, C = 4, 8 or 16 and K % 4 == 0, K <= 32 (<= 16 unless C = 8), ACT_NONE - the
 * layers above with 512 statistics rows - run f16x3 as acimg_conv2d_fwd_split3 below does (in_scale / in_shift applied in
 * fp32 BEFORE the 2^-2 scale and the split).  Its operand range (|w| < 63, |x'| < 2.6e5) and its floors (2^-23 absolute per
 * activation below |x'| = 0.5, 2^-35 per weight below |w| ~ 1.2e-4) apply to these shapes; outside that range the output
 * is not finite.  Per element |y - exact| <= ~2^-19 sum |x'| |w| + 2^-22 sum |w| + 2^-34 sum |x'|
 * (tests/split_format_ref.py: bound_f16x3, held per element by tests/test_operand_range_gpu.py).
 * Replaces: tf.layers.conv2d   models/unet_acresnet.py:159-168,173-182,82,89-94
 *           slim layers.conv2d / resnet_utils.conv2d_same   models/resnet50.py:109-121,205-209 */
int acimg_conv2d_fwd(const AcimgConvDesc* d, const float* x, const float* w, const float* bias,
                     float* y, const float* in_scale, const float* in_shift, int in_relu,
                     float* stats, void* ws, size_t ws_bytes, void* tickets, void* stream);
int acimg_conv2d_stats_rows(const AcimgConvDesc* d);
/* out[3] = {BM, BN, split-K factor} the forward launch will use (profiling / roofline bookkeeping) */
int acimg_conv2d_fwd_tiling(const AcimgConvDesc* d, int* out);
/* `tickets` argument of acimg_conv2d_fwd / _dgrad and acimg_deconv_fwd / _dgrad: NULL, or ACIMG_TICKET_WORDS ints of
 * ZEROED device memory (16-byte aligned) owned by the caller and written by nothing else.  With it, a split-K launch
 * combines its K ranges inside the kernel — one ticket per output tile, the last arriver adds the ranges in range
 * order and runs the epilogue — instead of through a separate reduce launch; every launch leaves the words at zero and
 * results are bit-identical to the reduce-launch path.  Launches sharing one ticket block must be ordered against each
 * other (one stream, as the recorded plans are): use one block per stream. */
#define ACIMG_TICKET_WORDS 4096

/* Tuning record of the launch heuristics.  acimg_config_default() fills in the compiled-in values;
 * acimg_configure() installs a record (validate, copy).  Call it before the first launch, from one thread; launches
 * only read it.  The library never reads the process environment (the Python host maps ACIMG_* variables onto this
 * call once, at load time: acimg/_lib.py). */
typedef struct AcimgConfig {
    int32_t splitk_cut;      /* f32 implicit GEMM: no K split at or above this many output tiles (320) */
    int32_t splitk_target;   /* ... otherwise split towards this many workgroups (768) */
    int32_t splitk_handoff;  /* 1: combine K ranges in-kernel when `tickets` is given; 0: always the reduce launch */
    int32_t wgrad_minpix;    /* weight gradients: at least this many pixels per slab (128) */
    int32_t wgrad_halo;      /* 1: the kernels that stage a tile with its halo once and form every tap from it, and the other
                                special forms of the U-Net layers - not weight gradients alone (the name stays, with the
                                record's layout and ACIMG_NO_WGRAD_HALO): the halo weight gradients of the few-channel and
                                32- / 64-channel layers and the tap-sharing weight gradient of the wide 3x3 layers with 32- /
                                48-pixel rows; the few-channel MFMA forward conv and data gradient; the narrow halo data
                                gradient (32 -> 4..16 channels); the pointwise 2x2 / stride-2 forms (32 -> 8: forward, data
                                and weight gradient); the halo forward conv / data gradient of the 32- / 64-channel layers;
                                the tap-sharing forward and data-gradient convs.  0: the per-tap / implicit-GEMM / direct
                                kernels for all of them */
    int32_t split3_tile_bm;  /* 0 = per-shape choice; else force the split-MFMA tile (experiments): 128x128, 64x128, */
    int32_t split3_tile_bn;  /*     128x64 */
    int32_t tail_split;      /* 1: trunk kernel cuts the tiles of the last partial round into K ranges */
    int32_t tail_s;          /* 0 = cost model; else force that many K ranges (experiments) */
    int32_t trunk_persistent;/* 128x128 trunk convs on the persistent kernel (a workgroup walks a tile list; the next tile's
                                first loads overlap the current tile's last K step and output stores): 0 never, 1 where it
                                was measured to pay (short-K, multi-round layers), 2 always */
    int32_t trunk_bk;        /* K-step depth of the persistent kernel: 0 / 32 (a 64-deep step, one workgroup per CU, was
                                measured slower in round 2 and removed; the field keeps the record's layout) */
    int32_t trunk_stagger;   /* persistent kernel: start the second half of the grid this many percent of a tile's
                                estimated time late (0 = together) */
    int32_t trunk_dma_pos;   /* persistent kernel: a K step's operand requests 0 = in one burst after the step barrier,
                                1 = spread under the MFMA block (B after the first sweep, A after the second)
                                (requests TWO steps ahead - a second barrier after the fragment reads frees the stage
                                early - were measured in round 3: 2.5 % slower over the trunk, removed) */
    int32_t trunk_ring;      /* 128-column trunk convs on the RING kernel (one workgroup per CU, three LDS slots, fragments
                                double buffered in registers, requests spread between the MFMAs): 0 never, 1 where it was
                                measured to pay, 2 always */
    int32_t trunk_ring_bm;   /* ring kernel's tile rows: 0 = per shape, else 128 or 256 (experiments) */
    int32_t trunk_halo;      /* 3x3 / stride-1 trunk convs on the HALO kernel (one patch of the activation planes staged per
                                channel chunk, all nine taps formed from it in LDS): 0 never, 1 where it was measured to
                                pay, 2 wherever it applies */
} AcimgConfig;
int acimg_config_default(AcimgConfig* cfg);
int acimg_configure(const AcimgConfig* cfg);
size_t acimg_conv2d_fwd_workspace(const AcimgConvDesc* d);

/* f16x3 ("split fp16") forward convolution for frozen weights (the ResNet-50 trunk): x and w are fp32,
 * each is split into hi = f16(v), lo = f16(v - hi) (22 mantissa bits) and every product is
 * ah*wh + ah*wl + al*wh on the fp16 matrix cores with fp32 accumulation (~2^-22 relative per product:
 * fp32-class results, same 1e-3 parity bar) at 3/16 of the exact-f32 MFMA cost.  Exact power-of-two
 * scaling (weights x2^10, activations x2^-2, accumulators x2^-8) keeps everything in fp16's range for
 * |w| < 63 and |x| < 2.6e5.  Below |x| = 0.5 the lo half of an activation is an fp16 subnormal: the split has an absolute floor
 * of 2^-23 per activation (2^-35 per weight, below |w| ~ 1.2e-4), so an activation near 2^-8 keeps about 14 bits.
 * Needs C % 32 == 0.  `wsplit` (caller-owned,
 * acimg_conv2d_split3_weight_bytes(d) bytes) is filled by acimg_conv2d_split3_prepare from the HWIO fp32
 * kernel: [hi|lo][ldw][R*S*C] fp16, followed - for the pre-split entry points acimg_conv2d_fwd_split3p / _split1p - by
 * the same weights in LDS-tile order (per 128 output channels and 32-deep K step the two 8 KiB plane images
 * [row][64 bytes], 16-byte groups swizzled as in the activation bricks below).  Semantics otherwise as acimg_conv2d_fwd (deferred BN on load, raw
 * output + statistics partials of acimg_conv2d_fwd_split3_stats_rows(d) rows; optional bias + d->act; no
 * split-K).
 * Row-run view (this entry only): with S == 1 and pad_l == 0, ldx < C is accepted when C % ldx == 0 — the C
 * "channels" of a tap are then the C / ldx consecutive pixels of an input row starting at ow*stride (windows of
 * neighbouring outputs overlap; (OW-1)*stride + C/ldx <= W).  The 7x7/2 stem on a zero-padded 4-channel frame is
 * such a conv: R = 7, S = 1, C = 32 = 7 pixels x 4 channels + one pixel of zero weights, ldx = 4.
 * ARITHMETIC: on the 3x3 / stride 1 / SAME layers with image rows of 32 or 48 pixels, C >= 64 and K > 32 (no in_scale, no
 * stats; wgrad_halo = 1) the same format with K summed chunk-major - 32 channels at a time, the nine taps inside - instead
 * of tap-major: the same products in another order.
 * OPERAND FORMS (this entry, _bf16 and the data gradients below): x / gy, the weight image and in_scale / in_shift 16-byte
 * aligned, ldgy % 4 == 0; y / dx, bias, residual and mask any float* with any leading dimension at or above the channel count
 * (per-tap kernel with scalar stores) EXCEPT the halo-16 forward shape, whose statistics rows were promised: ACIMG_EINVAL.
 * Replaces: slim layers.conv2d / conv2d_same in the trunk, models/resnet50.py:109-121. */
size_t acimg_conv2d_split3_weight_bytes(const AcimgConvDesc* d);
int acimg_conv2d_split3_prepare(const AcimgConvDesc* d, const float* w, void* wsplit, void* stream);
/* Up to 16 kernels in ONE launch (a model that trains re-splits its kernels every step): mode[i] = 0 -> the forward
 * image of acimg_conv2d_split3_prepare, 1 -> the data-gradient image of acimg_conv2d_split3_prepare_dgrad. */
int acimg_conv2d_split3_prepare_multi(int n, const AcimgConvDesc* const* descs, const float* const* w, void* const* out,
                                      const int* mode, void* stream);
int acimg_conv2d_fwd_split3_stats_rows(const AcimgConvDesc* d);
/* out[3] = {BM, BN, kernel of acimg_conv2d_fwd_split3p for this shape: 0 one tile per workgroup, 1 persistent, 2 ring} */
int acimg_conv2d_fwd_split3_tiling(const AcimgConvDesc* d, int* out);
int acimg_conv2d_fwd_split3(const AcimgConvDesc* d, const float* x, const void* wsplit, const float* bias,
                            float* y, const float* in_scale, const float* in_shift, int in_relu, float* stats,
                            void* stream);
/* Data gradient of a stride-1 conv on the same structure with a bf16 hi/lo split (gradients ~1e-7 are
 * outside fp16's range; bf16 keeps fp32's range, 16 mantissa bits, no scaling): a forward conv of gy with
 * the flipped + transposed kernel prepared by acimg_conv2d_split3_prepare_dgrad ([hi|lo][C][R*S*K] bf16,
 * acimg_conv2d_split3_dgrad_weight_bytes(d) bytes).  Needs K % 32 == 0.  residual / mask / lddx as in
 * acimg_conv2d_dgrad.
 * ARITHMETIC: on the 3x3 / SAME layers with image rows of 32 or 48 pixels, K >= 64 and C > 32 (wgrad_halo = 1) the same
 * format with K summed chunk-major (32 gy channels at a time, the nine taps inside) instead of tap-major. */
size_t acimg_conv2d_split3_dgrad_weight_bytes(const AcimgConvDesc* d);
int acimg_conv2d_split3_prepare_dgrad(const AcimgConvDesc* d, const float* w, void* wsplit, void* stream);
int acimg_conv2d_dgrad_split3(const AcimgConvDesc* d, const float* gy, int ldgy, const void* wsplit_t, float* dx,
                              int lddx, const float* residual, int ldres, const float* mask, int ldmask,
                              void* stream);

/* bf16 OPERAND ARITHMETIC (BASELINE configs[1], "bf16"): the same three convolutions with both GEMM operands ROUNDED to
 * bf16 and multiplied once per product (v_mfma_f32_16x16x32_bf16), fp32 accumulation; tensors in HBM, bias, batch
 * statistics, losses and the optimizer stay fp32 (the mixed-precision recipe of a bf16 network: what tf's
 * auto_mixed_precision / a bf16 cast at the conv inputs computes).  Same arguments, workspaces and epilogues as the
 * split3 entry points they mirror; 1/3 of the MFMAs, half the LDS traffic, results carry bf16's 8 mantissa bits per
 * operand (parity against the oracle WITH THE SAME ROUNDING: tests/test_unet_vae_gpu.py).
 *   acimg_conv2d_bf16_prepare : forward weight image (bf16 [hi|lo][ldw][R*S*C], acimg_conv2d_split3_weight_bytes)
 *   acimg_conv2d_fwd_bf16     : mirrors acimg_conv2d_fwd_split3
 *   acimg_conv2d_dgrad_bf16   : mirrors acimg_conv2d_dgrad_split3 (weights from acimg_conv2d_split3_prepare_dgrad)
 *   acimg_conv2d_wgrad_bf16   : mirrors acimg_conv2d_wgrad_split3
 * acimg_conv2d_split3_prepare_multi: mode 2 = the bf16 forward image.
 * Replaces: the conv2d calls of models/unet_architecture.py:159-213 under a bf16 policy. */
int acimg_conv2d_bf16_prepare(const AcimgConvDesc* d, const float* w, void* wsplit, void* stream);
int acimg_conv2d_fwd_bf16(const AcimgConvDesc* d, const float* x, const void* wsplit, const float* bias,
                          float* y, const float* in_scale, const float* in_shift, int in_relu, float* stats,
                          void* stream);
int acimg_conv2d_dgrad_bf16(const AcimgConvDesc* d, const float* gy, int ldgy, const void* wsplit_t, float* dx,
                            int lddx, const float* residual, int ldres, const float* mask, int ldmask,
                            void* stream);

/* Pre-split activation format: a tensor [rows][C] (C % 32 == 0, dense) is stored as TWO fp16 planes (hi at ptr, lo
 * `lo_off` bytes further, lo_off >= acimg_split_plane_bytes(rows, C), 16-byte aligned), hi = f16(v/4),
 * lo = f16(v/4 - hi): 22 mantissa bits in the same 4 bytes per element as fp32.  The elementwise producers below write
 * it (the BN affine + ReLU is already applied), and acimg_conv2d_fwd_split3p consumes it: both GEMM operands are then
 * plain 16-byte copies into LDS, so the K loop of the trunk convs carries no conversion / normalisation work at all.
 * A plane is laid out in LDS-TILE ORDER: ceil(rows / 16) x C / 32 bricks of 1 KiB, brick (row >> 4, c >> 5) at
 * ((row >> 4) * C / 32 + (c >> 5)) * 1024, inside it 16 rows (row & 15) of 64 bytes and the 16-byte group (c >> 3) & 3 of
 * a row at group ((c >> 3) ^ -(row >> 2)) & 3 - exactly the image the kernels keep in LDS, so an LDS-DMA request of the
 * K loop is one contiguous KiB (eight whole cache lines) instead of sixteen 64-byte pieces of sixteen rows.
 * When rows % 16 != 0 the last row of bricks has PAD ROWS (rows .. 16 ceil(rows / 16) - 1).  Their contents, and those of
 * any gap between the end of the hi plane and lo_off, are unspecified: buffers are shared between layers of different
 * shapes, so they may hold anything, NaN included.  No consumer lets them reach a result (convolution outputs,
 * statistics, fused tails, shortcuts read back from planes, acimg_gram_stats), and no producer writes outside
 * [0, plane_bytes) and [lo_off, lo_off + plane_bytes), plane_bytes = acimg_split_plane_bytes(rows, C).
 *   acimg_bn_relu_split:        planes = relu?(x*scale+shift)            (BN of a bottleneck conv, resnet50.py:109-121)
 *   acimg_bn_add_relu_split:     planes (+ optional fp32) = relu(a*sa+ta + shortcut); shortcut = b32*sb+tb
 *                                (projection) or the previous unit's planes (identity / subsample)   (resnet50.py:104-123)
 *   acimg_bn_relu_maxpool_split: planes = maxpool3x3/s2(relu(x*scale+shift))                        (resnet50.py:207-208) */
/* `ws` (optional, acimg_conv2d_fwd_split3p_workspace bytes, DEDICATED to these calls: its first 4 KiB are tile
 * tickets that must be zero before the first call and are left zero by every call) lets the kernel cut the tiles of
 * the last, partially filled round of workgroups into K ranges that meet in the workspace (deterministic: fixed
 * range order).  Without it every tile is computed by one workgroup. */
size_t acimg_conv2d_fwd_split3p_workspace(const AcimgConvDesc* d);
/* statistics rows acimg_conv2d_fwd_split3p writes for this shape under the current configuration (one per row tile of
 * the kernel it picks; acimg_conv2d_fwd_split1p keeps acimg_conv2d_fwd_split3_stats_rows) */
int acimg_conv2d_fwd_split3p_stats_rows(const AcimgConvDesc* d);
int acimg_conv2d_fwd_split3p(const AcimgConvDesc* d, const void* x_planes, size_t x_lo_off, const void* wsplit,
                             float* y, float* stats, void* ws, size_t ws_bytes, void* stream);
/* The same launch with fp16 OPERAND STORAGE (BASELINE configs[4]: "fp16 with fp32 loss accumulation"): only the hi
 * planes of activations and weights are fetched and multiplied - one fp16 MFMA per product instead of three, half the
 * operand bytes - with fp32 accumulation, fp32 batch-norm statistics and fp32 output.  Operands carry 11 significant
 * bits; everything else (arguments, tiling, statistics rows, workspace) is as for acimg_conv2d_fwd_split3p. */
int acimg_conv2d_fwd_split1p(const AcimgConvDesc* d, const void* x_planes, size_t x_lo_off, const void* wsplit,
                             float* y, float* stats, void* ws, size_t ws_bytes, void* stream);
/* The expanding 1x1 conv of an identity bottleneck unit in TWO PASSES, its raw output never stored (slim bottleneck,
 * models/resnet50.py:104-125: out = relu(BN(conv3(x)) + shortcut), batch statistics): the conv is short-K and 4x wide,
 * so its MFMA work is cheap and its output bytes are not.
 *   acimg_conv2d_fwd_split3p_stats: the K loop and the batch-norm partials only (rows as acimg_conv2d_fwd_split3p's);
 *   acimg_conv2d_fwd_split3p_tail:  the same tiles again with the layer's (scale, shift) from acimg_bn_finalize:
 *                                   relu(acc * scale + shift + shortcut) split into hi / lo planes in brick order;
 *                                   `sc_planes` is a split-format tensor of the output's shape (the unit's input),
 *                                   `out_planes` must not alias it.
 * Both need 128x128 tiles (>= 200 of them), K % 128 == 0, ldy == ldw == K, outputs < 2 GiB; same units in the same
 * order in both passes, so the statistics are those of exactly the values the second pass normalises.  Per output
 * element 4 B read + 4 B written instead of 4 written + 8 read + 4 written by conv + acimg_bn_add_relu_split. */
int acimg_conv2d_fwd_split3p_stats(const AcimgConvDesc* d, const void* x_planes, size_t x_lo_off, const void* wsplit,
                                   float* stats, void* ws, size_t ws_bytes, void* stream);
int acimg_conv2d_fwd_split3p_tail(const AcimgConvDesc* d, const void* x_planes, size_t x_lo_off, const void* wsplit,
                                  const float* scale, const float* shift, const void* sc_planes, size_t sc_lo_off,
                                  void* out_planes, size_t out_lo_off, void* ws, size_t ws_bytes, void* stream);
/* ... and of a unit with a PROJECTION shortcut (models/resnet50.py:112-118: shortcut = batch_norm(conv1x1(x))): `sc32` is the
 * raw fp32 [rows][K] output of the shortcut conv, (sc_scale, sc_shift) its affine from acimg_bn_finalize:
 * relu(acc * scale + shift + (sc32 * sc_scale + sc_shift)) -> split planes.  Same requirements as _tail. */
int acimg_conv2d_fwd_split3p_tail_proj(const AcimgConvDesc* d, const void* x_planes, size_t x_lo_off, const void* wsplit,
                                       const float* scale, const float* shift, const float* sc32, const float* sc_scale,
                                       const float* sc_shift, void* out_planes, size_t out_lo_off, void* ws, size_t ws_bytes,
                                       void* stream);
/* INPUT-SIDE batch-norm statistics of a 1x1 conv (round 4; replaces acimg_conv2d_fwd_split3p_stats + acimg_bn_finalize in
 * front of the fused tails above): for y = x w over `rows` pixels, sum_p y_n = w_n^T sum_p x and
 * sum_p y_n^2 = w_n^T (sum_p x x^T) w_n - the column sums and the C x C Gram matrix of the conv's INPUT (P C^2 MACs, a
 * quarter of the conv's, two fp16 MFMAs per product: a quadratic form only sees the symmetric part, hi hi^T + 2 hi lo^T).
 * Three launches on `stream` (csrc/gram.hip): Gram partials per pixel range (brick planes -> LDS by LDS-DMA, transposing
 * fragment reads), a deterministic reduce in double, and per 16 output channels the two forms by exact-f32 MFMA followed by
 * acimg_bn_finalize's arithmetic: `scale` / `shift` [K] for the conv's fused tail, the moving averages advanced (training
 * mode only; inference keeps acimg_bn_finalize with training = 0).
 *   x_planes / x_lo_off: the conv's input in split format [rows][C]; C = 64 or a multiple of 128 up to 512
 *   w: the conv's fp32 kernel [C][ldw] (TF layout [1, 1, C, K]); ws: acimg_gram_stats_workspace(rows, C) bytes, 16-byte aligned
 * Replaces: the moments slim batch_norm takes of conv3's output, models/resnet50.py:121-123 (is_training=True). */
size_t acimg_gram_stats_workspace(long rows, int C);
int acimg_gram_stats(const void* x_planes, size_t x_lo_off, long rows, int C, const float* w, int ldw, int K,
                     const float* gamma, const float* beta, float* moving_mean, float* moving_var, float decay, float eps,
                     float* scale, float* shift, void* ws, size_t ws_bytes, void* stream);
size_t acimg_split_plane_bytes(long rows, int C);
int acimg_bn_relu_split(const float* x, const float* scale, const float* shift, int relu, void* out,
                        size_t lo_off, long rows, int C, void* stream);
int acimg_bn_add_relu_split(const float* a, const float* sa, const float* ta, const float* b32,
                            const float* sb, const float* tb, const void* b_planes, size_t b_lo_off,
                            void* out_planes, size_t out_lo_off, float* out32, int N, int OH, int OW, int C,
                            int BH, int BW, int bstride, void* stream);
int acimg_bn_relu_maxpool_split(const float* x, const float* scale, const float* shift, void* out,
                                size_t lo_off, int N, int H, int W, int C, int OH, int OW, int pad_t, int pad_l,
                                void* stream);

/* Data gradient.  gy is the gradient w.r.t. the conv's PRE-activation output [N,OH,OW,K]
 * (pixel stride ldgy); dx = relu_mask(conv_T(gy, w) + residual): `residual` (optional, pixel
 * stride ldres) is another gradient flowing into x (fan-out), `mask` (optional, pixel stride
 * ldmask) is the saved post-ReLU activation x itself: dx is zeroed where mask <= 0, so dx is
 * the pre-activation gradient of the producing layer.  dx has pixel stride lddx (0 = d->ldx: the
 * gradient of a concat-slice input usually lives in its own, narrower buffer).  Geometries: stride 1 (direct),
 * stride == R == S with zero padding (non-overlapping patches, layer1/pool_2: scatter form), and any other
 * stride (the strided "pool" convs of models/unet_architecture.py:168-176, models/unet_sound.py:162-170) via a
 * zero-inserted copy of gy in the workspace followed by the stride-1 form.
 * ARITHMETIC: exact fp32 products EXCEPT, from 65536 input pixels (N H W) on (wgrad_halo = 1), the 3x3 layers with few
 * channels, which run bf16x3 (both operands split into bf16 hi / lo in fp32's exponent range: no scaling, no operand range,
 * no floor while gy stays fp32-normal; per product up to 2^-15 of |gy w|, acimg_conv2d_dgrad_split3 above): stride 1 or 2
 * without a mask, up4(K) = 8 or 16 gy channels into C % 4 == 0, C <= 32 (<= 16 unless up4(K) = 8; stride 2: C = 4, 8 or 12, read
 * from the zero-inserted VIEW of gy, no copy), and stride 1 / SAME with K = 32 into C <= 16 (mask and residual allowed).
 * OPERAND FORMS: gy, w, workspace and tickets 16-byte aligned, ldgy % 4 == 0; dx / residual / mask any float* and any
 * lddx / ldres / ldmask >= C (general kernel, same result) EXCEPT on the narrow-halo shape (the last one above), where a
 * dx / residual / mask off a 16-byte boundary or an lddx / ldres / ldmask that is no multiple of 4 is ACIMG_EINVAL.
 * Replaces: the Conv2DBackpropInput ops tf.gradients emits for the calls above
 *           (trainer/mfcctrainer.py:72-79). */
int acimg_conv2d_dgrad(const AcimgConvDesc* d, const float* gy, int ldgy, const float* w,
                       float* dx, int lddx, const float* residual, int ldres, const float* mask,
                       int ldmask, void* ws, size_t ws_bytes, void* tickets, void* stream);
size_t acimg_conv2d_dgrad_workspace(const AcimgConvDesc* d);

/* Weight + bias gradient: dw[R][S][C][ldw] = sum_pixels x (*) gy, db[k] = sum gy (db optional).
 * ARITHMETIC: exact fp32 products EXCEPT, from 65536 pixels on (wgrad_halo = 1), the 3x3 / stride 1 / SAME layers with
 * C < 32 (a multiple of 4) and K <= 32, which run bf16x3 - dw AND db - as acimg_conv2d_wgrad_split3 below does: per product
 * up to 2^-15 of |x gy|, no operand range and no floor while x and gy stay fp32-normal.
 * OPERAND FORMS (this entry, _split3, _bf16, _affine and acimg_deconv_wgrad): x, gy, dw, in_scale / in_shift and the workspace
 * 16-byte aligned, ldgy % 4 == 0; db any float*.  One value depends on that pointer: where acimg_conv2d_wgrad_bf16 needs no
 * slabs (at most wgrad_minpix pixels: the kernel writes dw and db itself, in 16-byte pieces), an aligned db is the sum of the
 * bf16-ROUNDED gy, and a db off a 16-byte boundary is the fp32 column sum of gy as given (its partials: the workspace).
 * Replaces: Conv2DBackpropFilter / BiasAddGrad (trainer/mfcctrainer.py:72-79). */
int acimg_conv2d_wgrad(const AcimgConvDesc* d, const float* x, const float* gy, int ldgy,
                       float* dw, float* db, void* ws, size_t ws_bytes, void* stream);
size_t acimg_conv2d_wgrad_workspace(const AcimgConvDesc* d);
/* the same on the bf16x3 MFMA path: x and gy are split into bf16 hi/lo on the fly (gradients need fp32's
 * range), 3 MFMAs per product, fp32 accumulate; fragments come out of LDS through ds_read_b64_tr_b16
 * because the reduction runs over pixels.  Same workspace as acimg_conv2d_wgrad. */
int acimg_conv2d_wgrad_split3(const AcimgConvDesc* d, const float* x, const float* gy, int ldgy,
                              float* dw, float* db, void* ws, size_t ws_bytes, void* stream);
int acimg_conv2d_wgrad_bf16(const AcimgConvDesc* d, const float* x, const float* gy, int ldgy,
                            float* dw, float* db, void* ws, size_t ws_bytes, void* stream);
/* A batch-norm + ReLU between two convs without a pass of its own (round 4): the consumer applies the producer's
 * (scale, shift) and the ReLU while it stages its input tile - x' = relu(x * in_scale[c] + in_shift[c]) inside the
 * image, zero padding after the affine - so the normalised activation is never written.  The forward entries above
 * already carry in_scale / in_shift / in_relu; this is the weight gradient of the same layer with the same view of
 * its input.  precision: 0 = the acimg_conv2d_fwd / _wgrad arithmetic, 1 = _split3, 2 = _bf16.  Only the halo
 * kernels stage through registers and can do this: acimg_conv2d_affine_input_ok(d, precision) is 1 when BOTH the
 * forward and the weight gradient of this layer take the affine (3x3 / stride 1 / SAME, <= 32 output channels, from
 * 65536 pixels on); acimg_conv2d_wgrad_affine fails loudly on any other shape.  Workspace: acimg_conv2d_wgrad_workspace.
 * Replaces: the read side of tf.layers.batch_normalization + tf.nn.relu between two tf.layers.conv2d
 * (models/unet_architecture.py:55-60). */
int acimg_conv2d_affine_input_ok(const AcimgConvDesc* d, int precision);
int acimg_conv2d_wgrad_affine(const AcimgConvDesc* d, int precision, const float* x, const float* in_scale,
                              const float* in_shift, int in_relu, const float* gy, int ldgy, float* dw, float* db,
                              void* ws, size_t ws_bytes, void* stream);

/* Transposed convolution, VALID (TF output = in*stride + max(kernel - stride, 0)):
 *   x : [N,H,W,C] low-res input, y : [N,OH,OW,K], w : [R][S][K][ldw>=C].
 *   kernel <= stride in both directions (unet_acresnet.py:210-217): scatter form, gaps receive the bias;
 *   kernel >= stride with overlap (unet_architecture.py:72,78 kernel [2,3]; unet_sound.py:82,85 kernels [3,2],
 *   [3,3]): zero-inserted copy of x in the workspace, then a stride-1 full correlation with the flipped kernel.
 * Every input pixel writes a disjoint RxS patch; the remaining positions get the bias only.
 * ARITHMETIC: exact fp32 products EXCEPT the 2x2 / stride-2 layer with C = 32 and K = 8 from 65536 INPUT pixels on
 * (wgrad_halo = 1; unet_architecture.py upsample_9), one 32 x 32 product per input pixel: acimg_deconv_fwd runs f16x3 - the
 * operand range |w| < 63, |x| < 2.6e5 and the floors 2^-23 per activation / 2^-35 per weight of acimg_conv2d_fwd_split3 apply,
 * the bias is added in fp32 - and acimg_deconv_dgrad / acimg_deconv_wgrad run bf16x3 (per product up to 2^-15 of |gy w| /
 * |gy x|; no range, no floor); the bias gradient of that route is an fp32 sum of gy and never meets the split.
 * OPERAND FORMS: x / gy, w, workspace and tickets 16-byte aligned; y / dx, bias and mask any float*, ldy / ldmask any value
 * at or above the channel count (the gap fill follows the scatter's epilogue onto scalar stores).
 * Replaces: tf.layers.conv2d_transpose  models/unet_acresnet.py:210-217 (call :86). */
int acimg_deconv_fwd(const AcimgConvDesc* d, const float* x, const float* w, const float* bias,
                     float* y, void* ws, size_t ws_bytes, void* tickets, void* stream);
int acimg_deconv_dgrad(const AcimgConvDesc* d, const float* gy, int ldgy, const float* w,
                       float* dx, const float* mask, int ldmask, void* ws, size_t ws_bytes,
                       void* tickets, void* stream);
int acimg_deconv_wgrad(const AcimgConvDesc* d, const float* x, const float* gy, int ldgy,
                       float* dw, float* db, void* ws, size_t ws_bytes, void* stream);
size_t acimg_deconv_workspace(const AcimgConvDesc* d);

/* ------------------------------------------------------------------------------------------
 * Batch-norm pieces of the frozen ResNet-50 trunk (slim batch_norm, decay .997, eps 1e-5,
 * batch statistics while training: models/vision.py:55-56, trainer/mfcctrainer.py:348-349).
 * ---------------------------------------------------------------------------------------- */
/* Reduce the per-row-block partials of acimg_conv2d_fwd into scale/shift:
 *   mean = S1/count, var = S2/count - mean^2 (biased), scale = gamma/sqrt(var+eps),
 *   shift = beta - mean*scale; if training: moving_mean/var <- decay*old + (1-decay)*new with the
 *   UNBIASED variance (fused-BN semantics); save_mean/save_invstd optional.
 * If training == 0 the moving statistics are used instead of the partials. */
int acimg_bn_finalize(const float* stats, int rows, int C, int ldstats, double count,
                      const float* gamma, const float* beta, float* moving_mean,
                      float* moving_var, float decay, float eps, int training, float* scale,
                      float* shift, float* save_mean, float* save_invstd, void* stream);

/* ------------------------------------------------------------------------------------------
 * DualCamNet classifier head on generated acoustic images (models/dualcamnet.py:82-106,
 * trainer/trainer_reconstructed_class.py:44-56).  The convs / FCs are acimg_conv2d_* (the temporal
 * 12x1x1 conv3d is a 12x1 conv over a [clips, 12, 36*48, 12] view).
 * ---------------------------------------------------------------------------------------- */
/* tf.nn.max_pool k x k, stride k, VALID (models/base.py:34-38): y [N, H/k, W/k, C]. */
int acimg_maxpool_fwd(const float* x, int ldx, float* y, int ldy, int N, int H, int W, int C, int k, void* stream);
/* gx[N,H,W,C] = gradient w.r.t. the PRE-activation of the ReLU that produced x: gy of the window at its first
 * maximum if x > 0, else 0 (positions outside every window get 0). */
int acimg_maxpool_relu_bwd(const float* x, int ldx, const float* gy, int ldgy, float* gx, int ldgx, int N, int H,
                           int W, int C, int k, void* stream);
/* tf.reduce_sum(x, axis=[1,2]) (dualcamnet.py:96): y[n][c] = sum_p x[n][p][c]; and its backward through the ReLU
 * that produced x: gx[n][p][c] = x > 0 ? gy[n][c] : 0. */
int acimg_spatial_sum(const float* x, int ldx, float* y, int N, int P, int C, void* stream);
int acimg_spatial_sum_relu_bwd(const float* x, int ldx, const float* gy, float* gx, int ldgx, int N, int P, int C,
                               void* stream);
/* logits [clips*F, ldl] -> mean over the F frames of a clip -> tf.losses.softmax_cross_entropy (mean over clips)
 * and tf.argmax accuracy (trainer_reconstructed_class.py:49-56): out[0] += loss, out[1] += #correct (zero them
 * first); g_logits (optional) = d loss / d logits.  labels: int32 class per clip.  classes <= 64. */
int acimg_clip_softmax_ce(const float* logits, int ldl, int clips, int F, int K, const int* labels, float* out,
                          float* g_logits, int ldg, void* stream);

/* Dataset-level evaluation of clip logits, accumulated on the device: a whole validation / test pass calls this once per
 * batch and reads `state` back once at its end.  Per clip the rule is acimg_clip_softmax_ce's: the fp32 sum of the F
 * frame logits in frame order, divided by F; softmax cross-entropy against labels[clip]; prediction = the lowest index
 * among exact ties at the maximum (tf.argmax).
 * state (acimg_clip_eval_state_bytes(K) = 32 + 4*K*K bytes, 8-byte aligned, ZEROED BY THE CALLER before a pass):
 *   double  loss_sum            sum of the per-clip losses
 *   int64   clips               clips with a label in [0, K)
 *   int64   correct             of those, prediction == label
 *   int64   invalid             clips with a label outside [0, K): counted here and in nothing else
 *   int32   confusion[K][K]     row = label, column = prediction
 * loss_sum is a SEQUENTIAL fold: starting from the value already in state, the fp32 loss of clip 0, 1, ..., clips-1
 * (converted to double) is added in that order, clips with an invalid label skipped.  The counters are integers; no
 * float atomics are used, so two identical passes leave bit-identical state.
 * clip_loss [clips] float32 (optional): per-clip loss, 0 for an invalid label.  clip_pred [clips] int32 (optional): the
 * prediction (also for an invalid label).  One launch per call whatever `clips` is (any clips >= 1); no host
 * synchronisation.  1 <= K <= 64, F >= 1, ldl >= K; logits, labels and state must be given (else ACIMG_EINVAL).
 * acimg_clip_eval_state_bytes returns 0 for K outside 1..64. */
size_t acimg_clip_eval_state_bytes(int K);
int acimg_clip_eval(const float* logits, int ldl, int clips, int F, int K, const int* labels, float* clip_loss,
                    int* clip_pred, void* state, void* stream);

/* Training-mode batch-norm + ReLU backward for the conv-BN-ReLU stacks of the RGB / spectrogram U-Nets
 * (tf.layers.batch_normalization(training=True) + relu, models/unet_architecture.py:161-166,
 * models/unet_sound.py:155-160).  x = the pre-BN conv output (bias included), gy = gradient w.r.t. the ReLU
 * output; the ReLU mask is recomputed as x*scale+shift > 0 (scale/shift/save_* from acimg_bn_finalize):
 *   dbeta = sum g, dgamma = sum g*xhat, gx = gamma*invstd*(g - dbeta/n - xhat*dgamma/n).
 * gx may alias gy.  C % 4 == 0, C <= 1024.  Deterministic (ordered partial sums). */
size_t acimg_bn_bwd_workspace(long rows, int C);
int acimg_bn_bwd(const float* x, int ldx, const float* gy, int ldgy, const float* scale, const float* shift,
                 const float* save_mean, const float* save_invstd, const float* gamma, long rows, int C,
                 float* gx, int ldgx, float* dgamma, float* dbeta, void* ws, size_t ws_bytes, void* stream);

/* out = relu(a*sa[c]+ta[c] + shortcut), shortcut = b*sb[c]+tb[c] (sb given) or b (identity),
 * b read with spatial subsampling `bstride` (resnet_utils.subsample, models/resnet50.py:107).
 * a,out: [N,OH,OW,C]; b: [N,OH*bstride.. ,C]. Replaces models/resnet50.py:123. */
int acimg_bn_add_relu(const float* a, const float* sa, const float* ta, const float* b,
                      const float* sb, const float* tb, float* out, int N, int OH, int OW, int C,
                      int BH, int BW, int bstride, void* stream);

/* pool1: out = maxpool3x3/s2 'SAME' over relu(x*scale+shift) (models/resnet50.py:207-208). */
int acimg_bn_relu_maxpool(const float* x, const float* scale, const float* shift, float* out,
                          int N, int H, int W, int C, int OH, int OW, int pad_t, int pad_l,
                          void* stream);

/* y = relu(x*scale+shift) materialised (conv_map output feature, models/resnet50.py:208-209) */
int acimg_bn_relu(const float* x, const float* scale, const float* shift, float* y, long rows,
                  int C, int ldx, int ldy, void* stream);

/* Backward of y = relu(gamma*(x-mean)*invstd+beta) in batch-statistics mode for a small-C map
 * (conv_map, C=12): g_x, dgamma, dbeta from g_y. x,gy,y,gx: [rows,C] dense. */
int acimg_bn_relu_bwd(const float* x, const float* y, const float* gy, const float* gamma,
                      const float* save_mean, const float* save_invstd, float* gx, float* dgamma,
                      float* dbeta, long rows, int C, void* stream);

/* [N,H,W,3] -> [N,H,W,4] zero padded (stem input; lets the stem use 16-byte loads) */
int acimg_pad_channels(const float* x, float* y, long pixels, int C, int Cp, void* stream);

/* [N,H,W,C] -> the interior (at pad_t, pad_l) of a [N,Hp,Wp,Cp] frame the caller zeroed once: explicit zero
 * padding for the stem (resnet_utils.conv2d_same pads 3 + 3 before the VALID 7x7/2, models/resnet50.py:205),
 * so that the stem can run as a row-run convolution (acimg_conv2d_fwd_split3). */
int acimg_pad_image(const float* x, float* y, int N, int H, int W, int C, int Cp, int Hp, int Wp, int pad_t,
                    int pad_l, void* stream);

/* ------------------------------------------------------------------------------------------
 * Generator-side elementwise / reduction ops (models/unet_acresnet.py, trainer/mfcctrainer.py)
 * ---------------------------------------------------------------------------------------- */
/* tf.tile of the MFCC vector: out[n,h,w,c] = mfcc[n,c]   (trainer/mfcctrainer.py:38-40) */
int acimg_tile_mfcc(const float* mfcc, float* out, int N, int HW, int C, void* stream);

/* Per-sample min-max normalisation o = (x-min)/(max-min) over `cnt` = P*C logical elements of
 * sample n (x pixel stride ldx, out pixel stride ldo, written at out+0: pass an offset pointer to
 * write into a concat slice).  mm[n] = {min, max, #argmin, #argmax} saved for backward.
 * Every sample is cut into pixel chunks (one workgroup each); the per-chunk partials live in `ws`
 * (acimg_minmax_workspace(N, P, C) bytes, scratch: nothing is kept there between calls).
 * Replaces models/unet_acresnet.py:55-58, :70-71. */
size_t acimg_minmax_workspace(int N, int P, int C);
int acimg_minmax_fwd(const float* x, int ldx, float* out, int ldo, float* mm, int N, int P, int C, void* ws,
                     size_t ws_bytes, void* stream);
/* Gradient incl. the reduce_min / reduce_max paths with equal tie splitting (App. B.8).
 * gx = [accumulate? gx : 0] + d/dx; then zeroed where relu_mask (=x itself) <= 0 if mask_relu. */
int acimg_minmax_bwd(const float* x, int ldx, const float* go, int ldgo, const float* mm,
                     float* gx, int ldgx, int N, int P, int C, int accumulate, int mask_relu, void* ws,
                     size_t ws_bytes, void* stream);

/* heads [N,2*Z] = (mean | std_raw) -> sigma = softplus(std_raw), z = mean + sigma*eps,
 * kl[n] = 0.5*sum(mean^2+sigma^2-log(1e-8+sigma^2)-1).  z has row stride ldz (pads untouched).
 * Replaces models/unet_acresnet.py:73-78 and trainer/mfcctrainer.py:56-58. */
int acimg_latent_fwd(const float* heads, const float* eps, float* z, int ldz, float* sigma,
                     float* kl, int N, int Z, void* stream);
/* g_heads from gz (row stride ldgz) and the KL term weighted by kl_weight (= latent_loss / N) */
int acimg_latent_bwd(const float* heads, const float* eps, const float* sigma, const float* gz,
                     int ldgz, float kl_weight, float* g_heads, int N, int Z, void* stream);

/* Same without the softplus: the second head IS sigma (models/unet_architecture.py:62-69,
 * models/unet_sound.py:65-72: guessed_z = mean + variance * samples).  heads = [N][2Z] = [mean | sigma];
 * kl[n] = 0.5 * sum_j (mu^2 + s^2 - log(1e-8 + s^2) - 1)  (trainer/trainer.py:61-62 takes the mean over j:
 * fold 1/Z into the weights). */
int acimg_latent_linear_fwd(const float* heads, const float* eps, float* z, int ldz, float* kl, int N, int Z,
                            void* stream);
int acimg_latent_linear_bwd(const float* heads, const float* eps, const float* gz, int ldgz, float kl_weight,
                            float* g_heads, int N, int Z, void* stream);

/* y = softplus(x) and gx = gy * sigmoid(x) on [rows][C] tensors with row strides (the std tower of the latent
 * associators: tf.nn.softplus(tf.layers.dense(...)), models/multimodal.py:47-48,106-107). */
int acimg_softplus_fwd(const float* x, int ldx, float* y, int ldy, int rows, int C, void* stream);
int acimg_softplus_bwd(const float* x, int ldx, const float* gy, int ldgy, float* gx, int ldgx, int rows, int C,
                       void* stream);

/* "Tap GEMM" form of a stride-1 VALID convolution with few output channels (d->K <= 64; the trunk's conv_map,
 * models/resnet50.py:205-209 / models/vision.py:60-66: 3x4, 2048 -> 12).  With T = R*S*K:
 *   pack:    wt[c][tap*K + k] = w[tap][c][k]                 (then split / multiply it as a 1x1 conv C -> T)
 *   gather:  y[(n,oh,ow)][k] = sum_taps z[(n,oh+r,ow+s)][tap*K + k]  from z = x . wt over the INPUT pixels;
 *            optional batch-norm partials stats[acimg_tapconv_stats_rows(d)][2][d->ldw]
 *   scatter: gz[(n,ih,iw)][tap*K + k] = gy[(n,ih-r,iw-s)][k]  (0 outside), so that dwt = x^T . gz is a 1x1
 *            weight gradient
 *   unpack:  dw[tap][c][k] = dwt[c][tap*K + k] + decay * w[tap][c][k]   (w optional: slim's L2 term)
 * d is the descriptor of the ORIGINAL convolution. */
int acimg_tapconv_stats_rows(const AcimgConvDesc* d);
int acimg_tapconv_pack(const AcimgConvDesc* d, const float* w, float* wt, int ldwt, void* stream);
int acimg_tapconv_unpack(const AcimgConvDesc* d, const float* dwt, int ldwt, const float* w, float decay, float* dw,
                         void* stream);
int acimg_tapconv_gather(const AcimgConvDesc* d, const float* z, int ldz, float* y, float* stats, void* stream);
int acimg_tapconv_scatter(const AcimgConvDesc* d, const float* gy, int ldgy, float* gz, int ldgz, void* stream);

/* Cross-modal triplet losses over B embedding pairs e0[B][D], e1[B][D] with int32 labels / scenario per sample
 * (trainer/trainer_three.py): distances as `_pairwise_distances` :551-591 computes them (squared form,
 * D[i][j] = max(|e0_j|^2 - 2 <e0_i, e1_j> + |e1_i|^2, 0)); a pair (i, j) is "same video" when label and scenario
 * agree (:593-624); hard = 0: batch-all loss `mix_all` :685-732 (sum over valid triplets of max(D[a][p] - D[a][n] +
 * margin, 0) / (number of positive ones + 1e-16)); hard = 1: batch-hard loss `mix_data_hard` :648-683.
 * out[0] = loss, out[1] = fraction of positive triplets, out[2] = positive count, out[3] = valid count.
 * The forward leaves what the backward needs in ws (acimg_triplet_loss_workspace(B) bytes, B <= 2048);
 * bwd: g0 / g1 (either may be null) (+)= weight * d loss / d e0, e1, with TensorFlow's gradient conventions
 * (tf.maximum passes the gradient at equality; reduce_max / reduce_min split it evenly among ties). */
size_t acimg_triplet_loss_workspace(int B);
int acimg_triplet_loss_fwd(const float* e0, int lde0, const float* e1, int lde1, const int* labels,
                           const int* scenario, int B, int D, float margin, int hard, void* ws, size_t ws_bytes,
                           float* out, void* stream);
int acimg_triplet_loss_bwd(const float* e0, int lde0, const float* e1, int lde1, int B, int D, float weight,
                           const void* ws, size_t ws_bytes, float* g0, int ldg0, float* g1, int ldg1,
                           int accumulate, void* stream);

/* Reconstruction loss on yhat = sigmoid output and its gradient w.r.t. the PRE-sigmoid logits:
 *   sums[0] += sum (yhat-y)^2, sums[1] += sum huber_1(yhat-y)   (caller zeroes sums)
 *   g_logit = (w_mse*2e + w_huber*clip(e,-1,1)) / count * yhat*(1-yhat)
 * Replaces tf.losses.mean_squared_error / huber_loss, trainer/mfcctrainer.py:47,50. */
/* `scratch` (optional; acimg_loss_scratch_bytes() bytes, zeroed ONCE by the caller and dedicated to acimg_recon_loss /
 * acimg_sumsq calls of one stream) makes the two sums bit-reproducible: the workgroups' partials are combined in
 * workgroup order by the last arriver instead of by float atomics. */
size_t acimg_loss_scratch_bytes(void);
int acimg_recon_loss(const float* yhat, const float* target, float* g_logit, float* sums,
                     long count, float w_mse, float w_huber, void* scratch, size_t scratch_bytes, void* stream);

/* dst[p][c] = (accumulate ? dst : 0) + src[p][c] for c < C, zeroed where mask[p][c] <= 0 (mask
 * optional): routes the gradient of one channel slice of a tf.concat back to its producer
 * (models/unet_acresnet2skip.py:82, models/unet_acresnet.py:197-198). */
int acimg_grad_slice(const float* src, int ldsrc, float* dst, int lddst, const float* mask, int ldmask,
                     long pixels, int C, int accumulate, void* stream);

/* out[5] = {mse, huber, latent, reg, total}: mse = sums[0]/count, huber = sums[1]/count,
 * latent = latent_w * mean_n kl[n] (kl may be NULL: auto-encoder mode), reg = half_wd * sums[2],
 * total = latent + w_mse*mse + w_huber*huber + reg   (trainer/mfcctrainer.py:46-62). */
int acimg_loss_finalize(const float* sums, const float* kl, int N, double count, float latent_w,
                        float half_wd, float w_mse, float w_huber, float* out, void* stream);

/* out[i] ~ N(0,1), i < n: Philox4x32-10 keyed by `seed`, counter = offset + i/4, Box-Muller.
 * Stands where the reference samples tf.random_normal (models/unet_acresnet.py:77). */
int acimg_randn(float* out, long n, uint64_t seed, uint64_t offset, void* stream);

/* stream-ordered memset to zero (loss accumulators, gradient buffers) */
int acimg_zero(void* ptr, size_t bytes, void* stream);
/* A load for stream-concurrency probes: ONE wave keeps `stream` busy for `cycles` shader cycles (s_memtime; bounded by
 * 2^32) and then writes the elapsed cycles to out[0] (4 bytes, device memory).  The host library uses it to find HIP
 * streams that really run beside each other (the runtime maps streams onto a few hardware queues). */
int acimg_spin(uint64_t cycles, void* out, void* stream);

/* out[c] += sum over pixels of (a-b)^2 for channel c (dense [pixels][C], C<=64; caller zeroes out):
 * the per-3-channel test MSEs of trainer/mfcctrainer.py:105-117 are sums of 3 of these / count. */
int acimg_sqerr_channels(const float* a, const float* b, long pixels, int C, float* out, void* stream);

/* sum of squares of a flat buffer into *out (+=; `scratch` as for acimg_recon_loss) — slim l2_regularizer terms
 * (models/vision.py:54, tf.losses.get_total_loss trainer/mfcctrainer.py:60). */
int acimg_sumsq(const float* x, long n, float* out, void* scratch, size_t scratch_bytes, void* stream);
/* y += a*x */
int acimg_axpy(float a, const float* x, float* y, long n, void* stream);

/* TF-1 Adam (tf.train.AdamOptimizer, trainer/mfcctrainer.py:72-79):
 *   m=b1 m+(1-b1)g; v=b2 v+(1-b2)g^2; p -= lr_t * m/(sqrt(v)+eps), lr_t precomputed by host. */
int acimg_adam_step(float* p, const float* g, float* m, float* v, long n, float lr_t, float beta1,
                    float beta2, float eps, float grad_scale, void* stream);

/* ------------------------------------------------------------------------------------------
 * Audio front end (dataloader/outdoor_data_mfcc.py:796-876): one 1024-sample int32 frame ->
 * 12 MFCCs: Tukey(.75) window, rFFT-1024 (Nyquist dropped), power, 24 mel filters, floor 1e-3,
 * log, DCT(12)*sqrt(2/24), lifter(22).  window[1024], melfb[512*24] (row-major [bin][filter]),
 * dctl[24*12] (DCT*norm*lifter folded) are float64 tables built by the host exactly as the
 * reference does; the kernel computes in fp64 like NumPy and rounds to float32 at the end (:823).
 * normalize != 0 also applies the per-vector min-max of _normalize_mfcc (:696-703).
 * ---------------------------------------------------------------------------------------- */
int acimg_mfcc_frontend(const int32_t* frames, const double* window, const double* melfb,
                        const double* dctl, float* out, int nframes, int normalize, void* stream);
/* the same on float32 frames: the low-passed ("silence") waveform of butter_lowpass_filter, which the reference
 * feeds to the same function (dataloader/outdoor_data_mfcc.py:791-792) */
int acimg_mfcc_frontend_f32(const float* frames, const double* window, const double* melfb,
                            const double* dctl, float* out, int nframes, int normalize, void* stream);

/* STFT magnitude of the older audio path (dataloader/outdoor_data.py:844-851: tf.contrib.signal.stft(frame_length 246,
 * frame_step 122, fft_length 512) + tf.abs): wav [clips][nsamples] float32 -> out [clips][frames][257] float32,
 * frames = 1 + (nsamples - frame_len) / step (pad_end = False; 12288 samples -> 99 x 257).  window[frame_len]
 * (periodic Hann, float32) and twiddle[256][2] (exp(-2 pi i j / 512), float32 from float64) are host tables.  norm
 * (optional, [clips]) divides every sample first: the `wav / max |wav|` of _build_wav_py_function (:577-596); get it
 * from acimg_absmax.  fp32 arithmetic like TensorFlow's rfft. */
int acimg_stft_mag(const float* wav, const float* norm, const float* window, const float* twiddle, float* out,
                   int clips, int nsamples, int frame_len, int step, int fft_len, void* stream);
/* out[r] = max_i |x[r][i]|   (x: [rows][n]) */
int acimg_absmax(const float* x, int rows, int n, float* out, void* stream);

/* tf.image.resize_bilinear(x, [OH, OW], align_corners=False) with TF-1 sampling (src = dst * in/out, no half-pixel
 * centres), NHWC float32.  Replaces: trainer/trainer.py:367-369 (99x257 spectrogram -> 193x257). */
int acimg_resize_bilinear(const float* x, float* y, int N, int H, int W, int C, int OH, int OW, void* stream);

/* scipy.signal.filtfilt(b, a, x) along the last axis for 11-tap (order-10) IIR filters, default padding (odd
 * extension, padlen 33), float64 arithmetic without fused multiply-adds, float32 out:
 * dataloader/outdoor_data_mfcc.py:565-575 (butter_lowpass_filter, the "silence" variant of the MFCC input).
 * x: [rows][n] int32 (x_is_int32 != 0, the raw audio frames) or float32; ba: b[11] then a[11] (a[0] = 1);
 * zi: scipy.signal.lfilter_zi(b, a) [10]; ws: acimg_filtfilt_workspace(rows, n) bytes. */
int acimg_filtfilt(const void* x, int x_is_int32, int rows, int n, const double* ba, const double* zi, float* out,
                   void* ws, size_t ws_bytes, void* stream);
size_t acimg_filtfilt_workspace(int rows, int n);

/* find_logen energy map (iouenergythreshold.py:294-323): mfcc image [pixels,12] -> [pixels] */
int acimg_find_logen(const float* mfcc_img, const double* idct /*12x24*/, float* out, long pixels,
                     void* stream);

/* Mean-threshold IoU of two energy maps per sample (iouenergythreshold.py:213-229): m = map > mean(map),
 * iou[n] = |m_a & m_b| / |m_a | m_b|.  map_a, map_b: [N][P] float32 (acimg_find_logen outputs). */
int acimg_mask_iou(const float* map_a, const float* map_b, int N, int P, float* iou, void* stream);

/* Consensus bounding-box IoU of the Flickr-SoundNet evaluation (showimages_bb.py:286-320), per sample n < N:
 *   m2   = map > mean(map)        (the fp64 mean of acimg_mask_iou, so both metrics threshold alike)
 *   m2   = cv2.resize(m2 * 1.0, (298, 224)) > 0.5   (INTER_LINEAR: half-pixel mapping, float32 weights clamped at the
 *          borders, applied in float64 without fused multiply-adds; the strict > 0.5 is decided exactly)
 *   mtot = min(1, sum over annotators k < 3 with xmax[k] != 0 of 0.5 * filled closed rectangle, clipped to the frame)
 *   iou  = sum(m2 * mtot) / sum((m2 | mtot > 0) + mtot - (mtot > 0));  0 / 0 = NaN as in the reference.
 * logen: [N][36*48] float32 (acimg_find_logen outputs); boxes: [N][4][3] int32 = xmin[3], xmax[3], ymin[3], ymax[3]
 * (dataloader/frames.py:290-297); iou: [N].  Optional (NULL = not written): counts [N][2] int32 = numerator and
 * denominator in half-units (exact integers; iou = counts[0] / counts[1]); mask_out [N][224][298] uint8 = the resized
 * mask m2 (0 / 1).  ws: acimg_box_iou_workspace(N) bytes.  Stream-ordered, deterministic, no atomics. */
int acimg_box_iou(const float* logen, const int32_t* boxes, int N, float* iou, int32_t* counts, uint8_t* mask_out,
                  void* ws, size_t ws_bytes, void* stream);
size_t acimg_box_iou_workspace(int N);

/* Localisation overlay, the picture of showvideo.py:213-233, showimages.py:136-154 and showimages_bb.py:240-285: the
 * energy map in the `lut_over` colours blended at alpha = alpha_num / alpha_den over the grey frame in the `lut_base`
 * colours (the reference: jet at 0.7 over gray), RGB8 at the frame's native 224 x 298.  Per sample n < N, inputs finite:
 *   g    = (F0 * 0.114f + F1 * 0.587f) + F2 * 0.299f in fp32, every product and sum rounded on its own: cv2.cvtColor(im,
 *          COLOR_BGR2GRAY) on a float image (:224 / :144 / :246), restated, not pinned
 *   g    = 1.0f on the outline of every annotator k < 3 with xmax[k] != 0 (boxes != NULL): with the corners sorted as
 *          acimg_box_iou sorts them, x0 <= x1 and y0 <= y1, a pixel (x, y) of the frame is on the outline when
 *          x0-1 <= x <= x1+1 and y0-1 <= y <= y1+1 and it is not strictly inside (x0+2 <= x <= x1-2 and y0+2 <= y <=
 *          y1-2).  This stands for cv2.rectangle(imgray, ..., (1, 1, 1), 3) (showimages_bb.py:247-250); it is THIS
 *          LIBRARY'S rule for a 3-pixel line - restated, not pinned, and the corner pixels are ours, not OpenCV's
 *   v    = cv2.resize(map, (298, 224)) of the energy map promoted to float64 (find_logen returns float64): INTER_LINEAR,
 *          half-pixel mapping, float32 weights clamped at the borders, float64 products and sums, horizontal then
 *          vertical, no fused multiply-adds - acimg_box_iou's resize before its threshold
 *   gmin, gmax over the sample's 224 x 298 values of g (outlines included); vmin, vmax over its values of v
 *   index(a) = trunc(t * 256) with t = (a - amin) / (amax - amin), an IEEE-correct division; 255 where t * 256 == 256;
 *          0 where amax == amin; fp32 for g, fp64 for v; clamped to 0..255 - matplotlib's Normalize() + colormap lookup
 *          (plt.imshow without vmin / vmax), pinned against matplotlib by the tests
 *   out[y][x][c] = (alpha_num * lut_over[index(v)][c] + (alpha_den - alpha_num) * lut_base[index(g)][c] + alpha_den / 2)
 *          / alpha_den in integer arithmetic: alpha_num = 0 gives the base layer, alpha_num = alpha_den the overlay.
 * frames: [N][224][298] pixels of ldf >= 3 floats (the first three are read); logen: [N][36*48] float32
 * (acimg_find_logen outputs); boxes: [N][4][3] int32 as acimg_box_iou reads them, or NULL (no outlines); lut_base,
 * lut_over: [256][3] uint8 device tables, used as given.  0 <= alpha_num <= alpha_den, 1 <= alpha_den <= 255.
 * out: sample n, row y starts at out + n * image_bytes + y * row_bytes and receives 894 bytes; row_bytes >= 894,
 * image_bytes >= 223 * row_bytes + 894; no other byte of the canvas is touched, so two panels side by side are two
 * calls with `out` offset.  ws: acimg_overlay_render_workspace(N) bytes, 8-byte aligned.  A null or ill-sized argument
 * is ACIMG_EINVAL, a short workspace ACIMG_EWORKSPACE, both before any launch.
 * Stream-ordered, deterministic, no atomics. */
int acimg_overlay_render(const float* frames, int ldf, const float* logen, const int32_t* boxes, const uint8_t* lut_base,
                         const uint8_t* lut_over, int alpha_num, int alpha_den, uint8_t* out, long row_bytes,
                         long image_bytes, int N, void* ws, size_t ws_bytes, void* stream);
size_t acimg_overlay_render_workspace(int N);

/* ------------------------------------------------------------------------------------------
 * TensorBoard summaries (acimg/logger.py, the logger of trainer/mfcctrainer.py:255-297,343-357): the two reductions that
 * turn device tensors into summary values without copying the tensors to the host.  (Added without raising
 * ACIMG_VERSION: nothing existing changed, and the number is pinned by the host tests.)
 * ---------------------------------------------------------------------------------------- */
/* tf.summary.image on float input (TF 1.x NormalizeFloatImage, restated, not pinned), three channels at a time.
 * x: images of HW pixels of ldc floats, image n at x + n * HW * ldc.  For every image n < n_images and group g < G the
 * slice S = channels c0 + 3g .. c0 + 3g + 2 of that image's HW pixels is rendered, in fp32:
 *   image_min, image_max = min / max over the FINITE values of S (+inf / -inf when there is none)
 *   image_min < 0:  m = max(|image_min|, |image_max|), scale = m < 1e-6f ? 0 : 127 / m, offset = 128
 *   otherwise:      scale = image_max < 1e-6f ? 0 : 255 / image_max, offset = 0          (IEEE-correct divisions)
 *   a pixel with a non-finite channel -> (255, 0, 0)
 *   every other channel value v -> (uint8) trunc(v * scale + offset): an fp32 multiply FOLLOWED BY an fp32 add, two
 *   roundings, never one fused operation (the source is compiled with contraction off); the integer is clamped to
 *   0 .. 255, which no finite v of S leaves.
 * out: uint8 [n_images][G][HW][3], dense, any alignment.  0 <= c0, c0 + 3G <= ldc, HW, G, n_images >= 1, no null
 * pointer: otherwise ACIMG_EINVAL before the launch.  ONE launch, one workgroup per (image, group): the reduction (min
 * and max: the same value in any order), then the store pass with plain vector-memory byte stores.  No atomics, no
 * workspace, stream-ordered, bit-identical from run to run. */
int acimg_summary_images(const float* x, int ldc, long HW, int c0, int G, int n_images, uint8_t* out, void* stream);

/* TF's summary histogram (histogram/histogram.cc, restated) of V boxes of one flat fp32 buffer in one launch sequence.
 * segments: V records of 13 int64 ON THE DEVICE: offset (floats from `base`), dims[4] (row-major internal dims, unused
 *   trailing dims 1), lo[4], hi[4]: the elements with lo[k] <= coordinate[k] < hi[k] for every k are the VALUES of the
 *   segment; the others (zero pads, another variable's columns) are read and ignored.  lo / hi are clamped to the dims; a
 *   record with a non-positive dim or a negative offset is an empty segment.
 * limits: L ascending doubles on the device, used as given.  Per segment v:
 *   counts[v][b]   uint64 [V][L]: values whose bucket is b = the index of the first limit greater than (double)value
 *                  (std::upper_bound; numpy.searchsorted(limits, value, side="right")); a value not below the last
 *                  limit is counted in bucket L - 1 (TF's table ends with DBL_MAX)
 *   stats[v]       double [V][4] = {min, max, sum, sum_squares} over the values, in fp64; {+inf, -inf, 0, 0} if none
 *   nonfinite[v]   uint64 [V]: values that are NaN or +-inf; they are left out of counts and stats
 * fp32 denormals are values, not zeros.  counts, min and max are exact; sum and sum_squares are summed in a fixed order
 * (per thread, lanes, waves, 8192-element chunks, then one workgroup per segment): bit-identical from run to run.  The
 * counters are privatised in LDS and reach `counts` through 64-bit INTEGER atomics; there is no floating atomic.
 * total_elements: the sum over the records of dims[0] * dims[1] * dims[2] * dims[3], the CALLER's promise (the host
 *   cannot see the table): it sizes the workspace, and the chunks of a table that holds more are not read.
 * PRECONDITION: every [offset, offset + product of dims) lies inside the buffer at `base`.
 * ws: 8-byte aligned, the workspace query's bytes (pure host arithmetic; 0 for a non-positive argument); short =
 * ACIMG_EWORKSPACE.  V, L, total_elements >= 1, L <= 4096, no null pointer: otherwise ACIMG_EINVAL.  Every refusal
 * precedes the first launch.  Three launches on `stream`: zero + chunk prefix, partial histograms (16-byte loads where
 * dims[3] % 4 == 0 and base + offset is 16-byte aligned, scalar loads otherwise), per-segment finish. */
int acimg_histogram_segments(const float* base, const int64_t* segments, int V, const double* limits, int L,
                             long total_elements, uint64_t* counts, double* stats, uint64_t* nonfinite, void* ws,
                             size_t ws_bytes, void* stream);
size_t acimg_histogram_segments_workspace(int V, int L, long total_elements);

/* Exact K nearest gallery rows of every query row, fp64 (what retrieve.py:53-57 computes with scipy cdist + argsort per
 * anchor, and knn.py:102-104 with KNeighborsClassifier(n_neighbors=15).kneighbors):
 *   dist2[q][j] = sum_d (query[q][d] - gallery[g][d])^2, summed in fp64 in direct-difference form (not the
 *                 |a|^2 - 2ab + |b|^2 expansion, which cancels and would reorder near neighbours), idx[q][j] = g;
 *   order: ascending by the pair (dist2, gallery index), i.e. ties go to the LOWER index; slots j >= G hold idx -1 and
 *   dist2 +inf.
 * query [Q][ldq], gallery [G][ldg] row-major; dist2 / idx [Q][K].  1 <= K <= 64, ld >= D >= 1, G >= 1 (else
 * ACIMG_EINVAL); Q == 0 is a no-op.  ws: acimg_knn_topk_workspace(Q, G, D, K) bytes (a host-only query; 0 = none
 * needed, short = ACIMG_EWORKSPACE).  Stream-ordered, no atomics: bit-identical from run to run.  Finite inputs. */
int acimg_knn_topk(const double* query, int ldq, int Q, const double* gallery, int ldg, int G, int D, int K,
                   double* dist2, int32_t* idx, void* ws, size_t ws_bytes, void* stream);
size_t acimg_knn_topk_workspace(int Q, int G, int D, int K);

/* The two numbers the latent-space evaluation reports from neighbour lists idx [Q][ldidx] (acimg_knn_topk output):
 *   pred[q]      = the most frequent gallery_labels[idx[q][j]] over j < K; on a tie the SMALLEST class
 *                  (KNeighborsClassifier.predict with uniform weights, knn.py:104: labels 3, 1, 3, 1 -> 1);
 *   first_hit[q] = 1-based rank of the first neighbour j < K whose label equals query_labels[q], 0 if none
 *                  (retrieve.py:60-82: a rank-r hit is 1 <= first_hit <= r).
 * idx entries -1 are skipped; labels outside [0, num_classes) never count (callers validate the ranges, and every
 * idx >= 0 must index gallery_labels).  1 <= K <= 64, ldidx >= K, 1 <= num_classes <= 64.  pred / first_hit: NULL =
 * not written; query_labels may be NULL when first_hit is. */
int acimg_knn_vote(const int32_t* idx, int ldidx, int Q, int K, const int32_t* gallery_labels,
                   const int32_t* query_labels, int num_classes, int32_t* pred, int32_t* first_hit, void* stream);

/* Exact two-component t-SNE of a latent dump, fp64 throughout (what knn.py:67-90 asks of sklearn.manifold.TSNE; the
 * algorithm is van der Maaten & Hinton's, the precision search sklearn's _binary_search_perplexity).  Four entries; an
 * iteration of the descent is acimg_tsne_gradient followed by acimg_tsne_update.  All are stream-ordered, take no
 * workspace, use no atomics and reduce in fixed trees: two runs give the same bits.  Inputs must be finite.
 *
 * acimg_tsne_affinities: conditional affinities of the rows of x [N][ldx].  For every row i, with
 *   d_ij = sum_d (x[i][d] - x[j][d])^2 (direct-difference form, summed in feature order),
 *   the search starts at beta = 1 with the bracket (-inf, +inf) and runs at most 100 steps.  A step forms, over j != i,
 *   p_j = exp(-d_ij * beta), S = sum p_j (S == 0 -> 1e-8), H = log S + beta * (sum d_ij p_j) / S and
 *   diff = H - log(perplexity); it stops when |diff| <= 1e-5; otherwise diff > 0 raises the lower end of the bracket to
 *   beta (beta doubles while the upper end is +inf, else moves to the bracket's middle) and diff <= 0 lowers the upper
 *   end (beta halves while the lower end is -inf, else moves to the middle).
 *   P[i][j] = p_j / S of the last step evaluated, P[i][i] = 0; beta[i] = the beta of that step; steps[i] = the number of
 *   steps evaluated (1..100; 100 without |diff| <= 1e-5 means the search ran out).  Columns j >= N of P are never
 *   written (nor read).  Row i of P also serves as the scratch of row i's distances while the call runs.
 *   N >= 4, D >= 1, ldx >= D, ldp >= N, 1 < perplexity < N - 1 (else ACIMG_EINVAL).
 *
 * acimg_tsne_symmetrize: in place, P[i][j] = P[j][i] = (P[i][j] + P[j][i]) / (2N) - one addition, one true division,
 *   formed once per unordered pair, so the result is symmetric bit for bit - and P[i][i] = 0.  Columns j >= N untouched.
 *
 * acimg_tsne_gradient: with w_ij = 1 / (1 + |Y[i] - Y[j]|^2) (Y [N][2], j != i), rows [N][6] receives
 *   rows[i][0..1] = sum_j P[i][j] w_ij (Y[i] - Y[j])   (x, y: the attractive sums, NOT exaggerated),
 *   rows[i][2..3] = sum_j w_ij^2 (Y[i] - Y[j])         (x, y: the repulsive sums, NOT divided by Z),
 *   rows[i][4]    = sum_j w_ij,
 *   rows[i][5]    = sum_{j: P[i][j] > 0} P[i][j] (log P[i][j] - log w_ij) when want_kl != 0, else 0 (the logarithms
 *                   cost about as much as the rest of the pass).
 *
 * acimg_tsne_update: Z = sum_i rows[i][4]; per element (c = 0, 1) g = 4 (e * rows[i][c] - rows[i][2 + c] / Z), then
 *   G = (g * V < 0) ? G + 0.2 : G * 0.8, G = max(G, 0.01); V = momentum * V - learning_rate * G * g; Y += V
 *   (Y, V, G [N][2], updated in place).  kl, when not NULL, receives kl[0] = sum_i rows[i][5] + log Z: the
 *   Kullback-Leibler divergence at the Y the rows were formed from, provided they were formed with want_kl and P sums
 *   to 1.  Y, V and G may be NULL together (kl not): then only kl[0] is formed, e.g. at the final Y.
 *   e, learning_rate > 0, momentum >= 0, all finite; N >= 1 (else ACIMG_EINVAL). */
int acimg_tsne_affinities(const double* x, int ldx, int N, int D, double perplexity, double* P, int ldp, double* beta,
                          int32_t* steps, void* stream);
int acimg_tsne_symmetrize(double* P, int ldp, int N, void* stream);
int acimg_tsne_gradient(const double* P, int ldp, int N, const double* Y, int want_kl, double* rows, void* stream);
int acimg_tsne_update(const double* rows, int N, double e, double momentum, double learning_rate, double* Y, double* V,
                      double* G, double* kl, void* stream);

/* Batch assembly out of a device-resident pool of decoded frames (acimg/data.py: DeviceDataLoader): the per-frame maps
 * of dataloader/outdoor_data_mfcc.py:634-703 applied while the N frames slots[0..N) of a batch are gathered.  (Added
 * without raising ACIMG_VERSION: nothing existing changed, and the number is pinned by the host tests.)
 * The pool, per slot s < nslots (the CALLER's number; it is not passed):
 *   pool_video    + s * video_stride  uint8 [pixels][3], stored (BGR) order; video_stride in BYTES, a multiple of 16 and
 *                                     >= 3 * pixels (else ACIMG_EINVAL); pool_video 16-byte aligned
 *   pool_acoustic + s * elems         float32 [elems], as acimg_sequence_example_decode leaves it (already flipped)
 *   pool_mfcc, pool_mfcc_low + s * 12 float32 [12]: the MFCC rows of the raw and of the low-passed audio frame
 *   pool_labels   + s * 2             int32 {class, location}
 * slots: int32 [N] ON THE DEVICE; repeats and any order are allowed.  PRECONDITION: 0 <= slots[n] < nslots - the host
 * cannot see the values, so nothing checks them, and an index outside the pool reads outside the pool.
 * Outputs, dense, frame n < N:
 *   video    [N][pixels][3]  video[n][p][c] = (float)pool[slots[n]][p][2 - c] * (float)(1.0 / 255.0): one fp32 multiply,
 *            bit-equal to NumPy's `v[..., ::-1].astype(np.float32) * np.float32(1.0 / 255.0)`
 *   acoustic [N][elems]      (a - min(a)) / max(a - min(a)) over the whole frame: a correctly rounded subtraction and
 *            DIVISION (no reciprocal), bit-equal to NumPy on finite input; a constant frame gives NaN (0 / 0) as NumPy
 *            does; non-finite input: unspecified.  elems <= 32768 (the frame is held in LDS), else ACIMG_EINVAL
 *   mfcc, mfcc_low [N][12]   the rows copied
 *   action [N][num_actions], location [N][num_locations]  one-hot float32; a label outside [0, width) leaves a zero row
 * ws: acimg_batch_gather_workspace(N, elems) bytes, 16-byte aligned (short = ACIMG_EWORKSPACE): receives [N][4] floats
 * {min(a), max(a - min(a)), 0, 0}, the two statistics of each frame's normalisation.  N <= 0, N > 65535, a null pointer,
 * a non-positive size: ACIMG_EINVAL; every refusal precedes the first launch.
 * TWO launches on `stream` (the video stream: 16-pixel chunks as 16-byte loads and float4 stores, a scalar path for the
 * pixels past the last chunk and for pixels % 4 != 0 or an unaligned `video`; then one workgroup per frame for everything
 * else), no atomics, reductions in a fixed order: bit-identical from run to run. */
int acimg_batch_gather(const uint8_t* pool_video, size_t video_stride, const float* pool_acoustic, const float* pool_mfcc,
                       const float* pool_mfcc_low, const int32_t* pool_labels, const int32_t* slots, int N, int pixels,
                       int elems, int num_actions, int num_locations, float* video, float* acoustic, float* mfcc,
                       float* mfcc_low, float* action, float* location, void* ws, size_t ws_bytes, void* stream);
size_t acimg_batch_gather_workspace(int N, int elems);

/* The correspondence pairs of dataloader/outdoor_data_mfcc.py:888-928 (`--correspondence 1`) out of the same pool: every
 * frame once as it is and once as "this frame, near-silence -> a flat map".  (Added without raising ACIMG_VERSION:
 * acimg_batch_gather is unchanged, and the number is pinned by the host tests.)
 * Pool arguments, sizes, alignment and `stream` exactly as acimg_batch_gather.  rows: int32 [N] ON THE DEVICE, ROW CODES:
 *   code >= 0  the REAL row of slot code;  code < 0  the SILENT row of slot ~code (= -code - 1).
 * Repeats, any order and both kinds of one slot are allowed.  PRECONDITION: the decoded slot lies inside the pool.
 * Outputs, dense, row n < N, s = the decoded slot:
 *   video, action, location  as acimg_batch_gather gives them for slot s, whatever the row's kind
 *   acoustic [N][elems]      real: as acimg_batch_gather, bit for bit.  silent: acoustic[n][i] = pool_mfcc_low[s][i % 12],
 *            the row tiled over elems / 12 pixels, NOT normalised.  elems % 12 != 0: ACIMG_EINVAL
 *   mfcc [N][12]             pool_mfcc[s] for a real row, pool_mfcc_low[s] for a silent one
 *   pair [N][2]              the one-hot correspondence label: {0, 1} real, {1, 0} silent (tf.one_hot(1 | 0, 2))
 * There is no mfcc_low output.  ws: acimg_batch_gather_pairs_workspace(N, elems) bytes, 16-byte aligned (short =
 * ACIMG_EWORKSPACE): receives [N][4] floats, {min(a), max(a - min(a)), 0, 0} for a real row, four zeros for a silent one.
 * Refusals: everything acimg_batch_gather refuses, and elems % 12 != 0; every one precedes the first launch.
 * TWO launches on `stream`: the video launch of acimg_batch_gather on the decoded slots, then one workgroup per row (the
 * branch on the kind is uniform in it): a silent row reads its 48 bytes and stores float4 when `acoustic` is 16-byte
 * aligned (with pool_acoustic, as for the real rows), else float by float.  No atomics: bit-identical from run to run. */
int acimg_batch_gather_pairs(const uint8_t* pool_video, size_t video_stride, const float* pool_acoustic,
                             const float* pool_mfcc, const float* pool_mfcc_low, const int32_t* pool_labels,
                             const int32_t* rows, int N, int pixels, int elems, int num_actions, int num_locations,
                             float* video, float* acoustic, float* mfcc, float* pair, float* action, float* location, void* ws,
                             size_t ws_bytes, void* stream);
size_t acimg_batch_gather_pairs_workspace(int N, int elems);

/* Baseline JPEG of RGB8 frames, 4:2:0, integer arithmetic throughout (tests/jpeg_ref.py restates it bit for bit; the
 * definition is DESIGN section 8).  Replaces: the `-vcodec libx264` ffmpeg run of showvideo.py:239-251 as the video track
 * of the clip `python -m acimg.show video --avi 1` writes (Motion-JPEG; H.264 is not reproduced).  (Added without raising
 * ACIMG_VERSION: nothing existing changed, and the number is pinned by the host tests.)
 * Geometry: 16 x 16 MCUs in raster order, mcu_w = ceil(W / 16), mcu_h = ceil(H / 16), the frame extended by replicating
 * its last column and row; per MCU six 8 x 8 blocks Y00 Y01 Y10 Y11 Cb Cr.  1 <= H, W <= 65535.
 *
 * acimg_jpeg_quant_tables (host only): out[128] = the Annex K luminance, then chrominance table in NATURAL order, scaled
 *   by s = 5000 / quality (quality < 50) or 200 - 2 quality: (base * s + 50) / 100 clamped to 1..255.  quality 1..100.
 * acimg_jpeg_blocks: rgb uint8 [n][H][W][3] dense, qtables uint8 [128] ON THE DEVICE (the layout above, entries >= 1)
 *   -> coef int16 [n][mcus][6][64] (acimg_jpeg_coef_bytes), each block in zig-zag order.  Colour (JFIF, full range):
 *   Y = (19595 R + 38470 G + 7471 B + 32768) >> 16, Cb = clamp(((-11059 R - 21709 G + 32768 B + 32767) >> 16) + 128),
 *   Cr = clamp(((32768 R - 27439 G - 5329 B + 32767) >> 16) + 128); chroma = (a + b + c + d + 1 + (column & 1)) >> 2 over
 *   2 x 2 pixels (`column` of the chroma sample); DCT on sample - 128 with T = rint(2^14 A): rows, (p + 256) >> 9,
 *   columns; c = sign(q) (|q| + (d >> 1)) / d with d = Q << 19; AC clamped to +-1023.  1 <= n <= 65535.  ONE launch, one
 *   workgroup per MCU.
 * acimg_jpeg_scan: coef (as above, 16-byte aligned) -> per frame i the entropy-coded segment - everything between the
 *   SOS header and EOI - at scan + i * frame_stride, and its length in scan_bytes[i] (int32 [n]); the bytes of a frame's
 *   stride beyond its length are not written.  A restart interval is restart_mcus (1..65535) consecutive MCUs (the last
 *   of a frame may be shorter); the DC predictors are 0 at its start, it is coded with the four typical Huffman tables of
 *   Annex K.3 (ZRL, EOB, a negative value v as v + 2^size - 1), padded to a byte with 1-bits, a 0x00 stuffed after every
 *   0xFF, and followed - but the last - by FF D0+m, m = 0, 1, ... modulo 8.  Coefficients are clamped as they are read (DC
 *   difference +-2047, AC +-1023), so no input can exceed the capacity.
 *   acimg_jpeg_scan_capacity: the most bytes a frame can take.  A block takes at most 22 bits of DC (11-bit code + 11
 *   bits) and 63 x 26 bits of AC (16-bit code + 10 bits) = 1660 bits, an MCU 9960 bits = 1245 bytes, twice that with
 *   every byte stuffed; an interval adds a stuffed pad byte and a marker: 2490 mcus + 4 intervals.  frame_stride below it,
 *   or a capacity beyond INT32_MAX: ACIMG_EINVAL.
 *   ws: 16-byte aligned, acimg_jpeg_scan_workspace bytes (two int32 per interval, one int32 and a 1248-byte slot per
 *   MCU, then a worst-case slot of 2490 restart_mcus + 2 bytes per interval); short = ACIMG_EWORKSPACE.
 *   THREE launches: one LANE per (frame, MCU) codes the MCU's unstuffed bits into its slot (its DC predictors are the
 *   previous MCU's DC values); one wave per (frame, interval) joins its MCUs' bits into bytes, pads and stuffs; one
 *   workgroup per frame forms the prefix of its interval lengths and copies intervals and markers densely.
 * The three queries are pure host arithmetic and return 0 for an argument outside its range.  A null pointer or an
 * argument outside its range: ACIMG_EINVAL; every refusal precedes the first launch.  No atomics, no floating point:
 * bit-identical from run to run and equal to the restatement on any machine. */
int acimg_jpeg_quant_tables(int quality, uint8_t* out);
size_t acimg_jpeg_coef_bytes(int n, int H, int W);
int acimg_jpeg_blocks(const uint8_t* rgb, int n, int H, int W, const uint8_t* qtables, int16_t* coef, void* stream);
size_t acimg_jpeg_scan_capacity(int H, int W, int restart_mcus);
size_t acimg_jpeg_scan_workspace(int n, int H, int W, int restart_mcus);
int acimg_jpeg_scan(const int16_t* coef, int n, int H, int W, int restart_mcus, uint8_t* scan, size_t frame_stride,
                    int32_t* scan_bytes, void* ws, size_t ws_bytes, void* stream);

/* cv2.resize(frame, (new_w, new_h), interpolation=cv2.INTER_CUBIC) of 8-bit 3-channel frames with a crop window fused
 * in.  Replaces: `_aspect_preserving_resize` + `_central_crop` of convert_data.py:53-67,120-138 (the frames of
 * `python -m acimg.convert`).  tests/convert_ref.py restates it bit for bit; the definition - OpenCV's scalar fixed-point
 * path - is DESIGN section 8.  (Added without raising ACIMG_VERSION: nothing existing changed, and the number is pinned
 * by the host tests.)
 *
 * acimg_resize_cubic_tables (host only, pure arithmetic): for the output coordinates d = first .. first + count - 1 of
 *   a resize of n_in to n_out samples, idx int32 [count][4] and coef int16 [count][4]:
 *     scale = 1.0 / ((double)n_out / n_in);  f = (float)((d + 0.5) * scale - 0.5);  s = floor(f);  f -= s  (no clamp of
 *     s or f at the border);  float32, A = -0.75f:  c0 = ((A (f+1) - 5A)(f+1) + 8A)(f+1) - 4A,
 *     c1 = ((A+2) f - (A+3)) f f + 1,  c2 = ((A+2)(1-f) - (A+3))(1-f)(1-f) + 1,  c3 = 1 - c0 - c1 - c2;
 *     coef[k] = saturate_int16(rint(c[k] * 2048.0f)), half to even, the sum NOT fixed up (2047 and 2049 occur);
 *     idx[k] = clamp(s - 1 + k, 0, n_in - 1).
 *   1 <= n_in, n_out <= 65535, 0 <= first, 1 <= count <= n_out - first, no null pointer: otherwise ACIMG_EINVAL.
 * acimg_resize_cubic_u8: n frames of H x W pixels of 3 bytes; frame i's top row starts at src + i * frame_stride +
 *   pixel_offset and row y lies y * row_stride bytes from it.  row_stride is SIGNED: negative for a bottom-up BMP, whose
 *   pixel_offset then points at the last stored row.  Nothing about src need be aligned (a BMP's pixels start at byte
 *   54 and its rows are padded to 4 bytes): the kernel loads bytes.  idx_y / coef_y [OH][4] and idx_x / coef_x [OW][4]
 *   ON THE DEVICE, the layout above, indices in PIXELS; they cover the crop window only.  An index outside the frame is
 *   clamped to it as it is read.  out: uint8 [n][OH][OW][3] dense, channel order as in src.
 *     horizontal pass first, per channel, int32, no shift:  h = sum_k src[row][idx_x[k]] * coef_x[k];
 *     vertical pass:  v = sum_k h[idx_y[k]] * coef_y[k];  out = clamp((v + (1 << 21)) >> 22, 0, 255).
 *   ONE launch per 65535 frames, one workgroup per (8 output rows, <= 320 output columns, frame); the horizontal pass
 *   of the source rows a band needs is held in LDS.  No workspace, no atomics, integer arithmetic: bit-identical from
 *   run to run and equal to the restatement on any machine.
 *   A null pointer, a size outside 1..65535 (n: any positive), |row_stride| < 3 W, or a frame whose rows do not lie
 *   inside [0, frame_stride) of its start: ACIMG_EINVAL; every refusal precedes the launch. */
int acimg_resize_cubic_tables(int n_in, int n_out, int first, int count, int32_t* idx, int16_t* coef);
int acimg_resize_cubic_u8(const uint8_t* src, size_t frame_stride, size_t pixel_offset, long row_stride, int n, int H, int W,
                          const int32_t* idx_y, const int16_t* coef_y, const int32_t* idx_x, const int16_t* coef_x, int OH,
                          int OW, uint8_t* out, void* stream);

/* Baseline JPEG files (SOF0: sequential DCT, Huffman, 8 bit) to B, G, R pixels, integer arithmetic throughout: the decoder
 * of `python -m acimg.convert_boxes`.  Replaces: the `cv2.imread` of convert_data2.py:157.  tests/jpeg_decode_ref.py
 * restates every stage bit for bit, and the pixels equal libjpeg-turbo's (Pillow's) on the files of
 * tests/golden/jpeg_decode_golden.npz; the definition is DESIGN section 8.  (Added without raising ACIMG_VERSION: nothing
 * existing changed, and the number is pinned by the host tests.)
 * Geometry: the images of one call share H, W (1..65535), comps (1 or 3) and the luma sampling hs x vs - 1x1, 2x1 or 2x2
 * over 1x1 chroma; 1x1 for one component.  An MCU is 8 hs x 8 vs pixels, mcu_w = ceil(W / (8 hs)), mcu_h = ceil(H /
 * (8 vs)), mcus = mcu_w mcu_h in raster order; it holds B = hs vs + 2 blocks (Y in raster order, Cb, Cr), B = 1 for one
 * component.  The host (acimg/jpeg.py: parse_jpeg) reads the markers and refuses everything else by name.
 *
 * acimg_jpeg_decode_entropy: data uint8 [data_bytes]: the entropy-coded segments of the n files, anywhere in it;
 *   desc int64 [n][4]: per image the first and the end byte of its segment in data, its restart interval in MCUs (0: none,
 *   the image is one interval) and the index of its first interval in `intervals`; intervals int32 [total_intervals][2]:
 *   first and end byte of a restart interval RELATIVE to the segment (the bytes between two RSTm markers; an image has
 *   ceil(mcus / restart) of them, in order); huff uint8 [n][6][ACIMG_JPEG_HUFF_BYTES]: DC then AC table of component 0, 1,
 *   2 (one component: the first two are read), each as
 *     uint16 look[256]   the next 8 bits -> (length << 8) | symbol for a code of at most 8 bits, else 0
 *     int32 maxcode[17]  [l], l = 1..16: the largest code of l bits, -1 where there is none ([0] unused)
 *     int32 valoff[17]   [l]: index in vals of the first symbol of l bits minus the smallest code of l bits
 *     uint8 vals[256]    HUFFVAL
 *   -> coef int16 [n][mcus][B][64] (acimg_jpeg_decode_coef_bytes), each block in NATURAL (row-major) order, and status
 *   int32 [n]: 0, or ACIMG_JPEG_STATUS_* of the image's first bad interval.  Per interval: DC predictors start at 0; bits
 *   MSB first, FF 00 is the byte FF, any other FF ends the interval's data; a DC symbol s (0..15) is followed by s bits v,
 *   the difference is v if v >= 2^(s-1), else v - 2^s + 1; an AC symbol (r, s): s > 0 skips r coefficients and stores the
 *   next, (15, 0) skips 16, (r, 0) otherwise ends the block.  Errors: no code of up to 16 bits matches (a DC symbol above
 *   15 counts as such), a coefficient would land past 63, more bits are used than the interval holds, a descriptor whose
 *   intervals do not lie inside the table.  The blocks of an interval from the error on are zeros.
 *   NOTHING IN data, desc OR intervals IS TRUSTED: every range is clamped to the range that holds it before it is used,
 *   no read leaves [data, data + data_bytes), no write leaves the image's own coefficient slot, every loop is bounded by
 *   the geometry; a corrupt image ends with a status and the other images of the call are unaffected.
 *   ONE launch: one workgroup (one wave) per image with its tables in LDS, ONE LANE per restart interval - a file without
 *   restart markers is decoded by a single lane, and the parallelism is the batch.
 * acimg_jpeg_decode_idct: coef, quant uint8 [n][3][64] (the table of component 0, 1, 2 in NATURAL order) -> planes uint8,
 *   per image B * mcus * 64 bytes (acimg_jpeg_decode_plane_bytes): the Y plane of (8 vs mcu_h) x (8 hs mcu_w) samples, then
 *   Cb and Cr of (8 mcu_h) x (8 mcu_w).  libjpeg's jpeg_idct_islow in 32-bit integers that wrap: x = coef * quant,
 *   CONST_BITS 13, PASS1_BITS 2, the constants 2446 3196 4433 6270 7373 9633 12299 15137 16069 16819 20995 25172 in its
 *   even / odd butterfly, columns first with (v + 2^10) >> 11, then rows with (v + 2^17) >> 18; + 128; clamp to 0..255.
 *   ONE launch, eight threads per block.
 * acimg_jpeg_decode_colour: planes -> bgr uint8 [n][H][W][3] dense, B G R (acimg_jpeg_decode_pixel_bytes).  Chroma is
 *   upsampled as libjpeg's fancy upsampling does, on the component's true size cw = ceil(W / hs), ch = ceil(H / vs):
 *     2x1: out[2i] = (3 a[i] + a[i-1] + 1) >> 2, out[2i+1] = (3 a[i] + a[i+1] + 2) >> 2; out[0] = a[0], out[2cw-1] = a[cw-1]
 *     2x2: s[i] = 3 row[i] + neighbour[i], the neighbour being the row above for an even and below for an odd output
 *          row (the first and last true row replicated); out[2i] = (3 s[i] + s[i-1] + 8) >> 4, out[2i+1] = (3 s[i] +
 *          s[i+1] + 7) >> 4, with s[-1] = s[0] and s[cw] = s[cw-1]
 *   then, cb and cr less 128: R = Y + ((91881 cr + 32768) >> 16), B = Y + ((116130 cb + 32768) >> 16), G = Y + ((-22554
 *   cb - 46802 cr + 32768) >> 16), clamped.  One component: B = G = R = Y.  ONE launch, one thread per pixel.
 * The three size queries are pure host arithmetic and return 0 for an argument outside its range.  A null pointer, a
 * geometry outside the above or a misaligned coef / huff / desc / intervals / planes (16 bytes): ACIMG_EINVAL; a buffer
 * shorter than its query: ACIMG_EWORKSPACE; every refusal precedes the launch.  No atomics, no floating point, every
 * output byte written by one thread: bit-identical from run to run and equal to the restatement on any machine. */
#define ACIMG_JPEG_HUFF_BYTES 904
#define ACIMG_JPEG_STATUS_BAD_CODE 1
#define ACIMG_JPEG_STATUS_RUN 2
#define ACIMG_JPEG_STATUS_EARLY_END 3
#define ACIMG_JPEG_STATUS_DESCRIPTOR 4
size_t acimg_jpeg_decode_coef_bytes(int n, int H, int W, int comps, int hs, int vs);
size_t acimg_jpeg_decode_plane_bytes(int n, int H, int W, int comps, int hs, int vs);
size_t acimg_jpeg_decode_pixel_bytes(int n, int H, int W);
int acimg_jpeg_decode_entropy(const uint8_t* data, size_t data_bytes, const int64_t* desc, const int32_t* intervals,
                              long total_intervals, const uint8_t* huff, int n, int H, int W, int comps, int hs, int vs,
                              int16_t* coef, size_t coef_bytes, int32_t* status, void* stream);
int acimg_jpeg_decode_idct(const int16_t* coef, const uint8_t* quant, int n, int H, int W, int comps, int hs, int vs,
                           uint8_t* planes, size_t plane_bytes, void* stream);

/* Progressive JPEG files (SOF2: spectral selection and successive approximation, Huffman, 8 bit; T.81 Annex G): the second
 * entropy stage.  It fills the coefficient slot of acimg_jpeg_decode_entropy - same layout, same geometry rules, same status
 * array - and acimg_jpeg_decode_idct / _colour follow unchanged: a complete progressive file holds exactly the coefficients
 * of its baseline twin, so the pixels equal libjpeg-turbo's bit for bit.  tests/jpeg_progressive_ref.py restates it; the
 * fixture is tests/golden/jpeg_progressive_golden.npz; DESIGN section 8 has the definition.  (Added without raising
 * ACIMG_VERSION: nothing existing changed, and the number is pinned by the host tests.)
 *   data uint8 [data_bytes]: the files' bytes from the first scan to the end of the last, anywhere in it.
 *   img int64 [n][4]: per image the first and the end byte of its bytes in data, the index of its first record in `scans`
 *     and the number of its scans (1..ACIMG_JPEG_PROG_MAX_SCANS), in file order.
 *   scans int32 [total_scans][ACIMG_JPEG_PROG_SCAN_FIELDS], one record per scan:
 *     [0] the scan's components as a bit mask (bit c: component c of the frame)      [1] Ss  [2] Se  [3] Ah  [4] Al
 *     [5..7] per component c the index in `huff` of the table the scan reads for it: its DC table in a first DC scan, its
 *            AC table in an AC scan; not read for a component outside the mask or in a DC refinement scan (-1 there)
 *     [8] the restart interval in the scan's own units - MCUs for a scan of several components, blocks of the component's
 *         own grid for a scan of one - 0: the scan is one interval
 *     [9] [10] first and end byte of the scan's entropy-coded segment RELATIVE to the image's first byte
 *     [11] index of its first interval in `intervals`; it has ceil(units / restart) of them, in order
 *     [12] its level: 0, or 1 + the highest level of an earlier scan of the image that shares a component with it and
 *          whose [Ss, Se] overlaps its own.  Scans of one level touch disjoint coefficients.    [13..15] zero
 *   intervals int32 [total_intervals][2]: first and end byte of a restart interval RELATIVE to its scan's segment.
 *   huff uint8 [total_tables][ACIMG_JPEG_HUFF_BYTES]: the pool of every table some scan names, in the layout above.
 *   -> coef, status as acimg_jpeg_decode_entropy.  The kernel zeroes the slot itself, then runs level after level; the
 *   unit of work is one (scan, interval) pair.  A scan of ONE component walks that component's own grid of
 *   ceil(ceil(W h / hmax) / 8) x ceil(ceil(H v / vmax) / 8) blocks in raster order (not the MCU-padded grid: luma blocks in
 *   the padding are reached by interleaved scans only); a scan of several walks the MCUs and in each the blocks of its
 *   components.  Per interval the DC predictors and EOBRUN start at 0.  DC first (Ss = 0, Ah = 0): as the baseline DC, the
 *   value shifted left by Al.  DC refinement: one bit per block, OR-ed in at bit Al.  AC first: symbol (r, s): s > 0 skips
 *   r coefficients and stores the next as value << Al; (15, 0) skips 16; (r < 15, 0) starts an end-of-band run of 2^r + r
 *   further bits blocks, this one included.  AC refinement: s must be 1, a sign bit follows (1: +2^Al, 0: -2^Al); the run
 *   r counts coefficients that are still zero only, and every nonzero coefficient passed on the way - also in the blocks
 *   of an end-of-band run - takes one correction bit, which adds 2^Al away from zero where bit Al is still clear; 16-bit
 *   arithmetic that wraps, as libjpeg's.
 *   Status: ACIMG_JPEG_STATUS_BAD_CODE (no code matches; a DC category above 15; an AC refinement size other than 1), _RUN
 *   (a coefficient would land past Se), _EARLY_END (more bits used than the interval holds), _DESCRIPTOR (an img or scan
 *   record outside the ranges above: mask 1..2^comps - 1, 0 <= Ss <= Se <= 63, Ss = 0 only with Se = 0, one component
 *   where Ss > 0, Ah and Al 0..13, a table index inside the pool, intervals inside the table, a level below the image's
 *   number of scans, zero padding).  An item that meets an error stops writing there; the image's status is the code of
 *   its first bad item in (scan, interval) order; later levels still run on what is there.  NOTHING IS TRUSTED, as above:
 *   byte ranges are clamped, every loop count comes from the geometry, no write leaves the image's slot.
 *   Caps: ACIMG_JPEG_PROG_MAX_SCANS scans a file (the records of one image are staged in LDS; one band per coefficient and
 *   component is 3 + 189 scans), ACIMG_JPEG_PROG_MAX_TABLES tables a file, ACIMG_JPEG_PROG_MAX_INTERVALS intervals a file;
 *   the host refuses a file beyond them by name.  Refusals as acimg_jpeg_decode_entropy (img, scans take desc's place).
 *   ONE launch: one workgroup (one wave) per image, one lane per (scan, interval) of the current level; tables are read
 *   from global memory.  No atomics: bit-identical from run to run. */
#define ACIMG_JPEG_PROG_MAX_SCANS 256
#define ACIMG_JPEG_PROG_MAX_TABLES 512
#define ACIMG_JPEG_PROG_MAX_INTERVALS (1 << 24)
#define ACIMG_JPEG_PROG_SCAN_FIELDS 16
int acimg_jpeg_decode_progressive(const uint8_t* data, size_t data_bytes, const int64_t* img, const int32_t* scans,
                                  long total_scans, const int32_t* intervals, long total_intervals, const uint8_t* huff,
                                  long total_tables, int n, int H, int W, int comps, int hs, int vs, int16_t* coef,
                                  size_t coef_bytes, int32_t* status, void* stream);
int acimg_jpeg_decode_colour(const uint8_t* planes, int n, int H, int W, int comps, int hs, int vs, uint8_t* bgr,
                             size_t bgr_bytes, void* stream);

/* Sample-rate conversion of one mono clip: `np.int32(librosa.core.resample(data * 1.0, fs, 12288))` of
 * convert_data2.py:35,48 - resampy's windowed-sinc interpolation (`kaiser_best`).  tests/resample_ref.py restates it bit for
 * bit; DESIGN section 8 has the definition and what of it is pinned.  (Added without raising ACIMG_VERSION.)
 * acimg_resample_length (host only): ratio = (double)rate_out / rate_in; *computed = (long)(len * ratio), the samples
 *   resampy forms; returns ceil(len * ratio), the length librosa pads them to with zeros.  0 for an argument below 1.
 * acimg_resample_sinc: x int32 [len]; win, delta fp64 [nwin] ON THE DEVICE: the right half of the filter (times ratio
 *   when ratio < 1) and its first differences with a 0 appended, num_table entries per zero crossing -> y fp64 [n_out]
 *   and / or yi int32 [n_out] (either may be null), n_out = acimg_resample_length(...).  Per output sample t, fp64, every
 *   product and every sum rounded on its own (nothing is contracted into a fused multiply-add):
 *     time = t * (1 / ratio);  n = (long)time;  scale = min(1, ratio);  step = (int)(scale * num_table)
 *     frac = scale * (time - n);  pos = frac * num_table;  o = (int)pos;  eta = pos - o
 *     y  = sum over i < min(n + 1, (nwin - o) / step), in order, of (win[o + i step] + eta delta[o + i step]) * x[n - i]
 *     frac = scale - frac;  pos, o, eta again
 *     y += sum over k < min(len - n - 1, (nwin - o) / step), in order, of (...) * x[n + k + 1]
 *   y[t] = 0 for t >= *computed.  yi[t] = y[t] truncated toward zero, clamped to the int32 range.  ONE launch, one thread
 *   per output sample; no atomics.  A null pointer, an argument below 1, n_out other than the query's value or a ratio
 *   below 1 / num_table: ACIMG_EINVAL before the launch. */
long acimg_resample_length(long len, int rate_in, int rate_out, long* computed);
int acimg_resample_sinc(const int32_t* x, long len, int rate_in, int rate_out, const double* win, const double* delta, int nwin,
                        int num_table, double* y, int32_t* yi, long n_out, void* stream);

/* ------------------------------------------------------------------------------------------
 * DEFLATE (RFC 1951) on the device: the compressor of the GZIP records and the PNG files the tools write
 * (`--deflate device`, `--png_deflate device`; the default stays the host's zlib).  csrc/deflate.hip has the stream layout,
 * the parse rule and the code construction, tests/deflate_ref.py restates them bit for bit, DESIGN section 8 has the
 * measurements.  (Added without raising ACIMG_VERSION.)
 * A payload is cut into blocks of ACIMG_DEFLATE_BLOCK bytes, coded independently (no match reaches before its block), each
 * as one stored or dynamic-Huffman block, whichever is smaller; every block but the last is followed by an empty stored
 * block (4 or 5 bytes, the sync-flush form), the last carries BFINAL.  The stream is the same from run to run.
 * acimg_deflate_bound (host only): the most bytes the stream of an n-byte payload can have, n + 10 ceil(n / BLOCK) + 5
 *   (a stored block costs 5 bytes, the marker behind it 5 more; the 5 cover the empty payload's stored block, which the
 *   CALLER writes: 01 00 00 FF FF).  0 for n < 0 or n > 2^40.
 * acimg_deflate_workspace (host only): bytes of `ws` for `count` payloads of `total_bytes` bytes together: per block a
 *   24-byte record, a byte count, an offset and a slot of BLOCK + 16 bytes, for total_bytes / BLOCK + count blocks.  0 for
 *   an argument below 1 or count > total_bytes.
 * acimg_deflate: in uint8 [sum of lengths] ON THE DEVICE, the payloads one behind the other; lengths long [count] ON THE
 *   HOST, each >= 1 -> out uint8 [out_bytes], the raw streams one behind the other with no gap, and out_sizes long [count]
 *   (device), each stream's bytes.  out_bytes >= the sum of acimg_deflate_bound(lengths[i]); only the streams' bytes are
 *   written.  ws 16-byte aligned, ws_bytes >= acimg_deflate_workspace(sum of lengths, count).  The block table is copied
 *   to the device and the stream is waited for once BEFORE the launches (the table is memory of the call); then three
 *   launches: one workgroup per block (match, histogram, codes, bits), one workgroup for the offsets, one per block for
 *   the dense copy.  A null pointer, count < 1, a length < 1, out_bytes below the bounds or a misaligned ws: ACIMG_EINVAL;
 *   ws_bytes too small: ACIMG_EWORKSPACE; all before anything is launched.
 * acimg_huffman_lengths: the code construction of the three alphabets on its own.  freq int32 [n][nsym] (device) ->
 *   lengths uint8 [n][nsym]: 0 for freq <= 0, 1 for a single used symbol, else a complete prefix code (Kraft sum exactly
 *   1) of lengths 1..limit that costs what an unlimited Huffman code costs whenever that fits the limit.  nsym 1..288,
 *   limit 1..15 with 2^limit >= nsym, n >= 1, else ACIMG_EINVAL.  One launch, one workgroup per histogram. */
#define ACIMG_DEFLATE_BLOCK 16384
size_t acimg_deflate_bound(long n);
size_t acimg_deflate_workspace(long total_bytes, int count);
int acimg_deflate(const uint8_t* in, const long* lengths, int count, uint8_t* out, size_t out_bytes, long* out_sizes, void* ws,
                  size_t ws_bytes, void* stream);
int acimg_huffman_lengths(const int32_t* freq, int n, int nsym, int limit, uint8_t* lengths, void* stream);

/* ------------------------------------------------------------------------------------------
 * INFLATE (RFC 1951) on the device: the reader of GZIP records (`DeviceDataLoader(inflate="device")`, `--inflate device`;
 * the default stays the host's zlib).  A general decoder: stored, fixed and dynamic blocks, whatever zlib's inflate
 * accepts, this library's own streams included; the output equals zlib's byte for byte.  csrc/inflate.hip has the plan,
 * tests/inflate_ref.py restates it, DESIGN section 8 has the measurements.  (Added without raising ACIMG_VERSION.)
 * Streams are RAW deflate (the caller strips gzip / zlib containers).  A stream of n bytes is cut into chunks of
 * `chunk_bytes` compressed bytes (a power of two, 256 .. 2^24); one call decodes every chunk of every stream:
 *   find     a workgroup per chunk j >= 1 looks for the lowest bit offset of the chunk that passes as the header of a
 *            non-final dynamic block (chunk 0 starts at bit 0);
 *   count    a wave per chunk with a start decodes without writing, up to the first block boundary that is a later
 *            chunk's start (its link) or past the BFINAL block;
 *   chain    the links are walked from chunk 0: the chunks on the chain are live and get their output offsets;
 *   decode   the live chunks decode again, into 16-bit symbols: a byte, or 0x8000 + (32768 - k) for "the byte k before
 *            this chunk's first";
 *   resolve  a workgroup per stream replaces the markers of each live chunk's last 32768 symbols, in chain order;
 *   finish   every symbol becomes its byte.
 * A chunk whose start is missing or wrong is decoded by the chunk before it: correctness never rests on the search.
 * acimg_inflate_workspace (host only): bytes of `ws` for `count` streams of `total_src` bytes that inflate to `total_out`
 *   bytes together: an AcimgInflateChunk for each of total_src / chunk_bytes + count chunks, an int32 per stream and a
 *   uint16 per output byte, each part rounded up to 16 bytes.  0 for an argument below 1, count > total_src or a bad
 *   chunk_bytes.
 * acimg_inflate: src uint8 ON THE DEVICE, the streams one behind the other; src_lengths and out_lengths long [count] ON
 *   THE HOST, each >= 1, an out_length below 2^31: the expected inflated sizes -> out uint8 [sum of out_lengths] (device),
 *   the outputs one behind the other; status int32 [count] (device): ACIMG_INFLATE_OK or the first failure of a live
 *   chunk; end_bits long [count] (device): the bit after the BFINAL block, 0 when status != 0.  The bytes of a stream
 *   whose status is not 0 are unspecified.  Nothing outside a stream's own output extent or outside ws is written,
 *   whatever the input.  The chunk table is copied to the device and the stream is waited for once BEFORE the launches;
 *   no read-back happens between them.  A null pointer, count < 1, a length < 1, an out_length >= 2^31, a bad chunk_bytes
 *   or a misaligned ws: ACIMG_EINVAL; ws_bytes too small: ACIMG_EWORKSPACE; all before anything is launched.
 * Debug view: after the call `ws` begins with the AcimgInflateChunk records of all chunks, stream after stream, chunk
 *   after chunk (ceil(src_length / chunk_bytes) per stream). */
#define ACIMG_INFLATE_OK 0
#define ACIMG_INFLATE_CORRUPT 1   /* an invalid code, code set or block type, LEN != ~NLEN, a distance before the stream */
#define ACIMG_INFLATE_SIZE 2      /* more or fewer bytes than out_length */
#define ACIMG_INFLATE_TRUNCATED 3 /* the stream ends before its BFINAL block does */
typedef struct AcimgInflateChunk {
    int64_t src_off, src_len;     /* host: the chunk's STREAM in `src` */
    int64_t out_off, out_len;     /* host: that stream's extent in `out` */
    int32_t stream, index;        /* host: the stream and the chunk's number j within it */
    int32_t first, nchunks;       /* host: the stream's first record and its number of chunks */
    int64_t start;                /* find: the chunk's first bit in the stream, -1: none */
    int64_t end;                  /* count: the bit where it stopped (the link, or the bit after the BFINAL block) */
    int64_t length;               /* count: the bytes it produces */
    int64_t offset;               /* chain: where they go in the stream's output (live chunks) */
    int32_t next;                 /* count: the chunk (number within the stream) it links to, -1: none */
    int32_t status;               /* count: ACIMG_INFLATE_* */
    int32_t live;                 /* chain: 1 on the chain from chunk 0 */
    int32_t reserved;
} AcimgInflateChunk;
size_t acimg_inflate_workspace(long total_src, long total_out, int count, int chunk_bytes);
int acimg_inflate(const uint8_t* src, const long* src_lengths, const long* out_lengths, int count, int chunk_bytes, uint8_t* out,
                  int32_t* status, long* end_bits, void* ws, size_t ws_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * The containers' checksums on the device, and the gather that assembles framed records there (`--assemble device` of
 * `python -m acimg.convert`, `png.encode_png_many`; the default stays the host).  csrc/checksum.hip has the algebra and
 * the plan, tests/checksum_ref.py restates the algebra, DESIGN section 8 has the measurements.  (Added without raising
 * ACIMG_VERSION.)
 * The definitions are the standards': CRC-32 reflected 0xEDB88320 and CRC-32C reflected 0x82F63B78, init and final XOR
 * 0xFFFFFFFF; kind 2 is kind 1 under the TFRecord mask, ((crc >> 15 | crc << 17) + 0xa282ead8); Adler-32 mod 65521 with
 * A starting at 1.  Every value equals zlib.crc32 / acimg_crc32c(data, n, 0) / zlib.adler32 bit for bit; no atomics, so a
 * second run gives the same bits.  A payload of 0 bytes yields the standard's value (0, 0, the mask of 0, 1) with no
 * segment launched for it.
 * A payload is cut on the grid of ACIMG_CHECKSUM_SEGMENT absolute bytes of `in`'s address range, one workgroup per cut.
 * acimg_checksum_workspace (host only): bytes of `ws` for `count` payloads of `total_bytes` bytes together: a 24-byte
 *   record and an 8-byte value for each of total_bytes / SEGMENT + 2 count segments and a 24-byte record per payload,
 *   each part rounded up to 16 bytes.  0 for total_bytes < 0 or count < 1.
 * acimg_checksum: in uint8 [sum of lengths] ON THE DEVICE, the payloads one behind the other (so a payload starts at any
 *   byte address); lengths long [count] ON THE HOST, each 0 .. 2^31 - 1 -> out uint32 [count] (device).  store_at: NULL, or
 *   long [count] ON THE HOST: where store_at[i] >= 0, payload i's value is also written little-endian into the four bytes
 *   at store_base + store_at[i] (device memory of the caller, any alignment; it may lie in `in`: every payload of the
 *   call has been read before the first store, so a value never depends on one); negative: no store.  ws 16-byte
 *   aligned.  The segment and
 *   payload tables (with the host-built multipliers x^(8 bytes behind) mod P) are copied to the device and the stream is
 *   waited for once BEFORE the launches (the tables are memory of the call); then two launches: one workgroup per segment,
 *   one wave per payload (reduction, init term, final XOR, mask, store).  A null pointer (store_base may be NULL without
 *   store_at), count < 1, a length < 0 or >= 2^31, an unknown kind or a misaligned ws: ACIMG_EINVAL; ws_bytes too small:
 *   ACIMG_EWORKSPACE; all before anything is launched.
 * acimg_record_gather_workspace (host only): 32 bytes per segment, rounded up to 16; 0 for nseg < 1.
 * acimg_record_gather: segments long [nseg][4] ON THE HOST, rows {dst_off, src_off, len, which}: the len bytes at
 *   src0 + src_off (which = 0: e.g. an uploaded skeleton) or src1 + src_off (which = 1: e.g. a pool of device frames) are
 *   copied to dst + dst_off.  A byte-exact copy; no offset or length has an alignment requirement, len may be 0, and
 *   bytes of dst that no segment covers are not written.  The host refuses (ACIMG_EINVAL) a null segments / dst / ws, a
 *   null source that a segment names, which outside {0, 1}, a negative offset or length, a segment that leaves
 *   [0, dst_bytes) and two segments that overlap in dst; a short ws is ACIMG_EWORKSPACE; the sources' extents are the
 *   caller's to know.  The table is copied and the stream waited for once before the ONE launch. */
#define ACIMG_CHECKSUM_CRC32         0   /* zlib / gzip / PNG */
#define ACIMG_CHECKSUM_CRC32C        1   /* Castagnoli: = acimg_crc32c(data, n, 0) */
#define ACIMG_CHECKSUM_CRC32C_MASKED 2   /* TFRecord: tfio.mask_crc of kind 1 */
#define ACIMG_CHECKSUM_ADLER32       3   /* zlib container */
#define ACIMG_CHECKSUM_SEGMENT 16384
size_t acimg_checksum_workspace(long total_bytes, int count);
int acimg_checksum(const uint8_t* in, const long* lengths, int count, int kind, uint32_t* out, uint8_t* store_base,
                   const long* store_at, void* ws, size_t ws_bytes, void* stream);
size_t acimg_record_gather_workspace(int nseg);
int acimg_record_gather(const uint8_t* src0, const uint8_t* src1, const long* segments, int nseg, uint8_t* dst, size_t dst_bytes,
                        void* ws, size_t ws_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * PNG decoding on the device, the part that is not DEFLATE (`python -m acimg.convert_collected`, `acimg.png.PngDecoder`):
 * the scanline filters of RFC 2083 section 6 undone for many images in one launch, and the samples of all 15 colour-type /
 * bit-depth forms, interlaced or not, turned into the uint8 [H, W, 3] B, G, R pixels `cv2.imread(path)` returns with its
 * default flag.  csrc/png_decode.hip has the plan, tests/png_decode_ref.py restates both stages, DESIGN section 8 has the
 * definition and the measurements.  (Added without raising ACIMG_VERSION.)
 * Size queries (host only; 0 for a dimension < 1, an illegal colour-type / depth pair, interlace outside {0, 1} or a result
 *   above 2^31 - 1): acimg_png_inflated_bytes = the bytes the file's zlib stream inflates to, rows * (1 + row bytes) summed
 *   over the passes that have a row and a column (one pass without interlace); acimg_png_sample_bytes = the same without
 *   the filter bytes; acimg_png_pixel_bytes = 3 H W.  Row bytes = ceil(width * channels * depth / 8).
 * acimg_png_unfilter: src uint8 [src_bytes] ON THE DEVICE, the inflated streams of `nfiles` files back to back; jobs long
 *   [njobs][ACIMG_PNG_JOB_FIELDS] ON THE HOST, one row per (file, pass that has a row and a column): {offset in src of the
 *   job's first filter byte, offset in dst, rows, bytes per row without the filter byte, the filter unit bpp = max(1, bits
 *   per pixel / 8) in {1, 2, 3, 4, 6, 8}, file index} -> dst uint8 [dst_bytes]: the job's rows * row bytes reconstructed
 *   bytes at its dst offset, and status int32 [nfiles] (device): ACIMG_PNG_OK, or ACIMG_PNG_BAD_FILTER for a file with a
 *   filter byte above 4 - such a row is copied as filter 0, so the file's bytes are unspecified but every write stays in
 *   its jobs' extents, and no other file is affected.  Arithmetic mod 256; left and upleft are 0 in a row's first bpp
 *   bytes, up and upleft in a JOB's first row (filters never cross passes); Average floors the 9-bit sum; Paeth ties go
 *   to left, then up.  One wave per job: a wavefront over bands of 64 rows, ceil(rows / 64) * (units + 63) steps, not rows * units.
 *   The host refuses (ACIMG_EINVAL) a null pointer, njobs or nfiles < 1, a misaligned ws, a bpp outside the set, rows or
 *   row bytes < 1, row bytes no multiple of bpp, a file index outside [0, nfiles) and a job that leaves src or dst; a short
 *   ws is ACIMG_EWORKSPACE; jobs that overlap in dst are the caller's to avoid.  The table is copied, status zeroed and
 *   the stream waited for once before the ONE launch.  acimg_png_unfilter_workspace: 48 bytes per job, rounded up to 16.
 * acimg_png_pixels: samples = acimg_png_unfilter's dst; files long [nfiles][ACIMG_PNG_FILE_FIELDS] ON THE HOST: {offset of
 *   the file's samples, H, W, colour type, bit depth, interlace, offset of its palette in `palette` (bytes), palette
 *   entries, offset in out}; palette uint8 [palette_bytes] (device; R, G, B per entry; may be NULL when no file has
 *   colour type 3) -> out: 3 H W bytes per file at its offset.  libpng's transforms as OpenCV sets them for IMREAD_COLOR:
 *   indices go through PLTE, grey of 1 / 2 / 4 bits is scaled by 255 / 85 / 17, 16-bit samples keep their high byte, grey
 *   is replicated, alpha is dropped (not composited), tRNS / gAMA and the other ancillary chunks have no effect, the
 *   order is B, G, R.  Interlaced files are gathered from their passes by the Adam7 table (x origins 0 4 0 2 0 1 0, steps
 *   8 8 4 4 2 2 1; y origins 0 0 4 0 2 0 1, steps 8 8 8 4 4 2 2); samples below 8 bits are packed MSB first, rows padded
 *   to a byte.  status int32 [nfiles] (device) is IN / OUT: the kernel only ever stores ACIMG_PNG_BAD_INDEX, for a file
 *   with a palette index at or beyond its PLTE length (that pixel becomes 0 0 0; a stated choice: libpng's behaviour
 *   there depends on its version) - so handing it acimg_png_unfilter's array keeps that stage's verdicts.  The host
 *   refuses (ACIMG_EINVAL) a null pointer, nfiles outside 1 .. 65535, a geometry the size queries give 0 for, a file that
 *   leaves samples / out / palette, a colour type 3 file with 0 or more than 256 entries; a short ws is ACIMG_EWORKSPACE.
 *   acimg_png_pixels_workspace: 72 bytes per file, rounded up to 16. */
#define ACIMG_PNG_OK         0
#define ACIMG_PNG_BAD_FILTER 1   /* a filter byte above 4 */
#define ACIMG_PNG_BAD_INDEX  2   /* a palette index at or beyond the PLTE length */
#define ACIMG_PNG_JOB_FIELDS  6
#define ACIMG_PNG_FILE_FIELDS 9
size_t acimg_png_inflated_bytes(int height, int width, int colour_type, int bit_depth, int interlace);
size_t acimg_png_sample_bytes(int height, int width, int colour_type, int bit_depth, int interlace);
size_t acimg_png_pixel_bytes(int height, int width);
size_t acimg_png_unfilter_workspace(int njobs);
int acimg_png_unfilter(const uint8_t* src, size_t src_bytes, const long* jobs, int njobs, int nfiles, uint8_t* dst, size_t dst_bytes,
                       int32_t* status, void* ws, size_t ws_bytes, void* stream);
size_t acimg_png_pixels_workspace(int nfiles);
int acimg_png_pixels(const uint8_t* samples, size_t sample_bytes, const long* files, int nfiles, const uint8_t* palette,
                     size_t palette_bytes, uint8_t* out, size_t out_bytes, int32_t* status, void* ws, size_t ws_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * Dataset records (host side, no GPU work; caller-owned memory like everything else): the GZIP TFRecord files of
 * tf.train.SequenceExample written by convert_data.py:247-279 and read by dataloader/outdoor_data_mfcc.py:62,263-343.
 * ---------------------------------------------------------------------------------------- */
/* Inflate a whole .tfrecord file image (GZIP auto-detected by its magic; anything else is copied).  *produced =
 * the inflated size, also when `out` is NULL / too small (ACIMG_EWORKSPACE): call once to size, once to fill. */
int acimg_gzip_inflate(const uint8_t* src, size_t src_len, uint8_t* out, size_t cap, size_t* produced);
/* Walk the TFRecord framing [u64 len][u32 masked crc32c(len)][data][u32 masked crc32c(data)] of an inflated file
 * image: returns the number of records (>= 0) and fills the payload offset / length of the first `cap` of them;
 * verify != 0 checks both checksums of every record.  Negative = ACIMG_E* (truncated / corrupt). */
long acimg_tfrecord_index(const uint8_t* buf, size_t len, uint64_t* offsets, uint64_t* lengths, long cap, int verify);
/* What `_parse_sequence` (dataloader/outdoor_data_mfcc.py:263-343) extracts from one serialized SequenceExample. */
typedef struct AcimgSequenceDims {
    int64_t classes, location;                        /* context 'classes', 'location' */
    int64_t audio_height, audio_width, audio_depth;   /* 'audio_image/{height,width,depth}' (0 if absent) */
    int64_t mics, samples;                            /* 'audio_data/{mics,samples}' */
    int64_t video_height, video_width, video_depth;   /* 'video/{height,width,depth}' */
    int64_t audio_image_steps, audio_data_steps, video_steps;   /* feature-list lengths (12 = one second) */
    int64_t audio_data_values;                        /* int32 values over all 'audio/data' steps */
} AcimgSequenceDims;
/* Decode one record: context scalars + list lengths into *dims; the raw tensors (tf.decode_raw) into the caller's
 * buffers when given (NULL = sizes only; capacities in ELEMENTS): audio_images float32 [steps][H][W][D] already
 * flipped left-right and up-down as :314-315 do, audio_samples int32 [values], video uint8 [steps][H][W][D]. */
int acimg_sequence_example_decode(const uint8_t* rec, size_t len, AcimgSequenceDims* dims, float* audio_images,
                                  size_t audio_images_cap, int32_t* audio_samples, size_t audio_samples_cap,
                                  uint8_t* video, size_t video_cap);

/* What `_parse_sequence` of the box-annotated loader (dataloader/frames.py:246-341, records written by
 * convert_data2.py:200-307) extracts from one serialized SequenceExample: no 'classes' / 'location' context. */
typedef struct AcimgBoxSequenceDims {
    int64_t mics, samples;                            /* context 'audio_data/{mics,samples}' */
    int64_t video_height, video_width, video_depth;   /* context 'video/{height,width,depth}' */
    int64_t box_rows;                                 /* rows of tf.reshape(decode_raw(xmin), [-1, 3]) (all five alike) */
    int64_t audio_data_steps, video_steps;            /* feature-list lengths */
    int64_t audio_data_values;                        /* int32 values over all 'audio/data' steps */
} AcimgBoxSequenceDims;
/* Decode one record: context scalars + list lengths into *dims; when given (NULL = sizes only; capacities in
 * ELEMENTS): boxes int32 [box_rows][4][3] = xmin, xmax, ymin, ymax rows (the layout acimg_box_iou reads), typescene
 * int32 [box_rows][3], audio int32 [audio_data_values] (tf.reshape [-1, samples]), video uint8 [steps][H][W][D].
 * The five box features and 'audio/data', 'video/image' and their context dimensions are required. */
int acimg_box_sequence_example_decode(const uint8_t* rec, size_t len, AcimgBoxSequenceDims* dims, int32_t* boxes,
                                      size_t box_cap, int32_t* typescene, size_t typescene_cap, int32_t* audio,
                                      size_t audio_cap, uint8_t* video, size_t video_cap);

/* ------------------------------------------------------------------------------------------
 * Host-side helper (no GPU): CRC-32C (Castagnoli) of a byte range, continuing from `crc` (0 to start) — the
 * checksum of TensorFlow checkpoint bundles and TFRecord files, used by the checkpoint / TFRecord readers
 * that stand where trainer/mfcctrainer.py:214-247 calls tf.train.Saver and
 * dataloader/outdoor_data_mfcc.py:558-575 reads TFRecords.
 * ---------------------------------------------------------------------------------------- */
uint32_t acimg_crc32c(const void* data, size_t n, uint32_t crc);

#ifdef __cplusplus
}
#endif
#endif /* ACIMG_H_ */
