"""CPU restatement of the two split-operand formats of the convolutions, their error bounds, and the operand sets that
drive them over the range include/acimg.h states (|w| < 63, |x| < 2.6e5).  Plain torch, no GPU.

The formats (csrc/common.hpp, `split4` in csrc/igemm_split3_kernel.hpp)
    f16x3   forward passes.  s = v * SCALE in fp32 (activations 2^-2, weights 2^10), hi = f16(s), lo = f16(s - hi) with the
            subtraction in fp32 (exact: hi is the nearest fp16 of s), every product hi*hi + hi*lo + lo*hi on the fp16 matrix
            cores with fp32 accumulation, accumulators times 2^-8.
    bf16x3  backward passes.  The same with bf16 halves and no scaling.

Derivation of `bound_f16x3`, per output element y = sum_k x_k w_k over the unfolded products (k = tap and input channel):

  * split residual of one operand.  s in [2^e, 2^(e+1)) has 24 significant bits, hi keeps 11, the residual r = s - hi is a
    multiple of 2^(e-23) with |r| <= 2^(e-11).  For |r| < 2^(e-12) its 11 bits fit lo exactly; else it has 12 bits and lo
    drops the last: the error is 0 or 2^(e-23), i.e. at most 2^-23 of the binade's bottom - between 2^-24 |s| (top of the
    binade) and 2^-23 |s| (bottom).  The bound counts 2^-24 |s| per operand, and the margin below pays for the binade.
  * the floor.  Once r is below fp16's smallest normal 2^-14, lo is a subnormal on the grid 2^-24 and the error is at most
    half a step, 2^-25 of s whatever its size: 2^-23 per activation (s = x / 4: every |x| < 0.5 has a subnormal lo) and
    2^-35 per weight (s = 1024 w: below |w| ~ 1.2e-4).  These are absolute, so they multiply the OTHER operand alone:
    2^-23 (1 (*) |w|) and 2^-35 (|x| (*) 1), each taken twice (the half step can meet the binade effect of the line above).
  * the dropped lo*lo product: |lo| <= 2^-11 |s| (1 + 2^-11) for both operands, 2^-22 |x w|; with random signs against the
    2^-24 terms it is carried as one more 2^-24 unit by the margin - the emulation below is the check, not this line.
  * accumulation: the matrix core adds a 32-deep K step into an fp32 accumulator, one rounding per step of at most 2^-24 of
    the running magnitude, itself at most |x| (*) |w|: ksteps = R S C / 32 of them; each K range that a tail split or a
    split-K hand-off adds to the total is one rounding more (`ranges`, at most 16: the largest count the forward tail
    split considers), and 2 more for the epilogue (the 2^-8 is exact; bias / store).
  The derived format coefficient is 3 (two residuals, lo*lo); the bound uses 8.  The CPU emulation of the format alone
  (tests/test_split_format_ref_cpu.py) reaches 1.5 times the coefficient-3 bound on binade edges and must stay within HALF of
  the bound here, so a kernel that misses the bound is at fault, not the format.

      bound = (8 + ksteps + ranges + 2) 2^-24 (|x| (*) |w|)  +  2 * 2^-23 (1 (*) |w|)  +  2 * 2^-35 (|x| (*) 1)

`bound_bf16x3`: bf16 keeps 8 + 8 bits, so the three format terms are 2^-18 instead of 2^-24; fp32's exponent range means no
floor (the gradients of the tests stay fp32-normal, |g| >= 2^-30 * small); the accumulation term is the same:

      bound = (8 * 2^-18 + (ksteps + ranges + 2) 2^-24) (|a| (*) |b|)

`BF16_FMT_FEW` = 16, the format coefficient of the cases added with the fp32 entry points' routes (FP32_CASES, "halo 64").  For
bf16x3 the 8 above is not a margin but the format's own worst case per product: hi keeps 8 bits, so |lo| <= 2^-8 |s|, and lo
keeps 8 bits of a residual below 2^(e-8): |s - hi - lo| <= 2^-17 of the binade's bottom; two residuals and the dropped lo*lo
make 2^-17 + 2^-17 + 2^-16 = 8 * 2^-18 of |a b|, approached when both operands sit just above a power of two.  Sums of
hundreds of comparable products stay far below it (the tap / per-tap / halo cases, 0.29 - 0.44 of their bound), but where ONE
product makes up an element the emulated format reaches 0.81 of it: a border element of the stride-2 data gradient sees one
tap, an `impulse` weight gradient one pixel, and gy channels 2^20 apart leave one channel of 8 or 32 in charge.  The format
alone has to stay within half of the bound, so these cases take twice the worst case.  (A dropped cross term is 2^-9 of a
product, still 35 - 62 times over the doubled bound.)  The three earlier backward cases keep 8.

Split planes (the pre-split trunk format, two fp16 planes holding x / 4): `plane_bound(v)` is what the format can hold of an
fp32 value v - by the first two items above the decoded value is within 2^-23 of the bottom of v's binade, or half a
subnormal step, 2^-23 absolute.  (2^-24 |v| is NOT met by the format: a quarter of all fp32 values with 24 significant
bits lose their last bit, which is more than 2^-24 |v| for every v that is not a power of two; the CPU test shows it.)
"""
import torch
import torch.nn.functional as F

F16_ASCALE, F16_WSCALE, F16_OUTSCALE = 0.25, 1024.0, 1.0 / 256.0       # csrc/common.hpp SPLIT3_*
MAX_RANGES = 16
U24, U18 = 2.0 ** -24, 2.0 ** -18
X_FLOOR, W_FLOOR = 2.0 ** -23, 2.0 ** -35
BF16_FMT_FEW = 16


# ---- the formats ---------------------------------------------------------------------------------------------------
def _split(v, scale, dtype):
    s = v.float() * torch.tensor(scale, dtype=torch.float32)        # scale in fp32
    hi = s.to(dtype)                                                # round to the 16-bit type
    lo = (s - hi.float()).to(dtype)                                 # subtract in fp32, round again
    return hi, lo


def split_f16(v, scale):
    """fp32 v -> (hi, lo) fp16 halves of v * scale, as split4<SplitF16> / split4_scaled form them"""
    return _split(v, scale, torch.float16)


def split_bf16(v):
    """fp32 v -> (hi, lo) bf16 halves, as split4<SplitBF16> forms them"""
    return _split(v, 1.0, torch.bfloat16)


def three_term(a_hi, a_lo, b_hi, b_lo, prod=torch.mul):
    """hi*hi + hi*lo + lo*hi in fp64; `prod` is the bilinear product of the two operands (elementwise by default, or one of
    the conv_* functions below)"""
    ah, al, bh, bl = (t.double() for t in (a_hi, a_lo, b_hi, b_lo))
    return prod(ah, bh) + prod(ah, bl) + prod(al, bh)


def _bound_products(a, b, prod):
    a, b = a.double().abs(), b.double().abs()
    return prod(a, b), prod(torch.ones_like(a), b), prod(a, torch.ones_like(b))


def bound_f16x3(ax, aw, ksteps, ranges=MAX_RANGES, prod=torch.mul):
    """per-output-element bound of an f16x3 product of activations |x| and weights |w| (module docstring)"""
    xw, ow, xo = _bound_products(ax, aw, prod)
    return (8 + ksteps + ranges + 2) * U24 * xw + 2 * X_FLOOR * ow + 2 * W_FLOOR * xo


def bound_bf16x3(aa, ab, ksteps, ranges=MAX_RANGES, prod=torch.mul, fmt=8):
    """per-output-element bound of a bf16x3 product (module docstring); fmt: the format coefficient (BF16_FMT_FEW)"""
    ab_, _, _ = _bound_products(aa, ab, prod)
    return (fmt * U18 + (ksteps + ranges + 2) * U24) * ab_


def floor_share(ax, aw, ksteps, ranges=MAX_RANGES, prod=torch.mul):
    """the part of bound_f16x3 that the two absolute floor terms make up, per output element"""
    xw, ow, xo = _bound_products(ax, aw, prod)
    fl = 2 * X_FLOOR * ow + 2 * W_FLOOR * xo
    return fl / ((8 + ksteps + ranges + 2) * U24 * xw + fl).clamp_min(1e-300)


def pow2_floor(v):
    """2^floor(log2 |v|) in fp64 (0 for 0)"""
    m, e = torch.frexp(v.double().abs())
    return torch.where(m > 0, torch.ldexp(torch.ones_like(m), e - 1), torch.zeros_like(m))


def plane_bound(v):
    """what a pair of split planes can hold of the fp32 value v (module docstring)"""
    return torch.maximum(pow2_floor(v) * 2.0 ** -23, torch.full_like(v.double(), X_FLOOR))


def emulate_f16x3(xa, w, prod, defect=None):
    """the f16x3 product of fp32 operands in exact arithmetic (fp64 products and sums), optionally with a planted defect:
    'flush' (subnormal lo halves read as zero), 'split_before_scale' (the activation split before the 2^-2 scale, the halves
    scaled in fp16 afterwards), 'no_hi_lo' (the x_hi * w_lo term dropped)"""
    if defect == "split_before_scale":
        xh, xl = split_f16(xa, 1.0)
        xh, xl = (xh.float() * F16_ASCALE).half(), (xl.float() * F16_ASCALE).half()
    else:
        xh, xl = split_f16(xa, F16_ASCALE)
    wh, wl = split_f16(w, F16_WSCALE)
    if defect == "flush":
        tiny = 2.0 ** -14
        xl = torch.where(xl.float().abs() < tiny, torch.zeros_like(xl), xl)
        wl = torch.where(wl.float().abs() < tiny, torch.zeros_like(wl), wl)
    if defect == "no_hi_lo":
        wl = torch.zeros_like(wl)
    return three_term(xh, xl, wh, wl, prod) * F16_OUTSCALE


def emulate_bf16x3(a, b, prod, defect=None):
    """the bf16x3 product in exact arithmetic, optionally with a dropped cross term: 'no_hi_lo' (a_hi * b_lo), 'no_lo_hi'
    (a_lo * b_hi)"""
    ah, al = split_bf16(a)
    bh, bl = split_bf16(b)
    if defect == "no_hi_lo":
        bl = torch.zeros_like(bl)
    elif defect == "no_lo_hi":
        al = torch.zeros_like(al)
    else:
        assert defect is None, defect
    return three_term(ah, al, bh, bl, prod)


def max_ratio(got, ref, bound):
    """largest |got - ref| / bound over the elements; inf when anything is not finite or off where the bound is zero"""
    got, ref = got.detach().cpu().double(), ref.detach().cpu().double()
    assert got.shape == ref.shape == bound.shape, (got.shape, ref.shape, bound.shape)
    if not bool(torch.isfinite(got).all()):
        return float("inf")
    err = (got - ref).abs()
    r = torch.where(bound > 0, err / bound.clamp_min(1e-300), torch.where(err > 0, torch.full_like(err, float("inf")),
                                                                          torch.zeros_like(err)))
    return float(r.max())


# ---- the bilinear products: 3x3 / 1x1, stride 1, SAME; NHWC activations, HWIO weights; fp64 ---------------------------
def conv_fwd(x, w):
    R, S = w.shape[0], w.shape[1]
    return F.conv2d(x.permute(0, 3, 1, 2), w.permute(3, 2, 0, 1), padding=(R // 2, S // 2)).permute(0, 2, 3, 1)


def conv_dgrad(gy, w):
    """dx[N,H,W,C] of conv_fwd for the output gradient gy[N,H,W,K]"""
    R, S = w.shape[0], w.shape[1]
    return F.conv_transpose2d(gy.permute(0, 3, 1, 2), w.permute(3, 2, 0, 1), padding=(R // 2, S // 2)).permute(0, 2, 3, 1)


def conv_wgrad(taps):
    """-> prod(x, gy) = dw[R,S,C,K] of conv_fwd with R = S = taps"""
    def prod(x, gy):
        Cc, K = x.shape[-1], gy.shape[-1]
        dw = torch.nn.grad.conv2d_weight(x.permute(0, 3, 1, 2), (K, Cc, taps, taps), gy.permute(0, 3, 1, 2),
                                         padding=(taps // 2, taps // 2))
        return dw.permute(2, 3, 1, 0)
    return prod


def same_pad2(size):
    """(output size, leading pad) of a 3-tap / stride-2 SAME conv as TensorFlow pads it: even sizes pad 0 before and 1 after,
    odd sizes 1 and 1"""
    out = -(-size // 2)
    return out, max((out - 1) * 2 + 3 - size, 0) // 2


def conv_fwd_s2(x, w):
    """3x3 / stride 2 / SAME: y[N,ceil(H/2),ceil(W/2),K] (here only as the map whose adjoint conv_dgrad_s2 is)"""
    H, W = x.shape[1], x.shape[2]
    (OH, pt), (OW, pl) = same_pad2(H), same_pad2(W)
    xp = F.pad(x.permute(0, 3, 1, 2), (pl, (OW - 1) * 2 + 3 - W - pl, pt, (OH - 1) * 2 + 3 - H - pt))
    return F.conv2d(xp, w.permute(3, 2, 0, 1), stride=2).permute(0, 2, 3, 1)


def conv_dgrad_s2(H, W):
    """-> prod(gy, w) = dx[N,H,W,C] of conv_fwd_s2 on an H x W input: every gy pixel scatters its 3x3 patch at stride 2 over
    the padded grid, of which rows pad_t .. pad_t + H - 1 and columns pad_l .. pad_l + W - 1 are the image"""
    (OH, pt), (OW, pl) = same_pad2(H), same_pad2(W)

    def prod(gy, w):
        assert gy.shape[1:3] == (OH, OW), (gy.shape, OH, OW)
        full = F.conv_transpose2d(gy.permute(0, 3, 1, 2), w.permute(3, 2, 0, 1), stride=2)       # 2 OH + 1 by 2 OW + 1
        return full[:, :, pt:pt + H, pl:pl + W].permute(0, 2, 3, 1)
    return prod


# 2x2 / stride-2 transposed conv, weights in TF layout [kh][kw][out][in]: non-overlapping patches
def deconv_fwd(x, w):
    """y[n][2i + r][2j + s][k] = sum_c x[n][i][j][c] w[r][s][k][c]"""
    return F.conv_transpose2d(x.permute(0, 3, 1, 2), w.permute(3, 2, 0, 1), stride=2).permute(0, 2, 3, 1)


def deconv_dgrad(gy, w):
    """dx[n][i][j][c] = sum_{r,s,k} gy[n][2i + r][2j + s][k] w[r][s][k][c]"""
    return F.conv2d(gy.permute(0, 3, 1, 2), w.permute(3, 2, 0, 1), stride=2).permute(0, 2, 3, 1)


def deconv_wgrad(x, gy):
    """dw[r][s][k][c] = sum_{n,i,j} gy[n][2i + r][2j + s][k] x[n][i][j][c]"""
    N, H, W, Cc = x.shape
    K = gy.shape[-1]
    g6 = gy.reshape(N, H, 2, W, 2, K).permute(2, 4, 5, 0, 1, 3).reshape(4 * K, N * H * W)
    return (g6 @ x.reshape(N * H * W, Cc)).reshape(2, 2, K, Cc)


def colsum(a, b):
    """the bias gradient as a product of `a` = ones with the output gradient"""
    return (a * b).sum((0, 1, 2))


def fwd_ksteps(R, S, Cc):
    return -(-R * S * Cc // 32)


# ---- operand sets (fixed seeds, every value fp32) --------------------------------------------------------------------
SETS = ("channels", "quiet", "loud", "deferred")


class Operands(object):
    """x: what the entry point is fed; in_scale: the consumer's own per-channel affine (relu(x * in_scale), shift 0) or None;
    xa: the activation the conv multiplies, fp32 (exact: the scales are powers of two); w: HWIO fp32"""

    def __init__(self, x, w, in_scale=None):
        self.x, self.w, self.in_scale = x, w, in_scale
        self.xa = x if in_scale is None else torch.relu(x * in_scale)


def _pow2(gen, n, lo, hi):
    """n exponents from [lo, hi], both ends present -> 2^e as fp32"""
    e = torch.randint(lo, hi + 1, (n,), generator=gen)
    e[0], e[1] = lo, hi
    return torch.ldexp(torch.ones(n), e)


LOUD_CHANNELS = (2, 3, 5)


def conv_operands(name, N, H, W, Cc, K, R, S, seed):
    g = torch.Generator().manual_seed(seed)
    he = (2.0 / (R * S * Cc)) ** 0.5
    x = torch.randn(N, H, W, Cc, generator=g)
    w = torch.randn(R, S, Cc, K, generator=g) * he
    if name == "quiet":
        # every activation in [2^-9, 2^-7]: its lo half is a subnormal of a few bits, the whole tensor sits on the floor
        x = (1.0 + 3.0 * torch.rand(N, H, W, Cc, generator=g)) * 2.0 ** -9
        return Operands(x, w * 2.0 ** -10)
    sx, sw = _pow2(g, Cc, -8, 6), _pow2(g, K, -10, 3)
    w = w * sw
    if name == "deferred":
        return Operands(x, w, in_scale=sx)
    x = torch.relu(x) * sx
    if name == "loud":
        for c in LOUD_CHANNELS:          # up to 3.8125 * 2^16 = 249856 < 2.5e5; 3.875 * 16 = 62
            if c < Cc:
                x[..., c] = torch.relu(torch.randn(N, H, W, generator=g)).clamp(max=3.8125) * 65536.0
        for k in LOUD_CHANNELS:
            if k < K:
                w[..., k] = torch.randn(R, S, Cc, generator=g).clamp(-3.875, 3.875) * 16.0
        x[0, 0, 0, LOUD_CHANNELS[0]], w[0, 0, 0, LOUD_CHANNELS[0]] = 3.8125 * 65536.0, -62.0      # the ends themselves
    else:
        assert name == "channels", name
    return Operands(x, w)


def grad_operands(N, H, W, Cc, K, R, S, seed, gy_hw=None):
    """backward operands: x and w as `channels`, gy with output channel k scaled by 2^g_k, g_k from [-30, -10]; gy_hw: the
    output grid where it is not the input's (strided and transposed convs)"""
    o = conv_operands("channels", N, H, W, Cc, K, R, S, seed)
    g = torch.Generator().manual_seed(seed + 1)
    OH, OW = gy_hw or (H, W)
    o.gy = torch.randn(N, OH, OW, K, generator=g) * _pow2(g, K, -30, -10)
    return o


# name -> (N, H, W, C, K, taps, operand sets, seed)
FWD_CASES = {
    "fly 1x1": (2, 9, 11, 64, 64, 1, SETS, 101),
    "fly 3x3": (2, 9, 11, 64, 128, 3, SETS, 102),
    "presplit 1x1": (3, 14, 19, 64, 128, 1, SETS, 103),
    "presplit 3x3": (2, 14, 19, 64, 128, 3, SETS, 104),
    "halo": (4, 112, 149, 32, 32, 3, ("channels",), 105),
    "halo 64": (3, 149, 147, 64, 32, 3, SETS, 107),              # launch_conv_halo16<..., 64, ...>: 18 K steps, no K split
    "few-channel": (3, 150, 160, 8, 8, 3, ("channels",), 106),
}
# name -> (N, H, W, C, K, taps, seed)
BWD_CASES = {
    "tap": (2, 36, 48, 128, 128, 3, 201),
    "per-tap": (3, 12, 16, 128, 64, 3, 202),
    "halo": (4, 112, 149, 32, 32, 3, 203),
    "halo 64": (3, 149, 147, 64, 32, 3, 204),       # dx: the 32 -> 64 instance (9 K steps); dw: wgrad_halo16_kernel<64, 3>
}


def fwd_operands(case, name):
    N, H, W, Cc, K, taps, sets, seed = FWD_CASES[case]
    assert name in sets
    return conv_operands(name, N, H, W, Cc, K, taps, taps, seed + 1000 * SETS.index(name))


def bwd_operands(case):
    N, H, W, Cc, K, taps, seed = BWD_CASES[case]
    return grad_operands(N, H, W, Cc, K, taps, taps, seed)


def bwd_fmt(case):
    """format coefficient of a backward case's bf16x3 bounds (module docstring)"""
    return 8 if case in ("tap", "per-tap", "halo") else BF16_FMT_FEW


def wgrad_counts(case, slabs):
    """(ksteps, ranges) of a weight gradient's accumulation term.  A K step is 32 pixels and a range is one pixel slab; `slabs`
    is the most the workspace query allows (at most 2048), and with only an upper limit known the longest chain is all the
    K steps in one slab: ksteps = pixels / 32.  The halo kernel's counts are fixed by its launch (csrc/conv_wgrad.hip,
    acimg_conv2d_wgrad_split3): 256 workgroups, one slab each, walk the tiles of 4 x 32 pixels (4 K steps) in turn and add
    their 4 row groups through LDS at the end; with the caps (2086 + 256) that path sat at 0.0008 of its bound."""
    N, H, W = BWD_CASES[case][:3]
    if case.startswith("halo"):                     # (64 channels: 8 waves of 4 rows each, nothing to add through LDS)
        tiles = N * -(-H // 4) * -(-W // 32)
        return -(-tiles // 256) * 4 + 4, 256
    return -(-N * H * W // 32), slabs


# ---- the same formats behind the fp32 entry points ------------------------------------------------------------------------
# From 65536 pixels on acimg_conv2d_fwd / _dgrad / _wgrad and acimg_deconv_* leave the exact-f32 implicit GEMM (csrc/conv_f32.hip, conv_wgrad.hip):
#   few     3x3 / 1 / SAME, 4 - 16 channels convolved: conv_few16_kernel (f16x3 forward, bf16x3 data gradient); the data
#           gradient of 8 -> 32 is the 16-row instance of the halo kernel; weight gradient wgrad_halo16_kernel<16, 3> (bf16x3)
#   few/2   3x3 / 2 / SAME data gradient: conv_few16_kernel over the zero-inserted view of gy
#   few/bwd 3x3 / 1 / SAME data gradient of a 32 -> 8 layer: 8 gy channels into 32, the 32-row instance of conv_few16_kernel
#           (the layer's forward and weight gradient convolve 32 channels: not few-channel routes)
#   point   2x2 / 2 transposed conv 32 -> 8: patch2_32x8_kernel (f16x3 forward, bf16x3 data gradient), patch2_wgrad_32x8_kernel
# Shapes: >= 65536 pixels, heights and widths off the 16 x 32 / 8 x 32 / 4 x 32 tile grids (150 x 160 has whole tile columns);
# 3 x 149 x 147 = 65709 pixels is odd: the last 16-pixel group of the pointwise kernels has 3 dead lanes, the last 32-pixel
# block of its weight gradient ends inside one lane's 8 pixels (65709 = 32 * 2053 + 8 + 5), rows of 147 and images of 21903
# pixels end inside a lane's 8 pixels (147 = 8 * 18 + 3, 21903 = 8 * 2737 + 7).
# name -> (N, H, W, C, K, kind, forward operand sets, seed)
FP32_CASES = {
    "few 8->8": (3, 147, 161, 8, 8, "few", SETS, 111),
    "few 4->8": (3, 150, 160, 4, 8, "few", SETS, 112),           # 4 channels ride the 8-channel image, upper half zero
    "few 16->16": (3, 149, 163, 16, 16, "few", SETS, 113),
    "few 8->32": (3, 150, 161, 8, 32, "few", SETS, 114),         # its data gradient: the narrow halo instance
    "few/2 even": (3, 150, 160, 8, 8, "few/2", (), 115),         # leading pads 0, 0
    "few/2 odd": (3, 149, 147, 8, 8, "few/2", (), 116),          # leading pads 1, 1
    "few 32->8": (3, 147, 150, 32, 8, "few/bwd", (), 118),       # data gradient only: 8 gy channels into 32 columns
    "pointwise": (3, 149, 147, 32, 8, "point", ("channels", "quiet", "loud"), 117),
}
FP32_FWD = [(case, name) for case, rec in FP32_CASES.items() for name in rec[6]]
FP32_BWD = list(FP32_CASES)
FP32_WGRAD = [case for case, rec in FP32_CASES.items() if rec[5] not in ("few/2", "few/bwd")]
IMPULSE_CASES = FP32_WGRAD + ["halo 64"]


def few16_ksteps(cin):
    """K steps of one output element on conv_few16_kernel: the nine taps of cin channels (4 ride the 8-channel image) in
    32-deep MFMAs of 32 / cin taps each - 3 for 8 channels, 5 for 16; no K split"""
    return -(-9 // (32 // max(cin, 8)))


def fp32_products(case):
    """{'fwd': (product, K steps), 'dgrad': (product, K steps), 'wgrad': product} of a case, the K steps as the launches state
    them: the few-channel kernel above; the narrow halo instance walks 9 taps of one 32-channel chunk; the pointwise kernels
    multiply ONE 32-deep step per output element (4 taps x 8 channels, or 32 channels) and split nothing.  No route here has
    a K split or a tail: the real `ranges` is 0, and the bounds keep the module's allowance of MAX_RANGES as every case does."""
    N, H, W, Cc, K, kind = FP32_CASES[case][:6]
    if kind == "point":
        return dict(fwd=(deconv_fwd, 1), dgrad=(deconv_dgrad, 1), wgrad=deconv_wgrad)
    if kind == "few/2":
        return dict(dgrad=(conv_dgrad_s2(H, W), few16_ksteps(K)))
    if kind == "few/bwd":
        return dict(dgrad=(conv_dgrad, few16_ksteps(K)))
    return dict(fwd=(conv_fwd, few16_ksteps(Cc)), dgrad=(conv_dgrad, few16_ksteps(K) if K <= 16 else fwd_ksteps(3, 3, K)),
                wgrad=conv_wgrad(3))


def fp32_operands(case, name):
    """forward operands; the pointwise weights come back in TF layout [kh][kw][out][in]"""
    N, H, W, Cc, K, kind, sets, seed = FP32_CASES[case]
    assert name in sets
    taps = 2 if kind == "point" else 3
    o = conv_operands(name, N, H, W, Cc, K, taps, taps, seed + 1000 * SETS.index(name))
    if kind == "point":
        o.w = o.w.permute(0, 1, 3, 2).contiguous()
    return o


def fp32_grad_operands(case):
    """backward operands (grad_operands); gy lives on the output grid: 2H x 2W (pointwise), ceil(H / 2) x ceil(W / 2) (few/2)"""
    N, H, W, Cc, K, kind, _, seed = FP32_CASES[case]
    taps = 2 if kind == "point" else 3
    grid = {"point": (2 * H, 2 * W), "few/2": (same_pad2(H)[0], same_pad2(W)[0])}.get(kind)
    o = grad_operands(N, H, W, Cc, K, taps, taps, seed + 500, gy_hw=grid)
    if kind == "point":
        o.w = o.w.permute(0, 1, 3, 2).contiguous()
    return o


def fp32_wgrad_counts(case):
    """(ksteps, ranges) of the accumulation term of a weight gradient behind the fp32 entries, from its launch.
    wgrad_halo16_kernel<16, 3, NNT> (few): min(512, tiles) workgroups walk the 8 x 32 pixel tiles; a tile row of 32 pixels is
    one K step; NNT = 1 (<= 16 output channels) or 2 column tiles leave 8 / NNT row groups of waves, each multiplying NNT
    rows per tile, which meet through LDS at the end (8 / NNT - 1 additions); one slab per workgroup.
    patch2_wgrad_32x8_kernel (point): 256 workgroups of 16 waves walk the 32-pixel blocks (one K step each), the 16 waves
    are added through LDS (15 additions), one slab per workgroup."""
    N, H, W, Cc, K, kind = FP32_CASES[case][:6]
    if kind == "point":
        blocks = -(-N * H * W // 32)
        return -(-blocks // (256 * 16)) + 15, 256
    assert kind == "few", kind
    tiles = N * -(-H // 8) * -(-W // 32)
    nb, nnt = min(512, tiles), (1 if K <= 16 else 2)
    return -(-tiles // nb) * nnt + 8 // nnt - 1, nb


def patch2_db_adds(pixels):
    """fp32 additions on the longest chain of the pointwise weight gradient's fused bias gradient: a lane adds the 16 gy
    values it loads of every block its wave walks, one thread per channel adds 16 waves x 8 lanes, the final column sum
    adds the 256 workgroups (in whatever order: at most 256).  The bias gradient never meets the split: its bound is the
    fp32 summation bound, adds * 2^-24 * sum |gy|."""
    blocks = -(-pixels // 32)
    return 16 * -(-blocks // (256 * 16)) + 16 * 8 + 256


def impulse_pixels(case):
    """flat indices, on the input grid, of the `impulse` set's pixels: the first and the last pixel of the tensor, the four
    pixels round a tile corner (tile rows of 8 for the few-channel weight gradient, 4 for the halo one; 32 columns), the end
    of a row and the start of the next, the end of an image and the start of the next; for the pointwise kernel (pixels
    flat along its K axis: 8 per lane, 32 per block) both sides of a lane, block, row and image boundary, the last whole
    block's end, and the last live pixel with its whole 8-pixel lane group"""
    if case in FP32_CASES:
        N, H, W, _, _, kind = FP32_CASES[case][:6]
    else:
        (N, H, W), kind = BWD_CASES[case][:3], "halo"
    P = N * H * W
    if kind == "point":
        last_block = (P - 1) // 32 * 32
        px = {0, 7, 8, 31, 32, W - 1, W, H * W - 1, H * W, last_block - 1, last_block, P - 1}
        px.update(range((P - 1) // 8 * 8, P))
        return sorted(px)
    th = 4 if kind == "halo" else 8
    at = lambda n, y, x: (n * H + y) * W + x
    return sorted({0, P - 1, at(0, th - 1, 31), at(0, th - 1, 32), at(0, th, 31), at(0, th, 32), at(0, 1, W - 1), at(0, 2, 0),
                   at(0, H - 1, W - 1), at(1, 0, 0), at(N - 1, H - 1, 0)})


def impulse_operands(case):
    """weight-gradient operands whose gy is zero except at impulse_pixels (the pointwise case: at all four output positions
    of each): x as `channels`, the nonzero gy values as grad_operands scales them.  Every dw element is then a sum of at
    most o.npix products (one or two, mostly), so the FORMAT term of the bound, BF16_FMT_FEW * 2^-18, is what the kernel is held to -
    over 70 000 dense pixels a dropped cross term averages out as 1 / sqrt(n) under the summed worst case - and every
    element names the pixels it was summed from, so the run checks the indexing as well.  Adding an exact zero rounds
    nothing: the accumulation term counts one rounding per nonzero pixel, (ksteps, ranges) = (o.npix, 0)."""
    o = fp32_grad_operands(case) if case in FP32_CASES else bwd_operands(case)
    point = case in FP32_CASES and FP32_CASES[case][5] == "point"
    px = torch.tensor(impulse_pixels(case))
    N, H, W = o.x.shape[:3]
    K = o.gy.shape[-1]
    keep = torch.zeros(N * H * W, dtype=torch.bool)
    keep[px] = True
    keep = keep.reshape(N, H, W, 1)
    if point:
        keep = keep.reshape(N, H, 1, W, 1, 1).expand(N, H, 2, W, 2, 1).reshape(N, 2 * H, 2 * W, 1)
    o.gy = torch.where(keep, o.gy, torch.zeros_like(o.gy))
    o.npix = len(px)
    return o


# ----------------------------------------------------------------------------------------------------------------------
# the activation-plane layout (include/acimg.h, "Pre-split activation format"): two fp16 planes, hi at byte 0 and lo at
# lo_off, each of whole 16-pixel x 32-channel bricks of 1 KiB.  These functions mirror csrc/split_planes.hpp, the one C++
# statement of the layout: plane_bytes its split_plane_bytes, brick_index its plane_off with swz.
# ----------------------------------------------------------------------------------------------------------------------
def plane_bytes(rows, Cc):
    """bytes of one split-format plane: whole 16-pixel x 32-channel bricks"""
    return -(-rows // 16) * 16 * Cc * 2


def brick_index(rows, Cc):
    """fp16 element index inside a split-format plane of every element of a [rows, C] tensor, row-major: brick (row >> 4,
    c >> 5) of 1 KiB, inside it row & 15 at 64 bytes and 16-byte group (c >> 3) & 3 at group ((c >> 3) ^ -(row >> 2)) & 3"""
    r = torch.arange(rows).view(-1, 1)
    c = torch.arange(Cc).view(1, -1)
    off = ((r >> 4) * (Cc // 32) + (c >> 5)) * 1024 + (r & 15) * 64 + ((((c >> 3) ^ (-(r >> 2))) & 3) << 4) + (c & 7) * 2
    return (off // 2).reshape(-1)


def unsplit(planes, lo_off, rows, Cc):
    """two fp16 planes in LDS-tile order (uint8 buffer) -> float64 [rows, C] (undoing the 2^-2 scale)"""
    idx = brick_index(rows, Cc).to(planes.device)
    n = plane_bytes(rows, Cc)
    hi = planes[:n].view(torch.float16)[idx].double()
    lo = planes[lo_off: lo_off + n].view(torch.float16)[idx].double()
    return ((hi + lo) * 4.0).reshape(rows, Cc).cpu()


def valid_halves(buf, lo_off, rows, Cc):
    """the valid rows' fp16 elements of both planes as int16 (bit patterns), row-major"""
    idx = brick_index(rows, Cc).to(buf.device)
    n = plane_bytes(rows, Cc)
    return torch.cat([buf[o:o + n].view(torch.int16)[idx] for o in (0, lo_off)])


# what the bytes of split planes outside the valid rows' elements may hold (include/acimg.h: unspecified): fp16 NaN, and a
# large finite value (0x7b7b = 6.2e4 per half, 2.5e5 after the x4 scale) that a ReLU or a max cannot hide; (fill byte, gap
# between the hi plane's end and lo_off)
POISONS = ((0xFF, 0), (0x7B, 4096))


def repack(planes, lo_off, rows, Cc, fill, gap=0, slack=4096):
    """a copy of split-format planes that keeps only the valid rows' elements: every other byte - the pad rows of the last
    brick row, a `gap`-byte hole between the planes, `slack` bytes after the lo plane - holds `fill`.  -> (buffer, lo_off)"""
    n = plane_bytes(rows, Cc)
    lo2 = n + gap
    out = torch.full((lo2 + n + slack,), fill, dtype=torch.uint8, device=planes.device)
    idx = brick_index(rows, Cc).to(planes.device)
    for src, dst in ((0, 0), (lo_off, lo2)):
        out[dst:dst + n].view(torch.float16)[idx] = planes[src:src + n].view(torch.float16)[idx]
    return out, lo2


def make_planes(plan, device, x, rows, Cc, relu=0):
    """split planes of x [.., C] (identity affine) through ops.bn_relu_split, in a zeroed buffer: (planes, lo_off)"""
    from acimg import ops

    lo = plane_bytes(rows, Cc)
    planes = torch.zeros(2 * lo, dtype=torch.uint8, device=device)
    ops.bn_relu_split(plan, x.reshape(rows, Cc).float().contiguous().to(device), torch.ones(Cc, device=device),
                      torch.zeros(Cc, device=device), relu, planes, lo, rows, Cc)
    return planes, lo
