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


def bound_bf16x3(aa, ab, ksteps, ranges=MAX_RANGES, prod=torch.mul):
    """per-output-element bound of a bf16x3 product (module docstring)"""
    ab_, _, _ = _bound_products(aa, ab, prod)
    return (8 * U18 + (ksteps + ranges + 2) * U24) * ab_


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


def emulate_bf16x3(a, b, prod):
    ah, al = split_bf16(a)
    bh, bl = split_bf16(b)
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
            x[..., c] = torch.relu(torch.randn(N, H, W, generator=g)).clamp(max=3.8125) * 65536.0
        for k in LOUD_CHANNELS:
            w[..., k] = torch.randn(R, S, Cc, generator=g).clamp(-3.875, 3.875) * 16.0
        x[0, 0, 0, LOUD_CHANNELS[0]], w[0, 0, 0, LOUD_CHANNELS[0]] = 3.8125 * 65536.0, -62.0      # the ends themselves
    else:
        assert name == "channels", name
    return Operands(x, w)


def grad_operands(N, H, W, Cc, K, R, S, seed):
    """backward operands: x and w as `channels`, gy with output channel k scaled by 2^g_k, g_k from [-30, -10]"""
    o = conv_operands("channels", N, H, W, Cc, K, R, S, seed)
    g = torch.Generator().manual_seed(seed + 1)
    o.gy = torch.randn(N, H, W, K, generator=g) * _pow2(g, K, -30, -10)
    return o


# name -> (N, H, W, C, K, taps, operand sets, seed)
FWD_CASES = {
    "fly 1x1": (2, 9, 11, 64, 64, 1, SETS, 101),
    "fly 3x3": (2, 9, 11, 64, 128, 3, SETS, 102),
    "presplit 1x1": (3, 14, 19, 64, 128, 1, SETS, 103),
    "presplit 3x3": (2, 14, 19, 64, 128, 3, SETS, 104),
    "halo": (4, 112, 149, 32, 32, 3, ("channels",), 105),
    "few-channel": (3, 150, 160, 8, 8, 3, ("channels",), 106),
}
# name -> (N, H, W, C, K, taps, seed)
BWD_CASES = {
    "tap": (2, 36, 48, 128, 128, 3, 201),
    "per-tap": (3, 12, 16, 128, 64, 3, 202),
    "halo": (4, 112, 149, 32, 32, 3, 203),
}


def fwd_operands(case, name):
    N, H, W, Cc, K, taps, sets, seed = FWD_CASES[case]
    assert name in sets
    return conv_operands(name, N, H, W, Cc, K, taps, taps, seed + 1000 * SETS.index(name))


def bwd_operands(case):
    N, H, W, Cc, K, taps, seed = BWD_CASES[case]
    return grad_operands(N, H, W, Cc, K, taps, taps, seed)


def wgrad_counts(case, slabs):
    """(ksteps, ranges) of a weight gradient's accumulation term.  A K step is 32 pixels and a range is one pixel slab; `slabs`
    is the most the workspace query allows (at most 2048), and with only an upper limit known the longest chain is all the
    K steps in one slab: ksteps = pixels / 32.  The halo kernel's counts are fixed by its launch (csrc/igemm.hip,
    acimg_conv2d_wgrad_split3): 256 workgroups, one slab each, walk the tiles of 4 x 32 pixels (4 K steps) in turn and add
    their 4 row groups through LDS at the end; with the caps (2086 + 256) that path sat at 0.0008 of its bound."""
    N, H, W = BWD_CASES[case][:3]
    if case == "halo":
        tiles = N * -(-H // 4) * -(-W // 32)
        return -(-tiles // 256) * 4 + 4, 256
    return -(-N * H * W // 32), slabs
