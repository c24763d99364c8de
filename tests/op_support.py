"""Helpers shared by the op-level GPU tests: error measures against an fp64 reference, TensorFlow's convolution geometry and
its fp64 statement, operand / buffer builders, dyadic data for exact reductions, and the forced trunk-kernel forms.  One
function per behaviour; where call sites differ (a floor, a fill value, whether the figure is printed) the difference is an
argument that every call site states."""
from collections import OrderedDict

import numpy as np
import torch
import torch.nn.functional as F

NAN = float("nan")


def up4(v):
    return (v + 3) & ~3


def raw_lib():
    """(acimg._lib, the loaded library): the raw C ABI"""
    from acimg import _lib as m
    return m, m.load()


# ----------------------------------------------------------------------------------------------------------------------
# error measures
# ----------------------------------------------------------------------------------------------------------------------
def rel_err(got, ref, floor, same_shape=True):
    """max |got - ref| / max(max |ref|, floor), in fp64; same_shape=False lets the two broadcast"""
    got = got.detach().cpu().double()
    ref = ref.detach().cpu().double()
    assert not same_shape or got.shape == ref.shape, (got.shape, ref.shape)
    return float((got - ref).abs().max() / max(float(ref.abs().max()), floor))


def l2_err(got, ref, floor):
    """|got - ref|_2 / max(|ref|_2, floor), in fp64"""
    got = got.detach().cpu().double()
    ref = ref.detach().cpu().double()
    return float((got - ref).norm() / max(float(ref.norm()), floor))


def close(got, ref, tol, what="", show=False):
    """rel_err(got, ref, 1e-12) is finite and <= tol; show: print the figure first"""
    got = got.detach().cpu().double()
    ref = ref.detach().cpu().double()
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    scale = max(ref.abs().max().item(), 1e-12)
    err = (got - ref).abs().max().item() / scale
    if show:
        print("%s: rel err %.3e (tol %.1e)" % (what, err, tol))
    assert np.isfinite(err) and err <= tol, "%s: rel err %.3e > %.1e" % (what, err, tol)


def close_at(default_tol, show=False):
    """`close` with a module's default tolerance: close(got, ref, tol=default_tol, what="")"""
    def check(got, ref, tol=default_tol, what=""):
        close(got, ref, tol, what, show)
    return check


def exact(got, ref, what):
    """bit-for-bit agreement with the fp64 reference; on a mismatch, say which cells differ (they name the tile, tap or row)"""
    got = got.detach().cpu().double()
    ref = ref.detach().cpu().double()
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    if not torch.equal(got, ref):
        bad = got != ref            # (NaN != anything)
        first = [(tuple(i), got[tuple(i)].item(), ref[tuple(i)].item()) for i in bad.nonzero()[:8].tolist()]
        raise AssertionError("%s: %d of %d elements differ; (index, got, ref): %s" % (what, int(bad.sum()), bad.numel(), first))


def bits_equal(a, b, what):
    assert torch.equal(a.view(torch.int32), b.view(torch.int32)), "%s differs between two identical calls" % what


def same_bits(a, b):
    """bit-identical (NaN included) fp32 tensors"""
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


# ----------------------------------------------------------------------------------------------------------------------
# TensorFlow convolution geometry and its fp64 statement
# ----------------------------------------------------------------------------------------------------------------------
def same_pads(size, k, s):
    """SAME along one axis: (output size, leading pad, trailing pad); the odd pad comes last"""
    out = -(-size // s)
    tot = max((out - 1) * s + k - size, 0)
    return out, tot // 2, tot - tot // 2


def conv_geom(H, W, R, S, stride, padding):
    """padding "SAME", "VALID" or an integer -> OH, OW, (pt, pb, pl, pr)"""
    if padding == "SAME":
        OH, pt, pb = same_pads(H, R, stride)
        OW, pl, pr = same_pads(W, S, stride)
    elif padding == "VALID":
        OH, OW = (H - R) // stride + 1, (W - S) // stride + 1
        pt = pb = pl = pr = 0
    else:
        p = padding
        OH, OW = (H + 2 * p - R) // stride + 1, (W + 2 * p - S) // stride + 1
        pt = pb = pl = pr = p
    return OH, OW, (pt, pb, pl, pr)


def tf_conv_ref(x, w, stride, pads, bias=None):
    """x NHWC fp64, w HWIO; pads = (pt, pb, pl, pr)"""
    xt = x.permute(0, 3, 1, 2)
    xt = F.pad(xt, (pads[2], pads[3], pads[0], pads[1]))
    y = F.conv2d(xt, w.permute(3, 2, 0, 1), bias, stride=stride)
    return y.permute(0, 2, 3, 1)


# ----------------------------------------------------------------------------------------------------------------------
# operands and buffers
# ----------------------------------------------------------------------------------------------------------------------
def rnd(gen, *shape):
    return torch.randn(*shape, generator=gen, dtype=torch.float64)


def dev(t, device):
    return t.float().contiguous().to(device)


def widen(t, ld, off=0, fill=NAN, dtype=torch.float32):
    """[..., n] -> [..., ld] of `dtype` on the CPU with t at columns off .. off + n and `fill` elsewhere (NaN: a column that
    must never be read shows when it is)"""
    out = torch.full(tuple(t.shape[:-1]) + (ld,), fill, dtype=dtype)
    out[..., off:off + t.shape[-1]] = t.to(dtype)
    return out


def pad_last(t, n):
    """zero padded to n channels, dtype kept"""
    return widen(t, n, fill=0.0, dtype=t.dtype)


SENTINEL = 7.0            # what the small-op tests fill outputs with: never a result of their data


def pads_untouched(t, C, what):
    assert (t[..., C:] == SENTINEL).all(), "%s: pad columns written" % what


def pad_w(w, cp, kp):
    """HWIO -> zero padded [R,S,cp,kp]"""
    R, S, Cc, K = w.shape
    out = torch.zeros(R, S, cp, kp, dtype=w.dtype)
    out[:, :, :Cc, :K] = w
    return out


# ----------------------------------------------------------------------------------------------------------------------
# dyadic data: reductions whose every partial sum is exact in fp32, so the kernel must equal fp64 bit for bit
# ----------------------------------------------------------------------------------------------------------------------
EXACT_LIMIT = 2.0 ** 24


def dyadic(g, shape, res, maxabs, lo=None):
    """multiples of `res` in [lo, maxabs] (lo defaults to -maxabs), fp64"""
    lo_k = int(round((-maxabs if lo is None else lo) / res))
    hi_k = int(round(maxabs / res))
    return torch.randint(lo_k, hi_k + 1, shape, generator=g).double() * res


def assert_f32(t, what):
    """every value is exactly representable in fp32"""
    assert torch.equal(t.float().double(), t), "%s is not exactly representable in fp32" % what


def assert_exact_sum(terms, res, what, dim=None):
    """sum |term| / res < 2^24: every partial sum of these terms is exact in fp32, in any order"""
    s = terms.abs().sum() if dim is None else terms.abs().sum(dim).max()
    assert float(s) / res < EXACT_LIMIT, "%s: magnitude bound violated (%.3g / %g >= 2^24)" % (what, float(s), res)


def bn_bwd_ref(xhat, gm, gamma, invstd):
    """fp64 statement of the comment above bn_bwd_reduce_kernel; gm = gy already masked by the ReLU"""
    n = xhat.shape[0]
    dbeta = gm.sum(0)
    dgamma = (gm * xhat).sum(0)
    gx = gamma * invstd * (gm - dbeta / n - xhat * (dgamma / n))
    return gx, dgamma, dbeta


def bn_bwd_dyadic_inputs(g, rows, C):
    """xhat in {+-0.5, +-1}, power-of-two invstd, dyadic mean: x - mean and (x - mean) * invstd are exact in fp32;
    dyadic gamma / beta with beta an odd multiple of 1/8 keep the pre-activation gamma*xhat + beta away from 0, so the
    recomputed ReLU mask cannot flip (FMA contraction included)"""
    xhat = torch.tensor([-1.0, -0.5, 0.5, 1.0], dtype=torch.float64)[torch.randint(0, 4, (rows, C), generator=g)]
    gy = torch.randint(-1, 2, (rows, C), generator=g).double()
    mean = torch.randint(-8, 9, (C,), generator=g).double() / 4
    invstd = 2.0 ** torch.randint(-1, 3, (C,), generator=g).double()
    sign = torch.randint(0, 2, (C,), generator=g).double() * 2 - 1
    gamma = sign * torch.randint(1, 5, (C,), generator=g).double() / 2
    beta = (2 * torch.randint(-4, 4, (C,), generator=g).double() + 1) / 8
    x = mean + xhat / invstd
    scale = gamma * invstd
    shift = beta - mean * scale
    pre = x * scale + shift
    assert (pre != 0).all(), "a pre-activation is exactly 0"
    for t, name in ((x, "x"), (mean, "mean"), (invstd, "invstd"), (gamma, "gamma"), (scale, "scale"),
                    (shift, "shift"), (pre, "pre-activation")):
        assert_f32(t, name)
    gm = gy * (pre > 0)
    del pre
    assert_exact_sum(gm, 1.0, "dbeta", dim=0)
    assert_exact_sum(gm * xhat, 0.5, "dgamma", dim=0)
    return x, gy, gm, xhat, mean, invstd, gamma, scale, shift


# ----------------------------------------------------------------------------------------------------------------------
# the trunk forward conv's kernel forms, forced through acimg_configure: name -> (overrides, the kernel it must reach:
# acimg_conv2d_fwd_split3_tiling()[2]: 0 one tile per workgroup, 1 persistent, 2 ring, 3 halo)
# ----------------------------------------------------------------------------------------------------------------------
TRUNK_FORMS = OrderedDict([
    ("one-tile whole", (dict(trunk_persistent=0, tail_split=0, trunk_ring=0), 0)),
    ("persistent whole", (dict(trunk_persistent=2, tail_split=0, trunk_ring=0), 1)),
    ("one-tile", (dict(trunk_persistent=0, trunk_ring=0), 0)),
    ("persistent", (dict(trunk_persistent=2, trunk_ring=0), 1)),
    ("staggered", (dict(trunk_persistent=2, trunk_stagger=50, trunk_ring=0), 1)),
    ("spread", (dict(trunk_persistent=2, trunk_dma_pos=1, trunk_ring=0), 1)),
    ("auto no ring", (dict(trunk_ring=0), None)),
    ("auto", (dict(), None)),
    ("ring256 whole", (dict(trunk_ring=2, trunk_ring_bm=256, tail_split=0), 2)),
    ("ring128 whole", (dict(trunk_ring=2, trunk_ring_bm=128, tail_split=0), 2)),
    ("ring256", (dict(trunk_ring=2, trunk_ring_bm=256), 2)),
    ("ring128", (dict(trunk_ring=2, trunk_ring_bm=128), 2)),
    ("ring256 s3", (dict(trunk_ring=2, trunk_ring_bm=256, tail_s=3), 2)),
    ("ring", (dict(trunk_ring=2), 2)),
    # the halo kernel takes the 3x3 cases only (the others stay on the shipped choice)
    ("halo whole", (dict(trunk_halo=2, tail_split=0), 3)),
    ("halo", (dict(trunk_halo=2), 3)),
    ("halo s3", (dict(trunk_halo=2, tail_s=3), 3)),
])


def trunk_forms(*names):
    """((name, overrides, kernel), ...) of the named forms, in the order asked for"""
    return tuple((n,) + TRUNK_FORMS[n] for n in names)
