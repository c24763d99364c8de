"""The exact-f32 few-channel kernels off the 3x3 / stride-1 / SAME path, held to EXACT answers.

wgrad_halo_kernel (exact-f32 MFMA weight gradient, 4 / 8 / 16 channels into <= 16 columns, from 65536 pixels on) and
direct_conv_kernel (one lane = one pixel, fp32 FMAs) serve every few-channel shape that the 16-bit-split MFMA forms
(wgrad_halo16_kernel, conv_few16_kernel) do not take: the final 1x1 layer of both single-modality U-Nets among them.  Both
compute in plain fp32, so with operands for which EVERY partial sum is an integer below 2^24 the result equals the fp64
reference bit for bit in any summation order: the comparisons here are torch.equal, and one dropped, doubled or misplaced pixel
among 66000 changes the answer.  Each test asserts that premise on the CPU (sum |x| |gy|, sum |x| |w| + |bias|, the statistics
partials per block) before it calls the GPU.  Two operand sets per case:
  dense: every operand a uniform integer in [-3, 3]: every pixel and tap counts;
  wide:  one operand holds integers in [-2047, 2047] (12 significant bits: a fall to bf16 or single-fp16 operands is wrong, not
         merely less accurate), the other a small integer (forward, data gradient) or a gy in {-1, 0, 1} that is non-zero at one
         element in sixteen (weight gradient).
The only tolerance in this file is the derived 2^-21 of the sigmoid cases (test_direct_conv_1x1).

Images: A = 1 x 229 x 287 and B = 2 x 181 x 182 OUTPUT pixels, the smallest of one and two images past 65536; both are ragged
in the 8 x 32 tile (OH % 8, OW % 32 != 0), in B the tile ranges cross the image boundary.

The case behind each kernel instance (launch_wgrad in csrc/conv_wgrad.hip, NKT = ceil((R S C + 1) / 16) row tiles;
launch_direct in csrc/conv_f32.hip; profiles/few_channel_f32/kernel_stats.txt is the kernel trace of this file):
  wgrad_halo_kernel<1, 1>   1x1 8->3 SAME (d_final of acimg/unet_vae.py) and 8->1; 1x3 4->4 SAME
  wgrad_halo_kernel<1, 2>   1x1 16->16; 2x2 4->8 VALID; 1x3 8->12 SAME
  wgrad_halo_kernel<1, 3>   2x2 8->8 SAME (pads 0 / 1); 3x3 4->16 VALID
  wgrad_halo_kernel<1, 5>   2x3 8->4 SAME (pad_t 0, pad_l 1); 3x3 8->8 VALID; 2x2 16->16 VALID
  wgrad_halo_kernel<1, 10>  3x3 16->16 VALID (KK = 144, the largest); 3x2 16->12 SAME
  wgrad_f32_kernel<128, 16, 4>  every one of these again with wgrad_halo = 0
  direct_conv_kernel<1, 1, 8>   forward 1x1 8->3, 8->1 and 8->8 at stride 2
  direct_conv_kernel<0, 0, 0>   forward 1x1 4->8 (one channel group) and 16->32 (four); the data gradients of 1x1 8->3 (gy padded
                                to 4 channels) and of 2x3 VALID 8->16
"""
import pytest
import torch
import torch.nn.functional as F

from op_support import exact, pad_last, up4, widen

pytestmark = pytest.mark.gpu

LIM = float(2 ** 24)
NAN = float("nan")
A = (1, 229, 287)
B = (2, 181, 182)


def ints(g, lo, hi, *shape):
    return torch.randint(lo, hi + 1, shape, generator=g).double()


def sparse_signs(g, *shape):
    """{-1, 0, 1}, non-zero at about one element in sixteen"""
    return (torch.rand(*shape, generator=g) < 1.0 / 16).double() * (2 * torch.randint(0, 2, shape, generator=g).double() - 1)


def still_nan(t, what):
    assert bool(torch.isnan(t).all()), "%s: written to" % what


# ------------------------------------------------------------------------------------------------
# wgrad_halo_kernel
# ------------------------------------------------------------------------------------------------
def geometry(img, R, S, padding):
    """input size and leading / trailing pads of a stride-1 conv with OH x OW output pixels (TensorFlow's SAME: the odd pad
    row / column comes last, so R = 2 pads 0 / 1)"""
    N, OH, OW = img
    if padding == "SAME":
        return OH, OW, ((R - 1) // 2, R - 1 - (R - 1) // 2, (S - 1) // 2, S - 1 - (S - 1) // 2)
    return OH + R - 1, OW + S - 1, (0, 0, 0, 0)


def wgrad_ref(x, gy, R, S, pads):
    """dW[r][s][c][k] = sum over pixels of x[n, oh + r - pad_t, ow + s - pad_l, c] gy[n, oh, ow, k]; fp64, tap by tap"""
    OH, OW = gy.shape[1], gy.shape[2]
    xp = F.pad(x, (0, 0, pads[2], pads[3], pads[0], pads[1]))
    dw = torch.zeros(R, S, x.shape[-1], gy.shape[-1], dtype=torch.float64)
    for r in range(R):
        for s in range(S):
            dw[r, s] = torch.einsum("nhwc,nhwk->ck", xp[:, r:r + OH, s:s + OW], gy)
    return dw


# name, output image, C, K, R, S, padding, NKT of the instance, extras: "pipe" = also with wgrad_minpix = 1024 (a workgroup
# walks four or five tiles), "nodb" = also with db = NULL
WGRAD_CASES = [
    ("1x1_8to3_same", A, 8, 3, 1, 1, "SAME", 1, ("pipe", "nodb")),
    ("1x1_8to1_same", B, 8, 1, 1, 1, "SAME", 1, ()),
    ("1x3_4to4_same", B, 4, 4, 1, 3, "SAME", 1, ("pipe",)),
    ("1x1_16to16", B, 16, 16, 1, 1, "SAME", 2, ("nodb",)),
    ("2x2_4to8_valid", A, 4, 8, 2, 2, "VALID", 2, ("pipe",)),
    ("1x3_8to12_same", B, 8, 12, 1, 3, "SAME", 2, ()),
    ("2x2_8to8_same", B, 8, 8, 2, 2, "SAME", 3, ("pipe",)),
    ("3x3_4to16_valid", A, 4, 16, 3, 3, "VALID", 3, ("nodb",)),
    ("2x3_8to4_same", A, 8, 4, 2, 3, "SAME", 5, ("nodb",)),
    ("3x3_8to8_valid", B, 8, 8, 3, 3, "VALID", 5, ("pipe",)),
    ("2x2_16to16_valid", A, 16, 16, 2, 2, "VALID", 5, ()),
    ("3x3_16to16_valid", A, 16, 16, 3, 3, "VALID", 10, ("pipe", "nodb")),
    ("3x2_16to12_same", B, 16, 12, 3, 2, "SAME", 10, ("pipe",)),
]


@pytest.mark.parametrize("opset", ["dense", "wide"])
@pytest.mark.parametrize("case", WGRAD_CASES, ids=[c[0] for c in WGRAD_CASES])
def test_wgrad_halo_exact(device, case, opset):
    """acimg_conv2d_wgrad on wgrad_halo_kernel<1, NKT>: dw and db exact against fp64 on both operand sets; x and gy are channel
    slices of wider buffers whose other channels hold NaN, dw and db start as NaN, the rows and columns of dw outside the layer
    stay NaN, columns K..up4(K) are exactly zero; two runs give the same bits; the multi-tile pipelined loop (wgrad_minpix =
    1024: 65 workgroups for 261 / 276 tiles), db = NULL and the per-tap route (wgrad_halo = 0) give the same exact answer."""
    from acimg import _lib, ops

    name, img, Cc, K, R, S, padding, nkt, extras = case
    N, OH, OW = img
    H, W, pads = geometry(img, R, S, padding)
    M, KK, Kp = N * OH * OW, R * S * Cc, up4(K)
    # the route: wgrad_halo_ok and not wgrad_halo16_ok (csrc/conv_wgrad.hip), and the instance its NKT chain picks
    assert M >= 65536 and Cc in (4, 8, 16) and Kp <= 16 and not (R == 3 and S == 3 and padding == "SAME")
    assert OH % 8 != 0 and OW % 32 != 0
    assert min(v for v in (1, 2, 3, 5, 10) if v >= (KK + 1 + 15) // 16) == nkt

    g = torch.Generator().manual_seed(1000 + 16 * KK + K + (opset == "wide"))
    if opset == "dense":
        x, gy = ints(g, -3, 3, N, H, W, Cc), ints(g, -3, 3, N, OH, OW, K)
    else:
        x, gy = ints(g, -2047, 2047, N, H, W, Cc), sparse_signs(g, N, OH, OW, K)
    # the premise of exactness: no sum of magnitudes reaches 2^24
    assert wgrad_ref(x.abs(), gy.abs(), R, S, pads).max().item() < LIM and gy.abs().sum((0, 1, 2)).max().item() < LIM
    ref_dw = pad_last(wgrad_ref(x, gy, R, S, pads), Kp).reshape(KK, Kp)
    ref_db = pad_last(gy.sum((0, 1, 2)), Kp)

    ldx, xoff, ldgy, goff, ldw = Cc + 8, 4, Kp + 8, 4, Kp + 4
    xd = widen(x, ldx, xoff).to(device)
    gyd = widen(pad_last(gy, Kp), ldgy, goff).to(device)       # (the layer's own pad channels K..up4(K) are zeros)
    d = ops.conv_desc(N, H, W, Cc, K, R, S, 1, padding, ldx=ldx, ldw=ldw)
    assert (d.OH, d.OW, d.pad_t, d.pad_l) == (OH, OW, pads[0], pads[2])

    def run(what, with_db=True):
        dw = torch.full((KK + 2, ldw), NAN, device=device)
        db = torch.full((ldw,), NAN, device=device)
        plan = ops.Plan(device, eager=True)
        ops.conv2d_wgrad(plan, d, ops.Ptr(xd, xoff), ops.Ptr(gyd, goff), ldgy, dw, db if with_db else None)
        torch.cuda.synchronize()
        dw, db = dw.cpu(), db.cpu()
        what = "%s %s, %s" % (name, opset, what)
        exact(dw[:KK, :Kp], ref_dw, what + ": dw[kk][n]")
        still_nan(dw[KK:], what + ": dw rows past R S C")
        still_nan(dw[:, Kp:], what + ": dw columns past up4(K)")
        if with_db:
            exact(db[:Kp], ref_db, what + ": db")
            still_nan(db[Kp:], what + ": db past up4(K)")
        else:
            still_nan(db, what + ": db (not asked for)")
        return dw, db

    dw1, db1 = run("one tile per workgroup")
    dw2, db2 = run("second run")
    assert torch.equal(dw1[:KK, :Kp], dw2[:KK, :Kp]) and torch.equal(db1[:Kp], db2[:Kp])
    if "nodb" in extras:
        run("db = NULL", with_db=False)
    if "pipe" in extras:
        tiles, grid = N * -(-OH // 8) * -(-OW // 32), -(-M // 1024)
        assert tiles >= 3 * grid and tiles % grid != 0
        try:
            _lib.configure(wgrad_minpix=1024)
            run("%d tiles on %d workgroups" % (tiles, grid))
        finally:
            _lib.configure()
    try:
        _lib.configure(wgrad_halo=0)
        run("per-tap kernel (wgrad_halo = 0)")
    finally:
        _lib.configure()


# ------------------------------------------------------------------------------------------------
# direct_conv_kernel, forward
# ------------------------------------------------------------------------------------------------
# name, N, H, W (input), C, K, stride
FWD_CASES = [
    ("8to3", 1, 229, 287, 8, 3, 1),
    ("8to1", 2, 181, 182, 8, 1, 1),
    ("4to8", 2, 181, 182, 4, 8, 1),
    ("16to32", 1, 229, 287, 16, 32, 1),
    ("8to8_stride2", 2, 361, 363, 8, 8, 2),
]


@pytest.mark.parametrize("opset", ["dense", "wide"])
@pytest.mark.parametrize("case", FWD_CASES, ids=[c[0] for c in FWD_CASES])
def test_direct_conv_1x1(device, case, opset):
    """acimg_conv2d_fwd with bias on direct_conv_kernel, 1x1 layers, x and y channel slices of wider NaN buffers.
    ACT_NONE and ACT_RELU: exact; channels K..up4(K) exactly zero, everything beyond up4(K) untouched.
    ACT_NONE with statistics: acimg_conv2d_stats_rows rows, EVERY partial row exact against the fp64 sums of its own block of
    pixels (256: the fused form, up to 16 output channels; 128 for the 32-channel layer, whose partials a second kernel forms
    from the stored tensor).  On the wide set only the sums: a squared output there passes 2^24.
    ACT_SIGMOID (the product's d_final) against fp64 sigmoid of the exact pre-activation, |err| <= 2^-21 absolute - derived, not
    tuned: expf within 2 ulp, one addition, one division within 2.5 ulp, a result in (0, 1]: at most 5 ulp (2^-24 each) of a
    value no larger than 1."""
    from acimg import ops

    name, N, H, W, Cc, K, stride = case
    OH, OW = -(-H // stride), -(-W // stride)
    M, Kp = N * OH * OW, up4(K)
    units = -(-M // 256) * -(-K // 8)
    # the route (direct_ok from 65536 pixels on; 1x1 is never the few-channel MFMA form), a last block with dead lanes, and a
    # grid of 8 ranges whose last workgroups find no unit
    assert M >= 65536 and Cc <= 16 and K <= 32 and M % 256 != 0 and units % 8 != 0

    g = torch.Generator().manual_seed(2000 + 64 * Cc + K + stride + (opset == "wide"))
    x = ints(g, -3, 3, N, H, W, Cc) if opset == "dense" else ints(g, -2047, 2047, N, H, W, Cc)
    w, b = ints(g, -3, 3, Cc, K), ints(g, -3, 3, K)
    xs = x[:, ::stride, ::stride]                    # (1x1 SAME at stride 2: no padding, input pixel 2 oh, 2 ow)
    assert (xs.abs() @ w.abs() + b.abs()).max().item() < LIM
    pre = xs @ w + b
    assert pre.shape == (N, OH, OW, K)

    ldx, xoff, ldy, yoff = Cc + 4, 4, Kp + 8, 4
    xd = widen(x, ldx, xoff).to(device)
    wd = pad_last(w, Kp).float().reshape(1, 1, Cc, Kp).to(device)
    bd = pad_last(b, Kp).float().to(device)
    plan = ops.Plan(device, eager=True)

    def run(act, stats=None):
        d = ops.conv_desc(N, H, W, Cc, K, 1, 1, stride, "SAME", ldx=ldx, ldy=ldy, act=act)
        assert (d.OH, d.OW, d.pad_t, d.pad_l) == (OH, OW, 0, 0)
        y = torch.full((N, OH, OW, ldy), NAN, device=device)
        ops.conv2d_fwd(plan, d, ops.Ptr(xd, xoff), wd, bd, ops.Ptr(y, yoff), stats=stats)
        torch.cuda.synchronize()
        y = y.cpu()
        what = "1x1 %s %s act %d" % (name, opset, act)
        still_nan(y[..., :yoff], what + ": channels before the slice")
        still_nan(y[..., yoff + Kp:], what + ": channels past up4(K)")
        exact(y[..., yoff + K:yoff + Kp], torch.zeros(N, OH, OW, Kp - K, dtype=torch.float64), what + ": channels K..up4(K)")
        return y[..., yoff:yoff + K], what

    y, what = run(ops.ACT_NONE)
    exact(y, pre, what)
    y, what = run(ops.ACT_RELU)
    exact(y, torch.relu(pre), what)

    d0 = ops.conv_desc(N, H, W, Cc, K, 1, 1, stride, "SAME", ldx=ldx, ldy=ldy, act=ops.ACT_NONE)
    rows = ops.conv2d_stats_rows(d0)
    bm, _, splits = ops.conv2d_fwd_tiling(d0)
    block = 256 if splits > 1 else bm
    assert block == (256 if K <= 16 else 128) and rows == -(-M // block)
    flat = torch.zeros(rows * block, K, dtype=torch.float64)
    flat[:M] = pre.reshape(M, K)
    blocks = flat.reshape(rows, block, K)
    ref_sum, ref_sq = blocks.sum(1), (blocks * blocks).sum(1)
    assert blocks.abs().sum(1).max().item() < LIM
    stats = torch.full((rows, 2, d0.ldw), NAN, device=device)
    y, what = run(ops.ACT_NONE, stats)
    exact(y, pre, what + " with statistics")
    exact(stats[:, 0, :K], ref_sum, what + ": sum of every block")
    if opset == "dense":
        assert ref_sq.max().item() < LIM
        exact(stats[:, 1, :K], ref_sq, what + ": sum of squares of every block")

    y, what = run(ops.ACT_SIGMOID)
    err = (y.double() - torch.sigmoid(pre)).abs().max().item()
    print("%s: sigmoid max |err| %.3e (bound %.3e)" % (what, err, 2.0 ** -21))
    assert err <= 2.0 ** -21, "%s: |err| %.3e > 2^-21" % (what, err)


# ------------------------------------------------------------------------------------------------
# direct_conv_kernel, data gradient (mode 1)
# ------------------------------------------------------------------------------------------------
# name, N, H, W (input of the layer = dx), C, K, R, S, padding
DGRAD_CASES = [
    ("1x1_8to3", 2, 181, 182, 8, 3, 1, 1, "SAME"),
    ("2x3_8to16_valid", 1, 229, 287, 8, 16, 2, 3, "VALID"),
]


@pytest.mark.parametrize("opset", ["dense", "wide"])
@pytest.mark.parametrize("case", DGRAD_CASES, ids=[c[0] for c in DGRAD_CASES])
def test_direct_conv_data_gradient(device, case, opset):
    """acimg_conv2d_dgrad without a mask on direct_conv_kernel<0, 0, 0> in mode 1 (a stride-1 conv over gy with flipped taps),
    with a residual, dx into a channel slice of a wider NaN buffer, gy a slice too: exact (dense: every operand in [-3, 3];
    wide: gy in [-2047, 2047])"""
    from acimg import ops

    name, N, H, W, Cc, K, R, S, padding = case
    Kp = up4(K)
    OH, OW = (H, W) if padding == "SAME" else (H - R + 1, W - S + 1)
    assert N * H * W >= 65536 and (N * H * W) % 256 != 0 and Kp <= 16 and Cc <= 32 and not (R == 3 and S == 3)
    g = torch.Generator().manual_seed(3000 + 16 * R * S + K + (opset == "wide"))
    gy = ints(g, -3, 3, N, OH, OW, K) if opset == "dense" else ints(g, -2047, 2047, N, OH, OW, K)
    w, res = ints(g, -3, 3, R, S, Cc, K), ints(g, -3, 3, N, H, W, Cc)

    def dgrad(gy_, w_, res_):
        """dx[n, oh + r, ow + s, c] += gy[n, oh, ow, k] w[r, s, c, k] (VALID, or 1x1), + residual; fp64, tap by tap"""
        dx = res_.clone()
        for r in range(R):
            for s in range(S):
                dx[:, r:r + OH, s:s + OW] += gy_ @ w_[r, s].t()
        return dx

    assert dgrad(gy.abs(), w.abs(), res.abs()).max().item() < LIM
    ref = dgrad(gy, w, res)

    ldgy, goff, lddx, xoff = Kp + 4, 4, Cc + 8, 4
    gyd = widen(pad_last(gy, Kp), ldgy, goff).to(device)
    wd = pad_last(w, Kp).float().to(device)
    dx = torch.full((N, H, W, lddx), NAN, device=device)
    d = ops.conv_desc(N, H, W, Cc, K, R, S, 1, padding)
    assert (d.OH, d.OW) == (OH, OW)
    plan = ops.Plan(device, eager=True)
    ops.conv2d_dgrad(plan, d, ops.Ptr(gyd, goff), ldgy, wd, ops.Ptr(dx, xoff), res.float().to(device), Cc, lddx=lddx)
    torch.cuda.synchronize()
    dx = dx.cpu()
    what = "data gradient %s %s" % (name, opset)
    exact(dx[..., xoff:xoff + Cc], ref, what)
    still_nan(dx[..., :xoff], what + ": channels before the slice")
    still_nan(dx[..., xoff + Cc:], what + ": channels past C")
