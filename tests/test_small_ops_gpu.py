"""Direct fp64 parity of the small training kernels: batch-norm backward and finalize, the DualCamNet pooling /
spatial-sum / clip cross-entropy ops, softplus and the latent heads, and the loss / norm reductions.

Reductions are fed dyadic data (multiples of a power of two, few mantissa bits).  When the sum of |term| / resolution
stays below 2^24 every partial sum is exact in fp32 whatever the summation order, so the kernel's result must equal the
fp64 reference bit for bit: a dropped row, a skipped tail, a doubled block or a wrong channel stride fails outright
instead of hiding inside a tolerance.  Each bound is asserted on the host.  One case per op uses ordinary randn data and
checks the non-reduction arithmetic at the module tolerance (2e-5 relative to max|ref|, looser only where stated).
"""
import functools

import pytest
import torch
import torch.nn.functional as F

import op_support
from op_support import (SENTINEL, assert_exact_sum, assert_f32, bits_equal, bn_bwd_dyadic_inputs, bn_bwd_ref, close_at, dev, dyadic,
                        exact, pads_untouched, rnd, widen)

pytestmark = pytest.mark.gpu

close = close_at(2e-5)           # tests/test_ops_gpu.py RTOL
rel_err = functools.partial(op_support.rel_err, floor=1e-12)


# ------------------------------------------------------------------------------------------------------------------
# acimg_bn_bwd
# ------------------------------------------------------------------------------------------------------------------
def run_bn_bwd(device, x, ldx, gy, ldgy, mean, invstd, gamma, scale, shift, rows, C, ldgx, inplace):
    from acimg import ops

    xd = widen(x, ldx, fill=float("nan")).to(device)          # pad columns are never read: NaN there would show up
    gyd = widen(gy, ldgy, fill=SENTINEL if inplace else float("nan")).to(device)
    gxd = gyd if inplace else torch.full((rows, ldgx), SENTINEL, device=device)
    dgamma = torch.full((C,), SENTINEL, device=device)
    dbeta = torch.full((C,), SENTINEL, device=device)
    plan = ops.Plan(device, eager=True)
    ops.bn_bwd(plan, xd, ldx, gyd, ldgy, dev(scale, device), dev(shift, device), dev(mean, device),
               dev(invstd, device), dev(gamma, device), rows, C, gxd, ldgx, dgamma, dbeta)
    torch.cuda.synchronize()
    return xd, gyd, gxd, dgamma, dbeta


# rows, C, ldx, ldgy, ldgx, in place.  blocks = min(256, ceil(rows / 256)); the finalize takes cw = 8 / 16 / 32
# channels per workgroup (C <= 8 / <= 16 / else) with ng = 32 / 16 / 8 partial-row groups; the reduce pass has
# 256 / (C / 4) row slots per sweep (C = 12, 20: 256 is not a multiple of C / 4, the last threads idle).
BN_BWD_CASES = [
    (37, 4, 4, 4, 4, False),                 # one block, tail loop only, cw = 8
    (37, 12, 16, 20, 24, False),             # idle row slots, every ld > C and distinct
    (37, 1020, 1024, 1028, 1032, False),     # c4n = 255: one row slot, one idle thread
    (257, 8, 8, 8, 8, False),                # 2 blocks
    (257, 20, 20, 20, 20, False),
    (2049, 16, 16, 16, 16, False),           # 9 blocks < ng = 16
    (2049, 12, 12, 12, 12, False),
    (4097, 16, 20, 24, 28, False),           # 17 blocks: ng < blocks < 2 ng
    (8193, 8, 8, 8, 8, False),               # 33 blocks > ng = 32: one two-in-flight trip, odd tail
    (8193, 20, 24, 28, 32, False),           # 33 blocks, ng = 8: two trips and the odd tail
    (8193, 128, 128, 128, 128, False),
    (8193, 1020, 1020, 1020, 1020, False),
    (65281, 32, 32, 32, 32, False),          # blocks capped at 256, one row in the last block
    (65281, 4, 4, 4, 4, False),
    (133504, 8, 8, 8, 8, False),             # U-Net first layer (2 x 224 x 298), ragged last block
    (133504, 64, 68, 72, 76, False),
    (133504, 32, 32, 36, 36, True),          # in place (gx is gy), ld > C, as unet_vae._cbr_back calls it
    (2049, 16, 16, 16, 16, True),
    (16384, 1024, 1024, 1024, 1024, False),  # c4n = 256
    (534016, 8, 8, 8, 8, False),             # production size: batch 8 x 224 x 298
    (534016, 32, 32, 32, 32, False),
]


@pytest.mark.parametrize("case", BN_BWD_CASES, ids=lambda c: "r%d_c%d_ld%d-%d-%d%s" % (
    c[0], c[1], c[2], c[3], c[4], "_inplace" if c[5] else ""))
def test_bn_bwd_dyadic(device, case):
    from acimg import ops

    rows, C, ldx, ldgy, ldgx, inplace = case
    g = torch.Generator().manual_seed(rows * 7 + C)
    x, gy, gm, xhat, mean, invstd, gamma, scale, shift = bn_bwd_dyadic_inputs(g, rows, C)
    gx_ref, dgamma_ref, dbeta_ref = bn_bwd_ref(xhat, gm, gamma, invstd)
    del gm, xhat
    xd, gyd, gxd, dgamma, dbeta = run_bn_bwd(device, x, ldx, gy, ldgy, mean, invstd, gamma, scale, shift, rows, C,
                                             ldgx, inplace)
    exact(dbeta, dbeta_ref, "dbeta")
    exact(dgamma, dgamma_ref, "dgamma")
    close(gxd[:, :C], gx_ref, what="gx")
    if ldgx > C:
        pads_untouched(gxd, C, "gx")
    if not inplace:
        # ordered partials, no atomics: a second call gives the same bits
        gx2 = torch.full_like(gxd, SENTINEL)
        dgamma2, dbeta2 = torch.empty_like(dgamma), torch.empty_like(dbeta)
        ops.bn_bwd(ops.Plan(device, eager=True), xd, ldx, gyd, ldgy, dev(scale, device), dev(shift, device),
                   dev(mean, device), dev(invstd, device), dev(gamma, device), rows, C, gx2, ldgx, dgamma2, dbeta2)
        torch.cuda.synchronize()
        bits_equal(gx2, gxd, "gx")
        bits_equal(dgamma2, dgamma, "dgamma")
        bits_equal(dbeta2, dbeta, "dbeta")


@pytest.mark.parametrize("rows,C", [(133504, 32), (20000, 128)])
def test_bn_bwd_float(device, rows, C):
    """randn activations with their own batch statistics: invstd / xhat / the apply arithmetic against fp64, and
    bit-identical repeats"""
    g = torch.Generator().manual_seed(rows + C)
    x = (rnd(g, rows, C) * 1.5 + rnd(g, C)).float().double()
    mean = x.mean(0).float().double()
    invstd = (1.0 / torch.sqrt(x.var(0, unbiased=False) + 1e-5)).float().double()
    gamma = (rnd(g, C).abs() + 0.5).float().double()
    beta = rnd(g, C).float().double()
    scale = (gamma * invstd).float().double()
    shift = (beta - mean * scale).float().double()
    pre = x * scale + shift
    gy = rnd(g, rows, C).float().double()
    # fp32 may round a pre-activation within ~1e-6 of 0 to the other side; no gradient there, so the mask cannot matter
    gy[pre.abs() < 1e-4] = 0.0
    gm = gy * (pre > 0)
    xhat = (x - mean) * invstd
    gx_ref, dgamma_ref, dbeta_ref = bn_bwd_ref(xhat, gm, gamma, invstd)
    ld = C + 4
    xd, gyd, gxd, dgamma, dbeta = run_bn_bwd(device, x, ld, gy, ld, mean, invstd, gamma, scale, shift, rows, C, ld,
                                             False)
    close(gxd[:, :C], gx_ref, what="gx")
    # fp32 sums of `rows` signed terms: cancellation leaves the result ~sqrt(rows) of sum |term|, so the fp32 rounding
    # of the partials is larger relative to the result (the stats sums of test_ops_gpu use 1e-4 for the same reason)
    close(dbeta, dbeta_ref, tol=1e-4, what="dbeta")
    close(dgamma, dgamma_ref, tol=1e-4, what="dgamma")
    print("bn_bwd float rows=%d C=%d: gx %.2e dbeta %.2e dgamma %.2e" % (
        rows, C, rel_err(gxd[:, :C], gx_ref), rel_err(dbeta, dbeta_ref), rel_err(dgamma, dgamma_ref)))
    from acimg import ops
    gx2 = torch.full_like(gxd, SENTINEL)
    dgamma2, dbeta2 = torch.empty_like(dgamma), torch.empty_like(dbeta)
    ops.bn_bwd(ops.Plan(device, eager=True), xd, ld, gyd, ld, dev(scale, device), dev(shift, device),
               dev(mean, device), dev(invstd, device), dev(gamma, device), rows, C, gx2, ld, dgamma2, dbeta2)
    torch.cuda.synchronize()
    bits_equal(gx2, gxd, "gx")
    bits_equal(dgamma2, dgamma, "dgamma")
    bits_equal(dbeta2, dbeta, "dbeta")


def test_bn_bwd_workspace_refused(device):
    """one byte less than acimg_bn_bwd_workspace is ACIMG_EWORKSPACE; the exact size is accepted"""
    from acimg import _lib, ops

    L = _lib.load()
    st = ops.current_stream_handle(device)
    for rows, C in ((37, 12), (133504, 32), (70000, 256)):
        need = int(L.acimg_bn_bwd_workspace(rows, C))
        x = torch.zeros(rows, C, device=device)
        gx = torch.zeros(rows, C, device=device)
        p = torch.zeros(C, device=device)
        dg, db = torch.zeros(C, device=device), torch.zeros(C, device=device)
        ws = torch.zeros(need, dtype=torch.uint8, device=device)
        args = (x.data_ptr(), C, x.data_ptr(), C, p.data_ptr(), p.data_ptr(), p.data_ptr(), p.data_ptr(), p.data_ptr(),
                rows, C, gx.data_ptr(), C, dg.data_ptr(), db.data_ptr(), ws.data_ptr())
        rc = L.acimg_bn_bwd(*args, need - 1, st)
        assert rc == -2 and "workspace" in _lib.last_error(), (rows, C, rc)
        assert L.acimg_bn_bwd(*args, need, st) == 0, _lib.last_error()
        torch.cuda.synchronize()
        del x, gx, ws


# ------------------------------------------------------------------------------------------------------------------
# acimg_bn_finalize
# ------------------------------------------------------------------------------------------------------------------
def finalize_ref(s1, s2, count, gamma, beta, mm, mv, decay, eps):
    m = s1 / count
    v = (s2 / count - m * m).clamp(min=0.0)
    invstd = 1.0 / torch.sqrt(v + eps)
    scale = gamma * invstd
    shift = beta - m * scale
    mm2 = decay * mm + (1 - decay) * m
    mv2 = decay * mv + (1 - decay) * v * (count / (count - 1.0))
    return m, invstd, scale, shift, mm2, mv2


def run_finalize(device, stats, rows, C, ld, count, gamma, beta, mm, mv, decay, eps, training):
    """outputs carry 4 sentinel floats past C: a write beyond the channel count shows up"""
    from acimg import ops

    def out():
        return torch.full((C + 4,), SENTINEL, device=device)

    scale, shift, smean, sinv = out(), out(), out(), out()
    mmd = torch.cat([mm.float(), torch.full((4,), SENTINEL, dtype=torch.float32)]).to(device)
    mvd = torch.cat([mv.float(), torch.full((4,), SENTINEL, dtype=torch.float32)]).to(device)
    ops.bn_finalize(ops.Plan(device, eager=True), stats, rows, C, ld, count, dev(gamma, device), dev(beta, device),
                    mmd, mvd, scale, shift, decay, eps, training, smean if training else None,
                    sinv if training else None)
    torch.cuda.synchronize()
    for t, name in ((scale, "scale"), (shift, "shift"), (smean, "save_mean"), (sinv, "save_invstd"),
                    (mmd, "moving_mean"), (mvd, "moving_var")):
        assert (t[C:] == SENTINEL).all(), "%s written past C" % name
    return scale[:C], shift[:C], smean[:C], sinv[:C], mmd[:C], mvd[:C]


# rows, C, ldstats: rows > 1024 and C <= 64 take the <8> template (8 channels per workgroup), the rest <32>
FINALIZE_CASES = [
    (2000, 12, 16),      # <8>, C not a multiple of 8
    (3001, 40, 44),      # <8>, 5 workgroups
    (1025, 64, 68),      # <8>, the smallest row count that takes it
    (1024, 64, 64),      # <32>: rows == 1024
    (300, 12, 16),       # <32>, C not a multiple of 32
    (517, 40, 48),       # <32>
    (2000, 100, 104),    # <32>: C > 64
    (7, 3, 4),           # fewer rows than row groups
]


@pytest.mark.parametrize("case", FINALIZE_CASES, ids=lambda c: "r%d_c%d_ld%d" % c)
def test_bn_finalize_dyadic(device, case):
    rows, C, ld = case
    g = torch.Generator().manual_seed(rows + 31 * C)
    # dyadic partial sums: s1 and s2 are exact in fp32 and fp64; per-channel offsets make the channels differ
    s1 = dyadic(g, (rows, C), 1 / 8, 4) + dyadic(g, (1, C), 1 / 8, 2)
    s2 = dyadic(g, (rows, C), 1 / 8, 8, lo=2)
    assert_exact_sum(s1, 1 / 8, "s1", dim=0)
    assert_exact_sum(s2, 1 / 8, "s2", dim=0)
    count = float(rows * 2)     # small count: the count / (count - 1) correction of the moving variance is visible
    stats = torch.full((rows, 2, ld), float("nan"), dtype=torch.float64)
    stats[:, 0, :C], stats[:, 1, :C] = s1, s2
    gamma, beta = rnd(g, C).abs() + 0.5, rnd(g, C)
    mm, mv = rnd(g, C), rnd(g, C).abs() + 0.1
    decay, eps = 0.25, 1e-3
    gamma, beta, mm, mv = [t.float().double() for t in (gamma, beta, mm, mv)]
    m, invstd, scale_r, shift_r, mm_r, mv_r = finalize_ref(s1.sum(0), s2.sum(0), count, gamma, beta, mm, mv, decay,
                                                           eps)
    scale, shift, smean, sinv, mmd, mvd = run_finalize(device, stats.float().to(device), rows, C, ld, count, gamma,
                                                       beta, mm, mv, decay, eps, True)
    # mean = (float)(s1 / count) from exact sums: the correctly rounded quotient
    exact(smean, m.float(), "save_mean")
    close(sinv, invstd, what="save_invstd")
    close(scale, scale_r, what="scale")
    close(shift, shift_r, what="shift")
    close(mmd, mm_r, what="moving_mean")
    close(mvd, mv_r, what="moving_var")

    # eval mode: no statistics, the moving averages are used and left as they are
    scale, shift, _, _, mm_e, mv_e = run_finalize(device, None, 0, C, ld, 0, gamma, beta, mm, mv, decay, eps, False)
    inv_e = 1.0 / torch.sqrt(mv + eps)
    close(scale, gamma * inv_e, what="eval scale")
    close(shift, beta - mm * gamma * inv_e, what="eval shift")
    exact(mm_e, mm, "eval moving_mean")
    exact(mv_e, mv, "eval moving_var")


@pytest.mark.parametrize("rows,C", [(2048, 32), (256, 96)])
def test_bn_finalize_offset_mean(device, rows, C):
    """realistic fp32 partials of data with |mean| / std ~ 4: var = E[x^2] - mean^2 cancels ~94 % of E[x^2]"""
    g = torch.Generator().manual_seed(rows + C)
    per = 64
    x = (4.0 * torch.where(rnd(g, C) > 0, 1.0, -1.0) + rnd(g, rows, per, C) * (0.8 + 0.4 * torch.rand(C, generator=g,
                                                                           dtype=torch.float64))).float()
    stats = torch.stack([x.sum(1), (x * x).sum(1)], 1)              # fp32 partials, as the conv epilogues leave them
    xd64 = x.double().reshape(-1, C)
    mean_r = xd64.mean(0)
    inv_r = 1.0 / torch.sqrt(xd64.var(0, unbiased=False) + 1e-5)
    ratio = (mean_r.abs() * inv_r).min().item()
    assert ratio > 3.0, ratio
    gamma, beta = torch.ones(C, dtype=torch.float64), torch.zeros(C, dtype=torch.float64)
    mm, mv = torch.zeros(C, dtype=torch.float64), torch.ones(C, dtype=torch.float64)
    _, _, smean, sinv, _, _ = run_finalize(device, stats.to(device), rows, C, C, float(rows * per), gamma, beta, mm,
                                           mv, 0.997, 1e-5, True)
    err = ((sinv.cpu().double() - inv_r).abs() / inv_r).max().item()
    print("bn_finalize |mean|/std >= %.1f, rows=%d C=%d: invstd rel err %.2e, mean rel err %.2e" % (
        ratio, rows, C, err, rel_err(smean, mean_r)))
    assert err <= 1e-4, "invstd rel err %.3e" % err
    close(smean, mean_r, what="mean")


# ------------------------------------------------------------------------------------------------------------------
# DualCamNet: VALID max pooling, spatial sum, clip softmax cross-entropy
# ------------------------------------------------------------------------------------------------------------------
def maxpool_ref(x, gy, k):
    """fp64 loop over the k*k window positions in row-major order: a later position takes over only when strictly
    greater, so the gradient goes to the FIRST maximum (tf.nn.max_pool's argmax), and only where x > 0"""
    N, H, W, C = x.shape
    OH, OW = H // k, W // k
    win = x[:, : OH * k, : OW * k].reshape(N, OH, k, OW, k, C)
    best = win[:, :, 0, :, 0].clone()
    arg = torch.zeros(N, OH, OW, C, dtype=torch.long)
    for r in range(k):
        for q in range(k):
            v = win[:, :, r, :, q]
            take = v > best
            best = torch.where(take, v, best)
            arg = torch.where(take, torch.full_like(arg, r * k + q), arg)
    gxw = torch.zeros(N, OH, k, OW, k, C, dtype=torch.float64)
    for r in range(k):
        for q in range(k):
            sel = (arg == r * k + q) & (win[:, :, r, :, q] > 0)
            gxw[:, :, r, :, q] = torch.where(sel, gy, torch.zeros_like(gy))
    gx = torch.zeros(N, H, W, C, dtype=torch.float64)      # the rows / columns VALID pooling drops get nothing
    gx[:, : OH * k, : OW * k] = gxw.reshape(N, OH * k, OW * k, C)
    return best, gx


# N, H, W, C, k, ldx, ldy (= ldgy), ldgx
MAXPOOL_CASES = [
    (2, 7, 9, 12, 2, 16, 20, 24),      # H, W odd: the last row and column are dropped
    (3, 11, 8, 32, 3, 36, 40, 44),     # 11 = 3*3 + 2, 8 = 3*2 + 2
    (2, 12, 15, 128, 3, 132, 136, 128),
    (1, 5, 5, 4, 2, 4, 4, 4),
]


@pytest.mark.parametrize("data", ["ties", "randn"])
@pytest.mark.parametrize("case", MAXPOOL_CASES, ids=lambda c: "n%d_%dx%d_c%d_k%d" % c[:5])
def test_maxpool(device, case, data):
    from acimg import ops

    N, H, W, C, k, ldx, ldy, ldgx = case
    OH, OW = H // k, W // k
    g = torch.Generator().manual_seed(H * W + C + k)
    if data == "ties":
        # post-ReLU values in {0, 1, 2}: many windows with repeated maxima, some all zero
        x = torch.randint(-2, 3, (N, H, W, C), generator=g).double().clamp(min=0)
    else:
        x = torch.relu(rnd(g, N, H, W, C)).float().double()
    gy = rnd(g, N, OH, OW, C).float().double()
    y_ref, gx_ref = maxpool_ref(x, gy, k)
    xd = widen(x, ldx, fill=float("nan")).to(device)
    yd = torch.full((N, OH, OW, ldy), SENTINEL, device=device)
    plan = ops.Plan(device, eager=True)
    ops.maxpool_fwd(plan, xd, ldx, yd, ldy, N, H, W, C, k)
    gyd = widen(gy, ldy, fill=float("nan")).to(device)
    gxd = torch.full((N, H, W, ldgx), SENTINEL, device=device)
    ops.maxpool_relu_bwd(plan, xd, ldx, gyd, ldy, gxd, ldgx, N, H, W, C, k)
    torch.cuda.synchronize()
    exact(yd[..., :C], y_ref, "maxpool fwd")
    exact(gxd[..., :C], gx_ref, "maxpool bwd")
    if ldy > C:
        pads_untouched(yd, C, "y")
    if ldgx > C:
        pads_untouched(gxd, C, "gx")
    assert (gxd[:, OH * k:, :, :C] == 0).all() and (gxd[:, :, OW * k:, :C] == 0).all(), "dropped rows got gradient"


# N, P, C, ldx: C = 128 is the model's width; 70 and 12 are not multiples of the 64-channel workgroup; P = 1 and 3
# leave some of the 4 row groups without rows
SPATIAL_CASES = [(3, 1, 128, 132), (2, 3, 70, 72), (2, 108, 12, 16), (4, 108, 128, 128), (2, 9, 70, 76)]


@pytest.mark.parametrize("case", SPATIAL_CASES, ids=lambda c: "n%d_p%d_c%d_ld%d" % c)
def test_spatial_sum(device, case):
    from acimg import ops

    N, P, C, ldx = case
    g = torch.Generator().manual_seed(N * P + C)
    x = dyadic(g, (N, P, C), 1 / 8, 4)
    assert_exact_sum(x, 1 / 8, "spatial sum", dim=1)
    gy = rnd(g, N, C).float().double()
    xd = widen(x, ldx, fill=float("nan")).to(device)
    y = torch.full((N, C + 4), SENTINEL, device=device)
    gxd = torch.full((N, P, ldx), SENTINEL, device=device)
    plan = ops.Plan(device, eager=True)
    ops.spatial_sum(plan, xd, ldx, y, N, P, C)
    torch.cuda.synchronize()
    # y is [N][C] densely: view the first N*C floats
    exact(y.view(-1)[: N * C].view(N, C), x.sum(1), "spatial_sum")
    assert (y.view(-1)[N * C:] == SENTINEL).all(), "spatial_sum wrote past N*C"
    ops.spatial_sum_relu_bwd(plan, xd, ldx, dev(gy, device), gxd, ldx, N, P, C)
    torch.cuda.synchronize()
    exact(gxd[..., :C], torch.where(x > 0, gy[:, None, :], torch.zeros_like(x)), "spatial_sum_relu_bwd")
    if ldx > C:
        pads_untouched(gxd, C, "gx")


def clip_ce_ref(logits, labels, F_):
    """fp64 F.cross_entropy of the frame-mean logits; its autograd gradient w.r.t. the per-frame logits"""
    lg = logits.clone().requires_grad_(True)
    clips = labels.shape[0]
    mean = lg.view(clips, F_, -1).mean(1)
    loss = F.cross_entropy(mean, labels)
    loss.backward()
    m = mean.detach()
    first_max = (m == m.max(1, keepdim=True).values).double().argmax(1)    # lowest index among exact ties
    return loss.detach(), float((first_max == labels).sum()), lg.grad


# clips, F, K
CLIP_CASES = [(5, 1, 1), (6, 12, 14), (4, 12, 63), (7, 1, 64), (5, 12, 64), (3, 1, 14)]


@pytest.mark.parametrize("data", ["dyadic", "randn"])
@pytest.mark.parametrize("case", CLIP_CASES, ids=lambda c: "clips%d_f%d_k%d" % c)
def test_clip_softmax_ce(device, case, data):
    from acimg import ops

    clips, F_, K = case
    g = torch.Generator().manual_seed(clips * 100 + F_ * 10 + K)
    if data == "dyadic":
        # logits up to +-80 (a missing max-subtraction overflows / underflows expf); multiples of 1/8 keep the frame
        # sums exact, so only the division by F rounds before the softmax
        base = dyadic(g, (clips, 1, K), 1 / 8, 76)
        logits = (base + dyadic(g, (clips, F_, K), 1 / 8, 4)).reshape(clips * F_, K)
    else:
        logits = (rnd(g, clips * F_, K) * 3).float().double()
    labels = torch.randint(0, K, (clips,), generator=g)
    if K > 1:
        lv = logits.view(clips, F_, K)
        top = lv.mean(1).argmax(1)
        # clip 0: an exact tie at the maximum, labelled with the lower index (counts as correct);
        # clip 1: the same tie labelled with the higher index (does not count); clip 2: a label that is not the max
        for n, lab_low in ((0, True), (1, False)):
            a = int(top[n])
            b = (a + 1 + int(torch.randint(0, K - 1, (1,), generator=g))) % K
            lo, hi = min(a, b), max(a, b)
            lv[n, :, b] = lv[n, :, a]
            labels[n] = lo if lab_low else hi
        labels[2] = (int(lv[2].mean(0).argmax()) + 1) % K
    ldl, ldg = K + 3, K + 5
    loss_r, acc_r, g_r = clip_ce_ref(logits, labels, F_)
    ld = widen(logits, ldl, fill=float("nan")).to(device)
    lab = labels.to(torch.int32).to(device)
    out = torch.zeros(2, device=device)
    gd = torch.full((clips * F_, ldg), SENTINEL, device=device)
    plan = ops.Plan(device, eager=True)
    ops.clip_softmax_ce(plan, ld, ldl, clips, F_, K, lab, out, gd, ldg)
    torch.cuda.synchronize()
    o1 = out.cpu().double().clone()
    close(o1[:1], loss_r.view(1), what="loss")
    assert o1[1].item() == acc_r, ("accuracy", o1[1].item(), acc_r)
    close(gd[:, :K], g_r, what="g_logits")
    pads_untouched(gd, K, "g_logits")
    print("clip_softmax_ce %s %s: loss %.2e g %.2e" % (case, data, rel_err(o1[:1], loss_r.view(1)),
                                                         rel_err(gd[:, :K], g_r)))
    # out accumulates; g_logits = None leaves the gradient alone
    gd_before = gd.clone()
    ops.clip_softmax_ce(plan, ld, ldl, clips, F_, K, lab, out, None, ldg)
    torch.cuda.synchronize()
    o2 = out.cpu().double()
    close(o2[:1], 2 * loss_r.view(1), what="loss, accumulated twice")
    assert o2[1].item() == 2 * acc_r
    assert torch.equal(gd, gd_before)


# ------------------------------------------------------------------------------------------------------------------
# softplus and the latent heads
# ------------------------------------------------------------------------------------------------------------------
def test_softplus(device):
    from acimg import ops

    g = torch.Generator().manual_seed(11)
    rows, C, ldx, ldy, ldg = 37, 50, 52, 56, 60
    edge = torch.tensor([-100.0, -89.0, -88.75, -88.5, -88.0, -87.5, -20.0, -1e-3, 0.0, 1e-3, 20.0, 87.5, 88.0,
                         88.5, 88.75, 89.0, 100.0], dtype=torch.float64)
    x = torch.cat([edge, torch.linspace(-100, 100, rows * C - 2 * edge.numel(), dtype=torch.float64), -edge])
    x = x[torch.randperm(x.numel(), generator=g)].reshape(rows, C).float().double()
    gy = rnd(g, rows, C).float().double()
    y_ref = F.softplus(x)
    gx_ref = gy * torch.sigmoid(x)
    xd = widen(x, ldx, fill=float("nan")).to(device)
    yd = torch.full((rows, ldy), SENTINEL, device=device)
    gxd = torch.full((rows, ldg), SENTINEL, device=device)
    plan = ops.Plan(device, eager=True)
    ops.softplus_fwd(plan, xd, ldx, yd, ldy, rows, C)
    ops.softplus_bwd(plan, xd, ldx, widen(gy, ldx, fill=float("nan")).to(device), ldx, gxd, ldg, rows, C)
    torch.cuda.synchronize()
    pads_untouched(yd, C, "y")
    pads_untouched(gxd, C, "gx")
    y = yd[:, :C].cpu().double()
    gx = gxd[:, :C].cpu().double()
    # tiny results are fp32 denormals or flushed to 0: the 1e-30 absolute term
    assert ((y - y_ref).abs() <= 2e-6 * y_ref.abs() + 1e-30).all(), "softplus: max err %.3e" % (
        ((y - y_ref).abs() / (y_ref.abs() + 1e-30)).max().item())
    assert torch.isfinite(gx).all()
    assert ((gx - gx_ref).abs() <= 2e-6 * gx_ref.abs() + 1e-30).all(), "softplus bwd"
    hi, lo = x >= 88.75, x <= -88.75
    assert hi.any() and lo.any()
    assert torch.equal(gx[hi], gy[hi]), "softplus bwd is not exactly gy for x >= 88.75"
    assert (gx[lo] == 0).all(), "softplus bwd is not exactly 0 for x <= -88.75"
    print("softplus: y %.2e gx %.2e" % (rel_err(y, y_ref), rel_err(gx, gx_ref)))


@pytest.mark.parametrize("Z", [150, 256, 300, 513])
def test_latent_linear(device, Z):
    """the U-Nets' linear sigma head: z = mu + s * eps, kl = 0.5 sum(mu^2 + s^2 - log(1e-8 + s^2) - 1), their fp64
    autograd gradient; s negative, exactly 0 and large"""
    from acimg import ops

    N, klw = 3, 0.5
    g = torch.Generator().manual_seed(Z)
    mu = rnd(g, N, Z)
    sg = rnd(g, N, Z)
    sg[:, ::7] = 0.0
    sg[:, 3::11] = 30.0 * torch.sign(sg[:, 3::11] + 0.5)
    sg[:, 5::13] = 0.1
    heads = torch.cat([mu, sg], 1).float().double().requires_grad_(True)
    eps = rnd(g, N, Z).float().double()
    gz = rnd(g, N, Z).float().double()
    m, s = heads[:, :Z], heads[:, Z:]
    z = m + s * eps
    kl = 0.5 * (m ** 2 + s ** 2 - torch.log(1e-8 + s ** 2) - 1).sum(1)
    ((z * gz).sum() + klw * kl.sum()).backward()
    ldz, ldgz = Z + 4, Z + 8
    hd, ed = dev(heads.detach(), device), dev(eps, device)
    zd = torch.full((N, ldz), SENTINEL, device=device)
    kld = torch.full((N + 1,), SENTINEL, device=device)
    gh = torch.full((N, 2 * Z), SENTINEL, device=device)
    plan = ops.Plan(device, eager=True)
    ops.latent_linear_fwd(plan, hd, ed, zd, ldz, kld, N, Z)
    ops.latent_linear_bwd(plan, hd, ed, widen(gz, ldgz, fill=float("nan")).to(device), ldgz, klw, gh, N, Z)
    torch.cuda.synchronize()
    close(zd[:, :Z], z, what="z")
    pads_untouched(zd, Z, "z")
    close(kld[:N], kl, what="kl")
    assert kld[N].item() == SENTINEL
    close(gh[:, :Z], heads.grad[:, :Z], what="g_mu")
    close(gh[:, Z:], heads.grad[:, Z:], what="g_sigma")
    print("latent_linear Z=%d: z %.2e kl %.2e g %.2e" % (Z, rel_err(zd[:, :Z], z), rel_err(kld[:N], kl),
                                                         rel_err(gh, heads.grad)))


@pytest.mark.parametrize("Z", [150, 300, 513])
def test_latent_softplus(device, Z):
    """the associators' softplus sigma head (acimg_latent_fwd / _bwd), raw sigma across [-20, 20] and exactly 0"""
    from acimg import ops

    N, klw = 3, 0.5
    g = torch.Generator().manual_seed(Z + 1)
    raw = rnd(g, N, Z) * 6
    raw[:, ::9] = 0.0
    raw[:, 4::17] = -20.0
    raw[:, 6::19] = 20.0
    heads = torch.cat([rnd(g, N, Z), raw], 1).float().double().requires_grad_(True)
    eps = rnd(g, N, Z).float().double()
    gz = rnd(g, N, Z).float().double()
    m, s = heads[:, :Z], F.softplus(heads[:, Z:])
    z = m + s * eps
    kl = 0.5 * (m ** 2 + s ** 2 - torch.log(1e-8 + s ** 2) - 1).sum(1)
    ((z * gz).sum() + klw * kl.sum()).backward()
    ldz = Z + 4
    hd, ed = dev(heads.detach(), device), dev(eps, device)
    zd = torch.full((N, ldz), SENTINEL, device=device)
    sd = torch.empty(N, Z, device=device)
    kld = torch.empty(N, device=device)
    gh = torch.empty(N, 2 * Z, device=device)
    plan = ops.Plan(device, eager=True)
    ops.latent_fwd(plan, hd, ed, zd, ldz, sd, kld, N, Z)
    ops.latent_bwd(plan, hd, ed, sd, widen(gz, ldz, fill=float("nan")).to(device), ldz, klw, gh, N, Z)
    torch.cuda.synchronize()
    close(sd, s, what="sigma")
    close(zd[:, :Z], z, what="z")
    pads_untouched(zd, Z, "z")
    close(kld, kl, what="kl")
    close(gh[:, :Z], heads.grad[:, :Z], what="g_mu")
    close(gh[:, Z:], heads.grad[:, Z:], what="g_sigma")
    print("latent softplus Z=%d: z %.2e kl %.2e g %.2e" % (Z, rel_err(zd[:, :Z], z), rel_err(kld, kl),
                                                           rel_err(gh, heads.grad)))


# ------------------------------------------------------------------------------------------------------------------
# loss and norm reductions
# ------------------------------------------------------------------------------------------------------------------
def recon_ref(yh, tgt, w_mse, w_huber):
    e = yh - tgt
    q = e.abs().clamp(max=1.0)
    mse_terms, hub_terms = e * e, 0.5 * q * q + (e.abs() - q)
    glogit = (w_mse * 2 * e + w_huber * e.clamp(-1.0, 1.0)) / yh.numel() * yh * (1 - yh)
    return mse_terms, hub_terms, glogit


def run_recon(device, yhd, tgd, count, w_mse, w_huber, with_grad=True):
    from acimg import ops

    sums = torch.zeros(2, device=device)
    gl = torch.full((count + 4,), SENTINEL, device=device) if with_grad else None
    ops.recon_loss(ops.Plan(device, eager=True), yhd, tgd, gl, sums, count, w_mse, w_huber)
    torch.cuda.synchronize()
    return sums, gl


def loss_tickets_zero(device):
    from acimg import ops

    assert (ops.loss_scratch(device)[:4] == 0).all(), "the recon_loss / sumsq hand-off ticket was left non-zero"


# 4k + 3 counts run the scalar tail; 327 683 reaches the 160-workgroup cap
@pytest.mark.parametrize("count", [1, 2, 3, 5, 4007, 327683])
def test_recon_loss_dyadic(device, count):
    g = torch.Generator().manual_seed(count)
    res = 1 / 16 if count < 10000 else 1 / 4
    yh = dyadic(g, (count,), res, 1 - res, lo=res)                  # sigmoid outputs in (0, 1)
    tgt = dyadic(g, (count,), res, 2.0, lo=-1.0)
    tgt[::5] = yh[::5] + 1.0                                        # |e| exactly 1 (both signs)
    tgt[1::5] = yh[1::5] - 1.0
    w_mse, w_huber = 0.75, 1.5
    mse_t, hub_t, gl_r = recon_ref(yh, tgt, w_mse, w_huber)
    assert_f32(tgt, "target")
    assert_exact_sum(mse_t, res * res, "mse")
    assert_exact_sum(hub_t, res * res / 2, "huber")
    yhd, tgd = dev(yh, device), dev(tgt, device)
    sums, gl = run_recon(device, yhd, tgd, count, w_mse, w_huber)
    exact(sums, torch.stack([mse_t.sum(), hub_t.sum()]), "recon sums")
    close(gl[:count], gl_r, what="g_logit")
    assert (gl[count:] == SENTINEL).all(), "g_logit written past count"
    sums2, _ = run_recon(device, yhd, tgd, count, w_mse, w_huber, with_grad=False)
    bits_equal(sums2, sums, "recon sums (g_logit = None)")
    loss_tickets_zero(device)


def test_recon_loss_float(device):
    """randn logits: the gradient arithmetic at the module tolerance, bit-identical repeats, and a sumsq call in
    between does not disturb the shared hand-off"""
    from acimg import ops

    count = 327683
    g = torch.Generator().manual_seed(3)
    yh = torch.sigmoid(rnd(g, count)).float().double()
    tgt = (torch.rand(count, generator=g, dtype=torch.float64) * 4 - 1.5).float().double()
    w_mse, w_huber = 0.75, 1.5
    mse_t, hub_t, gl_r = recon_ref(yh, tgt, w_mse, w_huber)
    yhd, tgd = dev(yh, device), dev(tgt, device)
    s1, gl = run_recon(device, yhd, tgd, count, w_mse, w_huber)
    close(s1, torch.stack([mse_t.sum(), hub_t.sum()]), what="recon sums")
    close(gl[:count], gl_r, what="g_logit")
    print("recon_loss float: sums %.2e g %.2e" % (rel_err(s1, torch.stack([mse_t.sum(), hub_t.sum()])),
                                                  rel_err(gl[:count], gl_r)))
    s2, gl2 = run_recon(device, yhd, tgd, count, w_mse, w_huber)
    bits_equal(s2, s1, "recon sums")
    bits_equal(gl2, gl, "g_logit")
    q = torch.zeros(1, device=device)
    ops.sumsq(ops.Plan(device, eager=True), tgd, count, q)
    s3, _ = run_recon(device, yhd, tgd, count, w_mse, w_huber)
    bits_equal(s3, s1, "recon sums after a sumsq")
    loss_tickets_zero(device)


@pytest.mark.parametrize("n", [1, 7, 1001, 2 * 1024 * 1024 + 3])
def test_sumsq(device, n):
    """n not a multiple of 4 (scalar tail); 2M + 3 reaches the 1024-workgroup cap.  sumsq accumulates into out"""
    from acimg import ops

    g = torch.Generator().manual_seed(n)
    res, mx = (1 / 4, 0.5) if n > 100000 else (1 / 8, 4.0)
    x = dyadic(g, (n,), res, mx)
    assert_exact_sum(x * x, res * res, "sumsq")
    out = torch.full((2,), 0.25, device=device)
    ops.sumsq(ops.Plan(device, eager=True), dev(x, device), n, out)
    torch.cuda.synchronize()
    exact(out, torch.tensor([0.25 + (x * x).sum().item(), 0.25]), "sumsq")
    loss_tickets_zero(device)
    if n > 100000:
        xf = rnd(g, n).float()
        xd = xf.to(device)
        o1, o2 = torch.zeros(1, device=device), torch.zeros(1, device=device)
        ops.sumsq(ops.Plan(device, eager=True), xd, n, o1)
        ops.sumsq(ops.Plan(device, eager=True), xd, n, o2)
        torch.cuda.synchronize()
        ref = (xf.double() ** 2).sum().view(1)
        close(o1, ref, what="sumsq randn")
        bits_equal(o2, o1, "sumsq randn")
        print("sumsq randn n=%d: %.2e" % (n, rel_err(o1, ref)))


@pytest.mark.parametrize("C", [1, 3, 12, 64])
@pytest.mark.parametrize("pixels", [5, 50001])
def test_sqerr_channels(device, C, pixels):
    """out[c] += sum_p (a - b)^2; C that do not divide 256, pixels * C below 256 and above the 512-workgroup cap"""
    from acimg import ops

    g = torch.Generator().manual_seed(C * 1000 + pixels)
    a = dyadic(g, (pixels, C), 1 / 8, 1)
    b = dyadic(g, (pixels, C), 1 / 8, 1)
    e2 = (a - b) ** 2
    assert_exact_sum(e2, 1 / 64, "sqerr", dim=0)
    base = dyadic(g, (C,), 1 / 8, 4)
    out = torch.cat([base, torch.full((4,), SENTINEL, dtype=torch.float64)]).float().to(device)
    ops.sqerr_channels(ops.Plan(device, eager=True), dev(a, device), dev(b, device), pixels, C, out)
    torch.cuda.synchronize()
    exact(out[:C], base + e2.sum(0), "sqerr_channels")
    assert (out[C:] == SENTINEL).all(), "sqerr_channels wrote past C"


@pytest.mark.parametrize("n", [1, 37, 63, 1000, 4099])
def test_absmax(device, n):
    """max |x| per row; rows whose largest magnitude is negative"""
    from acimg import ops

    rows = 6
    g = torch.Generator().manual_seed(n)
    x = dyadic(g, (rows, n), 1 / 8, 4)
    x[1::2, n // 2] = -5.0                   # odd rows: the largest magnitude is negative
    x[4] = rnd(g, n).float().double()          # one row of ordinary data
    out = torch.full((rows + 1,), SENTINEL, device=device)
    ops.absmax(ops.Plan(device, eager=True), dev(x, device), rows, n, out)
    torch.cuda.synchronize()
    exact(out[:rows], x.abs().max(1).values, "absmax")
    assert out[rows].item() == SENTINEL
