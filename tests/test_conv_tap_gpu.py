"""The tap-sharing split-operand convs (csrc/conv_tap_kernel.hpp: 3x3 / stride 1 / SAME, >= 64 reduction channels in chunks of
32, > 32 output columns, image rows of 32 or 48 pixels) through ops.conv2d_fwd_split3 / ops.conv2d_dgrad_split3
against the fp64 convolution on the CPU, at the bars test_split3_generator_convs holds the same arithmetic to: forward 2e-6 of
the tensor's max, data gradient 3e-5 with gy scaled by 1e-7.

The geometry is what can go wrong: row tiles of two image rows with a one-pixel halo whose rows above image 1 are image 0's
last rows in memory (an odd height's last tile holds one row), 32-channel chunks handed over through a register prefetch (an odd chunk count), column blocks of 128 or
64 with ragged columns, leading dimensions wider than the tensors, outputs that are slices of wider buffers.  x / gy live
inside NaN-filled buffers, so anything read from outside the tensor shows.  Shapes just outside the predicate must still match
on the per-tap kernel; the per-element bounds of tests/split_format_ref.py hold both forms over the stated operand range."""
import functools

import pytest
import torch

import conv_tap_cases as ct
import op_support
import split_format_ref as sf

pytestmark = pytest.mark.gpu

FWD_TOL, BWD_TOL = 2e-6, 3e-5      # tests/test_ops_gpu.py::test_split3_generator_convs
GSCALE = 1e-7
SENT = 1.25e30
GUARD = 4096                       # NaN floats in front of and behind x / gy
close = functools.partial(op_support.close, show=True)


@functools.lru_cache(maxsize=None)
def reference(N, H, W, Cc, K):
    """fp32 operands (held as fp64) and the fp64 results of the 3x3 SAME conv: pre-activation y and the data gradient of gy"""
    g = torch.Generator().manual_seed(N + H + W + Cc + K + 17)
    r = lambda *s: torch.randn(*s, generator=g).double()
    x, w, b = r(N, H, W, Cc), (r(3, 3, Cc, K) * (2.0 / (9 * Cc)) ** 0.5).float().double(), r(K)
    gy = (r(N, H, W, K) * GSCALE).float().double()
    res, mask = (r(N, H, W, Cc) * GSCALE).float().double(), r(N, H, W, Cc)
    sc = (r(Cc).abs() + 0.5).float().double()
    return dict(x=x, w=w, b=b, gy=gy, res=res, mask=mask, sc=sc, y=sf.conv_fwd(x, w) + b, dx=sf.conv_dgrad(gy, w))


def nan_guarded(t, ld, device):
    """[N, H, W, n] -> an ops.Ptr to the tensor with row pitch ld inside a NaN-filled buffer (NaN in the columns past n too)"""
    from acimg import ops

    rows, n = t.numel() // t.shape[-1], t.shape[-1]
    buf = torch.full((2 * GUARD + rows * ld,), float("nan"), dtype=torch.float32)
    buf[GUARD:GUARD + rows * ld].view(rows, ld)[:, :n] = t.reshape(rows, n).float()
    return ops.Ptr(buf.to(device), GUARD)


def prepared(device, d, w, dgrad=False):
    """-> (plan, the forward f16 image of w, or the flipped / transposed bf16 image of the data gradient)"""
    from acimg import ops

    plan = ops.Plan(device, eager=True)
    wd = w.float().contiguous().to(device)
    if dgrad:
        img = torch.zeros(ops.conv2d_split3_dgrad_weight_bytes(d), dtype=torch.uint8, device=device)
        ops.conv2d_split3_prepare_dgrad(plan, d, wd, img)
    else:
        img = torch.zeros(ops.conv2d_split3_weight_bytes(d), dtype=torch.uint8, device=device)
        ops.conv2d_split3_prepare(plan, d, wd, img)
    return plan, img


def run_fwd(device, case, ldx=None, affine=False, stats=False, check=True):
    """bias + ReLU into the upper half of a buffer twice as wide whose lower half holds a sentinel -> the output slice"""
    from acimg import ops

    N, H, W, Cc, K = case
    ref = reference(*case)
    ldx = ldx or Cc
    d = ops.conv_desc(N, H, W, Cc, K, 3, 3, 1, "SAME", ldx=ldx, ldy=2 * K, act=ops.ACT_RELU)
    plan, wf = prepared(device, d, ref["w"])
    ybuf = torch.full((N, H, W, 2 * K), SENT, device=device)
    kw = {}
    x = ref["x"]
    if affine:                    # relu(x * scale + 0) on load
        kw = dict(in_scale=ref["sc"].float().to(device), in_shift=torch.zeros(Cc, device=device), in_relu=1)
        x = torch.relu(ref["x"] * ref["sc"])
    if stats:
        kw["stats"] = torch.zeros(ops.conv2d_fwd_split3_stats_rows(d), 2, K, device=device)
    ops.conv2d_fwd_split3(plan, d, nan_guarded(ref["x"], ldx, device), wf, ops.Ptr(ybuf, K), bias=ref["b"].float().to(device), **kw)
    torch.cuda.synchronize()
    assert bool((ybuf[..., :K] == SENT).all()), "the lower half of the concat buffer was written"
    y = ybuf[..., K:]
    assert bool(torch.isfinite(y).all()), "forward %s: not finite" % (case,)
    if check:
        want = ref["y"] if not affine else sf.conv_fwd(x, ref["w"]) + ref["b"]
        close(y, torch.relu(want), FWD_TOL, "f16x3 fwd+bias+relu %s" % (case,))
    return y


def run_dgrad(device, case, ldg=None, fused=True, check=True):
    """dx into the first C columns of rows of C + 8 floats, the rest a sentinel; fused: residual + ReLU mask"""
    from acimg import ops

    N, H, W, Cc, K = case
    ref = reference(*case)
    ldg, lddx = ldg or K, Cc + 8
    d = ops.conv_desc(N, H, W, Cc, K, 3, 3, 1, "SAME")
    plan, wt = prepared(device, d, ref["w"], dgrad=True)
    dx = torch.full((N, H, W, lddx), SENT, device=device)
    args = (ref["res"].float().to(device), Cc, ref["mask"].float().to(device), Cc) if fused else ()
    ops.conv2d_dgrad_split3(plan, d, nan_guarded(ref["gy"], ldg, device), ldg, wt, dx, *args, lddx=lddx)
    torch.cuda.synchronize()
    assert bool((dx[..., Cc:] == SENT).all()), "columns past C of dx were written"
    got = dx[..., :Cc]
    assert bool(torch.isfinite(got).all()), "data gradient %s: not finite" % (case,)
    if check:
        want = (ref["dx"] + ref["res"]) * (ref["mask"] > 0) if fused else ref["dx"]
        close(got, want, BWD_TOL, "bf16x3 dgrad %s fused=%s" % (case, fused))
    return got


# production planes at batch 2 (the halo rows above image 1 are image 0's last rows in memory): NB = 128 and NB = 64
PLANES = [(2, 36, 48, 256, 128), (2, 36, 48, 128, 64), (2, 36, 48, 64, 64)]


@pytest.mark.parametrize("case", PLANES)
def test_production_planes_forward(device, case):
    run_fwd(device, case, ldx=case[3] + 8)


@pytest.mark.parametrize("fused", [True, False])
@pytest.mark.parametrize("case", PLANES)
def test_production_planes_dgrad(device, case, fused):
    """with residual + mask, and with neither (layer6/conv_1), lddx wider than C, gy with ldgy > K"""
    run_dgrad(device, case, ldg=case[4] + 4, fused=fused)


# chunk parity and ragged edges: width 32 with three chunks (an odd count exercises the prefetch's hand-over), a height the
# two-row tiles do not divide (the last tile holds one image row), 72 output columns / 72 dx columns; width 32 with ONE 64-column
# block, 40 of its columns live (conv_tap_kernel<SplitF16 / SplitBF16, 32, 64>: forward 96 -> 40, data gradient of 40 -> 96)
RAGGED = [(3, 7, 32, 96, 128), (1, 5, 48, 64, 64), (2, 4, 32, 96, 72), (2, 4, 48, 72 + 24, 72), (2, 4, 32, 72, 96),
          (2, 5, 32, 96, 40), (2, 5, 32, 40, 96)]


@pytest.mark.parametrize("case", RAGGED[:4] + [RAGGED[5]])
def test_ragged_forward(device, case):
    run_fwd(device, case, ldx=case[3] + 4)


@pytest.mark.parametrize("case", [RAGGED[0], RAGGED[1], RAGGED[4], RAGGED[6]])
def test_ragged_dgrad(device, case):
    """(2, 4, 32, 72->96): 72 columns of dx from three chunks of gy; (2, 5, 32, 40->96): 40 columns in one 64-column block"""
    run_dgrad(device, case, ldg=case[4] + 4)


# one step outside each bound of the predicate: rows of 64 and of 16 pixels, 32 reduction channels, 32 output columns.  These
# stay on the per-tap kernel and must match as before.
@pytest.mark.parametrize("case", [(2, 6, 64, 64, 64), (2, 12, 16, 64, 64), (2, 6, 48, 32, 64), (2, 6, 48, 64, 32)])
def test_outside_the_predicate(device, case):
    run_fwd(device, case, ldx=case[3] + 4)
    # for the data gradient the reduction runs over K and the columns are C: swap the two so the same bounds are stepped over
    N, H, W, Cc, K = case
    run_dgrad(device, (N, H, W, K, Cc), ldg=Cc + 4)


def test_in_scale_and_stats_stay_on_the_per_tap_kernel(device):
    """a call with an input affine and a call with statistics partials on a shape the predicate would otherwise take"""
    from acimg import ops

    case = (2, 6, 48, 64, 128)
    run_fwd(device, case, affine=True)
    run_fwd(device, case, stats=True)
    N, H, W, Cc, K = case
    ref = reference(*case)
    d = ops.conv_desc(N, H, W, Cc, K, 3, 3, 1, "SAME")
    plan, wf = prepared(device, d, ref["w"])
    y = torch.zeros(N, H, W, K, device=device)
    st = torch.zeros(ops.conv2d_fwd_split3_stats_rows(d), 2, K, device=device)
    ops.conv2d_fwd_split3(plan, d, ref["x"].float().to(device), wf, y, stats=st)
    torch.cuda.synchronize()
    flat = (ref["y"] - ref["b"]).reshape(-1, K)
    close(y, ref["y"] - ref["b"], FWD_TOL, "f16x3 fwd with statistics")
    close(st[:, 0].sum(0), flat.sum(0), 2e-4, "statistics sum")
    close(st[:, 1].sum(0), (flat * flat).sum(0), 2e-4, "statistics sum of squares")


def test_replay_and_old_kernel(device):
    """two runs agree bit for bit; the per-tap kernel (wgrad_halo = 0) agrees within the same bars"""
    from acimg import _lib as m

    case = (2, 36, 48, 128, 64)
    y1, y2 = run_fwd(device, case), run_fwd(device, case, check=False)
    d1, d2 = run_dgrad(device, case), run_dgrad(device, case, check=False)
    assert torch.equal(y1, y2) and torch.equal(d1, d2)
    try:
        m.configure(wgrad_halo=0)
        y0, d0 = run_fwd(device, case), run_dgrad(device, case)
    finally:
        m.configure()
    close(y1, y0, FWD_TOL, "tap form against the per-tap kernel, forward")
    close(d1, d0, BWD_TOL, "tap form against the per-tap kernel, data gradient")


# ---- per-element bounds over the stated operand range (tests/conv_tap_cases.py, tests/split_format_ref.py) -------------------
def tap_held(what, got, ref, bound):
    r = sf.max_ratio(got, ref, bound)
    print("RATIO %s | %.4f" % (what, r))
    assert r <= 1.0, "%s: %.4f of the bound" % (what, r)


@pytest.mark.parametrize("name", ct.FWD_SETS)
def test_forward_per_element_bound(device, name):
    from acimg import ops

    N, H, W, Cc, K = ct.BOUND_CASE
    o, ref, bound = ct.forward(name)
    d = ops.conv_desc(N, H, W, Cc, K, 3, 3, 1, "SAME")
    plan, wf = prepared(device, d, o.w)
    y = torch.full((N, H, W, K), float("nan"), device=device)
    ops.conv2d_fwd_split3(plan, d, o.x.to(device), wf, y)
    torch.cuda.synchronize()
    tap_held("conv tap f16x3 forward | " + name, y, ref, bound)


def test_dgrad_per_element_bound(device):
    from acimg import ops

    N, H, W, Cc, K = ct.BOUND_CASE
    o, ref, bound = ct.dgrad()
    d = ops.conv_desc(N, H, W, Cc, K, 3, 3, 1, "SAME")
    plan, wt = prepared(device, d, o.w, dgrad=True)
    dx = torch.full((N, H, W, Cc), float("nan"), device=device)
    ops.conv2d_dgrad_split3(plan, d, o.gy.to(device), K, wt, dx)
    torch.cuda.synchronize()
    tap_held("conv tap bf16x3 data gradient", dx, ref, bound)
