"""The tap-sharing bf16x3 weight gradient (csrc/wgrad_tap_kernel.hpp: 3x3 / stride 1 / SAME, >= 64 input channels, > 32
output columns, image rows of 32 or 48 pixels) against the fp64 autograd weight and bias gradient on the CPU, at the bound
test_split3_generator_convs holds the same arithmetic to: 3e-5 of the tensor's max, gy scaled by 1e-7.

The geometry is what can go wrong: row tiles of two image rows with a one-pixel halo (first / last row of an image, an odd
height's half-empty last tile), pixel splits that cross an image boundary, channel blocks of 32 with a ragged last block,
column blocks of 128 or 64 with ragged columns, leading dimensions wider than the tensors.  The form never uses more pixel
splits than there are row tiles, so no split is left without a tile; `test_more_splits_granted_than_tiles` is the shape where
that cap binds.  Shapes just outside the predicate must still match fp64 on the per-tap kernel."""
import ctypes as C
import functools

import pytest
import torch
import torch.nn.functional as F

import op_support
from op_support import up4, widen

pytestmark = pytest.mark.gpu

TOL = 3e-5             # tests/test_ops_gpu.py::test_split3_generator_convs: bf16x3 weight / bias gradient against fp64
GSCALE = 1e-7
close = functools.partial(op_support.close, show=True)


_REF = {}


def wgrad_reference(N, H, W, Cc, K):
    """x, gy (float32 values held as float64) and the fp64 autograd dW, db of the 3x3 SAME convolution; computed once"""
    key = (N, H, W, Cc, K)
    if key not in _REF:
        g = torch.Generator().manual_seed(N + H + W + Cc + K + 11)
        x = torch.randn(N, H, W, Cc, generator=g, dtype=torch.float64).float().double()
        gy = (torch.randn(N, H, W, K, generator=g, dtype=torch.float64) * GSCALE).float().double()
        w = torch.zeros(3, 3, Cc, K, dtype=torch.float64, requires_grad=True)
        b = torch.zeros(K, dtype=torch.float64, requires_grad=True)
        y = F.conv2d(x.permute(0, 3, 1, 2), w.permute(3, 2, 0, 1), b, padding=1).permute(0, 2, 3, 1)
        gw, gb = torch.autograd.grad(y, (w, b), gy)
        _REF[key] = (x, gy, gw, gb)
    return _REF[key]


def run_ops(device, case, ldx=None, gy_wide=False, with_db=True):
    from acimg import ops

    N, H, W, Cc, K = case
    x, gy, gw, gb = wgrad_reference(*case)
    kp = up4(K)
    d = ops.conv_desc(N, H, W, Cc, K, 3, 3, 1, "SAME", ldx=ldx)
    xd = (x.float() if ldx is None else widen(x, ldx)).contiguous().to(device)
    if gy_wide:                                    # gy is the upper half of a buffer twice as wide (a concat slice)
        ldg = 2 * kp
        gyd = ops.Ptr(widen(gy, ldg, off=kp).to(device), kp)
        if kp > K:
            gyd.t[..., kp + K:] = 0.0              # columns K .. kp of the slice are operands: zero
    else:
        ldg = kp
        gyd = widen(gy, kp, fill=0.0).to(device)
    dw = torch.full((3, 3, Cc, kp), 9.0, device=device)
    db = torch.full((kp,), 9.0, device=device) if with_db else None
    plan = ops.Plan(device, eager=True)
    ops.conv2d_wgrad_split3(plan, d, xd, gyd, ldg, dw, db)
    torch.cuda.synchronize()
    close(dw[..., :K], gw, TOL, "bf16x3 wgrad %s" % (case,))
    if with_db:
        close(db[:K], gb, TOL, "bf16x3 bgrad %s" % (case,))
    return dw, db


# production planes (batch 2: the pixel splits cross the image boundary), NB = 128 and NB = 64; gy as a channel slice
@pytest.mark.parametrize("case,gy_wide", [((2, 36, 48, 256, 128), False), ((2, 36, 48, 128, 64), True)])
def test_production_planes(device, case, gy_wide):
    run_ops(device, case, gy_wide=gy_wide)


def test_odd_height_without_bias(device):
    """1x5x48 64->64: the last row tile holds one image row; no bias gradient asked for"""
    run_ops(device, (1, 5, 48, 64, 64), with_db=False)


def test_more_splits_granted_than_tiles(device):
    """1x5x48 64->64 with 16 pixels per slab: 15 slabs granted, 3 row tiles -> 3 splits, every one with a tile"""
    from acimg import _lib as m

    try:
        m.configure(wgrad_minpix=16)
        run_ops(device, (1, 5, 48, 64, 64))
    finally:
        m.configure()


def test_width_32_ragged_channels_and_columns(device):
    """3x7x32 72->68: another width, a last channel block of 8 channels, 68 of 128 columns, x with ldx > C, gy a slice"""
    run_ops(device, (3, 7, 32, 72, 68), ldx=80, gy_wide=True)


# one step outside each bound of the predicate: rows of 64 and of 16 pixels, 32 input channels, 32 output columns.  These stay
# on the per-tap kernel and must match fp64 as before.
@pytest.mark.parametrize("case", [(2, 6, 64, 64, 64), (2, 12, 16, 64, 64), (2, 6, 48, 32, 64), (2, 6, 48, 64, 32)])
def test_outside_the_predicate(device, case):
    run_ops(device, case, gy_wide=True)


def test_caller_memory_replay_and_old_kernel(device):
    """2x36x48 128->64 through the C ABI: the workspace holds exactly the query's bytes, full of NaN; dw carries a sentinel
    tail and sentinel columns past the layer that must survive; two runs agree bit for bit (a replayed step is identical);
    the per-tap kernel (wgrad_halo = 0) agrees to 3e-5 of max."""
    from acimg import _lib as m
    from acimg import ops

    L = m.load()
    case = (2, 36, 48, 128, 64)
    N, H, W, Cc, K = case
    x, gy, gw, gb = wgrad_reference(*case)
    ldw, tail = K + 8, 1024
    d = ops.conv_desc(N, H, W, Cc, K, 3, 3, 1, "SAME", ldw=ldw)
    xd, gyd = x.float().to(device), gy.float().to(device)
    q = int(L.acimg_conv2d_wgrad_workspace(C.byref(d)))
    assert q > 0
    st = ops.current_stream_handle(device)
    SENT = 1.25e30

    def run():
        ws = torch.full((q,), 0xFF, dtype=torch.uint8, device=device)
        dwbuf = torch.full((9 * Cc * ldw + tail,), SENT, device=device)
        db = torch.full((ldw,), SENT, device=device)
        m.check(L.acimg_conv2d_wgrad_split3(C.byref(d), xd.data_ptr(), gyd.data_ptr(), K, dwbuf.data_ptr(), db.data_ptr(),
                                            ws.data_ptr(), q, st), "conv2d_wgrad_split3")
        torch.cuda.synchronize()
        return dwbuf, db

    dw1, db1 = run()
    dw2, db2 = run()
    assert torch.equal(dw1, dw2) and torch.equal(db1, db2)
    body = dw1[:9 * Cc * ldw].view(3, 3, Cc, ldw)
    assert (dw1[9 * Cc * ldw:] == SENT).all() and (body[..., K:] == SENT).all() and (db1[K:] == SENT).all()
    close(body[..., :K], gw, TOL, "bf16x3 wgrad (exact workspace)")
    close(db1[:K], gb, TOL, "bf16x3 bgrad (exact workspace)")
    try:
        m.configure(wgrad_halo=0)
        dw0, db0 = run()
    finally:
        m.configure()
    close(body[..., :K], dw0[:9 * Cc * ldw].view(3, 3, Cc, ldw)[..., :K], TOL, "tap form against the per-tap kernel")
    close(db1[:K], db0[:K], TOL, "tap form against the per-tap kernel, bias gradient")
