"""The caller owns every buffer (include/acimg.h): each entry point that takes a workspace is run through the raw C ABI
with EXACTLY the bytes its host-side query reports, poisoned with 0xFF (NaN), and with every output inside a guard arena
(tests/guard_arena.py) pre-filled with a sentinel.  An under-reporting query, a kernel that writes past its slabs or its
output extents, and a kernel that relies on scratch being zero all show up here; they do not behind `ops.Plan`, whose
workspace is the maximum over a test's ops, sits in allocator slack and is usually zero on a fresh process.

Per case (`run_case`):
  reference run  workspace 4 x query + 1 MiB, zeroed; plain output tensors; compared with the fp64 reference of the op at
                 the tolerance the existing test of that path uses (named next to each case);
  guarded run    workspace = the query, 0xFF (zero only where the header demands it: the first 4 KiB of the split3p
                 workspace, the loss scratch); rc == 0; documented elements bit-identical to the reference run; every other
                 byte of every output region still the sentinel; all guard bands intact; tickets / zero-on-exit words zero;
  short runs     ws_bytes = query - 16 (the last 16 bytes are canary), then ws = NULL: a negative code with every output
                 untouched, or rc == 0 with the reference run's result, bit for bit.  Only a case that declares a fallback
                 kernel (another summation order: the skinny forward, the loss sums' float atomics) may differ in bits; it
                 must then pass the reference run's own fp64 check.  Zero-on-exit words are zero after these calls too.
No case may fault: everything the library can reach lies inside memory the test owns."""
import ctypes as C
from collections import OrderedDict

import numpy as np
import pytest
import torch

from caller_memory_cases import DECONV_CASES, DGRAD_CASES, FWD_CASES, WGRAD_CASES
from caller_memory_support import (STATS_TOL, Case, Out, close, deconv_cases, dgrad_case, f32, first_lt, fwd_case, last_lt, run_case,
                                   wgrad_case)
from localize_ref import random_boxes
from op_support import raw_lib, tf_conv_ref, up4, widen
from retrieval_ref import int_features
from split_format_ref import brick_index, make_planes, plane_bytes, unsplit

pytestmark = pytest.mark.gpu


# =====================================================================================================================
# convolution family (the case builders: tests/caller_memory_support.py)
# =====================================================================================================================
@pytest.mark.parametrize("name", list(FWD_CASES))
def test_conv2d_fwd_caller_memory(device, name):
    run_case(device, fwd_case(device, name), "conv2d_fwd[%s]" % name)


@pytest.mark.parametrize("name", list(DGRAD_CASES))
def test_conv2d_dgrad_caller_memory(device, name):
    run_case(device, dgrad_case(device, name), "conv2d_dgrad[%s]" % name)


@pytest.mark.parametrize("name", list(WGRAD_CASES))
def test_conv2d_wgrad_caller_memory(device, name):
    run_case(device, wgrad_case(device, name), "conv2d_wgrad[%s]" % name)


@pytest.mark.parametrize("name", list(DECONV_CASES))
def test_deconv_caller_memory(device, name):
    fwd, dgr, wgr = deconv_cases(device, name)
    run_case(device, fwd, "deconv_fwd[%s]" % name)
    run_case(device, dgr, "deconv_dgrad[%s]" % name)
    run_case(device, wgr, "deconv_wgrad[%s]" % name)


# ---------------------------------------------------------------------------------------------------------------------
# non-default tuning: the sizing functions move with acimg_configure
# ---------------------------------------------------------------------------------------------------------------------
def test_queries_follow_the_tuning_record(device):
    """one forward / data-gradient shape and one weight-gradient shape under a tuning record that changes their split
    counts (split-K towards 96 workgroups instead of 768: 4 K ranges over 24 tiles instead of 9; 64 pixels per slab
    instead of 128: 19 slabs instead of 12): the queries must move with the launches"""
    from acimg import ops
    m, L = raw_lib()
    dflt = (int(L.acimg_conv2d_fwd_workspace(C.byref(ops.conv_desc(4, 12, 16, 128, 128, 3, 3, 1, "SAME")))),
            ops.conv2d_fwd_tiling(ops.conv_desc(4, 12, 16, 128, 128, 3, 3, 1, "SAME"))[2],
            int(L.acimg_conv2d_wgrad_workspace(C.byref(ops.conv_desc(8, 12, 16, 128, 144, 3, 3, 1, "SAME", ldw=148)))))
    try:
        m.configure(splitk_target=96, wgrad_minpix=64)
        d = ops.conv_desc(4, 12, 16, 128, 128, 3, 3, 1, "SAME")
        assert 1 < ops.conv2d_fwd_tiling(d)[2] < dflt[1] and int(L.acimg_conv2d_fwd_workspace(C.byref(d))) < dflt[0]
        assert int(L.acimg_conv2d_wgrad_workspace(C.byref(ops.conv_desc(8, 12, 16, 128, 144, 3, 3, 1, "SAME", ldw=148)))) > dflt[2]
        run_case(device, fwd_case(device, "splitk_handoff"), "conv2d_fwd[splitk_handoff, tuned]")
        run_case(device, dgrad_case(device, "s1_splitk_handoff"), "conv2d_dgrad[s1_splitk_handoff, tuned]")
        run_case(device, wgrad_case(device, "cols144_f32"), "conv2d_wgrad[cols144_f32, tuned]")
        run_case(device, wgrad_case(device, "cols144_split3"), "conv2d_wgrad[cols144_split3, tuned]")
    finally:
        m.configure()


# =====================================================================================================================
# pre-split planes: split3p / split1p / stats / tail / tail_proj with the tail-split workspace; gram_stats
# =====================================================================================================================
PRESPLIT_SHAPES = OrderedDict([("3x3_128_128", (8, 56, 75, 128, 128, 3, 3)), ("1x1_256_1024", (32, 28, 38, 256, 1024, 1, 1))])
# acimg_conv2d_fwd_split3_tiling under the default tuning record: (BM, BN, kernel: 0 one tile per workgroup, 1 persistent,
# 2 ring).  No query exposes whether the tail split engages for a shape: that it needs the workspace at all shows only in
# the poisoned / short runs below.
PRESPLIT_TILING = {"3x3_128_128": (128, 128, 0), "1x1_256_1024": (128, 128, 1)}


@pytest.mark.parametrize("entry", ["split3p", "split1p", "stats", "tail", "tail_proj"])
@pytest.mark.parametrize("shape", list(PRESPLIT_SHAPES))
def test_presplit_conv_caller_memory(device, shape, entry):
    """acimg_conv2d_fwd_split3p and its siblings with the DEDICATED tail-split workspace: first 4 KiB zero before and after,
    the rest poisoned.  Tolerances: 2e-6 against fp64 (test_presplit_activation_path, test_two_pass_conv3_equals_conv_then_
    bn_pass), 2e-4 statistics sums; split1p (operands keep 11 bits) against fp64 of the hi planes' values at the 2e-6 of
    test_fp16_operand_storage_conv"""
    from acimg import ops
    m, L = raw_lib()
    N, H, W, Cc, K, R, S = PRESPLIT_SHAPES[shape]
    g = torch.Generator().manual_seed(3 + Cc + K)
    x = torch.rand(N, H, W, Cc, generator=g)
    w = torch.randn(R, S, Cc, K, generator=g) * (2.0 / (R * S * Cc)) ** 0.5
    d = ops.conv_desc(N, H, W, Cc, K, R, S, 1, "SAME")
    rows = N * H * W
    st = ops.current_stream_handle(device)
    xp, lo_x = make_planes(ops.Plan(device, eager=True), device, x, rows, Cc, relu=1)
    wsplit = torch.zeros(ops.conv2d_split3_weight_bytes(d), dtype=torch.uint8, device=device)
    m.check(L.acimg_conv2d_split3_prepare(C.byref(d), w.to(device).data_ptr(), wsplit.data_ptr(), st), "prepare")
    torch.cuda.synchronize()
    q = ops.conv2d_fwd_split3p_workspace(d)
    til = tuple(ops.conv2d_fwd_split3_tiling(d))
    print("%s %s: tiling %s, workspace %d" % (entry, shape, til, q))
    assert til == PRESPLIT_TILING[shape], (shape, til)
    assert q >= 4096 + til[0] * til[1] * 4, q        # the ticket page and at least one fp32 tile to meet in
    xv = unsplit(xp, lo_x, rows, Cc).reshape(N, H, W, Cc)
    pads = (R // 2, R // 2, S // 2, S // 2)
    if entry == "split1p":
        n = plane_bytes(rows, Cc)
        idx = brick_index(rows, Cc)
        xv = (xp[:n].cpu().view(torch.float16)[idx].double() * 4.0).reshape(N, H, W, Cc)
        wv = (w * 1024.0).half().double() / 1024.0           # include/acimg.h: weights x 2^10 in fp16
    else:
        wv = w.double()
    ref = tf_conv_ref(xv, wv, 1, pads)
    flat = ref.reshape(rows, K)
    srows = ops.conv2d_fwd_split3p_stats_rows(d) if entry != "split1p" else ops.conv2d_fwd_split3_stats_rows(d)
    stats_out = Out(torch.float32, (srows + 3, 2, K), first_lt((srows + 3, 2, K), srows))

    def check_stats(o):
        close(o["stats"][:srows, 0].sum(0), flat.sum(0), tol=STATS_TOL, what="%s %s stats sum" % (entry, shape))
        close(o["stats"][:srows, 1].sum(0), (flat * flat).sum(0), tol=STATS_TOL, what="%s %s stats sumsq" % (entry, shape))

    if entry in ("split3p", "split1p"):
        fn = L.acimg_conv2d_fwd_split3p if entry == "split3p" else L.acimg_conv2d_fwd_split1p
        outs = OrderedDict(y=Out(torch.float32, (rows, K)), stats=stats_out)

        def call(ws, nb, p, tick):
            return fn(C.byref(d), xp.data_ptr(), lo_x, wsplit.data_ptr(), p["y"], p["stats"], ws, nb, st)

        def verify(o):
            close(o["y"], flat, tol=2e-6, what="%s %s" % (entry, shape))
            check_stats(o)
    elif entry == "stats":
        outs = OrderedDict(stats=stats_out)

        def call(ws, nb, p, tick):
            return L.acimg_conv2d_fwd_split3p_stats(C.byref(d), xp.data_ptr(), lo_x, wsplit.data_ptr(), p["stats"], ws, nb, st)
        verify = check_stats
    else:
        short = torch.rand(N, H, W, K, generator=g) * 2.0
        scale, shift = torch.rand(K, generator=g) + 0.5, torch.rand(K, generator=g) - 0.7
        sb, tb = torch.rand(K, generator=g) + 0.5, torch.rand(K, generator=g) - 0.5
        scd, shd, sbd, tbd = (t.to(device) for t in (scale, shift, sb, tb))
        lo_y = plane_bytes(rows, K)
        assert rows % 16 == 0                                # no pad rows: every byte of both planes is documented
        outs = OrderedDict(planes=Out(torch.uint8, (2 * lo_y,)))
        if entry == "tail":
            sp, _ = make_planes(ops.Plan(device, eager=True), device, short, rows, K, relu=1)
            shortcut = unsplit(sp, lo_y, rows, K)

            def call(ws, nb, p, tick):
                return L.acimg_conv2d_fwd_split3p_tail(C.byref(d), xp.data_ptr(), lo_x, wsplit.data_ptr(), scd.data_ptr(),
                                                       shd.data_ptr(), sp.data_ptr(), lo_y, p["planes"], lo_y, ws, nb, st)
        else:
            sc32 = (short - 1.0).to(device)
            shortcut = (short.double() - 1.0).reshape(rows, K) * sb.double() + tb.double()

            def call(ws, nb, p, tick):
                return L.acimg_conv2d_fwd_split3p_tail_proj(C.byref(d), xp.data_ptr(), lo_x, wsplit.data_ptr(), scd.data_ptr(),
                                                            shd.data_ptr(), sc32.data_ptr(), sbd.data_ptr(), tbd.data_ptr(),
                                                            p["planes"], lo_y, ws, nb, st)
        r64 = torch.relu(flat * scale.double() + shift.double() + shortcut)

        def verify(o):
            close(unsplit(o["planes"], lo_y, rows, K), r64, tol=2e-6, what="%s %s" % (entry, shape))
    run_case(device, Case(q, outs, call, verify, zero_head=4096, zero_exit=4096), "%s[%s]" % (entry, shape))


@pytest.mark.parametrize("shape", [(20011, 128, 512), (37, 64, 100), (4111, 384, 136)])
def test_gram_stats_caller_memory(device, shape):
    """acimg_gram_stats: scale / shift at 3e-6, moving averages at 2e-6 (test_gram_statistics_match_fp64); a short
    workspace is refused (tests/test_host_cpu.py::test_gram_stats_host_side: ACIMG_EINVAL)"""
    m, L = raw_lib()
    from acimg import ops
    rows, Cc, K = shape
    g = torch.Generator().manual_seed(11 + rows % 97 + Cc)
    x = torch.relu(torch.randn(rows, Cc, generator=g) + 0.3) * (0.5 + torch.rand(Cc, generator=g))
    ldw = up4(K)
    w = torch.zeros(Cc, ldw)
    w[:, :K] = torch.randn(Cc, K, generator=g) * (2.6 / Cc) ** 0.5
    gamma, beta = torch.rand(K, generator=g) + 0.5, torch.rand(K, generator=g) - 0.5
    mm0, mv0 = torch.randn(K, generator=g) * 0.1, torch.rand(K, generator=g) + 0.5
    xp, lo = make_planes(ops.Plan(device, eager=True), device, x, rows, Cc, relu=1)
    xv = unsplit(xp, lo, rows, Cc).double()
    y = xv @ w[:, :K].double()
    mean = y.mean(0)
    var = (y * y).mean(0) - mean * mean
    sc_ref = gamma.double() / torch.sqrt(var.float() + 1e-5).double()
    sh_ref = beta.double() - mean.float().double() * sc_ref
    unb = var * (rows / (rows - 1.0))
    wd, gd, bd = w.to(device), gamma.to(device), beta.to(device)
    q = int(L.acimg_gram_stats_workspace(rows, Cc))
    assert q > 0
    st = ops.current_stream_handle(device)
    outs = OrderedDict(scale=Out(torch.float32, (K + 4,), first_lt((K + 4,), K)), shift=Out(torch.float32, (K + 4,), first_lt((K + 4,), K)),
                       mm=Out(torch.float32, (K,), init=mm0), mv=Out(torch.float32, (K,), init=mv0))

    def call(ws, nb, p, tick):
        return L.acimg_gram_stats(xp.data_ptr(), lo, rows, Cc, wd.data_ptr(), ldw, K, gd.data_ptr(), bd.data_ptr(), p["mm"],
                                  p["mv"], 0.997, 1e-5, p["scale"], p["shift"], ws, nb, st)

    def verify(o):
        close(o["scale"][:K], sc_ref, tol=3e-6, what="gram scale %s" % (shape,))
        close(o["shift"][:K], sh_ref, tol=3e-6, what="gram shift %s" % (shape,))
        close(o["mm"], 0.997 * mm0.double() + 0.003 * mean, tol=2e-6, what="gram moving mean %s" % (shape,))
        close(o["mv"], 0.997 * mv0.double() + 0.003 * unb, tol=2e-6, what="gram moving variance %s" % (shape,))
    run_case(device, Case(q, outs, call, verify, short_code=-1), "gram_stats[%s]" % (shape,))


# =====================================================================================================================
# the other workspace takers, one multi-chunk shape each
# =====================================================================================================================
def test_minmax_caller_memory(device):
    """acimg_minmax_fwd / _bwd, 1728 pixels x 133 channels (32 chunks per sample), the output a slice at column 4 of a
    wider buffer: forward RTOL, mm exact, backward 1e-4 (test_minmax_float)"""
    m, L = raw_lib()
    from acimg import ops
    N, P, Cn, ldx, ldo, off = 2, 1728, 133, 136, 148, 4
    g = torch.Generator().manual_seed(P + Cn)
    x = f32(g, N, P, Cn).double().requires_grad_(True)
    a = x - x.amin(dim=(1, 2), keepdim=True)
    o = a / a.amax(dim=(1, 2), keepdim=True)
    go = f32(g, N, P, Cn).double()
    o.backward(go)
    q = int(L.acimg_minmax_workspace(N, P, Cn))
    assert q == N * 32 * 2 * 4
    st = ops.current_stream_handle(device)
    xd = widen(x.detach(), ldx).to(device)
    cols = torch.arange(ldo)
    omask = ((cols >= off) & (cols < off + Cn)).expand(N, P, ldo)
    outs = OrderedDict(out=Out(torch.float32, (N, P, ldo), omask), mm=Out(torch.float32, (N + 2, 4), first_lt((N + 2, 4), N)))

    def fwd(ws, nb, p, tick):
        return L.acimg_minmax_fwd(xd.data_ptr(), ldx, p["out"] + 4 * off, ldo, p["mm"], N, P, Cn, ws, nb, st)

    def verify(o_):
        close(o_["out"][..., off:off + Cn], o.detach(), what="minmax fwd")
        xm = x.detach()
        ref_mm = torch.stack([xm.amin((1, 2)), xm.amax((1, 2)), torch.ones(N, dtype=torch.float64), torch.ones(N, dtype=torch.float64)], 1)
        assert torch.equal(o_["mm"][:N].double(), ref_mm)
    ref = run_case(device, Case(q, outs, fwd, verify, short_code=-2), "minmax_fwd")
    mmd = ref["mm"][:N].contiguous().to(device)
    god = torch.full((N, P, ldo), float("nan"))
    god[..., off:off + Cn] = go.float()
    god = god.to(device)
    outs = OrderedDict(gx=Out(torch.float32, (N, P, ldx), last_lt((N, P, ldx), Cn)))

    def bwd(ws, nb, p, tick):
        return L.acimg_minmax_bwd(xd.data_ptr(), ldx, god.data_ptr() + 4 * off, ldo, mmd.data_ptr(), p["gx"], ldx, N, P, Cn, 0, 0,
                                  ws, nb, st)
    run_case(device, Case(q, outs, bwd, lambda o_: close(o_["gx"][..., :Cn], x.grad, tol=1e-4, what="minmax bwd"), short_code=-2),
             "minmax_bwd")


def test_bn_bwd_caller_memory(device):
    """acimg_bn_bwd at 2 x 224 x 298 rows x 32 channels (256 partial blocks): gx RTOL, dgamma / dbeta 1e-4
    (test_bn_bwd_float); short = ACIMG_EWORKSPACE (test_bn_bwd_workspace_refused)"""
    m, L = raw_lib()
    from acimg import ops
    rows, Cn, ld = 133504, 32, 36
    g = torch.Generator().manual_seed(rows + Cn)
    x = (f32(g, rows, Cn) * 1.5 + f32(g, Cn)).double()
    mean = x.mean(0).float().double()
    invstd = (1.0 / torch.sqrt(x.var(0, unbiased=False) + 1e-5)).float().double()
    gamma, beta = (f32(g, Cn).abs() + 0.5).double(), f32(g, Cn).double()
    scale = (gamma * invstd).float().double()
    shift = (beta - mean * scale).float().double()
    pre = x * scale + shift
    gy = f32(g, rows, Cn).double()
    gy[pre.abs() < 1e-4] = 0.0
    gm = gy * (pre > 0)
    xhat = (x - mean) * invstd
    dbeta, dgamma = gm.sum(0), (gm * xhat).sum(0)
    gx = gamma * invstd * (gm - dbeta / rows - xhat * (dgamma / rows))
    q = int(L.acimg_bn_bwd_workspace(rows, Cn))
    st = ops.current_stream_handle(device)
    xd, gyd = widen(x, ld).to(device), widen(gy, ld).to(device)
    pv = [t.float().to(device) for t in (scale, shift, mean, invstd, gamma)]
    outs = OrderedDict(gx=Out(torch.float32, (rows, ld), last_lt((rows, ld), Cn)), dgamma=Out(torch.float32, (Cn + 4,), first_lt((Cn + 4,), Cn)),
                       dbeta=Out(torch.float32, (Cn + 4,), first_lt((Cn + 4,), Cn)))

    def call(ws, nb, p, tick):
        return L.acimg_bn_bwd(xd.data_ptr(), ld, gyd.data_ptr(), ld, *[t.data_ptr() for t in pv], rows, Cn, p["gx"], ld,
                              p["dgamma"], p["dbeta"], ws, nb, st)

    def verify(o):
        close(o["gx"][:, :Cn], gx, what="bn_bwd gx")
        close(o["dbeta"][:Cn], dbeta, tol=1e-4, what="bn_bwd dbeta")
        close(o["dgamma"][:Cn], dgamma, tol=1e-4, what="bn_bwd dgamma")
    run_case(device, Case(q, outs, call, verify, short_code=-2), "bn_bwd")


@pytest.mark.parametrize("hard", [0, 1])
def test_triplet_caller_memory(device, hard):
    """acimg_triplet_loss_fwd + _bwd, B = 300 (several row blocks): the forward leaves the backward's state in the workspace,
    so it is poisoned before the forward only and both calls are guarded.  Tolerances of test_triplet_random: loss and
    fraction 1e-4, counts, gradients 1e-3"""
    m, L = raw_lib()
    from acimg import ops
    from oracle import triplet as ot
    B, D, ld = 300, 64, 68
    g = torch.Generator().manual_seed(100 + B)
    e0, e1 = f32(g, B, D, scale=0.05).double(), f32(g, B, D, scale=0.05).double()
    labels, scenario = torch.randint(0, 5, (B,), generator=g), torch.randint(0, 3, (B,), generator=g)
    a, b = e0.clone().requires_grad_(True), e1.clone().requires_grad_(True)
    loss, frac, npos, nvalid = (ot.mix_data_hard if hard else ot.mix_all)(a, b, labels, scenario, 0.2)
    ga, gb = torch.autograd.grad(loss, [a, b])
    q = ops.triplet_loss_workspace(B)
    st = ops.current_stream_handle(device)
    ad, bd = widen(e0, ld).to(device), widen(e1, ld).to(device)
    lab, sc = labels.int().to(device), scenario.int().to(device)
    outs = OrderedDict(out=Out(torch.float32, (8,), first_lt((8,), 4)), g0=Out(torch.float32, (B, ld), last_lt((B, ld), D)),
                       g1=Out(torch.float32, (B, ld), last_lt((B, ld), D)))

    def fwd(ws, nb, p, tick):
        return L.acimg_triplet_loss_fwd(ad.data_ptr(), ld, bd.data_ptr(), ld, lab.data_ptr(), sc.data_ptr(), B, D, 0.2, hard, ws, nb,
                                        p["out"], st)

    def bwd(ws, nb, p, tick):
        return L.acimg_triplet_loss_bwd(ad.data_ptr(), ld, bd.data_ptr(), ld, B, D, 0.5, ws, nb, p["g0"], ld, p["g1"], ld, 0, st)

    def rel(x, y):
        return float((x.double() - y).abs().max() / y.abs().max().clamp_min(1e-30))

    def verify(o):
        out = o["out"]
        assert float(out[3]) == float(nvalid)
        assert abs(float(out[2]) - float(npos)) <= max(2.0, 2e-5 * float(npos))
        assert abs(float(out[0]) - float(loss)) <= 1e-4 * abs(float(loss)) + 1e-7
        assert abs(float(out[1]) - float(frac)) <= 1e-4 * float(frac) + 1e-7
        assert rel(o["g0"][:, :D], 0.5 * ga) < 1e-3 and rel(o["g1"][:, :D], 0.5 * gb) < 1e-3
    run_case(device, Case(q, outs, [fwd, bwd], verify), "triplet[hard=%d]" % hard)


def test_filtfilt_caller_memory(device):
    """acimg_filtfilt, 150 rows (more than one workgroup) of 1024 float32 samples: bit-identical to SciPy
    (test_lowpass_filtfilt_matches_reference_golden)"""
    m, L = raw_lib()
    from acimg import ops
    from acimg.frontend import butter_lowpass, lfilter_zi
    from scipy import signal
    rows, n = 150, 1024
    rng = np.random.RandomState(9)
    x = (rng.randn(rows, n) * 500).astype(np.float32)
    b, a = butter_lowpass(125, 10)
    want = torch.from_numpy(np.float32(signal.filtfilt(b, a, x)))
    ba = torch.tensor(np.concatenate([b, a]), dtype=torch.float64, device=device)
    zi = torch.tensor(lfilter_zi(b, a), dtype=torch.float64, device=device)
    xd = torch.from_numpy(x).to(device)
    q = int(L.acimg_filtfilt_workspace(rows, n))
    st = ops.current_stream_handle(device)
    outs = OrderedDict(out=Out(torch.float32, (rows + 1, n), first_lt((rows + 1, n), rows)))
    run_case(device, Case(q, outs, lambda ws, nb, p, tick: L.acimg_filtfilt(xd.data_ptr(), 0, rows, n, ba.data_ptr(), zi.data_ptr(),
                                                                           p["out"], ws, nb, st),
                          lambda o: np.testing.assert_array_equal(o["out"][:rows].numpy(), want.numpy()), short_code=-2), "filtfilt")


def test_box_iou_caller_memory(device):
    """acimg_box_iou, 64 samples, all optional outputs: counts and mask exact, IoU to 1e-7 (tests/test_localize_gpu.py); a
    short workspace is ACIMG_EWORKSPACE, a NULL one a null argument (ACIMG_EINVAL), as tests/test_host_cpu.py pins them"""
    m, L = raw_lib()
    from acimg import ops
    import localize_ref as lref
    N = 64
    rng = np.random.RandomState(N)
    logen = (rng.rand(N, 36, 48) * rng.rand(N, 1, 1) * 3).astype(np.float32)
    boxes = random_boxes(rng, N)
    lg = torch.from_numpy(logen.reshape(N, 36 * 48)).to(device)
    bx = torch.from_numpy(np.ascontiguousarray(boxes, np.int32).reshape(N, 4, 3)).to(device)
    q = int(L.acimg_box_iou_workspace(N))
    st = ops.current_stream_handle(device)
    outs = OrderedDict(iou=Out(torch.float32, (N + 4,), first_lt((N + 4,), N)), counts=Out(torch.int32, (N + 2, 2), first_lt((N + 2, 2), N)),
                       mask=Out(torch.uint8, (N * 224 * 298 + 64,), first_lt((N * 224 * 298 + 64,), N * 224 * 298)))

    def verify(o):
        iou, counts = o["iou"].numpy(), o["counts"].numpy()
        mask = o["mask"][:N * 224 * 298].view(N, 224, 298).numpy()
        for n in range(N):
            num, den, want, m2 = lref.box_iou(logen[n], boxes[n])
            assert (counts[n, 0], counts[n, 1]) == (num, den), n
            assert np.array_equal(mask[n], m2.astype(np.uint8)), n
            if den == 0:
                assert np.isnan(iou[n]) and np.isnan(want), n
            else:
                assert abs(float(iou[n]) - want) <= 1e-7 * max(abs(want), 1e-30), (n, iou[n], want)
    run_case(device, Case(q, outs, lambda ws, nb, p, tick: L.acimg_box_iou(lg.data_ptr(), bx.data_ptr(), N, p["iou"], p["counts"], p["mask"],
                                                                          ws, nb, st), verify, short_code=-2, null_code=-1), "box_iou")


@pytest.mark.parametrize("Q,G,D,K", [(63, 50000, 12, 30), (63, 61, 150, 64)])
def test_knn_topk_caller_memory(device, Q, G, D, K):
    """acimg_knn_topk on integer-valued features (exact: tests/test_retrieval_gpu.py), the gallery cut into slabs that meet
    in the workspace, and a small gallery (K > G: -1 / +inf slots); include/acimg.h: short = ACIMG_EWORKSPACE"""
    m, L = raw_lib()
    from acimg import ops
    import retrieval_ref as rref
    rng = np.random.RandomState(Q * 7 + G + D + K)
    qf, gf = int_features(rng, Q, G, D)
    want_d, want_i = rref.kneighbors(qf, gf, K)
    qd, gd = widen(torch.from_numpy(qf), D + 3).double().to(device), widen(torch.from_numpy(gf), D + 5).double().to(device)
    qd[:, :D], gd[:, :D] = torch.from_numpy(qf).to(device), torch.from_numpy(gf).to(device)
    q = int(L.acimg_knn_topk_workspace(Q, G, D, K))
    st = ops.current_stream_handle(device)
    outs = OrderedDict(dist2=Out(torch.float64, (Q + 1, K), first_lt((Q + 1, K), Q)), idx=Out(torch.int32, (Q + 1, K), first_lt((Q + 1, K), Q)))

    def verify(o):
        assert np.array_equal(o["idx"][:Q].numpy(), want_i)
        assert np.array_equal(o["dist2"][:Q].numpy(), want_d)
    run_case(device, Case(q, outs, lambda ws, nb, p, tick: L.acimg_knn_topk(qd.data_ptr(), D + 3, Q, gd.data_ptr(), D + 5, G, D, K, p["dist2"],
                                                                           p["idx"], ws, nb, st), verify, short_code=-2),
             "knn_topk[%d,%d,%d,%d]" % (Q, G, D, K))


def test_loss_scratch_caller_memory(device):
    """acimg_recon_loss / acimg_sumsq with the dedicated scratch (zeroed once, as the header demands; its ticket back at
    zero after every call): 327 683 elements reach the workgroup cap.  RTOL (test_recon_loss_float, test_sumsq).  Without the
    scratch the header documents float atomics: the NULL run is compared at that tolerance instead of bit for bit."""
    m, L = raw_lib()
    from acimg import ops
    count = 327683
    g = torch.Generator().manual_seed(3)
    yh = torch.sigmoid(f32(g, count).double()).float().double()
    tgt = (torch.rand(count, generator=g, dtype=torch.float64) * 4 - 1.5).float().double()
    e = yh - tgt
    qq = e.abs().clamp(max=1.0)
    sums_ref = torch.stack([(e * e).sum(), (0.5 * qq * qq + (e.abs() - qq)).sum()])
    gl_ref = (0.75 * 2 * e + 1.5 * e.clamp(-1.0, 1.0)) / count * yh * (1 - yh)
    yhd, tgd = yh.float().to(device), tgt.float().to(device)
    q = int(L.acimg_loss_scratch_bytes())
    st = ops.current_stream_handle(device)
    zeros = torch.zeros(4)

    def verify_recon(o):
        close(o["sums"][:2], sums_ref, what="recon sums")
        close(o["g_logit"][:count], gl_ref, what="g_logit")
    run_case(device, Case(q, OrderedDict(g_logit=Out(torch.float32, (count + 5,), first_lt((count + 5,), count)),
                                         sums=Out(torch.float32, (4,), init=zeros)),
                          lambda ws, nb, p, tick: L.acimg_recon_loss(yhd.data_ptr(), tgd.data_ptr(), p["g_logit"], p["sums"], count, 0.75, 1.5,
                                                                     ws, nb, st),
                          verify_recon, zero_head=q, zero_exit=16, fallback=True), "recon_loss")
    run_case(device, Case(q, OrderedDict(out=Out(torch.float32, (4,), init=zeros)),
                          lambda ws, nb, p, tick: L.acimg_sumsq(tgd.data_ptr(), count, p["out"], ws, nb, st),
                          lambda o: close(o["out"][:1], (tgt * tgt).sum().view(1), what="sumsq"), zero_head=q, zero_exit=16, fallback=True), "sumsq")
