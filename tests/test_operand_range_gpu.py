"""The split-operand convolutions over the operand range include/acimg.h states, held to PER-ELEMENT bounds.

The other GPU tests feed these kernels unit-scale operands and divide the largest error by the largest magnitude of the whole
tensor; a batch norm follows every one of these convs and rescales each output channel on its own, so an error that is small
against the loudest channel can be large against a quiet one.  Here input and output channels differ by orders of magnitude
(tests/split_format_ref.py: `channels`, `quiet`, `loud`, `deferred`), the reference is fp64 on the CPU, and every output
element is held to the bound derived from the format in that module's docstring: |got - ref| <= bound elementwise, every
output finite; a failure reports the largest error / bound.  Each case prints its largest ratio ("RATIO ..." lines).

The same 16-bit split arithmetic runs behind the fp32 entry points from 65536 pixels on (acimg_conv2d_fwd / _dgrad / _wgrad on
the few-channel layers, acimg_deconv_* on the pointwise 32 -> 8 layer: sf.FP32_CASES); the second half of this file holds each
of those routes to the same bounds, asserts that the route was taken, and looks at the memory round every output."""
import ctypes as C
import functools

import pytest
import torch
import torch.nn.functional as F

import split_format_ref as sf
from op_support import trunk_forms
from split_format_ref import plane_bytes, unsplit

pytestmark = pytest.mark.gpu

U24 = sf.U24


def held(path, what, got, ref, bound, failures=None):
    """|got - ref| <= bound elementwise and everything finite; prints and returns the largest ratio"""
    got = got.detach().cpu().double()
    r = sf.max_ratio(got, ref, bound)
    print("RATIO %s | %s | %.4f" % (path, what, r))
    msg = None
    if not bool(torch.isfinite(got).all()):
        msg = "%s %s: %d outputs are not finite" % (path, what, int((~torch.isfinite(got)).sum()))
    elif not r <= 1.0:
        msg = "%s %s: largest error / bound = %.3f" % (path, what, r)
    if failures is None:
        assert msg is None, msg
    elif msg:
        failures.append(msg)
    return r


@functools.lru_cache(maxsize=None)
def forward_reference(case, name):
    """operands, fp64 conv and its bound [N,H,W,K] - computed once per operand set, shared, never written"""
    N, H, W, Cc, K, taps = sf.FWD_CASES[case][:6]
    o = sf.fwd_operands(case, name)
    ref = sf.conv_fwd(o.xa.double(), o.w.double())
    bound = sf.bound_f16x3(o.xa, o.w, sf.fwd_ksteps(taps, taps, Cc), prod=sf.conv_fwd)
    return o, ref, bound


def stats_held(path, what, stats, ref, bound, failures=None):
    """batch-norm partials [rows, 2, K] against each channel's OWN fp64 sums: the bound summed over the pixels (for the sum of
    squares: (y + e)^2 - y^2 = 2 y e + e^2 with |e| <= bound, and one fp32 rounding of each square)"""
    K = ref.shape[-1]
    flat, b = ref.reshape(-1, K), bound.reshape(-1, K)
    st = stats.detach().cpu().double()
    held(path, what + " stats sum", st[:, 0, :K].sum(0), flat.sum(0), b.sum(0), failures)
    held(path, what + " stats sumsq", st[:, 1, :K].sum(0), (flat * flat).sum(0),
         (2 * flat.abs() * b + b * b + U24 * flat * flat).sum(0), failures)


def split_weights(ops, plan, d, w, device):
    wsplit = torch.zeros(ops.conv2d_split3_weight_bytes(d), dtype=torch.uint8, device=device)
    ops.conv2d_split3_prepare(plan, d, w.to(device), wsplit)
    return wsplit


def on_the_fly(device, case, name, want_rows=None):
    from acimg import ops

    N, H, W, Cc, K, taps = sf.FWD_CASES[case][:6]
    o, ref, bound = forward_reference(case, name)
    d = ops.conv_desc(N, H, W, Cc, K, taps, taps, 1, "SAME")
    plan = ops.Plan(device, eager=True)
    wsplit = split_weights(ops, plan, d, o.w, device)
    rows = ops.conv2d_fwd_split3_stats_rows(d)
    if want_rows is not None:
        assert rows == want_rows
    y = torch.full((N, H, W, K), float("nan"), device=device)
    st = torch.full((rows, 2, K), float("nan"), device=device)
    kw = {}
    if o.in_scale is not None:
        kw = dict(in_scale=o.in_scale.to(device), in_shift=torch.zeros(Cc, device=device), in_relu=1)
    ops.conv2d_fwd_split3(plan, d, o.x.to(device), wsplit, y, stats=st, **kw)
    torch.cuda.synchronize()
    held("on-the-fly f16x3 " + case, name, y, ref, bound)
    stats_held("on-the-fly f16x3 " + case, name, st, ref, bound)


@pytest.mark.parametrize("name", sf.SETS)
@pytest.mark.parametrize("case", ["fly 1x1", "fly 3x3"])
def test_on_the_fly_f16x3_conv(device, case, name):
    """acimg_conv2d_fwd_split3, plain input and (`deferred`) with the consumer's own in_scale / in_relu; output and the
    statistics rows per channel.  `quiet` sits on the format's floor: the two absolute floor terms make up 97 % (1x1) / 95 %
    (3x3) of every element's bound (sf.floor_share) - below |x| = 2^-7 an activation keeps about 14 bits, the 2^-23 absolute
    floor of include/acimg.h, so a per-channel relative statement cannot be made for such a tensor"""
    on_the_fly(device, case, name)


def test_halo_form_f16x3_conv(device):
    """the halo form of acimg_conv2d_fwd_split3 (65536 pixels on, 32 -> 32 channels) on `channels`"""
    on_the_fly(device, "halo", "channels", want_rows=256)


@pytest.mark.parametrize("name", sf.SETS)
def test_halo_form_f16x3_conv_64_channels(device, name):
    """the 64 -> 32 instance of the halo form (launch_conv_halo16<SplitF16, 3, 64, 32, 0>: two 32-channel chunks per tap, 18 K
    steps) on every operand set, `deferred` with the consumer's own in_scale / in_relu; 149 x 147: tile rows and columns ragged"""
    on_the_fly(device, "halo 64", name, want_rows=256)


def test_few_channel_mfma_conv(device):
    """the few-channel MFMA form behind acimg_conv2d_fwd (8 -> 8 channels, taps along the GEMM's K axis) on `channels`"""
    from acimg import ops

    case = "few-channel"
    N, H, W, Cc, K, taps = sf.FWD_CASES[case][:6]
    o, ref, bound = forward_reference(case, "channels")
    d = ops.conv_desc(N, H, W, Cc, K, taps, taps, 1, "SAME")
    assert ops.conv2d_stats_rows(d) == 512                   # one statistics row per workgroup of the MFMA form
    plan = ops.Plan(device, eager=True)
    y = torch.full((N, H, W, K), float("nan"), device=device)
    ops.conv2d_fwd(plan, d, o.x.to(device), o.w.to(device), None, y)
    torch.cuda.synchronize()
    held("few-channel f16x3", "channels", y, ref, bound)


# the trunk's kernel forms as tests/test_split_planes_gpu.py forces them, and the kernel each must reach
# (acimg_conv2d_fwd_split3_tiling()[2]); 128x128 tiles also where the shipped rule would pick 64-row tiles (< 200 tiles)
TILE128 = dict(split3_tile_bm=128, split3_tile_bn=128)
TRUNK_FORMS = trunk_forms("one-tile", "persistent", "ring128", "halo")


def presplit_input(ops, plan, o, rows, Cc, device):
    """the activation planes of an operand set: `deferred` lets the producer carry the scale, so the split follows the affine"""
    lo = plane_bytes(rows, Cc)
    planes = torch.zeros(2 * lo, dtype=torch.uint8, device=device)
    if o.in_scale is not None:
        ops.bn_relu_split(plan, o.x.to(device), o.in_scale.to(device), torch.zeros(Cc, device=device), 1, planes, lo, rows, Cc)
    else:
        ops.bn_relu_split(plan, o.x.to(device), None, None, 0, planes, lo, rows, Cc)
    return planes, lo


@pytest.mark.parametrize("name", sf.SETS)
@pytest.mark.parametrize("case", ["presplit 1x1", "presplit 3x3"])
def test_presplit_trunk_conv(device, case, name):
    """acimg_bn_relu_split + acimg_conv2d_fwd_split3p in the trunk's kernel forms (one tile per workgroup, persistent, ring with
    128-row tiles, halo for 3x3), each with and without the tail workspace; output and statistics rows per channel"""
    from acimg import _lib, ops

    N, H, W, Cc, K, taps = sf.FWD_CASES[case][:6]
    o, ref, bound = forward_reference(case, name)
    d = ops.conv_desc(N, H, W, Cc, K, taps, taps, 1, "SAME")
    rows = N * H * W
    plan = ops.Plan(device, eager=True)
    planes, lo = presplit_input(ops, plan, o, rows, Cc, device)
    wsplit = split_weights(ops, plan, d, o.w, device)
    failures = []
    try:
        for form, cfg, kind in TRUNK_FORMS:
            if form == "halo" and taps != 3:
                continue
            _lib.configure(**dict(TILE128, **cfg))
            assert ops.conv2d_fwd_split3_tiling(d)[2] == kind, (form, ops.conv2d_fwd_split3_tiling(d))
            srows = ops.conv2d_fwd_split3p_stats_rows(d)
            for tail in (False, True):
                tws = torch.zeros(ops.conv2d_fwd_split3p_workspace(d), dtype=torch.uint8, device=device) if tail else None
                y = torch.full((N, H, W, K), float("nan"), device=device)
                st = torch.full((srows, 2, K), float("nan"), device=device)
                ops.conv2d_fwd_split3p(plan, d, planes, lo, wsplit, y, st, tail_ws=tws)
                torch.cuda.synchronize()
                what = "%s, %s%s" % (name, form, " + tail" if tail else "")
                held("pre-split f16x3 " + case, what, y, ref, bound, failures)
                stats_held("pre-split f16x3 " + case, what, st, ref, bound, failures)
    finally:
        _lib.configure()
    assert not failures, failures


@pytest.mark.parametrize("name", ["channels", "quiet", "loud"])
def test_two_pass_conv3(device, name):
    """acimg_conv2d_fwd_split3p_stats + _tail (identity shortcut from split planes) and _tail_proj (raw fp32 shortcut with its
    own affine): statistics per channel, and the output planes relu(conv * scale + shift + shortcut) with scale / shift /
    shortcut of per-channel magnitudes.  Bound: the conv's bound times |scale|; what the output planes can hold of the value
    (sf.plane_bound: 2^-23 of its binade, or the 2^-23 floor - NOT 2^-24 |v|, see that module); and 2^-24 of the magnitudes
    that meet in each of the epilogue's three fp32 roundings (the two fused multiply-adds and the add)."""
    from acimg import _lib, ops

    case = "presplit 1x1"
    N, H, W, Cc, K, taps = sf.FWD_CASES[case][:6]
    o, ref, bound = forward_reference(case, name)
    rows = N * H * W
    g = torch.Generator().manual_seed(301 + sf.SETS.index(name))
    # a batch norm's scale brings every channel to its own magnitude 2^[-8, 8] (the output is an activation: |v| < 2.6e5)
    mag = sf._pow2(g, K, -8, 8)
    peak = ref.reshape(rows, K).abs().amax(0).float()
    scale = (torch.rand(K, generator=g) + 0.5) * mag / sf.pow2_floor(peak).float()
    shift = (torch.rand(K, generator=g) - 0.5) * mag
    short = torch.relu(torch.randn(N, H, W, K, generator=g)) * mag
    sc32 = torch.randn(N, H, W, K, generator=g)
    sb, tb = (torch.rand(K, generator=g) + 0.5) * mag, (torch.rand(K, generator=g) - 0.5) * mag
    d = ops.conv_desc(N, H, W, Cc, K, 1, 1, 1, "SAME")
    plan = ops.Plan(device, eager=True)
    xp, lo_x = presplit_input(ops, plan, o, rows, Cc, device)
    lo_y = plane_bytes(rows, K)
    sp = torch.zeros(2 * lo_y, dtype=torch.uint8, device=device)
    ops.bn_relu_split(plan, short.to(device), None, None, 0, sp, lo_y, rows, K)
    wsplit = split_weights(ops, plan, d, o.w, device)
    tws = torch.zeros(ops.conv2d_fwd_split3p_workspace(d), dtype=torch.uint8, device=device)
    out_id = torch.zeros(2 * lo_y, dtype=torch.uint8, device=device)
    out_pj = torch.zeros(2 * lo_y, dtype=torch.uint8, device=device)
    D = lambda t: t.to(device)
    try:
        _lib.configure(**TILE128)            # the two passes take 128x128 tiles only (the shipped rule: from 200 tiles on)
        srows = ops.conv2d_fwd_split3p_stats_rows(d)
        st = torch.full((srows, 2, K), float("nan"), device=device)
        ops.conv2d_fwd_split3p_stats(plan, d, xp, lo_x, wsplit, st, tail_ws=tws)
        ops.conv2d_fwd_split3p_tail(plan, d, xp, lo_x, wsplit, D(scale), D(shift), sp, lo_y, out_id, lo_y, tail_ws=tws)
        ops.conv2d_fwd_split3p_tail_proj(plan, d, xp, lo_x, wsplit, D(scale), D(shift), D(sc32), D(sb), D(tb), out_pj, lo_y,
                                         tail_ws=tws)
        torch.cuda.synchronize()
    finally:
        _lib.configure()
    failures = []
    stats_held("two-pass f16x3", name, st, ref, bound, failures)
    s64, t64 = scale.double(), shift.double()
    held_short = unsplit(sp, lo_y, rows, K).reshape(N, H, W, K)          # the identity shortcut is what its planes hold
    proj_terms = [sc32.double() * sb.double(), tb.double().expand(N, H, W, K)]
    for what, planes, terms in (("identity tail", out_id, [held_short]), ("projection tail", out_pj, proj_terms)):
        pre = ref * s64 + t64 + sum(terms)
        mags = (ref * s64).abs() + t64.abs() + sum(t.abs() for t in terms)
        arith = bound * s64.abs() + 3 * U24 * mags
        b = arith + sf.plane_bound(pre.abs() + arith)
        got = unsplit(planes, lo_y, rows, K).reshape(N, H, W, K)
        held("two-pass f16x3", "%s, %s" % (name, what), got, torch.relu(pre), b, failures)
    assert not failures, failures


def producer_values(name, shape, seed, peak):
    """raw unit-scale values and a per-channel affine that puts channel c at magnitude 2^e_c, e_c from [-8, 6] (`loud`: three
    channels at 2^16 with the raw values clamped to +-peak); |shift| <= scale / 4"""
    g = torch.Generator().manual_seed(seed)
    Cc = shape[-1]
    raw = torch.randn(*shape, generator=g)
    mag = sf._pow2(g, Cc, -8, 6)
    if name == "loud":
        for c in sf.LOUD_CHANNELS:
            raw[..., c] = raw[..., c].clamp(-peak, peak)
            mag[c] = 65536.0
        raw[0, 0, 0, sf.LOUD_CHANNELS[0]] = peak
    scale = (torch.rand(Cc, generator=g) * 0.5 + 0.5) * mag
    shift = (torch.rand(Cc, generator=g) - 0.5) * 0.5 * mag
    return raw, mag, scale, shift


def planes_held(path, what, planes, lo, rows, Cc, v, arith, failures):
    """decoded planes against the fp64 value v: the producer's own fp32 roundings `arith`, then what the planes can hold"""
    got = unsplit(planes, lo, rows, Cc)
    held(path, what, got, v.reshape(rows, Cc), (arith + sf.plane_bound(v.abs() + arith)).reshape(rows, Cc), failures)


@pytest.mark.parametrize("name", ["channels", "loud"])
def test_split_plane_producers(device, name):
    """acimg_bn_relu_split (a power-of-two scale: exact in fp32, the planes alone; and a general scale / shift),
    acimg_bn_add_relu_split (projection shortcut with the fp32 copy; identity shortcut read back from planes at stride 2) and
    acimg_bn_relu_maxpool_split: every decoded element within sf.plane_bound of the fp64 value - 2^-23 of the value's binade
    or the 2^-23 floor - plus 2^-24 of the magnitudes that meet in each fp32 rounding of the producer's own arithmetic"""
    from acimg import ops

    plan = ops.Plan(device, eager=True)
    D = lambda t: t.to(device)
    failures = []
    path = "producers"
    N, OH, OW, Cc = 2, 7, 9, 64
    rows = N * OH * OW
    lo = plane_bytes(rows, Cc)
    new = lambda: torch.zeros(2 * lo, dtype=torch.uint8, device=device)
    # bn_relu_split
    a, mag, sa, ta = producer_values(name, (N, OH, OW, Cc), 401, 3.5)
    out = new()
    ops.bn_relu_split(plan, D(a), D(mag), D(torch.zeros(Cc)), 1, out, lo, rows, Cc)
    torch.cuda.synchronize()
    v = torch.relu(a.double() * mag.double())
    planes_held(path, name + ", bn_relu_split exact scale", out, lo, rows, Cc, v, torch.zeros_like(v), failures)
    out = new()
    ops.bn_relu_split(plan, D(a), D(sa), D(ta), 1, out, lo, rows, Cc)
    torch.cuda.synchronize()
    pre = a.double() * sa.double() + ta.double()
    arith = 2 * U24 * ((a.double() * sa.double()).abs() + ta.double().abs())
    planes_held(path, name + ", bn_relu_split", out, lo, rows, Cc, torch.relu(pre), arith, failures)
    # bn_add_relu_split, projection shortcut (raw fp32 + affine), planes + fp32 copy
    a, _, sa, ta = producer_values(name, (N, OH, OW, Cc), 402, 1.6)
    b, _, sb, tb = producer_values(name, (N, OH, OW, Cc), 403, 1.6)
    out = new()
    out32 = torch.full((N, OH, OW, Cc), float("nan"), device=device)
    ops.bn_add_relu_split(plan, D(a), D(sa), D(ta), D(b), D(sb), D(tb), None, 0, out, lo, out32, N, OH, OW, Cc, OH, OW, 1)
    torch.cuda.synchronize()
    ta64, tb64 = ta.double().expand_as(a), tb.double().expand_as(a)
    pa, pb = a.double() * sa.double(), b.double() * sb.double()
    v = torch.relu(pa + ta64 + pb + tb64)
    arith = 4 * U24 * (pa.abs() + ta64.abs() + pb.abs() + tb64.abs())
    held(path, name + ", bn_add_relu_split fp32 copy", out32, v, arith, failures)
    planes_held(path, name + ", bn_add_relu_split projection", out, lo, rows, Cc, v, arith, failures)
    # identity shortcut read back from split planes, stride 2
    BH, BW = 2 * OH - 1, 2 * OW
    praw, pmag, _, _ = producer_values(name, (N, BH, BW, Cc), 404, 1.6)
    prow = N * BH * BW
    plo = plane_bytes(prow, Cc)
    pplanes = torch.zeros(2 * plo, dtype=torch.uint8, device=device)
    ops.bn_relu_split(plan, D(praw), D(pmag), D(torch.zeros(Cc)), 1, pplanes, plo, prow, Cc)
    out = new()
    ops.bn_add_relu_split(plan, D(a), D(sa), D(ta), None, None, None, pplanes, plo, out, lo, None, N, OH, OW, Cc, BH, BW, 2)
    torch.cuda.synchronize()
    prev = unsplit(pplanes, plo, prow, Cc).reshape(N, BH, BW, Cc)[:, ::2, ::2]     # what the shortcut's planes hold
    v = torch.relu(pa + ta64 + prev)
    arith = 3 * U24 * (pa.abs() + ta64.abs() + prev.abs())
    planes_held(path, name + ", bn_add_relu_split identity", out, lo, rows, Cc, v, arith, failures)
    # bn_relu_maxpool_split: 3x3 / stride 2 / SAME, 13 x 17 -> 7 x 9
    H, W = 2 * OH - 1, 2 * OW - 1
    x, _, sc, sh = producer_values(name, (N, H, W, Cc), 405, 3.5)
    out = new()
    ops.bn_relu_maxpool_split(plan, D(x), D(sc), D(sh), out, lo, N, H, W, Cc, OH, OW, 1, 1)
    torch.cuda.synchronize()
    px = x.double() * sc.double()
    pool = lambda t: F.max_pool2d(F.pad(t.permute(0, 3, 1, 2), (1, 1, 1, 1), value=-1e30), 3, 2).permute(0, 2, 3, 1)
    v = pool(torch.relu(px + sh.double()))
    assert v.shape == (N, OH, OW, Cc)
    arith = pool(2 * U24 * (px.abs() + sh.double().abs().expand_as(px)))
    planes_held(path, name + ", bn_relu_maxpool_split", out, lo, rows, Cc, v, arith, failures)
    assert not failures, failures


def test_gram_statistics_per_channel(device):
    """acimg_gram_stats on `channels`-like operands (input channel c at 2^e_c, output channel k's weights at 2^f_k), the
    smallest shape of test_gram_statistics_match_fp64: the resulting batch-norm scale and shift against fp64 statistics of
    y = x w over the values the planes hold, PER CHANNEL at that test's tolerance 3e-6 - the scale against its own
    magnitude, the shift beta - mean * scale against the magnitudes of its two terms (the tensor-wide form of that test divides
    by the largest channel's scale, 2^13 times a quiet channel's here)"""
    from acimg import ops

    rows, Cc, K = 37, 64, 100
    g = torch.Generator().manual_seed(501)
    x = torch.relu(torch.randn(rows, Cc, generator=g) + 0.3) * sf._pow2(g, Cc, -8, 6)
    ldw = -(-K // 4) * 4
    w = torch.zeros(Cc, ldw)
    w[:, :K] = torch.randn(Cc, K, generator=g) * (2.6 / Cc) ** 0.5 * sf._pow2(g, K, -10, 3)
    gamma, beta = torch.rand(K, generator=g) + 0.5, torch.rand(K, generator=g) - 0.5
    mm, mv = (torch.randn(K, generator=g) * 0.1).to(device), (torch.rand(K, generator=g) + 0.5).to(device)
    lo = plane_bytes(rows, Cc)
    plan = ops.Plan(device, eager=True)
    xp = torch.zeros(2 * lo, dtype=torch.uint8, device=device)
    ops.bn_relu_split(plan, x.to(device), None, None, 0, xp, lo, rows, Cc)
    ws = torch.zeros(ops.gram_stats_workspace(rows, Cc), dtype=torch.uint8, device=device)
    sc = torch.full((K,), float("nan"), device=device)
    sh = torch.full((K,), float("nan"), device=device)
    ops.gram_stats(plan, xp, lo, rows, Cc, w.to(device), ldw, K, gamma.to(device), beta.to(device), mm, mv, sc, sh, ws,
                   decay=0.997, eps=1e-5)
    torch.cuda.synchronize()
    y = unsplit(xp, lo, rows, Cc).double() @ w[:, :K].double()
    mean = y.mean(0)
    var = (y * y).mean(0) - mean * mean
    sc_ref = gamma.double() / torch.sqrt(var + 1e-5)
    sh_ref = beta.double() - mean * sc_ref
    tol = 3e-6
    held("gram_stats", "channels, scale", sc, sc_ref, tol * sc_ref.abs())
    held("gram_stats", "channels, shift", sh, sh_ref, tol * (beta.double().abs() + (mean * sc_ref).abs()))


def wgrad_slabs(ops, d):
    """the most K ranges (pixel slabs) the weight gradient of `d` adds up: what its workspace is sized for, at most 2048"""
    from acimg import _lib

    nbytes = int(_lib.load().acimg_conv2d_wgrad_workspace(C.byref(d)))
    return max(1, min(2048, nbytes // ((d.R * d.S * d.C + 1) * d.ldw * 4) - 1))


@pytest.mark.parametrize("case", list(sf.BWD_CASES))
def test_bf16x3_backward_convs(device, case):
    """acimg_conv2d_dgrad_split3 and acimg_conv2d_wgrad_split3 on the tap, per-tap and halo kernels: x and w as `channels`, the
    output gradient's channel k at 2^g_k, g_k from [-30, -10]; dx, dw and db against sf.bound_bf16x3 (weight gradient: a
    K step is 32 pixels, a range is one pixel slab: sf.wgrad_counts)"""
    from acimg import ops

    N, H, W, Cc, K, taps = sf.BWD_CASES[case][:6]
    o = sf.bwd_operands(case)
    x, w, gy = o.x.double(), o.w.double(), o.gy.double()
    d = ops.conv_desc(N, H, W, Cc, K, taps, taps, 1, "SAME")
    plan = ops.Plan(device, eager=True)
    wt = torch.zeros(ops.conv2d_split3_dgrad_weight_bytes(d), dtype=torch.uint8, device=device)
    ops.conv2d_split3_prepare_dgrad(plan, d, o.w.to(device), wt)
    dx = torch.full((N, H, W, Cc), float("nan"), device=device)
    ops.conv2d_dgrad_split3(plan, d, o.gy.to(device), K, wt, dx)
    dw = torch.full((taps, taps, Cc, K), float("nan"), device=device)
    db = torch.full((K,), float("nan"), device=device)
    ops.conv2d_wgrad_split3(plan, d, o.x.to(device), o.gy.to(device), K, dw, db)
    torch.cuda.synchronize()
    failures = []
    path = "bf16x3 backward " + case
    fmt = sf.bwd_fmt(case)
    held(path, "dx", dx, sf.conv_dgrad(gy, w),
         sf.bound_bf16x3(o.gy, o.w, sf.fwd_ksteps(taps, taps, K), prod=sf.conv_dgrad, fmt=fmt), failures)
    wg = sf.conv_wgrad(taps)
    ksteps, slabs = sf.wgrad_counts(case, wgrad_slabs(ops, d))
    print("wgrad %s: %d K steps, %d slabs" % (case, ksteps, slabs))
    held(path, "dw", dw, wg(x, gy), sf.bound_bf16x3(o.x, o.gy, ksteps, ranges=slabs, prod=wg, fmt=fmt), failures)
    colsum = lambda a, b: (a * b).sum((0, 1, 2))
    held(path, "db", db, gy.sum((0, 1, 2)),
         sf.bound_bf16x3(torch.ones_like(o.gy), o.gy, ksteps, ranges=slabs, prod=colsum, fmt=fmt), failures)
    assert not failures, failures


# =====================================================================================================================
# the split-operand routes behind the fp32 entry points (sf.FP32_CASES)
# =====================================================================================================================
SENT = -7777.0            # pad channels, pad columns and the memory past the last pixel are pre-filled with it
TAIL = 64                 # floats past the last pixel
WS_BYTE = 0xA5            # ... and the plan's workspace with this byte, where its footprint tells the route
FEW_FWD = [(c, n) for c, n in sf.FP32_FWD if sf.FP32_CASES[c][5] == "few"]
FEW_BWD = [c for c in sf.FP32_BWD if sf.FP32_CASES[c][5] != "point"]
FEW_WGRAD = [c for c in sf.FP32_WGRAD if sf.FP32_CASES[c][5] == "few"]
FEW = sf.BF16_FMT_FEW


def guarded(device, shape, ld):
    """an output [..., ld] filled with the sentinel (the part to be written: NaN by the caller), TAIL floats more behind it"""
    n = 1
    for v in shape:
        n *= v
    flat = torch.full((n * ld + TAIL,), SENT, device=device)
    return flat, flat[:n * ld].view(*shape, ld)


def untouched(what, flat, view, lo, hi):
    """channels [lo, hi) of every pixel and the tail still hold the sentinel"""
    assert bool((view[..., lo:hi] == SENT).all()), what + ": pad channels written"
    assert bool((flat[-TAIL:] == SENT).all()), what + ": memory past the last pixel written"


def poisoned_workspace(plan, nbytes):
    plan.ws.require(nbytes)
    plan.ws.allocate()
    plan.ws.buf.fill_(WS_BYTE)
    return plan.ws.buf


@functools.lru_cache(maxsize=None)
def fp32_forward_reference(case, name):
    """operands, fp64 product (no bias) and its bound - computed once per operand set, shared, never written"""
    prod, ksteps = sf.fp32_products(case)["fwd"]
    o = sf.fp32_operands(case, name)
    return o, prod(o.xa.double(), o.w.double()), sf.bound_f16x3(o.xa, o.w, ksteps, prod=prod)


@functools.lru_cache(maxsize=None)
def fp32_grad_reference(case):
    """backward operands, fp64 data gradient and its bound"""
    prod, ksteps = sf.fp32_products(case)["dgrad"]
    o = sf.fp32_grad_operands(case)
    return o, prod(o.gy.double(), o.w.double()), sf.bound_bf16x3(o.gy, o.w, ksteps, prod=prod, fmt=FEW)


@functools.lru_cache(maxsize=None)
def fp32_wgrad_reference(case, impulse):
    """weight-gradient operands (dense: the backward operands; or the `impulse` set), fp64 dw with its bound, fp64 db"""
    wg = sf.fp32_products(case)["wgrad"]
    if impulse:
        o = sf.impulse_operands(case)
        counts = (o.npix, 0)
    else:
        o, counts = fp32_grad_reference(case)[0], sf.fp32_wgrad_counts(case)
    bound = sf.bound_bf16x3(o.x, o.gy, counts[0], ranges=counts[1], prod=wg, fmt=FEW)
    return o, wg(o.x.double(), o.gy.double()), bound, o.gy.double().sum((0, 1, 2)), counts


@pytest.mark.parametrize("case,name", FEW_FWD)
def test_few_channel_forward_route(device, case, name):
    """acimg_conv2d_fwd on conv_few16_kernel MODE 0 (f16x3; 8 -> 8, 4 -> 8 in the 8-channel image, 16 -> 16, 8 -> 32) over every
    operand set - `loud` at the ends of the stated range, `deferred` with the affine the route takes
    (acimg_conv2d_affine_input_ok) - into a wider pixel stride: every element within its bound, the statistics rows per
    channel, pad channels and the memory past the last pixel untouched.  Route: one statistics row per workgroup, 512."""
    from acimg import ops

    N, H, W, Cc, K = sf.FP32_CASES[case][:5]
    o, ref, bound = fp32_forward_reference(case, name)
    d = ops.conv_desc(N, H, W, Cc, K, 3, 3, 1, "SAME", ldy=K + 4)
    assert ops.conv2d_stats_rows(d) == 512
    kw = {}
    if o.in_scale is not None:
        assert ops.conv2d_affine_input_ok(d, 0)
        kw = dict(in_scale=o.in_scale.to(device), in_shift=torch.zeros(Cc, device=device), in_relu=1)
    plan = ops.Plan(device, eager=True)
    flat, y = guarded(device, (N, H, W), K + 4)
    y[..., :K] = float("nan")
    st = torch.full((512, 2, K), float("nan"), device=device)
    ops.conv2d_fwd(plan, d, o.x.to(device), o.w.to(device), None, y, stats=st, **kw)
    torch.cuda.synchronize()
    failures = []
    held("fp32 entry, " + case + " fwd", name, y[..., :K], ref, bound, failures)
    stats_held("fp32 entry, " + case + " fwd", name, st, ref, bound, failures)
    untouched(case + " fwd", flat, y, K, K + 4)
    assert not failures, failures


@pytest.mark.parametrize("case", FEW_BWD)
def test_few_channel_data_gradient_routes(device, case):
    """acimg_conv2d_dgrad on conv_few16_kernel MODE 1 (bf16x3): stride 1, and stride 2 over the zero-inserted view of gy with
    leading pads 0 (even sizes) and 1 (odd); the 8 -> 32 layer on the 16-row halo instance; the 32 -> 8 layer on the few-channel
    kernel's 32-row instance (conv_few16_kernel<SplitBF16, 8, 32, 1, 8>: 8 gy channels into 32).  gy channels at 2^-30 .. 2^-10,
    dx into a wider pixel stride with the pad channels and the memory behind it untouched.  Route: the workspace query's
    own size for the narrow halo instance; for the few-channel kernel the shape rule of the conv it is - gy's K channels
    into C (acimg_conv2d_stats_rows of that conv: 512) - and the workspace's footprint: the kernel's weight image
    (2 x 16 rows, or 32 for more than 16 channels of dx, x 96 or 160 bf16) and not a byte more, where the zero-inserted copy
    or the direct kernel would differ."""
    import ctypes as C

    from acimg import _lib, ops

    N, H, W, Cc, K, kind = sf.FP32_CASES[case][:6]
    o, ref, bound = fp32_grad_reference(case)
    d = ops.conv_desc(N, H, W, Cc, K, 3, 3, 2 if kind == "few/2" else 1, "SAME")
    assert (d.pad_t, d.pad_l) == ((H % 2, W % 2) if kind == "few/2" else (1, 1)) and o.gy.shape[1:3] == (d.OH, d.OW)
    query = int(_lib.load().acimg_conv2d_dgrad_workspace(C.byref(d)))
    narrow = K == 32
    if narrow:
        assert query == 2 * 16 * 288 * 2 + 256
    else:
        assert ops.conv2d_stats_rows(ops.conv_desc(N, H, W, K, Cc, 3, 3, 1, "SAME")) == 512
    plan = ops.Plan(device, eager=True)
    ws = poisoned_workspace(plan, query)
    flat, dx = guarded(device, (N, H, W), Cc + 4)
    dx[..., :Cc] = float("nan")
    ops.conv2d_dgrad(plan, d, o.gy.to(device), K, o.w.to(device), dx, lddx=Cc + 4)
    torch.cuda.synchronize()
    image = 2 * (16 if narrow or Cc <= 16 else 32) * (288 if narrow else (96 if K <= 8 else 160)) * 2
    assert int(ws[image - 1]) != WS_BYTE and bool((ws[image:] == WS_BYTE).all()), "the workspace's footprint is another route's"
    held("fp32 entry, " + case, "dx", dx[..., :Cc], ref, bound)
    untouched(case + " dx", flat, dx, Cc, Cc + 4)


@pytest.mark.parametrize("impulse", [False, True], ids=["dense", "impulse"])
@pytest.mark.parametrize("case", FEW_WGRAD)
def test_few_channel_weight_gradient_route(device, case, impulse):
    """acimg_conv2d_wgrad on wgrad_halo16_kernel<16, 3> (bf16x3 on a zero-padded channel tile): dense gradients with the
    launch's real counts (sf.fp32_wgrad_counts), and the `impulse` set - gy nonzero at a handful of pixels round the tensor's
    ends and a tile's, a row's and an image's boundary - where each dw element is one or two products and the format term
    alone is the bound; dw with pad columns, db.  Route: acimg_conv2d_affine_input_ok (forward AND weight gradient on the
    halo kernels)."""
    from acimg import ops

    N, H, W, Cc, K = sf.FP32_CASES[case][:5]
    o, ref, bound, dbref, counts = fp32_wgrad_reference(case, impulse)
    d = ops.conv_desc(N, H, W, Cc, K, 3, 3, 1, "SAME", ldw=K + 4)
    assert ops.conv2d_affine_input_ok(d, 0)
    plan = ops.Plan(device, eager=True)
    flat, dw = guarded(device, (3, 3, Cc), K + 4)
    dw[..., :K] = float("nan")
    db = torch.full((K + TAIL,), SENT, device=device)
    ops.conv2d_wgrad(plan, d, o.x.to(device), o.gy.to(device), K, dw, db)
    torch.cuda.synchronize()
    failures = []
    path, what = "fp32 entry, " + case, "impulse " if impulse else ""
    print("wgrad %s: %d K steps, %d slabs" % (case, counts[0], counts[1]))
    held(path, what + "dw", dw[..., :K], ref, bound, failures)
    held(path, what + "db", db[:K], dbref,
         sf.bound_bf16x3(torch.ones_like(o.gy), o.gy, counts[0], ranges=counts[1], prod=sf.colsum, fmt=FEW), failures)
    untouched(case + " dw", flat, dw, K, K + 4)
    assert bool((db[K:] == SENT).all()), "memory past db written"
    assert not failures, failures


def pointwise_desc(ops, **kw):
    N, H, W, Cc, K = sf.FP32_CASES["pointwise"][:5]
    assert N * H * W >= 65536 and N * H * W % 2 == 1           # the last 16-pixel group and 32-pixel block are ragged
    return ops.deconv_desc(N, H, W, Cc, K, 2, 2, 2, **kw)


@pytest.mark.parametrize("name", sf.FP32_CASES["pointwise"][6])
def test_pointwise_forward_route(device, name):
    """acimg_deconv_fwd on patch2_32x8_kernel<SplitF16, 0> (one 32-deep step per output element) with 65709 input pixels - the
    last 16-pixel group has 3 dead lanes - on `channels`, `quiet` and `loud` (the ends of the stated range), with a bias of
    each channel's own magnitude (one more fp32 rounding, of |bias|: where the bias outweighs the product that rounding IS
    the bound, so ratios near 1 here are the add, not the format), into the upper channel slice of a wider pixel stride: the
    lower slice and the memory behind the tensor untouched.  (Route: the three pointwise kernels share one shape rule;
    test_pointwise_weight_gradient_route shows it taken by its workspace footprint.)"""
    from acimg import ops

    N, H, W, Cc, K = sf.FP32_CASES["pointwise"][:5]
    o, ref, bound = fp32_forward_reference("pointwise", name)
    g = torch.Generator().manual_seed(601)
    bias = torch.randn(K, generator=g) * ref.reshape(-1, K).abs().amax(0).float()
    d = pointwise_desc(ops, ldy=2 * K)
    plan = ops.Plan(device, eager=True)
    flat, y = guarded(device, (N, 2 * H, 2 * W), 2 * K)
    y[..., K:] = float("nan")
    ops.deconv_fwd(plan, d, o.x.to(device), o.w.to(device), bias.to(device), ops.Ptr(flat, K))
    torch.cuda.synchronize()
    held("fp32 entry, pointwise fwd", name, y[..., K:], ref + bias.double(), bound + U24 * bias.double().abs().expand_as(bound))
    untouched("pointwise fwd", flat, y, 0, K)


def test_pointwise_data_gradient_route(device):
    """acimg_deconv_dgrad on patch2_32x8_kernel<SplitBF16, 1> with and without the ReLU mask (the layer's own post-ReLU
    input: half of it zeros), gy channels at 2^-30 .. 2^-10, dx with pad channels; dead lanes as in the forward"""
    from acimg import ops

    N, H, W, Cc, K = sf.FP32_CASES["pointwise"][:5]
    o, ref, bound = fp32_grad_reference("pointwise")
    d = pointwise_desc(ops, ldx=Cc + 4)
    plan = ops.Plan(device, eager=True)
    gyd, wd = o.gy.to(device), o.w.to(device)
    mask = o.x.to(device)
    assert 0.3 < float((o.x > 0).float().mean()) < 0.7
    failures = []
    for what, m in (("dx", None), ("dx, ReLU mask", mask)):
        flat, dx = guarded(device, (N, H, W), Cc + 4)
        dx[..., :Cc] = float("nan")
        ops.deconv_dgrad(plan, d, gyd, K, wd, dx, m, Cc if m is not None else 0)
        torch.cuda.synchronize()
        held("fp32 entry, pointwise", what, dx[..., :Cc], ref if m is None else ref * (o.x > 0).double(), bound, failures)
        untouched("pointwise " + what, flat, dx, Cc, Cc + 4)
    assert not failures, failures


@pytest.mark.parametrize("impulse", [False, True], ids=["dense", "impulse"])
def test_pointwise_weight_gradient_route(device, impulse):
    """acimg_deconv_wgrad on patch2_wgrad_32x8_kernel: 65709 pixels end the last 32-pixel block inside one lane's 8 pixels, and
    rows of 147 and images of 21903 pixels end inside a lane's 8 pixels (the carry).  Dense gradients with the launch's
    counts, and the `impulse` set: gy nonzero round a lane, block, row and image boundary, at the last live pixel and through
    its lane group - each dw element one or two products.  The fused bias gradient against the fp64 column sum of gy, bound:
    fp32 summation over the values each chain adds (sf.patch2_db_adds) - on `impulse` a dead lane's gy counted as live would be
    far outside it.  dw with pad columns.  Route: the workspace's footprint - 256 slabs of 32 x ldw (pad columns unwritten)
    and 256 x 8 bias partials, nothing behind them."""
    import ctypes as C

    from acimg import _lib, ops

    N, H, W, Cc, K = sf.FP32_CASES["pointwise"][:5]
    o, ref, bound, dbref, counts = fp32_wgrad_reference("pointwise", impulse)
    ldw = Cc + 4
    d = pointwise_desc(ops, ldw=ldw)
    plan = ops.Plan(device, eager=True)
    ws = poisoned_workspace(plan, int(_lib.load().acimg_deconv_workspace(C.byref(d))))
    flat, dw = guarded(device, (2, 2, K), ldw)
    dw[..., :Cc] = float("nan")
    db = torch.full((K + TAIL,), SENT, device=device)
    ops.deconv_wgrad(plan, d, o.x.to(device), o.gy.to(device), K, dw, db)
    torch.cuda.synchronize()
    foot = 256 * (32 * ldw + 8) * 4
    slabs = ws[:256 * 32 * ldw * 4].view(256 * 32, ldw * 4)
    assert bool((slabs[:, Cc * 4:] == WS_BYTE).all()) and bool((ws[foot:] == WS_BYTE).all()), "not the pointwise kernel's slabs"
    assert not bool((ws[foot - 4:foot] == WS_BYTE).all()) and not bool((slabs[-1, Cc * 4 - 4:Cc * 4] == WS_BYTE).all())
    failures = []
    path, what = "fp32 entry, pointwise", "impulse " if impulse else ""
    print("wgrad pointwise: %d K steps, %d slabs" % counts)
    held(path, what + "dw", dw[..., :Cc], ref, bound, failures)
    adds = sf.patch2_db_adds(N * H * W)
    held(path, what + "db", db[:K], dbref, adds * U24 * o.gy.double().abs().sum((0, 1, 2)), failures)
    untouched("pointwise dw", flat, dw, Cc, ldw)
    assert bool((db[K:] == SENT).all()), "memory past db written"
    assert not failures, failures


def test_halo_weight_gradient_on_impulses(device):
    """acimg_conv2d_wgrad_split3 at 64 -> 32 (wgrad_halo16_kernel<64, 3>, 4-row tiles) on the `impulse` set"""
    from acimg import ops

    case = "halo 64"
    N, H, W, Cc, K, taps = sf.BWD_CASES[case][:6]
    o = sf.impulse_operands(case)
    wg = sf.conv_wgrad(taps)
    d = ops.conv_desc(N, H, W, Cc, K, taps, taps, 1, "SAME")
    assert ops.conv2d_affine_input_ok(d, 1)                   # forward and weight gradient on the halo kernels
    plan = ops.Plan(device, eager=True)
    dw = torch.full((taps, taps, Cc, K), float("nan"), device=device)
    db = torch.full((K,), float("nan"), device=device)
    ops.conv2d_wgrad_split3(plan, d, o.x.to(device), o.gy.to(device), K, dw, db)
    torch.cuda.synchronize()
    failures = []
    held("bf16x3 backward " + case, "impulse dw", dw, wg(o.x.double(), o.gy.double()),
         sf.bound_bf16x3(o.x, o.gy, o.npix, ranges=0, prod=wg, fmt=FEW), failures)
    held("bf16x3 backward " + case, "impulse db", db, o.gy.double().sum((0, 1, 2)),
         sf.bound_bf16x3(torch.ones_like(o.gy), o.gy, o.npix, ranges=0, prod=sf.colsum, fmt=FEW), failures)
    assert not failures, failures
