"""The split-operand convolutions over the operand range include/acimg.h states, held to PER-ELEMENT bounds.

The other GPU tests feed these kernels unit-scale operands and divide the largest error by the largest magnitude of the whole
tensor; a batch norm follows every one of these convs and rescales each output channel on its own, so an error that is small
against the loudest channel can be large against a quiet one.  Here input and output channels differ by orders of magnitude
(tests/split_format_ref.py: `channels`, `quiet`, `loud`, `deferred`), the reference is fp64 on the CPU, and every output
element is held to the bound derived from the format in that module's docstring: |got - ref| <= bound elementwise, every
output finite; a failure reports the largest error / bound.  Each case prints its largest ratio ("RATIO ..." lines)."""
import ctypes as C
import functools

import pytest
import torch
import torch.nn.functional as F

import split_format_ref as sf
from test_ops_gpu import plane_bytes, unsplit

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
TRUNK_FORMS = (("one-tile", dict(trunk_persistent=0, trunk_ring=0), 0), ("persistent", dict(trunk_persistent=2, trunk_ring=0), 1),
               ("ring128", dict(trunk_ring=2, trunk_ring_bm=128), 2), ("halo", dict(trunk_halo=2), 3))


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
    held(path, "dx", dx, sf.conv_dgrad(gy, w), sf.bound_bf16x3(o.gy, o.w, sf.fwd_ksteps(taps, taps, K), prod=sf.conv_dgrad),
         failures)
    wg = sf.conv_wgrad(taps)
    ksteps, slabs = sf.wgrad_counts(case, wgrad_slabs(ops, d))
    print("wgrad %s: %d K steps, %d slabs" % (case, ksteps, slabs))
    held(path, "dw", dw, wg(x, gy), sf.bound_bf16x3(o.x, o.gy, ksteps, ranges=slabs, prod=wg), failures)
    colsum = lambda a, b: (a * b).sum((0, 1, 2))
    held(path, "db", db, gy.sum((0, 1, 2)), sf.bound_bf16x3(torch.ones_like(o.gy), o.gy, ksteps, ranges=slabs, prod=colsum),
         failures)
    assert not failures, failures
