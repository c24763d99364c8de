"""The split-operand formats restated on the CPU (tests/split_format_ref.py): the formats alone meet the bounds that
tests/test_operand_range_gpu.py holds the kernels to, with half of each bound to spare, on every operand set those tests use;
and three defects a kernel could have each miss a bound by a factor of 4 or more.  The same for the routes behind the fp32
entry points (sf.FP32_CASES: few-channel 3x3, its stride-2 data gradient, the pointwise transposed conv), route by route, with
a dropped cross term as the bf16x3 defect and the `impulse` set for the weight gradients."""
import functools

import pytest
import torch

import split_format_ref as sf

FWD = [(case, name) for case, rec in sf.FWD_CASES.items() for name in rec[6]]
DEFECTS = ("flush", "split_before_scale", "no_hi_lo")


@functools.lru_cache(maxsize=None)
def forward_ratios(case, name):
    """error / bound of the emulated f16x3 conv of one operand set: the format, then each planted defect"""
    N, H, W, Cc, K, taps = sf.FWD_CASES[case][:6]
    o = sf.fwd_operands(case, name)
    ref = sf.conv_fwd(o.xa.double(), o.w.double())
    bound = sf.bound_f16x3(o.xa, o.w, sf.fwd_ksteps(taps, taps, Cc), prod=sf.conv_fwd)
    return {d: sf.max_ratio(sf.emulate_f16x3(o.xa, o.w, sf.conv_fwd, d), ref, bound) for d in (None,) + DEFECTS}


def test_split_matches_the_kernel_statement():
    """hi is the nearest 16-bit value of the scaled operand, lo the nearest of the fp32 residual; hi + lo holds 22 (16) bits"""
    g = torch.Generator().manual_seed(1)
    v = torch.randn(4096, generator=g) * torch.ldexp(torch.ones(4096), torch.randint(-12, 12, (4096,), generator=g))
    hi, lo = sf.split_f16(v, 0.25)
    s = v * 0.25
    assert hi.dtype == lo.dtype == torch.float16
    assert torch.equal(hi, s.half()) and torch.equal(lo, (s - s.half().float()).half())
    big = s.abs() >= 0.25                                        # residual grid 2^(e-23) >= the subnormal grid: 22 bits
    assert float(((hi.double() + lo.double() - s.double()).abs() / s.double().abs())[big].max()) <= 2.0 ** -23
    assert float((hi.double() + lo.double() - s.double()).abs()[~big].max()) <= 2.0 ** -25      # the floor: half a subnormal step
    bh, bl = sf.split_bf16(v)
    assert bh.dtype == bl.dtype == torch.bfloat16
    assert torch.equal(bh, v.bfloat16()) and torch.equal(bl, (v - v.bfloat16().float()).bfloat16())
    assert float(((bh.double() + bl.double() - v.double()).abs() / v.double().abs()).max()) <= 2.0 ** -17
    a, b = torch.tensor([3.0, 5.0]), torch.tensor([0.5, 0.25])
    assert torch.equal(sf.three_term(a, a * 0.5, b, b * 2), (a * b + a * b * 2 + a * 0.5 * b).double())


@pytest.mark.parametrize("case,name", FWD)
def test_f16x3_format_within_half_of_its_bound(case, name):
    r = forward_ratios(case, name)[None]
    print("RATIO emulated f16x3 | %s | %s | %.4f" % (case, name, r))
    assert r <= 0.5, (case, name, r)


@pytest.mark.parametrize("defect", DEFECTS)
def test_planted_f16x3_defect_exceeds_the_bound(defect):
    """each defect is 4 times over the bound on at least one operand set the GPU tests use"""
    rs = {(case, name): forward_ratios(case, name)[defect] for case, name in FWD}
    worst = max(rs, key=rs.get)
    print("RATIO planted %s | %s | %.1f" % (defect, worst, rs[worst]))
    assert rs[worst] >= 4.0, (defect, rs)


def test_operand_sets_reach_the_stated_range():
    """the sets put operands at both ends of |w| < 63, |x| < 2.6e5 and on the floors, and nothing beyond"""
    for case, name in FWD:
        o = sf.fwd_operands(case, name)
        assert o.x.dtype == o.w.dtype == o.xa.dtype == torch.float32
        assert float(o.xa.abs().max()) <= 2.5e5 and float(o.w.abs().max()) <= 62.0
        assert float(o.xa.min()) >= 0.0
        if name == "loud":
            assert float(o.xa.abs().max()) > 2.0e5 and float(o.w.abs().max()) > 50.0
            assert float(sf.conv_fwd(o.xa.double().abs(), o.w.double().abs()).max()) < 1e30
        if name == "quiet":
            assert 2.0 ** -9 <= float(o.xa.min()) and float(o.xa.max()) <= 2.0 ** -7
        if name in ("channels", "deferred"):
            amp = o.xa.reshape(-1, o.xa.shape[-1]).amax(0)
            assert float(amp.max() / amp.min()) >= 2.0 ** 12
            wamp = o.w.reshape(-1, o.w.shape[-1]).abs().amax(0)
            assert float(wamp.max() / wamp.min()) >= 2.0 ** 11
        if name == "deferred":
            assert torch.equal(o.xa, torch.relu(o.x.double() * o.in_scale.double()).float())      # the affine is exact in fp32
    for case, name in sf.FP32_FWD:
        o = sf.fp32_operands(case, name)
        Cc, K, kind = sf.FP32_CASES[case][3:6]
        assert o.x.dtype == o.w.dtype == o.xa.dtype == torch.float32 and float(o.xa.min()) >= 0.0
        assert o.w.shape == ((2, 2, K, Cc) if kind == "point" else (3, 3, Cc, K))
        assert float(o.xa.abs().max()) <= 2.5e5 and float(o.w.abs().max()) <= 62.0
        if name == "loud":
            assert float(o.xa.abs().max()) > 2.0e5 and float(o.w.abs().max()) > 50.0
        if name == "quiet":
            assert 2.0 ** -9 <= float(o.xa.min()) and float(o.xa.max()) <= 2.0 ** -7
        if name in ("channels", "deferred"):                     # (4 channels draw 4 exponents: both ends are among them)
            amp = o.xa.reshape(-1, Cc).amax(0)
            assert float(amp.max() / amp.min()) >= 2.0 ** 12
            wamp = o.w.abs().amax((0, 1, 3) if kind == "point" else (0, 1, 2))
            assert float(wamp.max() / wamp.min()) >= 2.0 ** 11
        if name == "deferred":
            assert torch.equal(o.xa, torch.relu(o.x.double() * o.in_scale.double()).float())
    grads = [sf.bwd_operands(case) for case in sf.BWD_CASES] + [sf.fp32_grad_operands(case) for case in sf.FP32_BWD]
    for case in sf.IMPULSE_CASES:
        o = sf.impulse_operands(case)
        lit = (o.gy != 0).any(-1)
        point = case == "pointwise"
        assert int(lit.sum()) == o.npix * (4 if point else 1) and 10 <= o.npix <= 20
        assert bool(lit.reshape(-1)[0]) and bool(lit.reshape(-1)[-1])          # the first and the last pixel of the tensor
        grads.append(o)
    for o in grads:
        gamp = o.gy.reshape(-1, o.gy.shape[-1]).abs().amax(0)
        assert float(gamp.max() / gamp.min()) >= 2.0 ** 18 and float(o.gy.abs().max()) < 2.0 ** -7
        nz = o.gy[o.gy != 0].abs()
        assert float(nz.min()) > 2.0 ** -100                     # fp32-normal with room: bf16x3 has no floor here
    for H in (149, 150):                                         # the stride-2 cases: leading pad 1 (odd) and 0 (even)
        assert sf.same_pad2(H) == ((H + 1) // 2, H % 2)


# ---- the routes behind the fp32 entry points ---------------------------------------------------------------------------
CROSS = ("no_hi_lo", "no_lo_hi")
FEW = sf.BF16_FMT_FEW
FP32_FWD_ROUTES = sorted(set(case for case, _ in sf.FP32_FWD)) + ["halo 64"]


@functools.lru_cache(maxsize=None)
def fp32_forward_ratios(case, name):
    prod, ksteps = sf.fp32_products(case)["fwd"]
    o = sf.fp32_operands(case, name)
    ref = prod(o.xa.double(), o.w.double())
    bound = sf.bound_f16x3(o.xa, o.w, ksteps, prod=prod)
    return {d: sf.max_ratio(sf.emulate_f16x3(o.xa, o.w, prod, d), ref, bound) for d in (None,) + DEFECTS}


@functools.lru_cache(maxsize=None)
def fp32_backward_ratios(case):
    """dx: the emulated bf16x3 data gradient and each dropped cross term; dw: the emulated dense weight gradient"""
    o = sf.fp32_grad_operands(case)
    pr = sf.fp32_products(case)
    prod, ksteps = pr["dgrad"]
    ref, bound = prod(o.gy.double(), o.w.double()), sf.bound_bf16x3(o.gy, o.w, ksteps, prod=prod, fmt=FEW)
    rs = {"dx": {d: sf.max_ratio(sf.emulate_bf16x3(o.gy, o.w, prod, d), ref, bound) for d in (None,) + CROSS}}
    if "wgrad" in pr:
        wg = pr["wgrad"]
        ks, slabs = sf.fp32_wgrad_counts(case)
        rs["dw"] = {None: sf.max_ratio(sf.emulate_bf16x3(o.x, o.gy, wg), wg(o.x.double(), o.gy.double()),
                                       sf.bound_bf16x3(o.x, o.gy, ks, ranges=slabs, prod=wg, fmt=FEW))}
    return rs


def test_new_products_are_adjoints_of_each_other():
    """<fwd(x, w), gy> = <x, dgrad(gy, w)> = <w, wgrad(x, gy)> for the stride-2 conv (both parities of H and W) and the
    transposed conv, and the transposed conv against its definition tap by tap"""
    g = torch.Generator().manual_seed(2)
    R = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    for H, W in ((10, 12), (11, 13), (10, 13), (11, 12)):
        x, w = R(2, H, W, 3), R(3, 3, 3, 5)
        y = sf.conv_fwd_s2(x, w)
        assert y.shape == (2, (H + 1) // 2, (W + 1) // 2, 5)
        gy = R(*y.shape)
        assert abs(float((y * gy).sum() - (x * sf.conv_dgrad_s2(H, W)(gy, w)).sum())) < 1e-10
        win = x[:, 2 - H % 2:5 - H % 2, 2 - W % 2:5 - W % 2]           # output (1, 1): rows 2 - pad_t .., columns 2 - pad_l ..
        assert float((y[:, 1, 1] - torch.einsum("nrsc,rsck->nk", win, w)).abs().max()) < 1e-12
    x, w = R(2, 5, 7, 6), R(2, 2, 4, 6)
    y = sf.deconv_fwd(x, w)
    for r in range(2):
        for s in range(2):
            assert float((y[:, r::2, s::2] - torch.einsum("nijc,kc->nijk", x, w[r, s])).abs().max()) < 1e-12
    gy = R(*y.shape)
    assert abs(float((y * gy).sum() - (x * sf.deconv_dgrad(gy, w)).sum())) < 1e-10
    assert abs(float((y * gy).sum() - (w * sf.deconv_wgrad(x, gy)).sum())) < 1e-10


@pytest.mark.parametrize("case,name", sf.FP32_FWD)
def test_fp32_route_f16x3_format_within_half_of_its_bound(case, name):
    r = fp32_forward_ratios(case, name)[None]
    print("RATIO emulated f16x3 | %s | %s | %.4f" % (case, name, r))
    assert r <= 0.5, (case, name, r)


@pytest.mark.parametrize("defect", DEFECTS)
@pytest.mark.parametrize("case", FP32_FWD_ROUTES)
def test_planted_f16x3_defect_exceeds_the_bound_on_every_route(case, defect):
    """route by route: each defect is 4 times over the bound on at least one operand set the GPU test of that route uses"""
    if case in sf.FP32_CASES:
        rs = {name: fp32_forward_ratios(case, name)[defect] for name in sf.FP32_CASES[case][6]}
    else:
        rs = {name: forward_ratios(case, name)[defect] for name in sf.FWD_CASES[case][6]}
    worst = max(rs, key=rs.get)
    print("RATIO planted %s | %s | %s | %.1f" % (defect, case, worst, rs[worst]))
    assert rs[worst] >= 4.0, (case, defect, rs)


@pytest.mark.parametrize("case", sf.FP32_BWD)
def test_fp32_route_bf16x3_format_within_half_of_its_bound(case):
    for what, rs in fp32_backward_ratios(case).items():
        print("RATIO emulated bf16x3 | %s | %s | %.4f" % (case, what, rs[None]))
        assert rs[None] <= 0.5, (case, what, rs[None])


@pytest.mark.parametrize("case", sf.FP32_BWD)
def test_dropped_cross_term_exceeds_the_bf16x3_bound_on_every_route(case):
    """either cross term dropped from the data gradient is 4 times over the bound on `grad_operands`"""
    rs = fp32_backward_ratios(case)["dx"]
    for d in CROSS:
        print("RATIO planted %s | %s dx | %.1f" % (d, case, rs[d]))
        assert rs[d] >= 4.0, (case, rs)


@pytest.mark.parametrize("case", sf.IMPULSE_CASES)
def test_impulse_weight_gradient_sees_a_dropped_cross_term(case):
    """the `impulse` set: the format alone within half of the bound, either cross term dropped 4 times over it - the dense
    weight gradient cannot see one (its ratio with the term dropped is printed beside)"""
    o = sf.impulse_operands(case)
    wg = sf.fp32_products(case)["wgrad"] if case in sf.FP32_CASES else sf.conv_wgrad(3)
    ref, bound = wg(o.x.double(), o.gy.double()), sf.bound_bf16x3(o.x, o.gy, o.npix, ranges=0, prod=wg, fmt=FEW)
    assert int((ref != 0).sum()) >= ref.numel() // 4
    rs = {d: sf.max_ratio(sf.emulate_bf16x3(o.x, o.gy, wg, d), ref, bound) for d in (None,) + CROSS}
    print("RATIO emulated bf16x3 | %s | impulse dw | %.4f" % (case, rs[None]))
    assert rs[None] <= 0.5, (case, rs)
    for d in CROSS:
        print("RATIO planted %s | %s impulse dw | %.1f" % (d, case, rs[d]))
        assert rs[d] >= 4.0, (case, rs)


@pytest.mark.parametrize("case", list(sf.BWD_CASES))
def test_bf16x3_format_within_half_of_its_bound(case):
    N, H, W, Cc, K, taps = sf.BWD_CASES[case][:6]
    o = sf.bwd_operands(case)
    x, w, gy = o.x.double(), o.w.double(), o.gy.double()
    rs = {}
    fmt = sf.bwd_fmt(case)
    rs["dx"] = sf.max_ratio(sf.emulate_bf16x3(o.gy, o.w, sf.conv_dgrad), sf.conv_dgrad(gy, w),
                            sf.bound_bf16x3(o.gy, o.w, sf.fwd_ksteps(taps, taps, K), prod=sf.conv_dgrad, fmt=fmt))
    wg = sf.conv_wgrad(taps)
    rs["dw"] = sf.max_ratio(sf.emulate_bf16x3(o.x, o.gy, wg), wg(x, gy),
                            sf.bound_bf16x3(o.x, o.gy, *sf.wgrad_counts(case, 1), prod=wg, fmt=fmt))
    for what, r in rs.items():
        print("RATIO emulated bf16x3 | %s | %s | %.4f" % (case, what, r))
        assert r <= 0.5, (case, what, r)


def test_split_planes_hold_what_plane_bound_says():
    """decoded planes of the producers' operand sets: within plane_bound, and NOT within 2^-24 |v| (the format drops the
    24th bit of a quarter of all values)"""
    worst_rel = 0.0
    for name in ("channels", "loud", "quiet"):
        v = sf.fwd_operands("presplit 1x1", name).xa
        hi, lo = sf.split_f16(v, sf.F16_ASCALE)
        got = (hi.double() + lo.double()) * 4.0
        assert bool(torch.isfinite(got).all())
        err = (got - v.double()).abs()
        assert bool((err <= sf.plane_bound(v)).all()), name
        nz = v != 0
        worst_rel = max(worst_rel, float((err[nz] / v.double()[nz].abs()).max()))
        if name != "quiet":
            over = (err > torch.maximum(v.double().abs() * 2.0 ** -24, torch.full_like(err, 2.0 ** -23)))
            assert float(over.double().mean()) >= 0.02, (name, float(over.double().mean()))
    assert worst_rel > 2.0 ** -15                                # the floor: quiet activations keep ~14 bits


# ---- the activation-plane layout ---------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge

    ge.build()
    from acimg import _lib

    return _lib.load()


# rows, C; 5320 x 256 is a trunk row count that is 8 mod 16 (the Gram statistics read such planes)
PLANE_SHAPES = [(1, 32), (5, 32), (16, 64), (17, 96), (40, 128), (5320, 256)]


@pytest.mark.parametrize("rows,Cc", PLANE_SHAPES)
def test_brick_index_is_a_layout_of_the_plane(lib, rows, Cc):
    """every element of a [rows, C] tensor has its own fp16 slot inside the plane, the slots fill the plane when there are no
    pad rows, and the plane is as large as the library says"""
    idx = sf.brick_index(rows, Cc)
    n = sf.plane_bytes(rows, Cc)
    assert n == lib.acimg_split_plane_bytes(rows, Cc)
    assert idx.numel() == rows * Cc and idx.unique().numel() == rows * Cc
    assert int(idx.min()) >= 0 and int(idx.max()) < n // 2
    if rows % 16 == 0:
        assert torch.equal(idx.sort().values, torch.arange(n // 2))


def test_brick_index_matches_the_header_by_hand():
    """byte = ((row >> 4) * C / 32 + (c >> 5)) * 1024 + (row & 15) * 64 + (((c >> 3) ^ -(row >> 2)) & 3) * 16 + (c & 7) * 2
    (include/acimg.h, "Pre-split activation format"), worked out by hand"""
    for rows, Cc, row, c, byte in ((1, 32, 0, 0, 0),
                                   (1, 32, 0, 9, 16 + 2),                       # group 1 stays group 1 in rows 0 .. 3
                                   (16, 32, 5, 0, 5 * 64 + 3 * 16),             # rows 4 .. 7: group g at g ^ 3
                                   (16, 32, 5, 17, 5 * 64 + 1 * 16 + 2),        # group 2 at 2 ^ 3 = 1
                                   (40, 64, 17, 40, 3 * 1024 + 64 + 16),        # brick (1, 1) of 2 per row; group 5 & 3 = 1 at 1 ^ 0
                                   (5320, 256, 5319, 255, (332 * 8 + 7) * 1024 + 7 * 64 + 0 * 16 + 14)):    # group 3 at 3 ^ 3 = 0
        assert int(sf.brick_index(rows, Cc)[row * Cc + c]) * 2 == byte, (rows, Cc, row, c)
