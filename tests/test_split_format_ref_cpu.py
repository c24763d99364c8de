"""The split-operand formats restated on the CPU (tests/split_format_ref.py): the formats alone meet the bounds that
tests/test_operand_range_gpu.py holds the kernels to, with half of each bound to spare, on every operand set those tests use;
and three defects a kernel could have each miss a bound by a factor of 4 or more."""
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
    for case in sf.BWD_CASES:
        o = sf.bwd_operands(case)
        gamp = o.gy.reshape(-1, o.gy.shape[-1]).abs().amax(0)
        assert float(gamp.max() / gamp.min()) >= 2.0 ** 18 and float(o.gy.abs().max()) < 2.0 ** -7
        nz = o.gy[o.gy != 0].abs()
        assert float(nz.min()) > 2.0 ** -100                     # fp32-normal with room: bf16x3 has no floor here


@pytest.mark.parametrize("case", list(sf.BWD_CASES))
def test_bf16x3_format_within_half_of_its_bound(case):
    N, H, W, Cc, K, taps = sf.BWD_CASES[case][:6]
    o = sf.bwd_operands(case)
    x, w, gy = o.x.double(), o.w.double(), o.gy.double()
    rs = {}
    rs["dx"] = sf.max_ratio(sf.emulate_bf16x3(o.gy, o.w, sf.conv_dgrad), sf.conv_dgrad(gy, w),
                            sf.bound_bf16x3(o.gy, o.w, sf.fwd_ksteps(taps, taps, K), prod=sf.conv_dgrad))
    wg = sf.conv_wgrad(taps)
    rs["dw"] = sf.max_ratio(sf.emulate_bf16x3(o.x, o.gy, wg), wg(x, gy),
                            sf.bound_bf16x3(o.x, o.gy, *sf.wgrad_counts(case, 1), prod=wg))
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
