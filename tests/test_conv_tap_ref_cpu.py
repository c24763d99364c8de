"""The formats alone, on exactly the operand sets and the shape tests/test_conv_tap_gpu.py holds the tap-sharing convs to per
element (tests/conv_tap_cases.py): the emulated f16x3 forward and bf16x3 data gradient stay within HALF of the bounds, so a GPU
miss is the kernel's fault and not the format's; a dropped cross term (`no_hi_lo`) exceeds them."""
import pytest

import conv_tap_cases as ct
import split_format_ref as sf


@pytest.mark.parametrize("name", ct.FWD_SETS)
def test_f16x3_format_within_half_of_the_forward_bound(name):
    o, ref, bound = ct.forward(name)
    r = sf.max_ratio(sf.emulate_f16x3(o.xa, o.w, sf.conv_fwd), ref, bound)
    print("RATIO emulated f16x3 | conv tap | %s | %.4f" % (name, r))
    assert r <= 0.5, (name, r)


def test_bf16x3_format_within_half_of_the_dgrad_bound():
    o, ref, bound = ct.dgrad()
    r = sf.max_ratio(sf.emulate_bf16x3(o.gy, o.w, sf.conv_dgrad), ref, bound)
    print("RATIO emulated bf16x3 | conv tap | dx | %.4f" % r)
    assert r <= 0.5, r


def test_dropped_cross_term_exceeds_the_bounds():
    """`no_hi_lo` planted in the forward (on at least one operand set) and in the data gradient"""
    rs = {}
    for name in ct.FWD_SETS:
        o, ref, bound = ct.forward(name)
        rs[name] = sf.max_ratio(sf.emulate_f16x3(o.xa, o.w, sf.conv_fwd, "no_hi_lo"), ref, bound)
    print("RATIO planted no_hi_lo | conv tap forward | %s" % ", ".join("%s %.1f" % kv for kv in rs.items()))
    assert max(rs.values()) > 1.0, rs
    o, ref, bound = ct.dgrad()
    r = sf.max_ratio(sf.emulate_bf16x3(o.gy, o.w, sf.conv_dgrad, "no_hi_lo"), ref, bound)
    print("RATIO planted no_hi_lo | conv tap dx | %.1f" % r)
    assert r > 1.0, r
