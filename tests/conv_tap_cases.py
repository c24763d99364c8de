"""Operands and bounds that tests/test_conv_tap_gpu.py holds the tap-sharing convs (csrc/conv_tap_kernel.hpp) to, per output
element, and that tests/test_conv_tap_ref_cpu.py holds the formats alone to at half the bound: the operand sets of
tests/split_format_ref.py on a shape the tap form takes (two images of three row tiles, 48-pixel rows, two 32-channel chunks,
one 128-column block).  K is summed chunk-major there, in as many 32-deep steps as tap-major: ksteps = fwd_ksteps(3, 3, C)."""
import functools

import split_format_ref as sf

BOUND_CASE = (2, 6, 48, 64, 128)         # N, H, W, C, K
BOUND_SEED = 301
FWD_SETS = ("channels", "quiet", "loud")


@functools.lru_cache(maxsize=None)
def forward(name):
    """-> (operands, fp64 reference, per-element bound) of the f16x3 forward conv on one operand set"""
    N, H, W, Cc, K = BOUND_CASE
    o = sf.conv_operands(name, N, H, W, Cc, K, 3, 3, BOUND_SEED + 1000 * sf.SETS.index(name))
    return o, sf.conv_fwd(o.xa.double(), o.w.double()), sf.bound_f16x3(o.xa, o.w, sf.fwd_ksteps(3, 3, Cc), prod=sf.conv_fwd)


@functools.lru_cache(maxsize=None)
def dgrad():
    """-> (operands, fp64 reference, per-element bound) of the bf16x3 data gradient on `grad_operands`, with the format
    coefficient of the existing "tap" case"""
    N, H, W, Cc, K = BOUND_CASE
    o = sf.grad_operands(N, H, W, Cc, K, 3, 3, BOUND_SEED + 500)
    bound = sf.bound_bf16x3(o.gy, o.w, sf.fwd_ksteps(3, 3, K), prod=sf.conv_dgrad, fmt=sf.bwd_fmt("tap"))
    return o, sf.conv_dgrad(o.gy.double(), o.w.double()), bound
