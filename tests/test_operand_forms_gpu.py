"""The fall-throughs of tests/operand_form_cases.py on the GPU: an output or epilogue operand (y / dx, bias, residual, mask, db)
that is one float past a 16-byte boundary, or whose leading dimension is the channel count plus 1 or 2, must not change what
an entry point computes - only which kernel computes it.  Per (row, operand, form) ONE call through the raw C ABI with exactly
the workspace bytes the query reports (poisoned), every output inside a guard arena and pre-filled with a sentinel, the odd
operand carved out of its region at the wanted offset and stride (tests/caller_memory_support.py: run_guarded):
  rc == 0; the documented elements equal the fp64 reference of the row (computed once per row) at max(the row's tolerance,
  RTOL): an odd form may move a 16-bit-split shape onto the exact-f32 kernel, never the other way;
  every other byte of every output region - before the offset, between the rows, after the last row - keeps the sentinel;
  all guard bands intact, tickets zero.
Only forms whose kernel touches that operand with scalar accesses are here (csrc/igemm_kernel.hpp: epi_store with e.vec == 0,
which the implicit GEMMs, the split-K reducers and the sub-pixel / patch scatters share; skinny_dgrad_kernel; the slab reducers
and wgrad_f32_kernel for db; deconv_gap_fill_kernel's scalar half; colsum_final_kernel).  Odd forms of operands the kernels read
in 16-byte pieces are refusals, and refusals are CPU tests (tests/test_operand_forms_cpu.py): none is launched here.
Statistics are requested only with ACIMG_ACT_NONE (with an activation their meaning follows the kernel: include/acimg.h)."""
import pytest

import operand_form_cases as of
from caller_memory_cases import FWD_CASES
from caller_memory_support import (deconv_cases, dgrad_case, fwd_case, run_guarded, split_dgrad_case, split_fwd_case, wgrad_case)

pytestmark = pytest.mark.gpu


def ids(table):
    return ["%s-%s-%s" % t for t in table]


FWD = of.fall_throughs("conv2d_fwd")
DGRAD = of.fall_throughs("conv2d_dgrad")
WGRAD = [t for e in ("conv2d_wgrad", "conv2d_wgrad_split3", "conv2d_wgrad_bf16", "conv2d_wgrad_affine") for t in of.fall_throughs(e)]
DECONV_FWD, DECONV_DGRAD, DECONV_WGRAD = (of.fall_throughs(e) for e in ("deconv_fwd", "deconv_dgrad", "deconv_wgrad"))
SPLIT_FWD, SPLIT_DGRAD = of.fall_throughs("conv2d_fwd_split3"), of.fall_throughs("conv2d_dgrad_split3")


def test_the_table_covers_the_routes():
    """y and bias on the skinny, direct, split-K, 256x16, tap-sharing routes; dx / residual / mask on the skinny, direct,
    few-channel, sub-pixel, patch-scatter, dilated, tap-sharing and halo-16 routes; y and bias on every transposed-conv route;
    db at +4 on every weight-gradient row; nothing of the routes that refuse"""
    have = lambda table, row, ops_: all(any(t[0] == row and t[1] == o for t in table) for o in ops_)
    for row in ("skinny", "direct_relu", "direct_stride2", "splitk_reduce_launch", "splitk_handoff", "splitk_stats", "tile_256x16"):
        assert have(FWD, row, ("y", "bias")), row
    for row in ("skinny", "direct", "few_channel_stride1", "few_channel_stride2", "subpixel_3x3_same", "patch_scatter", "dilated_3x3_same",
                "dilated_then_igemm_65536", "s1_splitk_handoff"):
        assert have(DGRAD, row, ("dx", "residual")), row
    assert have(DGRAD, "patch_scatter", ("mask",)) and have(DGRAD, "skinny", ("mask",))
    assert have(SPLIT_FWD, "tap_sharing", ("y", "bias")) and not any(t[0] == "halo16" for t in SPLIT_FWD)
    for row in ("tap_sharing", "halo16"):
        assert have(SPLIT_DGRAD, row, ("dx", "residual", "mask")), row
    assert not any(t[0] == "few_channel_mfma" for t in FWD) and not any(t[0] == "halo16_narrow" for t in DGRAD)
    assert len(WGRAD) == 13 and all(t[1:] == ("db", "+4") for t in WGRAD + DECONV_WGRAD) and len(DECONV_WGRAD) == 5
    assert all(have(DECONV_FWD, row, ("y", "bias")) and have(DECONV_DGRAD, row, ("dx",)) for row, *_ in DECONV_WGRAD)


@pytest.mark.parametrize("row,operand,form", FWD, ids=ids(FWD))
def test_conv2d_fwd_operand_forms(device, row, operand, form):
    act, with_stats = FWD_CASES[row][1:3]
    case = fwd_case(device, row, forms={operand: form}, stats=with_stats and act == 0)
    run_guarded(device, case, "conv2d_fwd[%s] %s %s" % (row, operand, form))


@pytest.mark.parametrize("row,operand,form", DGRAD, ids=ids(DGRAD))
def test_conv2d_dgrad_operand_forms(device, row, operand, form):
    run_guarded(device, dgrad_case(device, row, forms={operand: form}), "conv2d_dgrad[%s] %s %s" % (row, operand, form))


@pytest.mark.parametrize("row,operand,form", WGRAD, ids=ids(WGRAD))
def test_conv2d_wgrad_operand_forms(device, row, operand, form):
    run_guarded(device, wgrad_case(device, row, forms={operand: form}), "conv2d_wgrad[%s] %s %s" % (row, operand, form))


@pytest.mark.parametrize("row,operand,form", DECONV_FWD, ids=ids(DECONV_FWD))
def test_deconv_fwd_operand_forms(device, row, operand, form):
    run_guarded(device, deconv_cases(device, row, forms={operand: form})[0], "deconv_fwd[%s] %s %s" % (row, operand, form))


@pytest.mark.parametrize("row,operand,form", DECONV_DGRAD, ids=ids(DECONV_DGRAD))
def test_deconv_dgrad_operand_forms(device, row, operand, form):
    run_guarded(device, deconv_cases(device, row, forms={operand: form})[1], "deconv_dgrad[%s] %s %s" % (row, operand, form))


@pytest.mark.parametrize("row,operand,form", DECONV_WGRAD, ids=ids(DECONV_WGRAD))
def test_deconv_wgrad_operand_forms(device, row, operand, form):
    run_guarded(device, deconv_cases(device, row, forms={operand: form})[2], "deconv_wgrad[%s] %s %s" % (row, operand, form))


@pytest.mark.parametrize("row,operand,form", SPLIT_FWD, ids=ids(SPLIT_FWD))
def test_conv2d_fwd_split3_operand_forms(device, row, operand, form):
    shape, tol_f, tol_d = of.SPLIT_CASES[row]
    run_guarded(device, split_fwd_case(device, shape, tol_f, forms={operand: form}), "conv2d_fwd_split3[%s] %s %s" % (row, operand, form))


@pytest.mark.parametrize("row,operand,form", SPLIT_DGRAD, ids=ids(SPLIT_DGRAD))
def test_conv2d_dgrad_split3_operand_forms(device, row, operand, form):
    shape, tol_f, tol_d = of.SPLIT_CASES[row]
    run_guarded(device, split_dgrad_case(device, shape, tol_d, forms={operand: form}), "conv2d_dgrad_split3[%s] %s %s" % (row, operand, form))
