"""Operand forms of the convolution family (include/acimg.h, "OPERAND FORMS"): which entry point must do what when ONE operand
of an otherwise legal call sits one float past a 16-byte boundary ("+4") or has the smallest legal leading dimension plus 1 or
2 ("ld+1", "ld+2").  tests/test_operand_forms_cpu.py walks the refusals with fake pointers, tests/test_operand_forms_gpu.py
runs the forms that must succeed inside guard bands.

The expectations are the header's contract, not a run:
  wide-access operands (x, gy, w, weight images, split planes, in_scale / in_shift, dw, tickets; ldx, ldw, ldgy)
      -> ACIMG_EINVAL, the operand's name in the text; the workspace -> ACIMG_EWORKSPACE ("workspace");
  outputs and epilogue operands (y / dx, bias, residual, mask, db) -> the call succeeds on a general kernel,
      EXCEPT on the routes whose query promised one kernel (ROUTE_PROMISED) -> ACIMG_EINVAL naming the operand.
Rows are the shapes of tests/caller_memory_cases.py (the smallest per route) plus SPLIT_CASES / PRESPLIT_CASES below."""
from collections import OrderedDict

from caller_memory_cases import DECONV_CASES, DGRAD_CASES, FWD_CASES, WGRAD_CASES

OK, EINVAL, EWORKSPACE, ELAUNCH = 0, -1, -2, -3
POINTER_FORMS = ("+4",)
LD_FORMS = ("ld+1", "ld+2")

# on-the-fly split entries (acimg_conv2d_fwd_split3 / _bf16, _dgrad_split3 / _bf16): (shape, forward tolerance, data-gradient
# tolerance: tests/test_conv_tap_gpu.py FWD_TOL / BWD_TOL, the halo kernel's 3e-5 of DGRAD_CASES["halo16_narrow"])
SPLIT_CASES = OrderedDict([
    ("tap_sharing", ((2, 36, 48, 128, 128, 3, 3, 1, "SAME"), 2e-6, 3e-5)),     # conv_tap_kernel, forward and data gradient
    ("halo16", ((4, 112, 149, 32, 32, 3, 3, 1, "SAME"), 2e-6, 3e-5)),          # conv_halo16_kernel: forward refused, dgrad falls through
])
# pre-split trunk entries: the two shapes of tests/test_caller_memory_gpu.py::test_presplit_conv_caller_memory
PRESPLIT_CASES = OrderedDict([("3x3_128_128", (8, 56, 75, 128, 128, 3, 3)), ("1x1_256_1024", (32, 28, 38, 256, 1024, 1, 1))])

# (table, row) whose sizing / statistics-rows query promised one kernel: an odd output or epilogue operand is refused
ROUTE_PROMISED = {("conv2d_fwd", "few_channel_mfma"), ("conv2d_dgrad", "halo16_narrow"), ("conv2d_fwd_split3", "halo16"),
                  ("conv2d_fwd_bf16", "halo16")}

# entry point -> (wide-access pointers, wide-access leading dimensions, takes a workspace, output / epilogue operands with a
# leading dimension, output / epilogue operands without one)
ENTRIES = OrderedDict([
    ("conv2d_fwd", (("x", "w", "in_scale", "in_shift", "tickets"), ("ldx", "ldw"), True, ("y",), ("bias",))),
    ("conv2d_dgrad", (("gy", "w", "tickets"), ("ldgy", "ldw"), True, ("dx", "residual", "mask"), ())),
    ("conv2d_wgrad", (("x", "gy", "dw"), ("ldx", "ldgy", "ldw"), True, (), ("db",))),
    ("conv2d_wgrad_split3", (("x", "gy", "dw"), ("ldx", "ldgy", "ldw"), True, (), ("db",))),
    ("conv2d_wgrad_bf16", (("x", "gy", "dw"), ("ldx", "ldgy", "ldw"), True, (), ("db",))),
    ("conv2d_wgrad_affine", (("x", "in_scale", "in_shift", "gy", "dw"), ("ldx", "ldgy", "ldw"), True, (), ("db",))),
    ("deconv_fwd", (("x", "w", "tickets"), ("ldx", "ldw"), True, ("y",), ("bias",))),
    ("deconv_dgrad", (("gy", "w", "tickets"), ("ldgy", "ldw"), True, ("mask",), ("dx",))),
    ("deconv_wgrad", (("x", "gy", "dw"), ("ldx", "ldgy", "ldw"), True, (), ("db",))),
    ("conv2d_fwd_split3", (("x", "wsplit", "in_scale", "in_shift"), ("ldx", "ldw"), False, ("y",), ("bias",))),
    ("conv2d_fwd_bf16", (("x", "wsplit", "in_scale", "in_shift"), ("ldx", "ldw"), False, ("y",), ("bias",))),
    ("conv2d_dgrad_split3", (("gy", "wsplit_t"), ("ldgy", "ldw"), False, ("dx", "residual", "mask"), ())),
    ("conv2d_dgrad_bf16", (("gy", "wsplit_t"), ("ldgy", "ldw"), False, ("dx", "residual", "mask"), ())),
    # the trunk kernels store y in whole 16-byte pieces of dense rows: y / ldy are wide-access operands of these entries
    ("conv2d_fwd_split3p", (("x_planes", "wsplit", "y"), ("ldy", "ldw"), True, (), ())),
    ("conv2d_fwd_split1p", (("x_planes", "wsplit", "y"), ("ldy", "ldw"), True, (), ())),
    ("conv2d_fwd_split3p_stats", (("x_planes", "wsplit"), ("ldw",), True, (), ())),
    ("conv2d_fwd_split3p_tail", (("x_planes", "wsplit", "scale", "shift", "shortcut", "out_planes"), ("ldw",), True, (), ())),
    ("conv2d_fwd_split3p_tail_proj", (("x_planes", "wsplit", "scale", "shift", "shortcut", "sc_scale", "sc_shift", "out_planes"),
                                      ("ldw",), True, (), ())),
    ("conv2d_split3_prepare", (("w", "wsplit"), ("ldx", "ldw"), False, (), ())),
    ("conv2d_bf16_prepare", (("w", "wsplit"), ("ldx", "ldw"), False, (), ())),
    ("conv2d_split3_prepare_dgrad", (("w", "wsplit"), ("ldx", "ldw"), False, (), ())),
    ("conv2d_split3_prepare_multi", (("w", "wsplit"), ("ldx", "ldw"), False, (), ())),
])


def entry_rows(entry):
    """the rows an entry point is walked on -> [(row name, row record)]"""
    if entry == "conv2d_fwd":
        return list(FWD_CASES.items())
    if entry == "conv2d_dgrad":
        return list(DGRAD_CASES.items())
    if entry.startswith("conv2d_wgrad"):
        want = {"conv2d_wgrad": ("f32",), "conv2d_wgrad_split3": ("split3",), "conv2d_wgrad_bf16": ("bf16",),
                "conv2d_wgrad_affine": ("affine0", "affine1")}[entry]
        return [(n, c) for n, c in WGRAD_CASES.items() if c[1] in want]
    if entry.startswith("deconv"):
        return list(DECONV_CASES.items())
    if entry.startswith("conv2d_fwd_split3p") or entry == "conv2d_fwd_split1p":
        return list(PRESPLIT_CASES.items())
    # the on-the-fly entries and the prepare calls: the split shapes; the data-gradient image needs K % 32 == 0 (both have it)
    return list(SPLIT_CASES.items())


def present(entry, row, operand):
    """does the row's call pass this optional operand at all? (a NULL pointer has no form)"""
    if entry == "conv2d_dgrad":
        shape, with_res, with_mask, tickets, tol = DGRAD_CASES[row]
        return {"residual": with_res, "mask": with_mask}.get(operand, True)
    if entry == "deconv_dgrad" and operand == "mask":
        return row != "direct_dgrad"           # the direct route exists only without a mask
    return True


def outcomes(entry):
    """-> [(row, operand, form, expected code, word the error text must contain or None)] for every operand of the entry"""
    wide, lds, has_ws, out_ld, out_plain = ENTRIES[entry]
    table = []
    for row, _ in entry_rows(entry):
        promised = (entry, row) in ROUTE_PROMISED
        for op in wide:
            table.append((row, op, "+4", EINVAL, op))
        for ld in lds:
            table.append((row, ld, "ld+1", EINVAL, ld))
        if has_ws:
            table.append((row, "workspace", "+4", EWORKSPACE, "workspace"))
        for op in out_ld + out_plain:
            if not present(entry, row, op):
                continue
            for form in POINTER_FORMS + (LD_FORMS if op in out_ld else ()):
                table.append((row, op, form, EINVAL if promised else OK, op if promised else None))
    return table


def refusals(entry):
    return [t for t in outcomes(entry) if t[3] != OK]


def fall_throughs(entry):
    """the (row, operand, form) that must succeed: output and epilogue operands only - tests/test_operand_forms_gpu.py
    launches nothing else in an odd form"""
    return [t[:3] for t in outcomes(entry) if t[3] == OK]
