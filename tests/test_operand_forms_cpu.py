"""The refusals of tests/operand_form_cases.py without a GPU: every convolution-family entry point, on every row of its
table, with ONE operand in an odd form and every other argument legal, must return the code the table names - with the
operand's name in the text - before its first launch.  Pattern of tests/test_host_cpu.py::
test_short_or_missing_workspace_is_refused_before_any_launch: fake pointers stand for the tensors, so a form the library
fails to refuse reaches a launch and comes back as ACIMG_ELAUNCH on a machine without a GPU, which is what the failure
message then shows.  Every call here is therefore one that must never launch."""
import ctypes as C
import re

import pytest

import operand_form_cases as of
from caller_memory_cases import DECONV_CASES, DGRAD_CASES, FWD_CASES, WGRAD_CASES
from op_support import up4


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge

    ge.build()
    from acimg import _lib

    return _lib.load()


_BIG = (C.c_char * 8192)()
A = C.addressof(_BIG) + (-C.addressof(_BIG)) % 256          # a fake, 256-byte aligned "device pointer": never dereferenced


class Odd(object):
    """the one operand of a call that is not in its usual form"""

    def __init__(self, operand, form):
        self.operand, self.form = operand, form

    def ptr(self, name):
        return A + 4 if (name == self.operand and self.form == "+4") else A

    def ld(self, name, smallest, usual):
        """usual, or (this is the odd operand) the smallest legal leading dimension plus 1 or 2"""
        if name != self.operand or not self.form.startswith("ld+"):
            return usual
        return smallest + int(self.form[3:])


def _conv_call(lib, entry, row, odd):
    """-> rc of the entry point on the row with `odd` applied; every other argument as the GPU cases pass it"""
    from acimg import ops
    p, ld = odd.ptr, odd.ld
    if entry == "conv2d_fwd":
        shape, act = FWD_CASES[row][:2]
        N, H, W, Cc, K = shape[:5]
        q = lib.acimg_conv2d_fwd_workspace(C.byref(ops.conv_desc(*shape, ldy=K + 4, act=act)))
        d = ops.conv_desc(*shape, ldx=ld("ldx", Cc, Cc), ldy=ld("y", K, K + 4), ldw=ld("ldw", up4(K), up4(K)), act=act)
        return lib.acimg_conv2d_fwd(C.byref(d), p("x"), p("w"), p("bias"), p("y"), p("in_scale"), p("in_shift"), 1, None,
                                    p("workspace"), q, p("tickets"), None)
    if entry == "conv2d_dgrad":
        shape, with_res, with_mask = DGRAD_CASES[row][:3]
        N, H, W, Cc, K = shape[:5]
        q = lib.acimg_conv2d_dgrad_workspace(C.byref(ops.conv_desc(*shape, ldw=K)))
        d = ops.conv_desc(*shape, ldw=ld("ldw", K, K))
        return lib.acimg_conv2d_dgrad(C.byref(d), p("gy"), ld("ldgy", K, K + 4), p("w"), p("dx"), ld("dx", Cc, Cc + 4),
                                      p("residual") if with_res else None, ld("residual", Cc, Cc + 8),
                                      p("mask") if with_mask else None, ld("mask", Cc, Cc + 4), p("workspace"), q, p("tickets"), None)
    if entry.startswith("conv2d_wgrad"):
        shape, kind = WGRAD_CASES[row][:2]
        N, H, W, Cc, K = shape[:5]
        kp = up4(K)
        q = lib.acimg_conv2d_wgrad_workspace(C.byref(ops.conv_desc(*shape, ldw=kp + 4)))
        d = ops.conv_desc(*shape, ldx=ld("ldx", Cc, Cc), ldw=ld("ldw", kp, kp + 4))
        tail = (p("gy"), ld("ldgy", kp, kp + 4), p("dw"), p("db"), p("workspace"), q, None)
        if entry == "conv2d_wgrad_affine":
            return lib.acimg_conv2d_wgrad_affine(C.byref(d), int(kind[-1]), p("x"), p("in_scale"), p("in_shift"), 1, *tail)
        return getattr(lib, "acimg_" + entry)(C.byref(d), p("x"), *tail)
    if entry.startswith("deconv"):
        shape = DECONV_CASES[row][0]
        N, H, W, Cc, K = shape[:5]
        q = lib.acimg_deconv_workspace(C.byref(ops.deconv_desc(*shape, ldy=2 * K)))
        d = ops.deconv_desc(*shape, ldx=ld("ldx", Cc, Cc), ldy=ld("y", K, 2 * K), ldw=ld("ldw", Cc, Cc))
        if entry == "deconv_fwd":
            return lib.acimg_deconv_fwd(C.byref(d), p("x"), p("w"), p("bias"), p("y"), p("workspace"), q, p("tickets"), None)
        if entry == "deconv_dgrad":
            return lib.acimg_deconv_dgrad(C.byref(d), p("gy"), ld("ldgy", K, 2 * K), p("w"), p("dx"),
                                          p("mask") if row != "direct_dgrad" else None, ld("mask", Cc, Cc), p("workspace"), q,
                                          p("tickets"), None)
        return lib.acimg_deconv_wgrad(C.byref(d), p("x"), p("gy"), ld("ldgy", K, 2 * K), p("dw"), p("db"), p("workspace"), q, None)
    if entry in ("conv2d_fwd_split3", "conv2d_fwd_bf16"):
        shape = of.SPLIT_CASES[row][0]
        N, H, W, Cc, K = shape[:5]
        d = ops.conv_desc(*shape, ldx=ld("ldx", Cc, Cc), ldy=ld("y", K, K + 4), ldw=ld("ldw", K, K))
        return getattr(lib, "acimg_" + entry)(C.byref(d), p("x"), p("wsplit"), p("bias"), p("y"), p("in_scale"), p("in_shift"), 1,
                                              None, None)
    if entry in ("conv2d_dgrad_split3", "conv2d_dgrad_bf16"):
        shape = of.SPLIT_CASES[row][0]
        N, H, W, Cc, K = shape[:5]
        d = ops.conv_desc(*shape, ldw=ld("ldw", K, K))
        return getattr(lib, "acimg_" + entry)(C.byref(d), p("gy"), ld("ldgy", K, K), p("wsplit_t"), p("dx"), ld("dx", Cc, Cc + 4),
                                              p("residual"), ld("residual", Cc, Cc + 8), p("mask"), ld("mask", Cc, Cc + 4), None)
    if entry.startswith("conv2d_fwd_split3p") or entry == "conv2d_fwd_split1p":
        N, H, W, Cc, K, R, S = of.PRESPLIT_CASES[row]
        rows = N * H * W
        d = ops.conv_desc(N, H, W, Cc, K, R, S, 1, "SAME", ldy=ld("ldy", K, K), ldw=ld("ldw", K, K))
        q = lib.acimg_conv2d_fwd_split3p_workspace(C.byref(d))
        lo_x, lo_y = lib.acimg_split_plane_bytes(rows, Cc), lib.acimg_split_plane_bytes(rows, K)
        head = (C.byref(d), p("x_planes"), lo_x, p("wsplit"))
        if entry in ("conv2d_fwd_split3p", "conv2d_fwd_split1p"):
            return getattr(lib, "acimg_" + entry)(*head, p("y"), A, p("workspace"), q, None)
        if entry == "conv2d_fwd_split3p_stats":
            return lib.acimg_conv2d_fwd_split3p_stats(*head, A, p("workspace"), q, None)
        if entry == "conv2d_fwd_split3p_tail":
            return lib.acimg_conv2d_fwd_split3p_tail(*head, p("scale"), p("shift"), p("shortcut"), lo_y, p("out_planes"), lo_y,
                                                     p("workspace"), q, None)
        return lib.acimg_conv2d_fwd_split3p_tail_proj(*head, p("scale"), p("shift"), p("shortcut"), p("sc_scale"), p("sc_shift"),
                                                      p("out_planes"), lo_y, p("workspace"), q, None)
    # the prepare calls
    shape = of.SPLIT_CASES[row][0]
    N, H, W, Cc, K = shape[:5]
    d = ops.conv_desc(*shape, ldx=ld("ldx", Cc, Cc), ldw=ld("ldw", K, K))
    if entry == "conv2d_split3_prepare_multi":
        for mode in (0, 1, 2):
            descs = (C.POINTER(type(d)) * 1)(C.pointer(d))
            ws, outs, modes = (C.c_void_p * 1)(p("w")), (C.c_void_p * 1)(p("wsplit")), (C.c_int * 1)(mode)
            rc = lib.acimg_conv2d_split3_prepare_multi(1, descs, ws, outs, modes, None)
            if rc != of.EINVAL:
                return rc
        return rc
    return getattr(lib, "acimg_" + entry)(C.byref(d), p("w"), p("wsplit"), None)


CODES = {of.OK: "ACIMG_OK", of.EINVAL: "ACIMG_EINVAL", of.EWORKSPACE: "ACIMG_EWORKSPACE", of.ELAUNCH: "ACIMG_ELAUNCH (reached a launch)"}


@pytest.mark.parametrize("entry", list(of.ENTRIES))
def test_odd_operand_forms_are_refused_by_name_before_any_launch(lib, entry):
    from acimg import _lib
    table = of.refusals(entry)
    assert table, entry
    failed = []
    for row, operand, form, code, word in table:
        rc = _conv_call(lib, entry, row, Odd(operand, form))
        text = _lib.last_error() if rc else ""
        # (a misplaced pointer, and every form a promised route refuses, is reported as a matter of alignment)
        outputs = of.ENTRIES[entry][3] + of.ENTRIES[entry][4]
        aligned = code != of.EINVAL or not (form == "+4" or operand in outputs) or "aligned" in text
        # the name as a word of its own: "w" is not named by "workspace", nor "x" by "exceeds"
        named = re.search(r"(?<![A-Za-z0-9_])%s(?![A-Za-z0-9_])" % re.escape(word), text) is not None
        if rc != code or not named or not aligned:
            failed.append("%s[%s] %s %s: %s (%r), expected %s naming %r" % (entry, row, operand, form, CODES.get(rc, rc), text,
                                                                            CODES[code], word))
    assert not failed, "%d of %d forms:\n%s" % (len(failed), len(table), "\n".join(failed))


def test_every_entry_point_and_every_row_is_walked():
    """the table reaches every convolution-family entry point that takes tensors, and every row of the shape tables"""
    import os
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "acimg.h")).read()
    declared = set(re.findall(r"\bint acimg_((?:conv2d|deconv)_[a-z0-9_]+)\s*\(", hdr))
    queries = {n for n in declared if n.endswith(("_stats_rows", "_tiling", "_affine_input_ok"))}
    assert declared - queries == set(of.ENTRIES), (declared - queries) ^ set(of.ENTRIES)
    seen = {(e, r) for e in of.ENTRIES for r, _ in of.entry_rows(e)}
    for e, tab in (("conv2d_fwd", FWD_CASES), ("conv2d_dgrad", DGRAD_CASES), ("deconv_fwd", DECONV_CASES)):
        assert all((e, r) in seen for r in tab)
    assert {r for e, r in seen if e.startswith("conv2d_wgrad")} == set(WGRAD_CASES)
    # the narrow-halo data gradient: every odd form of dx / residual / mask is ACIMG_EINVAL naming the operand - not the
    # ACIMG_EWORKSPACE of the route below it
    narrow = [t for t in of.refusals("conv2d_dgrad") if t[0] == "halo16_narrow" and t[1] in ("dx", "residual", "mask")]
    assert len(narrow) == 9 and all(t[3] == of.EINVAL for t in narrow)
