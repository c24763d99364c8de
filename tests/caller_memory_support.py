"""The guard-band runner of the raw C ABI and the per-entry case builders of the convolution family, shared by
tests/test_caller_memory_gpu.py (workspace and output extents) and tests/test_operand_forms_gpu.py (operand forms).

A `Case` is one entry point on one shape: its workspace query, its outputs (`Out`: the memory handed over, pads included, and
which elements of it are documented), the call(s) and the fp64 check.  `run_case` is the full protocol of
test_caller_memory_gpu.py (reference run, guarded run, short runs); `run_guarded` is its guarded run alone, checked against
fp64 directly.  The builders take `forms = {operand: form}` (tests/operand_form_cases.py): the operand is then carved out of
its region one float past a 16-byte boundary ("+4") or with the smallest legal leading dimension plus 1 or 2 ("ld+1",
"ld+2"); without it every operand has the form the builders always used.  The fp64 problem of a row (inputs and reference)
is computed once per process and never written to."""
import ctypes as C
import functools
from collections import OrderedDict
from types import SimpleNamespace

import numpy as np
import torch
import torch.nn.functional as F

from caller_memory_cases import DECONV_CASES, DGRAD_CASES, FWD_CASES, RTOL, WGRAD_CASES
from guard_arena import CANARY, GuardArena
from op_support import close_at, conv_geom, raw_lib, tf_conv_ref, up4, widen

STATS_TOL = 2e-4       # ... and its batch-norm partial sums (fp32 sums of many signed terms)
SENT = 0x7B            # 0x7B7B7B7B = 1.3e36 as a float, 2071690107 as an int: finite, never a result
WS_FILL = 0xFF         # NaN in every float format
close = close_at(RTOL, show=True)
# form -> (floats past a 16-byte boundary, floats added to the smallest legal leading dimension)
FORMS = {None: (0, 0), "+4": (1, 0), "ld+1": (0, 1), "ld+2": (0, 2)}


def f32(g, *shape, scale=1.0):
    return (torch.randn(*shape, generator=g, dtype=torch.float64) * scale).float()


def last_lt(shape, n):
    """mask of the documented elements of a [..., ld] buffer: the first n of every row"""
    return (torch.arange(shape[-1]) < n).expand(*shape)


def first_lt(shape, n):
    m = torch.zeros(*shape, dtype=torch.bool)
    m[:n] = True
    return m


class Out(object):
    """an output buffer: dtype, full shape of the memory handed over (pads included), mask of the documented elements
    (None: all), init = a sentinel byte, or a tensor for in/out buffers the caller must initialise (accumulators)"""

    def __init__(self, dtype, shape, mask=None, init=SENT):
        self.dtype, self.shape, self.mask, self.init = dtype, tuple(int(s) for s in shape), mask, init
        self.nbytes = int(np.prod(self.shape)) * torch.empty((), dtype=dtype).element_size() if self.shape else 0

    def paint(self, u8):
        if isinstance(self.init, torch.Tensor):
            u8.copy_(self.init.contiguous().view(-1).view(torch.uint8).to(u8.device))
        else:
            u8.fill_(self.init)

    def typed(self, u8):
        return u8.cpu().view(self.dtype).view(*self.shape)


class Case(object):
    """calls: [fn(ws_ptr, ws_bytes, ptr, tickets_ptr) -> rc], run in order (state carried through the workspace:
    triplet fwd + bwd); verify(outs): the fp64 check; zero_head: leading workspace bytes the header wants zero before
    the first call; zero_exit: leading bytes (ticket words) it promises to leave zero after every call; short_code: the
    code a short workspace must be refused with (None: any negative code, or a legal fallback), null_code: the same for
    ws = NULL where the entry point names that another way; fallback: the entry point documents another kernel (another
    summation order) for a short or missing workspace - only then may a short run that returns 0 differ in bits from the
    reference run, and it must pass the fp64 check instead"""

    def __init__(self, query, outs, calls, verify, tickets=False, zero_head=0, zero_exit=0, short_code=None, null_code=None,
                 fallback=False, keep=None):
        self.query, self.outs, self.verify = int(query), outs, verify
        self.calls = calls if isinstance(calls, (list, tuple)) else [calls]
        self.tickets, self.zero_head, self.zero_exit, self.keep = tickets, int(zero_head), int(zero_exit), keep
        self.short_code, self.null_code = short_code, short_code if null_code is None else null_code
        self.fallback = fallback


def _bits(t):
    return t.contiguous().view(-1).view(torch.uint8)


class Guarded(object):
    """a case's workspace (exactly the queried bytes), outputs and tickets as regions of one guard arena"""

    def __init__(self, device, case, what):
        from acimg import ops
        self.case, self.what = case, what
        self.tbytes = 4 * ops.TICKET_WORDS
        q = case.query
        sizes = [q] + [o.nbytes for o in case.outs.values()] + ([self.tbytes] if case.tickets else [])
        self.arena = GuardArena.for_sizes(device, sizes)
        self.wsr = self.arena.region(q, name="workspace")
        self.regs = OrderedDict((n, self.arena.region(o.nbytes, name=n)) for n, o in case.outs.items())
        self.tr = self.arena.region(self.tbytes, fill=0, name="tickets") if case.tickets else None
        self.ptr = {n: r.ptr for n, r in self.regs.items()}
        self.tick = self.tr.ptr if self.tr is not None else None

    def paint(self, short=False):
        case, q = self.case, self.case.query
        self.wsr.fill(WS_FILL)
        if case.zero_head:
            self.wsr.u8[:case.zero_head].zero_()
        if short:
            self.wsr.u8[q - 16:].fill_(CANARY)
        for n, o in case.outs.items():
            o.paint(self.regs[n].u8)
        if self.tr is not None:
            self.tr.fill(0)

    def outputs(self):
        return OrderedDict((n, o.typed(self.regs[n].u8)) for n, o in self.case.outs.items())

    def untouched(self, got, stage, everything):
        """sentinel bytes: outside the documented elements, or (a refused call) everywhere"""
        for n, o in self.case.outs.items():
            if isinstance(o.init, torch.Tensor):
                if everything:
                    assert torch.equal(_bits(got[n]), _bits(o.init)), "%s, %s: %s changed by a refused call" % (self.what, stage, n)
                continue
            if everything or o.mask is not None:
                sel = got[n] if everything else got[n][~o.mask]
                bad = _bits(sel).ne(o.init)
                assert not bool(bad.any()), "%s, %s: output %r written outside its documented extent (%d bytes)" % (
                    self.what, stage, n, int(bad.sum()))

    def tickets_zero(self, stage):
        if self.tr is not None:
            assert not bool(self.tr.u8.any()), "%s, %s: tickets left non-zero" % (self.what, stage)


def _launch(case, what, ws_ptr, ws_bytes, ptr, tick, arena=None, stage=""):
    """every call of the case; one synchronize + arena check per call; stops at the first refusal"""
    for i, fn in enumerate(case.calls):
        rc = fn(ws_ptr, ws_bytes, ptr, tick)
        torch.cuda.synchronize()
        if arena is not None:
            arena.check("%s, %s, call %d" % (what, stage, i))
        if rc != 0:
            return rc
    return 0


def run_guarded(device, case, what):
    """ONE call through the raw C ABI with exactly the queried workspace (poisoned) and every output inside guard bands,
    pre-filled with the sentinel: rc == 0, the documented elements pass the case's fp64 check, every other byte of every
    output region still holds the sentinel, all guard bands are intact, tickets zero"""
    m, L = raw_lib()
    G = Guarded(device, case, what)
    G.paint()
    rc = _launch(case, what, G.wsr.ptr, case.query, G.ptr, G.tick, G.arena, "guarded run")
    assert rc == 0, "%s: guarded run (ws = the query, %d bytes) rc=%d: %s" % (what, case.query, rc, m.last_error())
    got = G.outputs()
    case.verify(got)
    G.untouched(got, "guarded run", False)
    G.tickets_zero("guarded run")
    if case.zero_exit:
        assert not bool(G.wsr.u8[:case.zero_exit].any()), "%s: zero-on-exit words of the workspace left non-zero" % what
    return got


def run_case(device, case, what):
    from acimg import ops
    m, L = raw_lib()
    q = case.query

    # ---- reference run: roomy, zeroed workspace; plain tensors ---------------------------------------------------------
    ws = torch.zeros(4 * q + (1 << 20), dtype=torch.uint8, device=device)
    bufs = OrderedDict((n, torch.empty(max(o.nbytes, 16), dtype=torch.uint8, device=device)) for n, o in case.outs.items())
    for n, o in case.outs.items():
        o.paint(bufs[n][:o.nbytes])
    tick = torch.zeros(ops.TICKET_WORDS, dtype=torch.int32, device=device) if case.tickets else None
    rc = _launch(case, what, ws.data_ptr(), ws.numel(), {n: b.data_ptr() for n, b in bufs.items()},
                 tick.data_ptr() if case.tickets else None)
    assert rc == 0, "%s: reference run rc=%d: %s" % (what, rc, m.last_error())
    ref = OrderedDict((n, o.typed(bufs[n][:o.nbytes])) for n, o in case.outs.items())
    case.verify(ref)
    if case.tickets:
        assert int(tick.abs().max()) == 0, "%s: reference run left tickets non-zero" % what
    del ws, bufs

    # ---- guarded run: exactly the queried bytes, poisoned; outputs between guard bands ---------------------------------
    G = Guarded(device, case, what)
    arena, wsr, ptr = G.arena, G.wsr, G.ptr

    def same_as_reference(got, stage):
        for n, o in case.outs.items():
            a = got[n] if o.mask is None else got[n][o.mask]
            b = ref[n] if o.mask is None else ref[n][o.mask]
            if not torch.equal(_bits(a), _bits(b)):
                return False, n
        return True, None

    G.paint()
    rc = _launch(case, what, wsr.ptr, q, ptr, G.tick, arena, "guarded run")
    assert rc == 0, "%s: guarded run (ws = the query, %d bytes) rc=%d: %s" % (what, q, rc, m.last_error())
    got = G.outputs()
    ok, n = same_as_reference(got, "guarded run")
    assert ok, "%s: output %r differs between a zeroed roomy workspace and a poisoned exact one" % (what, n)
    G.untouched(got, "guarded run", False)
    G.tickets_zero("guarded run")
    if case.zero_exit:
        assert not bool(wsr.u8[:case.zero_exit].any()), "%s: zero-on-exit words of the workspace left non-zero" % what

    # ---- short runs: query - 16 bytes, then no workspace at all -------------------------------------------------------
    if q > 0:
        assert q >= 16, "%s: a query of %d bytes leaves no 16 bytes to cut" % (what, q)
        for stage, p, nb in (("short run (query - 16)", wsr.ptr, q - 16), ("NULL workspace", None, 0)):
            G.paint(short=True)
            rc = _launch(case, what, p, nb, ptr, G.tick, arena, stage)
            assert bool((wsr.u8[q - 16:] == CANARY).all()), "%s, %s: the 16 bytes past ws_bytes were written" % (what, stage)
            got = G.outputs()
            if rc < 0:
                print("%s, %s: refused rc=%d (%s)" % (what, stage, rc, m.last_error()))
                want = case.short_code if p is not None else case.null_code
                if want is not None:
                    assert rc == want, (what, stage, rc, want)
                G.untouched(got, stage, True)
            else:
                assert rc == 0 and case.short_code is None, (what, stage, rc)
                ok, n = same_as_reference(got, stage)
                assert ok or case.fallback, "%s, %s: rc == 0 but output %r differs from the reference run" % (what, stage, n)
                if not ok:       # a declared fallback kernel (for the loss sums the float atomics the header documents for a
                    # call without scratch): the reference run's own fp64 check at the op's existing tolerance
                    print("%s, %s: fallback path, %r not bit-identical; fp64 check" % (what, stage, n))
                    case.verify(got)
                G.untouched(got, stage, False)
            G.tickets_zero(stage)
            if case.zero_exit and p is not None:        # "left zero by every call": accepted or refused
                assert not bool(wsr.u8[:min(case.zero_exit, nb)].any()), "%s, %s: zero-on-exit words left non-zero" % (what, stage)
    return ref


# =====================================================================================================================
# operand forms
# =====================================================================================================================
def operand_form(forms, name, channels, ld):
    """(floats past a 16-byte boundary, leading dimension) of operand `name` under forms = {operand: form}; "ld+n" counts
    from the smallest legal leading dimension, the channel count; an operand without a form keeps `ld`"""
    off, extra = FORMS[(forms or {}).get(name)]
    return off, (channels + extra) if extra else ld


def pixel_out(pix, ch, ld, off=0):
    """the output [*pix][ch] with pixel stride ld, its first element `off` floats into its (256-byte aligned) region ->
    (Out, documented(t): the [*pix][ch] elements of the typed region).  Everything else of the region - the floats before
    the offset, the ld - ch floats after every pixel, the tail - must keep the sentinel"""
    pix = tuple(int(v) for v in pix)
    if not off:
        shape = pix + (ld,)
        return Out(torch.float32, shape, last_lt(shape, ch)), (lambda t: t[..., :ch])
    n = int(np.prod(pix))
    total = off + n * ld + 3
    mask = torch.zeros(total, dtype=torch.bool)
    mask[off:off + n * ld].view(n, ld)[:, :ch] = True
    return Out(torch.float32, (total,), mask), (lambda t: t[off:off + n * ld].view(*(pix + (ld,)))[..., :ch])


def place(t, ld, off, device):
    """the input operand t [..., ch] on the device with pixel stride ld, its first element `off` floats past a 16-byte
    boundary, NaN everywhere else -> (the tensor that owns the memory, the operand's address)"""
    ch = t.shape[-1]
    n = t.numel() // ch
    buf = torch.full((off + n * ld + 3,), float("nan"), dtype=torch.float32)
    buf[off:off + n * ld].view(n, ld)[:, :ch] = t.reshape(n, ch).float()
    buf = buf.to(device)
    assert buf.data_ptr() % 16 == 0
    return buf, buf.data_ptr() + 4 * off


# =====================================================================================================================
# convolution family
# =====================================================================================================================
def conv_inputs(case, seed, wscale=0.1):
    N, H, W, Cc, K, R, S, stride, padding = case
    g = torch.Generator().manual_seed(seed)
    OH, OW, pads = conv_geom(H, W, R, S, stride, padding)
    x, w, b = f32(g, N, H, W, Cc), f32(g, R, S, Cc, K, scale=wscale), f32(g, K)
    gy, res, mask = f32(g, N, OH, OW, K), f32(g, N, H, W, Cc), f32(g, N, H, W, Cc)
    return g, OH, OW, pads, x, w, b, gy, res, mask


@functools.lru_cache(maxsize=None)
def fwd_problem(name):
    """inputs and fp64 reference of a forward row (conv + bias before the activation: raw), computed once"""
    shape, act, with_stats, branch, tol = FWD_CASES[name]
    N, H, W, Cc, K, R, S, stride, padding = shape
    g, OH, OW, pads, x, w, b, _, _, _ = conv_inputs(shape, 11 + sum(v for v in shape if isinstance(v, int)),
                                                    wscale=0.05 if branch == "skinny" else (2.0 / (R * S * Cc)) ** 0.5)
    raw = tf_conv_ref(x.double(), w.double(), stride, pads, b.double())
    return SimpleNamespace(OH=OH, OW=OW, x=x, w=w, b=b, raw=raw, yref=torch.relu(raw) if act else raw)


def fwd_case(device, name, configure=None, forms=None, stats=None):
    """stats: None = as the table says; False = without the statistics buffer"""
    from acimg import ops
    m, L = raw_lib()
    shape, act, with_stats, branch, tol = FWD_CASES[name]
    if stats is not None:
        with_stats = stats
    N, H, W, Cc, K, R, S, stride, padding = shape
    P = fwd_problem(name)
    OH, OW, raw, yref = P.OH, P.OW, P.raw, P.yref
    yoff, ldy = operand_form(forms, "y", K, K + 4)
    boff, _ = operand_form(forms, "bias", K, K)
    d = ops.conv_desc(N, H, W, Cc, K, R, S, stride, padding, ldy=ldy, act=act)
    til = ops.conv2d_fwd_tiling(d)
    q = int(L.acimg_conv2d_fwd_workspace(C.byref(d)))
    if branch.startswith("splitk"):
        assert til[2] > 1 and q > 0
    elif branch == "unsplit":
        assert til[2] == 1 and q == 0
    elif branch == "256x16":
        assert til[:2] == (256, 16) and til[2] > 1
    elif branch == "few16":
        assert ops.conv2d_stats_rows(d) == 512 and ops.conv2d_affine_input_ok(d, 0)
    elif branch == "direct":
        assert ops.conv2d_stats_rows(d) == -(-N * OH * OW // 256) and not ops.conv2d_affine_input_ok(d, 0)
    xd, wd = P.x.to(device), P.w.to(device)
    bd, bptr = place(P.b, K, boff, device)
    rows = ops.conv2d_stats_rows(d)
    yout, ydoc = pixel_out((N, OH, OW), K, ldy, yoff)
    outs = OrderedDict(y=yout)
    if with_stats:
        outs["stats"] = Out(torch.float32, (rows + 3, 2, d.ldw), first_lt((rows + 3, 2, d.ldw), rows))
    # the few-channel direct kernel takes neither an odd y nor an odd bias: those forms run on the implicit GEMM
    direct = branch == "direct" and not forms

    def call(ws, nb, p, tick):
        return L.acimg_conv2d_fwd(C.byref(d), xd.data_ptr(), wd.data_ptr(), bptr, p["y"] + 4 * yoff, None, None, 0,
                                  p.get("stats"), ws, nb, tick if branch.endswith("tickets") else None,
                                  ops.current_stream_handle(device))

    def verify(o):
        close(ydoc(o["y"]), yref, tol=tol if not forms else max(tol, RTOL), what="conv2d_fwd %s" % name)
        if with_stats:
            # the implicit-GEMM epilogue sums conv + bias BEFORE the activation; the few-channel direct kernel with an
            # activation leaves its statistics to a pass over the stored (activated) tensor (include/acimg.h; the same
            # thing with ACIMG_ACT_NONE, which every batch-norm layer uses)
            flat = (yref if act and direct else raw).reshape(-1, K)
            close(o["stats"][:rows, 0, :K].sum(0), flat.sum(0), tol=STATS_TOL, what="conv2d_fwd %s stats sum" % name)
            close(o["stats"][:rows, 1, :K].sum(0), (flat * flat).sum(0), tol=STATS_TOL, what="conv2d_fwd %s stats sumsq" % name)
    # skinny: without its full workspace the dense layer runs as a split-K implicit GEMM (another summation order)
    return Case(q, outs, call, verify, tickets=branch.endswith("tickets"), fallback=branch == "skinny", keep=(xd, wd, bd, d))


@functools.lru_cache(maxsize=None)
def dgrad_problem(name):
    shape, with_res, with_mask, tickets, tol = DGRAD_CASES[name]
    N, H, W, Cc, K, R, S, stride, padding = shape
    small = name in ("halo16_narrow", "few_channel_stride2", "few_channel_stride1", "dilated_then_igemm_65536")
    g, OH, OW, pads, x, w, b, gy, res, mask = conv_inputs(shape, 5 + sum(v for v in shape if isinstance(v, int)),
                                                          wscale=0.05 if name == "skinny" else 0.1)
    if small:
        gy, res = gy * 1e-3, res * 1e-3          # gradients of the size the bf16x3 forms were made for (fp16 would lose them)
    xr = x.double().requires_grad_(True)
    y = tf_conv_ref(xr, w.double(), stride, pads)
    (gx,) = torch.autograd.grad(y, (xr,), gy.double())
    ref = gx + (res.double() if with_res else 0)
    if with_mask:
        ref = ref * (mask > 0).double()
    return SimpleNamespace(w=w, gy=gy, res=res, mask=mask, ref=ref)


def dgrad_case(device, name, forms=None):
    from acimg import ops
    m, L = raw_lib()
    shape, with_res, with_mask, tickets, tol = DGRAD_CASES[name]
    N, H, W, Cc, K, R, S, stride, padding = shape
    P = dgrad_problem(name)
    ref = P.ref
    ldgy = K + 4
    xoff, lddx = operand_form(forms, "dx", Cc, Cc + 4)
    roff, ldres = operand_form(forms, "residual", Cc, Cc + 8)
    moff, ldmask = operand_form(forms, "mask", Cc, Cc + 4)
    d = ops.conv_desc(N, H, W, Cc, K, R, S, stride, padding, ldw=K)
    q = int(L.acimg_conv2d_dgrad_workspace(C.byref(d)))
    gyd, wd = widen(P.gy, ldgy).to(device), P.w.to(device)
    resd, rptr = place(P.res, ldres, roff, device)
    maskd, mptr = place(P.mask, ldmask, moff, device)
    dxout, dxdoc = pixel_out((N, H, W), Cc, lddx, xoff)
    outs = OrderedDict(dx=dxout)

    def call(ws, nb, p, tick):
        return L.acimg_conv2d_dgrad(C.byref(d), gyd.data_ptr(), ldgy, wd.data_ptr(), p["dx"] + 4 * xoff, lddx,
                                    rptr if with_res else None, ldres, mptr if with_mask else None,
                                    ldmask, ws, nb, tick if tickets else None, ops.current_stream_handle(device))

    def verify(o):
        close(dxdoc(o["dx"]), ref, tol=tol if not forms else max(tol, RTOL), what="conv2d_dgrad %s" % name)
    return Case(q, outs, call, verify, tickets=tickets, keep=(gyd, wd, resd, maskd, d))


@functools.lru_cache(maxsize=None)
def wgrad_problem(name):
    """inputs and the library-independent fp64 reference of a weight-gradient row (bf16: fp64 of the ROUNDED operands;
    affine: of the materialised relu(x * scale + shift))"""
    shape, entry, tol = WGRAD_CASES[name]
    N, H, W, Cc, K, R, S, stride, padding = shape
    g, OH, OW, pads, x, w, b, gy, _, _ = conv_inputs(shape, 3 + sum(v for v in shape if isinstance(v, int)))
    if name != "skinny":
        gy = gy * 1e-2
    P = SimpleNamespace(x=x, gy=gy, scale=None, shift=None)
    wz = torch.zeros(R, S, Cc, K, dtype=torch.float64, requires_grad=True)
    if entry.startswith("affine"):
        P.scale, P.shift = (torch.rand(Cc, generator=g) + 0.5).float(), f32(g, Cc, scale=0.5)
        yr = tf_conv_ref(torch.relu(x.double() * P.scale.double() + P.shift.double()), wz, stride, pads)
        (P.gw,) = torch.autograd.grad(yr, (wz,), gy.double())
        P.gb = gy.double().sum((0, 1, 2))
    else:
        rnd_ = (lambda t: t.to(torch.bfloat16).double()) if entry == "bf16" else (lambda t: t.double())
        yr = tf_conv_ref(rnd_(x), wz, stride, pads)
        (P.gw,) = torch.autograd.grad(yr, (wz,), rnd_(gy))
        P.gb = rnd_(gy).sum((0, 1, 2))
    return P


def wgrad_case(device, name, forms=None):
    from acimg import ops
    m, L = raw_lib()
    shape, entry, tol = WGRAD_CASES[name]
    N, H, W, Cc, K, R, S, stride, padding = shape
    P = wgrad_problem(name)
    x, gy = P.x, P.gy
    kp = up4(K)
    ldw, ldgy = kp + 4, kp + 4
    d = ops.conv_desc(N, H, W, Cc, K, R, S, stride, padding, ldw=ldw)
    q = int(L.acimg_conv2d_wgrad_workspace(C.byref(d)))
    affine = entry.startswith("affine")
    prec = int(entry[-1]) if affine else 0
    if affine:
        assert ops.conv2d_affine_input_ok(d, prec)
        scd, shd = P.scale.to(device), P.shift.to(device)
    xd = x.to(device)
    gyd = widen(gy, ldgy, fill=0.0).to(device)           # columns K .. kp are operands (zero); beyond kp never read
    gyd[..., kp:] = float("nan")
    st = ops.current_stream_handle(device)
    if affine:
        # the reference of the existing test: the SAME entry family on the materialised tensor (roomy zeroed workspace)
        xmat = torch.relu(xd * scd + shd)
        rws = torch.zeros(4 * q + (1 << 20), dtype=torch.uint8, device=device)
        rdw = torch.zeros(R, S, Cc, ldw, device=device)
        rdb = torch.zeros(ldw, device=device)
        fn = L.acimg_conv2d_wgrad_split3 if prec == 1 else L.acimg_conv2d_wgrad
        m.check(fn(C.byref(d), xmat.data_ptr(), gyd.data_ptr(), ldgy, rdw.data_ptr(), rdb.data_ptr(), rws.data_ptr(),
                   rws.numel(), st), "reference wgrad")
        torch.cuda.synchronize()
        gw, gb = rdw[..., :K].cpu().double(), rdb[:K].cpu().double()
        del rws, xmat
        # ... and, independent of the library, fp64 of the same product at the tolerance of the non-affine case on the same
        # kernel (halo16_split3: 4e-5, few_channel_halo: 2e-5)
        gw64, gb64, tol64 = P.gw, P.gb, 4e-5 if prec == 1 else 2e-5
    else:
        gw, gb = P.gw, P.gb
    # columns [K, kp) are the zero padding of the GEMM (written, zero); [kp, ldw) is outside the layer: untouched
    boff, _ = operand_form(forms, "db", kp, ldw)
    dbout, dbdoc = pixel_out((), kp, ldw, boff)
    outs = OrderedDict(dw=Out(torch.float32, (R, S, Cc, ldw), last_lt((R, S, Cc, ldw), kp)), db=dbout)
    ftol = tol if not forms else max(tol, RTOL)

    def call(ws, nb, p, tick):
        if affine:
            return L.acimg_conv2d_wgrad_affine(C.byref(d), prec, xd.data_ptr(), scd.data_ptr(), shd.data_ptr(), 1, gyd.data_ptr(),
                                               ldgy, p["dw"], p["db"] + 4 * boff, ws, nb, st)
        fn = {"f32": L.acimg_conv2d_wgrad, "split3": L.acimg_conv2d_wgrad_split3, "bf16": L.acimg_conv2d_wgrad_bf16}[entry]
        return fn(C.byref(d), xd.data_ptr(), gyd.data_ptr(), ldgy, p["dw"], p["db"] + 4 * boff, ws, nb, st)

    def verify(o):
        db = dbdoc(o["db"])
        close(o["dw"][..., :K], gw, tol=ftol, what="conv2d_wgrad %s" % name)
        close(db[:K], gb, tol=ftol, what="conv2d_wgrad %s bias gradient" % name)
        if affine:
            close(o["dw"][..., :K], gw64, tol=tol64, what="conv2d_wgrad %s against fp64" % name)
            close(db[:K], gb64, tol=tol64, what="conv2d_wgrad %s bias gradient against fp64" % name)
        assert float(o["dw"][..., K:kp].abs().max() if kp > K else 0.0) == 0.0
    return Case(q, outs, call, verify, keep=(xd, gyd, d))


@functools.lru_cache(maxsize=None)
def deconv_problem(name):
    shape, tol_f, tol_d, tol_w = DECONV_CASES[name]
    N, H, W, Cc, K, R, S, s = shape
    g = torch.Generator().manual_seed(77 + N + Cc)
    x, w, b = f32(g, N, H, W, Cc), f32(g, R, S, K, Cc, scale=0.1), f32(g, K)
    xr, wr = x.double().requires_grad_(True), w.double().requires_grad_(True)
    y = F.conv_transpose2d(xr.permute(0, 3, 1, 2), wr.permute(3, 2, 0, 1), b.double(), stride=s,
                           output_padding=(max(s - R, 0), max(s - S, 0))).permute(0, 2, 3, 1)
    OH, OW = int(y.shape[1]), int(y.shape[2])
    gy = f32(g, N, OH, OW, K)
    gxr, gwr = torch.autograd.grad(y, (xr, wr), gy.double())
    mask = f32(g, N, H, W, Cc)
    return SimpleNamespace(x=x, w=w, b=b, y=y.detach(), gy=gy, gxr=gxr, gwr=gwr, mask=mask)


def deconv_cases(device, name, forms=None):
    """(forward, data gradient, weight gradient) of a transposed-conv row; forms name y / bias (forward), dx / mask (data
    gradient), db (weight gradient)"""
    from acimg import ops
    m, L = raw_lib()
    shape, tol_f, tol_d, tol_w = DECONV_CASES[name]
    N, H, W, Cc, K, R, S, s = shape
    P = deconv_problem(name)
    y, gy, mask = P.y, P.gy, P.mask
    ldgy = 2 * K
    yoff, ldy = operand_form(forms, "y", K, 2 * K)
    boff, _ = operand_form(forms, "bias", K, K)
    xoff, _ = operand_form(forms, "dx", Cc, Cc)
    moff, ldmask = operand_form(forms, "mask", Cc, Cc)
    dboff, _ = operand_form(forms, "db", K, K)
    if forms:
        tol_f, tol_d, tol_w = max(tol_f, RTOL), max(tol_d, RTOL), max(tol_w, RTOL)
    d = ops.deconv_desc(N, H, W, Cc, K, R, S, s, ldy=ldy)
    OH, OW = d.OH, d.OW
    assert tuple(y.shape[1:3]) == (OH, OW)
    with_mask = name != "direct_dgrad"
    q = int(L.acimg_deconv_workspace(C.byref(d)))
    xd, wd, gyd = P.x.to(device), P.w.to(device), widen(gy, ldgy).to(device)
    bd, bptr = place(P.b, K, boff, device)
    maskd, mptr = place(mask, ldmask, moff, device)
    st = ops.current_stream_handle(device)
    keep = (xd, wd, bd, gyd, maskd, d)
    yout, ydoc = pixel_out((N, OH, OW), K, ldy, yoff)
    fwd = Case(q, OrderedDict(y=yout),
               lambda ws, nb, p, tick: L.acimg_deconv_fwd(C.byref(d), xd.data_ptr(), wd.data_ptr(), bptr, p["y"] + 4 * yoff, ws, nb, tick, st),
               lambda o: close(ydoc(o["y"]), y, tol=tol_f, what="deconv_fwd %s" % name), tickets=True, keep=keep)
    dref = P.gxr * (mask > 0).double() if with_mask else P.gxr
    dxout, dxdoc = pixel_out((N, H, W), Cc, Cc, xoff)
    dgr = Case(q, OrderedDict(dx=dxout),
               lambda ws, nb, p, tick: L.acimg_deconv_dgrad(C.byref(d), gyd.data_ptr(), ldgy, wd.data_ptr(), p["dx"] + 4 * xoff,
                                                            mptr if with_mask else None, ldmask, ws, nb, tick, st),
               lambda o: close(dxdoc(o["dx"]), dref, tol=tol_d, what="deconv_dgrad %s" % name), tickets=True, keep=keep)
    dbout, dbdoc = pixel_out((), K, K, dboff)

    def verify_w(o):
        close(o["dw"], P.gwr, tol=tol_w, what="deconv_wgrad %s" % name)
        close(dbdoc(o["db"]), gy.double().sum((0, 1, 2)), tol=tol_w, what="deconv_wgrad %s bias gradient" % name)
    wgr = Case(q, OrderedDict(dw=Out(torch.float32, (R, S, K, Cc)), db=dbout),
               lambda ws, nb, p, tick: L.acimg_deconv_wgrad(C.byref(d), xd.data_ptr(), gyd.data_ptr(), ldgy, p["dw"],
                                                            p["db"] + 4 * dboff, ws, nb, st),
               verify_w, keep=keep)
    return fwd, dgr, wgr


# ---------------------------------------------------------------------------------------------------------------------
# the on-the-fly split entries (acimg_conv2d_fwd_split3 / _dgrad_split3): no workspace; weights prepared through the raw ABI
# ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def split_problem(shape):
    """a 3x3 / stride-1 / SAME layer: inputs, fp64 forward (conv + bias) and fp64 data gradient (+ residual, masked)"""
    N, H, W, Cc, K, R, S, stride, padding = shape
    g, OH, OW, pads, x, w, b, gy, res, mask = conv_inputs(shape, 23 + sum(v for v in shape if isinstance(v, int)),
                                                          wscale=(2.0 / (R * S * Cc)) ** 0.5)
    gy, res = gy * 1e-3, res * 1e-3
    xr = x.double().requires_grad_(True)
    y = tf_conv_ref(xr, w.double(), stride, pads)
    (gx,) = torch.autograd.grad(y, (xr,), gy.double())
    return SimpleNamespace(x=x, w=w, b=b, gy=gy, res=res, mask=mask, y=y.detach() + b.double(),
                           dx=(gx + res.double()) * (mask > 0).double())


def split_fwd_case(device, shape, tol, forms=None):
    """acimg_conv2d_fwd_split3 (f16x3): y / bias in the given forms"""
    from acimg import ops
    m, L = raw_lib()
    N, H, W, Cc, K, R, S, stride, padding = shape
    P = split_problem(shape)
    yoff, ldy = operand_form(forms, "y", K, K + 4)
    boff, _ = operand_form(forms, "bias", K, K)
    d = ops.conv_desc(N, H, W, Cc, K, R, S, stride, padding, ldy=ldy)
    st = ops.current_stream_handle(device)
    xd, wd = P.x.to(device), P.w.to(device)
    img = torch.zeros(ops.conv2d_split3_weight_bytes(d), dtype=torch.uint8, device=device)
    m.check(L.acimg_conv2d_split3_prepare(C.byref(d), wd.data_ptr(), img.data_ptr(), st), "prepare")
    bd, bptr = place(P.b, K, boff, device)
    yout, ydoc = pixel_out((N, H, W), K, ldy, yoff)
    return Case(0, OrderedDict(y=yout),
                lambda ws, nb, p, tick: L.acimg_conv2d_fwd_split3(C.byref(d), xd.data_ptr(), img.data_ptr(), bptr, p["y"] + 4 * yoff,
                                                                  None, None, 0, None, st),
                lambda o: close(ydoc(o["y"]), P.y, tol=max(tol, RTOL) if forms else tol, what="conv2d_fwd_split3 %s" % (shape,)),
                keep=(xd, wd, img, bd, d))


def split_dgrad_case(device, shape, tol, forms=None):
    """acimg_conv2d_dgrad_split3 (bf16x3) with residual and mask: dx / residual / mask in the given forms"""
    from acimg import ops
    m, L = raw_lib()
    N, H, W, Cc, K, R, S, stride, padding = shape
    P = split_problem(shape)
    xoff, lddx = operand_form(forms, "dx", Cc, Cc + 4)
    roff, ldres = operand_form(forms, "residual", Cc, Cc + 8)
    moff, ldmask = operand_form(forms, "mask", Cc, Cc + 4)
    d = ops.conv_desc(N, H, W, Cc, K, R, S, stride, padding)
    st = ops.current_stream_handle(device)
    gyd, wd = P.gy.to(device), P.w.to(device)
    img = torch.zeros(ops.conv2d_split3_dgrad_weight_bytes(d), dtype=torch.uint8, device=device)
    m.check(L.acimg_conv2d_split3_prepare_dgrad(C.byref(d), wd.data_ptr(), img.data_ptr(), st), "prepare_dgrad")
    resd, rptr = place(P.res, ldres, roff, device)
    maskd, mptr = place(P.mask, ldmask, moff, device)
    dxout, dxdoc = pixel_out((N, H, W), Cc, lddx, xoff)
    return Case(0, OrderedDict(dx=dxout),
                lambda ws, nb, p, tick: L.acimg_conv2d_dgrad_split3(C.byref(d), gyd.data_ptr(), K, img.data_ptr(), p["dx"] + 4 * xoff,
                                                                    lddx, rptr, ldres, mptr, ldmask, st),
                lambda o: close(dxdoc(o["dx"]), P.dx, tol=max(tol, RTOL) if forms else tol, what="conv2d_dgrad_split3 %s" % (shape,)),
                keep=(gyd, wd, img, resd, maskd, d))
