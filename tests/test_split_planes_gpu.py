"""Consumers and producers of the split-plane activation format (include/acimg.h, "Pre-split activation format") at row
counts that are not multiples of 16.  A plane holds whole 16-row bricks, so the last brick row has pad rows; the model
shares its plane arenas between layers of different shapes, so those rows (and any gap between the hi plane and lo_off)
hold whatever an earlier layer left there.  The format leaves them unspecified; here every consumer runs twice on the same
valid rows - once with zeros around them, once with poison (fp16 NaN, a large finite pattern) - and its results must be
the same bits; one poisoned run of each is also checked against fp64.  Producers must not write outside the two plane
extents.  Finally the model: ResNet50Model with Gram statistics against the statistics pass at a batch whose trunk row
counts are 8 mod 16, on poisoned arenas."""
import pytest
import torch

from op_support import close_at, same_bits, same_pads, trunk_forms
from split_format_ref import POISONS, make_planes, plane_bytes, repack, unsplit, valid_halves

pytestmark = pytest.mark.gpu

SENTINEL = 0xA5
close = close_at(2e-5)           # tests/test_ops_gpu.py RTOL


def sentinel_out(rows, Cc, device, gap=4096, slack=4096):
    """an output buffer for a split-format producer, every byte SENTINEL: (buffer, lo_off)"""
    n = plane_bytes(rows, Cc)
    return torch.full((2 * n + gap + slack,), SENTINEL, dtype=torch.uint8, device=device), n + gap


def assert_extents_only(buf, lo_off, rows, Cc, what):
    """no byte outside [0, plane_bytes) and [lo_off, lo_off + plane_bytes) was written"""
    n = plane_bytes(rows, Cc)
    keep = torch.ones(buf.numel(), dtype=torch.bool, device=buf.device)
    keep[:n] = False
    keep[lo_off:lo_off + n] = False
    bad = int((buf[keep] != SENTINEL).sum())
    assert bad == 0, "%s: %d bytes written outside the plane extents" % (what, bad)


def conv_ref(x, w, R):
    return torch.nn.functional.conv2d(x.double().permute(0, 3, 1, 2), w.double().permute(3, 2, 0, 1),
                                      padding=R // 2).permute(0, 2, 3, 1)


# trunk-kernel forms (as test_ops_gpu.py::test_trunk_kernel_variants_agree forces them) and the kernel each must reach
# (acimg_conv2d_fwd_split3_tiling()[2]: 0 one tile per workgroup, 1 persistent, 2 ring, 3 halo); "auto" is the shipped
# choice.  The forced forms take 128x128 tiles also where the shipped rule would pick 64-row tiles (< 200 tiles).
TILE128 = dict(split3_tile_bm=128, split3_tile_bn=128)
FORMS = trunk_forms("one-tile whole", "persistent whole", "one-tile", "persistent", "ring256", "ring128", "halo") + (
    ("auto", None, None),)


def _halo_fits(W):
    return ((W + 16) >> 4) + 8 + (W >> 4) + 1 <= 18      # csrc/conv_trunk.hip halo_applies: an 18-brick patch


@pytest.mark.parametrize("case", [(7, 28, 38, 128, 512, 1),      # rows % 16 = 8 (the trunk's own residue, N odd)
                                  (7, 56, 75, 64, 256, 1),       # 8
                                  (5, 28, 38, 512, 256, 1),      # 8, 84 tiles
                                  (3, 7, 13, 128, 256, 1),       # 1
                                  (5, 14, 19, 256, 256, 3),      # 2
                                  (37, 5, 3, 32, 128, 3),        # 11: several images per tile
                                  (1, 13, 37, 64, 128, 3),       # 1
                                  (3, 5, 13, 32, 128, 3),        # 3
                                  (1, 9, 39, 64, 128, 3),        # 15
                                  (1, 101, 255, 32, 128, 3)])    # 11: an odd-sized image, too wide for the halo form
def test_trunk_conv_ignores_pad_rows(device, case):
    """acimg_conv2d_fwd_split3p (+ statistics) in every form, and acimg_conv2d_fwd_split1p: fp32 output and statistics rows
    the same bits on zeroed and on poisoned planes; the poisoned runs against fp64"""
    from acimg import _lib, ops

    N, H, W, Cc, K, R = case
    g = torch.Generator().manual_seed(31 + N * H * W + Cc)
    x = torch.rand(N, H, W, Cc, generator=g) - 0.25
    w = torch.randn(R, R, Cc, K, generator=g) * (2.0 / (R * R * Cc)) ** 0.5
    d = ops.conv_desc(N, H, W, Cc, K, R, R, 1, "SAME")
    rows = N * H * W
    assert rows % 16
    plan = ops.Plan(device, eager=True)
    planes, lo = make_planes(plan, device, x, rows, Cc)
    clean, lo_c = repack(planes, lo, rows, Cc, 0)
    dirty = [repack(planes, lo, rows, Cc, fill, gap) for fill, gap in POISONS]
    wsplit = torch.zeros(ops.conv2d_split3_weight_bytes(d), dtype=torch.uint8, device=device)
    ops.conv2d_split3_prepare(plan, d, w.to(device), wsplit)
    tws = torch.zeros(ops.conv2d_fwd_split3p_workspace(d), dtype=torch.uint8, device=device)
    ref = conv_ref(x, w, R)
    xq = (x * 0.25).to(torch.float16).double() * 4.0            # fp16 operand storage: hi planes only
    wq = (w * 1024.0).to(torch.float16).double() / 1024.0
    ref1 = conv_ref(xq, wq, R)

    def run(buf, lo_off, terms, srows):
        y = torch.full((N, H, W, K), float("nan"), device=device)
        # (every statistics row is written by the split3p forms; the split1p row count is an upper bound: zeros)
        st = torch.full((srows, 2, K), float("nan") if terms == 3 else 0.0, device=device)
        ops.conv2d_fwd_split3p(plan, d, buf, lo_off, wsplit, y, st, tail_ws=tws, terms=terms)
        torch.cuda.synchronize()
        assert int(tws[:4096].view(torch.int32).abs().sum()) == 0
        return y, st

    reached = {}
    try:
        forms = [(name, cfg, kind, 3) for name, cfg, kind in FORMS] + [("fp16 operands", None, None, 1)]
        for name, cfg, kind, terms in forms:
            if kind == 3 and not (R == 3 and _halo_fits(W)):
                continue
            _lib.configure(**(dict(TILE128, **cfg) if cfg is not None else {}))
            reached[name] = ops.conv2d_fwd_split3_tiling(d)
            if kind is not None:
                assert reached[name][2] == kind, (name, reached[name])
            if kind == 2:
                assert reached[name][0] == cfg["trunk_ring_bm"], (name, reached[name])
            srows = ops.conv2d_fwd_split3p_stats_rows(d) if terms == 3 else ops.conv2d_fwd_split3_stats_rows(d)
            y0, st0 = run(clean, lo_c, terms, srows)
            for (buf, lo_d), (fill, gap) in zip(dirty, POISONS):
                y, st = run(buf, lo_d, terms, srows)
                what = "%s %s poison 0x%02x gap %d" % (name, case, fill, gap)
                assert same_bits(y, y0), "output depends on pad rows: " + what
                assert same_bits(st, st0), "statistics depend on pad rows: " + what
            # the poisoned run against fp64 (the last one: "identical" must not mean "identically wrong")
            r = ref if terms == 3 else ref1
            close(y, r, tol=2e-6, what="conv " + what)
            close(st[:, 0].sum(0), r.reshape(-1, K).sum(0), tol=2e-4, what="stats sum " + what)
            close(st[:, 1].sum(0), (r.reshape(-1, K) ** 2).sum(0), tol=2e-4, what="stats sumsq " + what)
    finally:
        _lib.configure()
    assert len(reached) == (9 if R == 3 and _halo_fits(W) else 8)


@pytest.mark.parametrize("case", [(7, 28, 38, 128, 512),     # rows % 16 = 8: the 28x38 units at N = 7
                                  (7, 56, 75, 64, 256),      # 8: the 56x75 units
                                  (1, 1, 25617, 128, 256),   # 1
                                  (1, 1, 25603, 64, 256),    # 3
                                  (1, 101, 255, 64, 256),    # 11
                                  (1, 1, 25615, 256, 256)])  # 15
def test_two_pass_and_gram_ignore_pad_rows(device, case):
    """The conv3 path of an identity / projection unit: acimg_gram_stats, acimg_conv2d_fwd_split3p_stats and the fused tails
    (_tail reading its shortcut from planes, _tail_proj) on zeroed and on poisoned input and shortcut planes: scale /
    shift, moving averages, statistics rows and the valid rows of the output planes the same bits, against fp64; the
    tails write nothing outside the two plane extents of their output"""
    from acimg import ops

    N, H, W, Cc, K = case
    rows = N * H * W
    assert rows % 16
    g = torch.Generator().manual_seed(17 + rows + Cc)
    x = torch.relu(torch.randn(rows, Cc, generator=g) + 0.3)
    w = torch.randn(Cc, K, generator=g) * (2.0 / Cc) ** 0.5
    short = torch.rand(rows, K, generator=g) * 2.0 - 0.5
    sc32 = torch.randn(rows, K, generator=g)
    scale, shift = torch.rand(K, generator=g) + 0.5, torch.rand(K, generator=g) - 0.7
    sb, tb = torch.rand(K, generator=g) + 0.5, torch.rand(K, generator=g) - 0.5
    gamma, beta = torch.rand(K, generator=g) + 0.5, torch.rand(K, generator=g) - 0.5
    mm0, mv0 = torch.randn(K, generator=g) * 0.1, torch.rand(K, generator=g) + 0.5
    d = ops.conv_desc(N, H, W, Cc, K, 1, 1, 1, "SAME")
    assert tuple(ops.conv2d_fwd_split3_tiling(d)[:2]) == (128, 128)       # the two-pass gate: >= 200 128x128 tiles
    plan = ops.Plan(device, eager=True)
    xp, lo_x = make_planes(plan, device, x, rows, Cc)
    sp, lo_s = make_planes(plan, device, short, rows, K)
    wd = w.to(device)
    wsplit = torch.zeros(ops.conv2d_split3_weight_bytes(d), dtype=torch.uint8, device=device)
    ops.conv2d_split3_prepare(plan, d, wd.reshape(1, 1, Cc, K).contiguous(), wsplit)
    tws = torch.zeros(ops.conv2d_fwd_split3p_workspace(d), dtype=torch.uint8, device=device)
    gws = torch.zeros(ops.gram_stats_workspace(rows, Cc), dtype=torch.uint8, device=device)
    srows = ops.conv2d_fwd_split3p_stats_rows(d)
    D = lambda t: t.to(device)  # noqa: E731

    def run(fill, gap):
        xq, lq = repack(xp, lo_x, rows, Cc, fill, gap)
        sq, ls = repack(sp, lo_s, rows, K, fill, gap)
        sc, sh = torch.full((K,), float("nan"), device=device), torch.full((K,), float("nan"), device=device)
        mm, mv = D(mm0), D(mv0)
        ops.gram_stats(plan, xq, lq, rows, Cc, wd, K, K, D(gamma), D(beta), mm, mv, sc, sh, gws, decay=0.997, eps=1e-5)
        st = torch.full((srows, 2, K), float("nan"), device=device)
        ops.conv2d_fwd_split3p_stats(plan, d, xq, lq, wsplit, st, tail_ws=tws)
        out_id, lo_o = sentinel_out(rows, K, device)
        ops.conv2d_fwd_split3p_tail(plan, d, xq, lq, wsplit, D(scale), D(shift), sq, ls, out_id, lo_o, tail_ws=tws)
        out_pj, _ = sentinel_out(rows, K, device)
        ops.conv2d_fwd_split3p_tail_proj(plan, d, xq, lq, wsplit, D(scale), D(shift), D(sc32), D(sb), D(tb), out_pj, lo_o,
                                         tail_ws=tws)
        torch.cuda.synchronize()
        assert int(tws[:4096].view(torch.int32).abs().sum()) == 0
        for o, nm in ((out_id, "tail"), (out_pj, "tail_proj")):
            assert_extents_only(o, lo_o, rows, K, "%s %s" % (nm, case))
        return dict(gram=torch.stack([sc, sh, mm, mv]), stats=st, tail=valid_halves(out_id, lo_o, rows, K),
                    tail_proj=valid_halves(out_pj, lo_o, rows, K)), (out_id, out_pj, lo_o)

    r0, _ = run(0, 0)
    for fill, gap in POISONS:
        r, (out_id, out_pj, lo_o) = run(fill, gap)
        what = "%s poison 0x%02x gap %d" % (case, fill, gap)
        for k in r0:
            assert same_bits(r[k], r0[k]), "%s depends on pad rows: %s" % (k, what)
    # the (last) poisoned run against fp64 on the values the planes hold
    xv, sv = unsplit(xp, lo_x, rows, Cc), unsplit(sp, lo_s, rows, K)
    y = xv @ w.double()
    mean, var = y.mean(0), y.var(0, unbiased=False)
    sc, sh, mm, mv = r["gram"].cpu().double()
    close(sc, gamma.double() / torch.sqrt(var + 1e-5), tol=3e-6, what="gram scale " + what)
    close(sh, beta.double() - mean * gamma.double() / torch.sqrt(var + 1e-5), tol=3e-6, what="gram shift " + what)
    close(mm, 0.997 * mm0.double() + 0.003 * mean, tol=2e-6, what="gram moving mean " + what)
    close(mv, 0.997 * mv0.double() + 0.003 * y.var(0, unbiased=True), tol=2e-6, what="gram moving variance " + what)
    close(r["stats"][:, 0].sum(0), y.sum(0), tol=2e-4, what="stats sum " + what)
    close(r["stats"][:, 1].sum(0), (y * y).sum(0), tol=2e-4, what="stats sumsq " + what)
    z = y * scale.double() + shift.double()
    close(unsplit(out_id, lo_o, rows, K), torch.relu(z + sv), tol=2e-6, what="tail " + what)
    close(unsplit(out_pj, lo_o, rows, K), torch.relu(z + sc32.double() * sb.double() + tb.double()), tol=2e-6,
          what="tail_proj " + what)


@pytest.mark.parametrize("case", [(3, 7, 13, 64, 1),      # rows % 16 = 1, shortcut rows the same
                                  (1, 9, 39, 96, 1),      # 15
                                  (3, 5, 13, 32, 2),      # 3, shortcut 3 x 9 x 26 (14)
                                  (37, 5, 3, 128, 2),     # 11, shortcut 37 x 9 x 6 (14)
                                  (7, 14, 19, 256, 2)])   # 10, shortcut 7 x 27 x 38 (6): a 28x38 -> 14x19 unit shape
def test_unit_output_shortcut_from_planes_ignores_pad_rows(device, case):
    """acimg_bn_add_relu_split reading an identity shortcut from split planes (stride 1, or every second pixel of a
    larger tensor): output planes (valid rows) and the fp32 copy the same bits on zeroed and on poisoned shortcut planes,
    against fp64; nothing written outside the output's plane extents"""
    from acimg import ops

    N, OH, OW, Cc, s = case
    BH, BW = (OH, OW) if s == 1 else (2 * OH - 1, 2 * OW)
    rows, prow = N * OH * OW, N * BH * BW
    g = torch.Generator().manual_seed(5 + rows + Cc)
    a, sa, ta = torch.randn(N, OH, OW, Cc, generator=g), torch.randn(Cc, generator=g), torch.randn(Cc, generator=g)
    prev = torch.relu(torch.randn(N, BH, BW, Cc, generator=g))
    plan = ops.Plan(device, eager=True)
    pp, plo = make_planes(plan, device, prev, prow, Cc)
    D = lambda t: t.float().contiguous().to(device)  # noqa: E731

    def run(fill, gap):
        bq, lb = repack(pp, plo, prow, Cc, fill, gap)
        out, lo = sentinel_out(rows, Cc, device)
        out32 = torch.full((N, OH, OW, Cc), float("nan"), device=device)
        ops.bn_add_relu_split(plan, D(a), D(sa), D(ta), None, None, None, bq, lb, out, lo, out32, N, OH, OW, Cc, BH, BW, s)
        torch.cuda.synchronize()
        assert_extents_only(out, lo, rows, Cc, "bn_add_relu_split %s" % (case,))
        return valid_halves(out, lo, rows, Cc), out32, out, lo

    h0, o0, _, _ = run(0, 0)
    for fill, gap in POISONS:
        h, o, out, lo = run(fill, gap)
        what = "%s poison 0x%02x gap %d" % (case, fill, gap)
        assert torch.equal(h, h0), "planes depend on the shortcut's pad rows: " + what
        assert same_bits(o, o0), "fp32 output depends on the shortcut's pad rows: " + what
    ref = torch.relu(a.double() * sa.double() + ta.double() + unsplit(pp, plo, prow, Cc).view(N, BH, BW, Cc)[:, ::s, ::s])
    close(o, ref, what="unit out fp32 " + what)
    close(unsplit(out, lo, rows, Cc), ref.reshape(rows, Cc), tol=1e-6, what="unit out planes " + what)


@pytest.mark.parametrize("rows_hw", [(1, 3, 5), (3, 7, 13), (5, 14, 19), (1, 9, 39)])   # rows % 16 = 15, 1, 2, 15
def test_split_producers_write_only_plane_extents(device, rows_hw):
    """bn_relu_split, bn_add_relu_split (projection shortcut, fp32 copy) and bn_relu_maxpool_split into a buffer filled
    with a sentinel, lo_off = plane_bytes + 4 KiB, 4 KiB of slack: every byte outside [0, plane_bytes) and [lo_off,
    lo_off + plane_bytes) keeps the sentinel; the valid rows decode to the fp64 value (pad rows: unspecified)"""
    import torch.nn.functional as F

    from acimg import ops

    N, OH, OW = rows_hw
    Cc = 64
    rows = N * OH * OW
    g = torch.Generator().manual_seed(rows)
    plan = ops.Plan(device, eager=True)
    D = lambda t: t.float().contiguous().to(device)  # noqa: E731
    x, sc, sh = torch.randn(N, OH, OW, Cc, generator=g), torch.randn(Cc, generator=g), torch.randn(Cc, generator=g)
    # bn_relu_split
    out, lo = sentinel_out(rows, Cc, device)
    ops.bn_relu_split(plan, D(x), D(sc), D(sh), 1, out, lo, rows, Cc)
    torch.cuda.synchronize()
    assert_extents_only(out, lo, rows, Cc, "bn_relu_split")
    close(unsplit(out, lo, rows, Cc), torch.relu(x.double() * sc + sh).reshape(rows, Cc), tol=5e-7, what="bn_relu_split")
    # bn_add_relu_split, projection shortcut (raw fp32 + affine)
    b, sb, tb = torch.randn(N, OH, OW, Cc, generator=g), torch.randn(Cc, generator=g), torch.randn(Cc, generator=g)
    out, lo = sentinel_out(rows, Cc, device)
    out32 = torch.empty(N, OH, OW, Cc, device=device)
    ops.bn_add_relu_split(plan, D(x), D(sc), D(sh), D(b), D(sb), D(tb), None, 0, out, lo, out32, N, OH, OW, Cc, OH, OW, 1)
    torch.cuda.synchronize()
    assert_extents_only(out, lo, rows, Cc, "bn_add_relu_split")
    ref = torch.relu(x.double() * sc + sh + b.double() * sb + tb)
    close(out32, ref, what="bn_add_relu_split fp32")
    close(unsplit(out, lo, rows, Cc), ref.reshape(rows, Cc), tol=5e-7, what="bn_add_relu_split planes")
    # bn_relu_maxpool_split: 3x3 / 2 SAME pooling of a 2 OH x 2 OW input -> OH x OW
    H, W = 2 * OH, 2 * OW
    xin = torch.randn(N, H, W, Cc, generator=g)
    ph, pt, pb = same_pads(H, 3, 2)
    pw, pl, pr = same_pads(W, 3, 2)
    prow = N * ph * pw
    assert prow == rows
    out, lo = sentinel_out(prow, Cc, device)
    ops.bn_relu_maxpool_split(plan, D(xin), D(sc), D(sh), out, lo, N, H, W, Cc, ph, pw, pt, pl)
    torch.cuda.synchronize()
    assert_extents_only(out, lo, prow, Cc, "bn_relu_maxpool_split")
    xa = torch.relu(xin.double() * sc + sh).permute(0, 3, 1, 2)
    ref = F.max_pool2d(F.pad(xa, (pl, pr, pt, pb), value=-1e30), 3, 2).permute(0, 2, 3, 1)
    close(unsplit(out, lo, prow, Cc), ref.reshape(prow, Cc), tol=5e-7, what="bn_relu_maxpool_split")


# relative tolerances of the model-level comparison: about ten times the gram-vs-statistics-pass spread measured on
# MI355X (one poisoned forward at N = 7: scale 3.9e-6, shift 1.9e-6, moving mean 7.6e-7, moving variance 1.2e-7, conv_map
# output 4.1e-5 - conv_map normalises over only 7 x 12 x 16 outputs, which magnifies the trunk's last-bit differences)
MODEL_TOL = {"scale": 4e-5, "shift": 4e-5, "moving_mean": 1e-5, "moving_variance": 1e-5, "conv_map": 4e-4}


def _model_errors(mg, sg, mp, sp):
    """{tensor: max |gram - pass| / max |pass|} over every batch-norm scale / shift, moving statistic and conv_map"""
    def rel(a, b):
        a, b = a.detach().double().cpu(), b.detach().double().cpu()
        return float((a - b).abs().max() / max(float(b.abs().max()), 1e-30))

    assert sorted(mg._aff_cache) == sorted(mp._aff_cache)
    errs = {}
    for scope in mg._aff_cache:
        for a, b, k in zip(mg._aff_cache[scope], mp._aff_cache[scope], ("scale", "shift")):
            errs["%s %s" % (scope, k)] = rel(a, b)
    for n in sp.store.vars:
        if n.endswith(("moving_mean", "moving_variance")):
            errs[n] = rel(sg.store.p(n), sp.store.p(n))
    errs["conv_map"] = rel(mg.output, mp.output)
    return errs


def test_model_gram_statistics_ignore_pad_rows(device):
    """ResNet50Model(gram=True) against gram=False at N = 7 (trunk rows 56 x 75 x 7 and 28 x 38 x 7, both 8 mod 16): the
    same weights and images, training-mode forwards.  The Gram statistics must run on units of both pipeline stages.
    Every batch-norm scale / shift (the two-pass units' and all those downstream of them), every trunk moving statistic
    and conv_map's output must agree to MODEL_TOL: the two statistics paths differ by rounding only.  Twice: after two
    forwards on fresh arenas (the second one sees the pad rows the first one left: the stale activations of real use),
    and after one more forward on arenas poisoned with a large finite pattern."""
    from acimg.session import Session
    from acimg.vision import ResNet50Model

    N = 7
    g = torch.Generator().manual_seed(2024)
    images = torch.rand(N, 224, 298, 3, generator=g) * 2.0 - 1.0
    models = {}
    for gram in (True, False):
        sess = Session(device)
        m = ResNet50Model(input_shape=[224, 298, 3], num_classes=None, gram=gram)
        feed = sess.zeros(N, 224, 298, 3)
        m._build_model(feed, session=sess)
        sess.finalize()
        m.initialize(seed=1238)
        feed.copy_(images.to(device))
        names = [c[0] for c in m.plan_train.calls]
        gram_at = [i for i, n in enumerate(names) if n == "gram_stats"]
        if gram:
            assert m.stages == 2 and any(i < m.stage_calls for i in gram_at) and any(i >= m.stage_calls for i in gram_at), \
                "gram_stats must run in both trunk stages"
        else:
            assert not gram_at and "conv2d_fwd_split3p_stats" in names
        models[gram] = (m, sess)

    def forward(poison=None):
        for m, _ in models.values():
            if poison is not None:
                for name in dir(m):
                    if name.startswith("planes_") and isinstance(getattr(m, name), torch.Tensor):
                        getattr(m, name).fill_(poison)
            m.plan_train.run()
        torch.cuda.synchronize()

    (mg, sg), (mp, sp) = models[True], models[False]
    forward()                       # fresh arenas: every pad row still zero
    for stage, poison in (("stale", None), ("poisoned", 0x7B)):
        forward(poison)
        errs = _model_errors(mg, sg, mp, sp)
        for kind, tol in MODEL_TOL.items():
            ks = [k for k in errs if k.endswith(kind)]
            worst = max(ks, key=lambda k: errs[k] if errs[k] == errs[k] else float("inf"))
            print("model gram vs statistics pass, %s arenas: %-15s worst %.3e (%s) over %d tensors"
                  % (stage, kind, errs[worst], worst, len(ks)))
        for kind, tol in MODEL_TOL.items():
            bad = {k: v for k, v in errs.items() if k.endswith(kind) and not v <= tol}
            assert not bad, "%s arenas: %s beyond %.0e: %s" % (stage, kind, tol, sorted(bad.items())[:3])
