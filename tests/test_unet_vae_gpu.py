"""Parity of the RGB / spectrogram U-Net VAE train step (BASELINE configs[0]/[1]) against the CPU
oracle (fp64): outputs, loss terms, every gradient, BN moving statistics and one TF-1 Adam update, through the C ABI.
Tolerance: 1e-3 relative (north_star), observed ~1e-5."""
import functools
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "acoustic-image-generation_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

from op_support import l2_err, rel_err  # noqa: E402

pytestmark = pytest.mark.gpu


rel = functools.partial(rel_err, floor=1e-30, same_shape=False)


def _hip_masks(m):
    """the ReLU on/off pattern of the HIP run, keyed like the oracle's ReLUs"""
    masks = {name: (L.relu_output() > 0).cpu() for name, L in m.layers.items()}
    masks["dense"] = (m.dns1 > 0).cpu()
    masks["conv2d"] = (m.c2d.t > 0).cpu()
    return masks


def _oracle_step(orc, x, eps, masks, kl_grad_at=None):
    """one oracle train step on the HIP run's ReLU pattern, kept lean: what the tests compare, with the graph and the
    intermediate activations released (an fp64 step at batch 16 holds several GB while it runs).  `flips` of `total`:
    pre-activations of the oracle's own evaluation that lie on the other side of zero from the HIP run's"""
    r = orc.train_step(x, eps, apply=False, relu_masks=masks, kl_grad_at=kl_grad_at)
    own = r["fw"]["masks"]
    assert set(own) == set(masks) and all(own[k].shape == masks[k].shape for k in masks)
    out = dict(output=r["fw"]["output"].detach(), mean=r["fw"]["mean"].detach(), variance=r["fw"]["variance"].detach(),
               losses=r["losses"], grads={k: v.detach() for k, v in r["grads"].items()},
               new_stats={k: v.detach() for k, v in r["new_stats"].items()},
               flips=sum(int((own[k] != masks[k]).sum()) for k in masks), total=sum(v.numel() for v in masks.values()))
    del r, own
    return out


def _build_step(model, precision, N):
    """trainer at batch N, same parameters on both sides (biases / gamma / beta randomised so those paths carry signal)"""
    from acimg.session import Session
    from acimg.trainer_vae import TrainerVAE
    from acimg import unet_vae
    from oracle import unet_vae as ouv

    sess = Session(torch.device("cuda:0"))
    tr = TrainerVAE(getattr(unet_vae, model)(precision=precision), learning_rate=1e-3, session=sess)
    tr._build_functions(batch_size=N)
    params = ouv.init_params(model, seed=7, dtype=torch.float64, bias_std=0.05, bn_jitter=0.1)
    tr.model.initialize(state={k: v.float() for k, v in params.items()})
    x, eps = ouv.synthetic_batch(model, N, seed=11, dtype=torch.float64)
    return tr, sess, params, x, eps


def _step_against_fp64(model, tr, sess, params, x, eps, flips_ok, kl_at_hip=False):
    """one step of the fp32-class product against the fp64 oracle: outputs, loss terms, every gradient, the moving
    statistics and one TF-1 Adam update; flips_ok(flips, total) judges the ReLU census.
    kl_at_hip: the oracle differentiates the KL term at the HIP run's latent statistics (oracle/unet_vae.py `losses`).  At
    batch 16 one of the 2048 variance outputs is 3.1e-4, next to the peak of the KL gradient sg / (1e-8 + sg^2) at 1e-4, and
    that one value, a near-cancelling sum of 32256 terms, moves the variance head's gradient and the encoder's behind it by
    up to 8e-3 between fp32 and fp64 evaluations of the oracle itself (4.8e-5 once both differentiate at the same point)."""
    from oracle import unet_vae as ouv
    from oracle import tfsem

    dev = torch.device("cuda:0")
    orc = ouv.Oracle(model, learning_rate=1e-3, dtype=torch.float64, params=params)
    r = tr.train_step(x.float().to(dev), eps.float().to(dev), apply=False)
    torch.cuda.synchronize()
    m = tr.model
    cout = m.COUT
    # The oracle differentiates the same piecewise-linear function: ReLU on/off patterns are taken from the HIP run
    # (5 flips out of ~2e7 pre-activations move this model's gradients by up to 1e-2 — fp32 vs fp64 runs of the
    # oracle itself show it); forward values are compared independently of that below.
    ref = _oracle_step(orc, x, eps, _hip_masks(m), (m.mean.cpu(), m.variance.cpu()) if kl_at_hip else None)
    flips, total = ref["flips"], ref["total"]
    print("%s: ReLU pattern differs from the fp64 oracle's in %d of %d places (rate %.2e)" %
          (model, flips, total, flips / total))
    assert flips_ok(flips, total), (flips, total)
    # forward
    assert rel(m.output[..., :cout], ref["output"]) < 1e-4, "output"
    assert rel(m.mean, ref["mean"]) < 1e-4 and rel(m.variance, ref["variance"]) < 1e-4
    for k in ("mse", "huber", "latent", "reg", "loss"):
        assert abs(r[k] - ref["losses"][k]) <= 1e-4 * abs(ref["losses"][k]) + 1e-9, (k, r[k], ref["losses"][k])
    # gradients (the regulariser's gradient included)
    grads = sess.store.grad_dict()
    worst = ("", 0.0)
    for name, gref in ref["grads"].items():
        if name.endswith("/bias") and "/layer" in name:
            # a conv bias under a batch norm has an exactly-zero gradient (the mean subtraction removes it):
            # both sides must see ~0 relative to the gradient of the kernel next to it
            kmax = float(ref["grads"][name[:-4] + "kernel"].abs().max())
            assert float(grads[name].abs().max()) < 1e-4 * kmax and float(gref.abs().max()) < 1e-9 * kmax, name
            continue
        e = rel(grads[name], gref)
        if e > 1e-4:
            print("   %-40s rel err %.2e" % (name, e))
        if e > worst[1]:
            worst = (name, e)
    print("%s: worst gradient %s rel err %.2e" % (model, worst[0], worst[1]))
    assert worst[1] < 1e-3, worst
    # BN moving statistics advanced with the batch statistics (unbiased variance)
    st = sess.store.state_dict()
    for name, v in ref["new_stats"].items():
        assert rel(st[name], v) < 1e-4, name
    # one Adam step from the same state: compare with TF-1 Adam (fp64) applied to OUR gradients
    before = {k: v.clone() for k, v in st.items()}
    tr.train_step(None, eps.float().to(dev), apply=True)
    torch.cuda.synchronize()
    after = sess.store.state_dict()
    g2 = sess.store.grad_dict()
    for name in ref["grads"]:
        p0 = before[name].double()
        want, _, _ = tfsem.adam_tf1(p0, g2[name].double(), torch.zeros_like(p0), torch.zeros_like(p0), 1, 1e-3)
        assert float((after[name].double() - want).abs().max()) < 2e-6, name


@pytest.mark.parametrize("model,precision", [("UNet", "split"), ("UNetSound", "split"), ("UNetSound", "f32")])
def test_unet_vae_train_step(model, precision):
    tr, sess, params, x, eps = _build_step(model, precision, 2)
    _step_against_fp64(model, tr, sess, params, x, eps, lambda flips, total: flips < 200)


# the layers the benched batch (32) runs with batch norm + ReLU applied while the consumer stages its tiles; batch 16 has the
# same selection (tests/test_oracle_cpu.py pins it)
DEFERRED_AT_THE_BENCHED_SELECTION = ["layer1/conv_1", "layer1/pool_2", "layer2/conv_1", "layer2/pool_2", "layer3/conv_1",
                                     "layer7/conv_1", "layer8/conv_1", "layer9/conv_1"]


def _peak_rss_gb():
    import resource

    return resource.getrusage(resource.RUSAGE_SELF).ru_maxrss / 2.0 ** 20


@pytest.mark.parametrize("precision", ["split", "bf16"])
def test_unet_vae_train_step_at_the_benched_selection(precision):
    """BASELINE configs[1] as bench.py times it: batch 16 picks the same kernels for every layer as batch 32 (few-channel
    MFMA and halo forms from 65536 output pixels, split / bf16 layers from 16384, the eight deferred batch norms), which
    batches 2 and 6 of the tests above do not.  The whole step against the fp64 oracle: `split` to the batch-2 bounds (the
    ReLU census as a rate; the KL term differentiated at the HIP run's latent statistics, see `_step_against_fp64`), `bf16`
    to the batch-6 rule (3x the fp32 oracle's own spread)."""
    N = 16
    tr, sess, params, x, eps = _build_step("UNet", precision, N)
    m = tr.model
    assert sorted(n for n, L in m.layers.items() if L.deferred) == DEFERRED_AT_THE_BENCHED_SELECTION
    assert sum(1 for L in m.layers.values() if m._use_split(L.d)) == 11
    if precision == "split":
        _step_against_fp64("UNet", tr, sess, params, x, eps, lambda flips, total: flips <= 1e-5 * total, kl_at_hip=True)
    else:
        _bf16_step_against_fp64(tr, sess, params, x, eps, fp32_class_check=False)
    print("peak RSS of this process: %.2f GB" % _peak_rss_gb())


def test_unet_vae_batch32_properties():
    """BASELINE configs[1] size (batch 32, 224x298x3): loss decreases over a few steps, nothing is NaN, and the
    moving statistics stay finite — size-independent sanity at the full bench shape."""
    from acimg.session import Session
    from acimg.trainer_vae import TrainerVAE
    from acimg.unet_vae import UNet

    dev = torch.device("cuda:0")
    sess = Session(dev)
    tr = TrainerVAE(UNet(), learning_rate=1e-3, session=sess)
    g = tr._build_functions(batch_size=32)
    tr.model.initialize(seed=3)
    gen = torch.Generator().manual_seed(5)
    g.images.copy_(torch.rand(32, 224, 298, 3, generator=gen))
    first = tr.train_step()
    for _ in range(8):
        last = tr.train_step()
    assert all(v == v for v in last.values())
    assert last["loss"] < first["loss"], (first, last)
    st = sess.store.state_dict()
    assert all(torch.isfinite(v).all() for v in st.values())


def _bf16(t):
    return t.float().to(torch.bfloat16).double()


@pytest.mark.parametrize("case", [(2, 56, 75, 64, 64, 3), (4, 28, 38, 128, 96, 3), (2, 112, 149, 32, 32, 3),
                                  (3, 40, 52, 64, 128, 1), (1, 159, 161, 32, 128, 1)])
def test_bf16_operand_convs(case):
    """BASELINE configs[1] "bf16": acimg_conv2d_fwd_bf16 / _dgrad_bf16 / _wgrad_bf16 are EXACTLY the convolutions of
    the bf16-rounded operands accumulated in fp32 (one v_mfma_f32_16x16x32_bf16 per product): compared with fp64
    convolutions of the same rounded operands (2e-5: fp32 accumulation order), incl. the fused bias gradient and the
    batch-norm statistics of the forward.  (1, 159, 161, 32 -> 128): 25599 pixels are 200 row tiles of 128, from which on the
    forward takes the 128 x 128 tile (igemm_split3_kernel<128, 128, 2, 4, 512, SplitBF16, 1>; csrc/conv_split.hip pick_split3),
    the last tile one row short; the other shapes with more than 64 columns stay on 64 x 128."""
    from acimg import ops

    dev = torch.device("cuda:0")
    N, H, W, Cc, K, R = case
    g = torch.Generator().manual_seed(31 + Cc + K)
    x = torch.randn(N, H, W, Cc, generator=g)
    w = torch.randn(R, R, Cc, K, generator=g) * (2.0 / (R * R * Cc)) ** 0.5
    b = torch.randn(K, generator=g) * 0.1
    gy = torch.randn(N, H, W, K, generator=g) * 1e-3
    d = ops.conv_desc(N, H, W, Cc, K, R, R, 1, "SAME")
    plan = ops.Plan(dev, eager=True)
    xd, wd, bd, gyd = x.to(dev), w.to(dev), b.to(dev), gy.to(dev)
    wimg = torch.zeros(ops.conv2d_split3_weight_bytes(d), dtype=torch.uint8, device=dev)
    ops.conv2d_split3_prepare(plan, d, wd, wimg, bf16=True)
    y = torch.full((N, H, W, K), float("nan"), device=dev)
    rows = ops.conv2d_fwd_split3_stats_rows(d)
    if K > 64:         # one statistics row per row tile: 128 rows from 200 tiles of 128 x 128 on, 64 below
        M = N * H * W
        assert rows == -(-M // (128 if -(-M // 128) * -(-K // 128) >= 200 else 64)), rows
        assert rows == (200 if M == 25599 else -(-M // 64))
    st = torch.zeros(rows, 2, K, device=dev)
    ops.conv2d_fwd_split3(plan, d, xd, wimg, y, stats=st, bias=bd, bf16=True)
    wt = torch.zeros(ops.conv2d_split3_dgrad_weight_bytes(d), dtype=torch.uint8, device=dev)
    ops.conv2d_split3_prepare_dgrad(plan, d, wd, wt)
    dx = torch.full((N, H, W, Cc), float("nan"), device=dev)
    ops.conv2d_dgrad_split3(plan, d, gyd, K, wt, dx, bf16=True)
    dw = torch.full((R, R, Cc, K), float("nan"), device=dev)
    db = torch.full((K,), float("nan"), device=dev)
    ops.conv2d_wgrad_split3(plan, d, xd, gyd, K, dw, db, bf16=True)
    torch.cuda.synchronize()

    xr = _bf16(x).permute(0, 3, 1, 2).requires_grad_(True)
    wr = _bf16(w).permute(3, 2, 0, 1).requires_grad_(True)
    yr = torch.nn.functional.conv2d(xr, wr, b.double(), padding=R // 2)
    gr = _bf16(gy).permute(0, 3, 1, 2)
    gx, gw = torch.autograd.grad(yr, (xr, wr), gr)
    assert rel(y, yr.detach().permute(0, 2, 3, 1)) < 2e-5
    flat = yr.detach().permute(0, 2, 3, 1).reshape(-1, K)
    assert rel(st[:, 0].sum(0), flat.sum(0)) < 2e-4 and rel(st[:, 1].sum(0), (flat * flat).sum(0)) < 2e-4
    assert rel(dx, gx.permute(0, 2, 3, 1)) < 2e-5
    assert rel(dw, gw.permute(2, 3, 1, 0)) < 2e-5
    assert rel(db, gr.sum((0, 2, 3))) < 2e-5
    # and they are NOT the fp32-class result: the rounding is really there
    y32 = torch.nn.functional.conv2d(x.double().permute(0, 3, 1, 2), w.double().permute(3, 2, 0, 1), b.double(),
                                     padding=R // 2).permute(0, 2, 3, 1)
    assert rel(y, y32) > 2e-4


l2rel = functools.partial(l2_err, floor=1e-30)


def test_unet_vae_bf16_train_step():
    """BASELINE configs[1] (unet_architecture, bf16): one train step with precision="bf16" against the oracle computing
    the SAME arithmetic (oracle/unet_vae.py `_Bf16Conv`: operands of the selected convs rounded to bf16 in the forward,
    data- and weight-gradient products).

    What "the same" can mean here: rounded arithmetic is discontinuous — a pre-activation that differs by fp32
    accumulation order between two CORRECT evaluations rounds to the neighbouring bf16 value with probability ~5e-5
    per element, and those 0.4 % steps cascade through seven rounded layers (ReLU patterns then differ in ~2e-4 of
    the places).  The oracle itself, evaluated in fp32 and in fp64, differs by 2.5e-3 (max) / 4e-4 (L2) in the output
    and by up to 10 % in small gradients.  So the kernels are pinned EXACTLY at the op level
    (test_bf16_operand_convs: 2e-5 against fp64 convolutions of the rounded operands), and the whole step is held to
    the oracle's own fp32-vs-fp64 spread: every error of the product against the fp64 oracle must stay within 3x the
    error of the fp32 oracle against the fp64 oracle (same ReLU pattern on all three)."""
    N = 6                  # 6 x 56 x 49 >= 16384 pixels: layers 2, 3, 7 and 8 run on the bf16 kernels (7 convs)
    tr, sess, params, x, eps = _build_step("UNet", "bf16", N)
    m = tr.model
    nsplit = sum(1 for L in m.layers.values() if m._use_split(L.d))
    assert nsplit >= 7, nsplit                       # the bf16 kernels really carry the model's large convs
    _bf16_step_against_fp64(tr, sess, params, x, eps, fp32_class_check=True)


def _bf16_step_against_fp64(tr, sess, params, x, eps, fp32_class_check):
    """one precision="bf16" step against the fp64 same-rounding oracle, every error within 3x the fp32 oracle's own spread
    (test_unet_vae_bf16_train_step); fp32_class_check: and the output is NOT the fp32-class result"""
    from oracle import unet_vae as ouv

    dev = torch.device("cuda:0")
    model = "UNet"
    r = tr.train_step(x.float().to(dev), eps.float().to(dev), apply=False)
    torch.cuda.synchronize()
    m = tr.model
    masks = _hip_masks(m)
    ref = _oracle_step(ouv.Oracle(model, learning_rate=1e-3, dtype=torch.float64, params=params, bf16_operands=True), x, eps,
                       masks)
    flips, total = ref["flips"], ref["total"]
    print("bf16 UNet: ReLU pattern differs from the same-rounding oracle's in %d of %d places" % (flips, total))
    assert flips < 1e-3 * total
    ref32 = _oracle_step(ouv.Oracle(model, learning_rate=1e-3, dtype=torch.float32, params=params, bf16_operands=True), x,
                         eps, masks)
    out = m.output[..., :m.COUT]
    e_max, f_max = rel(out, ref["output"]), rel(ref32["output"], ref["output"])
    e_l2, f_l2 = l2rel(out, ref["output"]), l2rel(ref32["output"], ref["output"])
    print("bf16 UNet output: max err %.2e (fp32 oracle: %.2e), L2 err %.2e (fp32 oracle: %.2e)" % (e_max, f_max, e_l2, f_l2))
    assert e_l2 < 3 * f_l2 + 1e-5 and e_max < 3 * f_max + 1e-4
    assert e_l2 < 2e-3
    for k in ("mse", "huber", "latent", "reg", "loss"):
        spread = abs(ref32["losses"][k] - ref["losses"][k])
        # absolute floor 5e-9: the KL term (~1e-6 here) is a sum of mu^2 + var - log var - 1 near its zero, i.e. cancellation:
        # the oracle's own fp32 / fp64 evaluations differ by 3e-10 in it, and the few-channel layers' 22-bit (f16 hi / lo)
        # operands on the MFMA form (round 4) move it by ~3e-9 where the exact-fp32 direct kernel moved it by < 1e-9
        assert abs(r[k] - ref["losses"][k]) <= 3 * spread + 1e-4 * abs(ref["losses"][k]) + 5e-9, (k, r[k], ref["losses"][k])
    grads = sess.store.grad_dict()
    worst = ("", 0.0, 0.0)
    for name, gref in ref["grads"].items():
        if name.endswith("/bias") and "/layer" in name:
            continue
        e, f = l2rel(grads[name], gref), l2rel(ref32["grads"][name], gref)
        assert e < 3 * f + 1e-3, (name, e, f)
        if e > worst[1]:
            worst = (name, e, f)
    print("bf16 UNet: worst gradient %s L2 err %.2e (fp32 oracle: %.2e)" % worst)
    st = sess.store.state_dict()
    for name, v in ref["new_stats"].items():
        assert l2rel(st[name], v) < 3 * l2rel(ref32["new_stats"][name], v) + 1e-4, name
    if fp32_class_check:
        # it is bf16 arithmetic: the fp32-class oracle is NOT matched to 1e-3
        del ref, ref32
        free32 = ouv.Oracle(model, learning_rate=1e-3, dtype=torch.float64, params=params).train_step(x, eps, apply=False)
        assert rel(out, free32["fw"]["output"]) > 1e-3


def test_deferred_batch_norm_equals_the_materialised_one():
    """`UNet(defer_bn=True)` (default, round 4): conv_1 / pool outputs read only by the next 3x3 conv are never normalised in
    memory - the consumer's forward and weight gradient apply relu(x * scale + shift) while staging - against
    `defer_bn=False` (every layer runs its normalise + ReLU pass) on the same parameters and batch: which layers deferred,
    losses, output, every gradient.  Batch 16: all three stages of 56x74 and above are over the halo kernels' size rule
    (the eight layers the benched batch 32 defers)."""
    from acimg.session import Session
    from acimg.trainer_vae import TrainerVAE
    from acimg import unet_vae
    from oracle import unet_vae as ouv

    dev = torch.device("cuda:0")
    N = 16
    params = ouv.init_params("UNet", seed=9, dtype=torch.float64, bias_std=0.05, bn_jitter=0.1)
    x, eps = ouv.synthetic_batch("UNet", N, seed=13, dtype=torch.float64)
    res = []
    for defer in (False, True):
        sess = Session(dev)
        tr = TrainerVAE(unet_vae.UNet(precision="split", defer_bn=defer), learning_rate=1e-3, session=sess)
        tr._build_functions(batch_size=N)
        tr.model.initialize(state={k: v.float() for k, v in params.items()})
        r = tr.train_step(x.float().to(dev), eps.float().to(dev), apply=False)
        torch.cuda.synchronize()
        m = tr.model
        deferred = sorted(n for n, L in m.layers.items() if L.deferred)
        res.append((r, m.output[..., :m.COUT].clone(), {k: v.clone() for k, v in sess.store.grad_dict().items()}, deferred,
                    {n: L.relu_output().clone() for n, L in m.layers.items()}))
    (r0, o0, g0, d0, y0), (r1, o1, g1, d1, y1) = res
    assert d0 == [] and d1 == ["layer1/conv_1", "layer1/pool_2", "layer2/conv_1", "layer2/pool_2", "layer3/conv_1", "layer7/conv_1",
                               "layer8/conv_1", "layer9/conv_1"], d1
    for k in ("mse", "huber", "latent", "reg", "loss"):
        assert abs(r0[k] - r1[k]) <= 1e-5 * abs(r0[k]) + 1e-9, (k, r0[k], r1[k])
    assert rel(o1, o0) < 1e-5
    for n in y0:
        assert rel(y1[n], y0[n]) < 1e-5, n
    worst = max((rel(g1[k], g0[k]), k) for k in g0)
    print("deferred vs materialised batch norm: worst gradient %s %.2e" % (worst[1], worst[0]))
    assert worst[0] < 2e-4, worst
