"""End-to-end GPU parity of the HIP train step against the CPU oracle on identical weights, inputs and
noise: loss terms, generated image, mean/std, EVERY gradient, post-Adam weights after 1 and 3 steps,
batch-norm moving statistics, and the evaluation pass.

Tolerance (BASELINE.json north_star): outputs and losses within 1e-3 relative (max-norm, relative to
the tensor's max magnitude), for BOTH trunk arithmetic modes: exact-f32 MFMA ("f32", observed ~1e-5)
and split-fp16 MFMA ("f16x3": hi/lo fp16 operands, three MFMAs per product, fp32 accumulate).  Gradients are held to the same 1e-3 (max-norm and L2).  A ReLU pre-activation within fp32
rounding of zero (a few of the 2.5 M per step; e.g. `conv4`: 2.3e-7 here vs 0.0 in the oracle) picks a
different but equally valid subgradient, so for the BACKWARD comparison the oracle takes the ReLU on/off
patterns from the HIP run (both sides then differentiate the same piecewise-linear function); forward
values are compared independently and the number of such flips is printed.
"""
import functools

import numpy as np
import pytest
import torch

import op_support
from model_support import MASK_PAIRS, build, saved_activations

pytestmark = pytest.mark.gpu

TOL = 1e-3
# ReLU outputs (and min-max tie-set members) that may switch side between the HIP run and a free-running oracle: both
# are fp32 evaluations of the same graph, so a pre-activation within rounding of zero may land on either side.  The
# bound is a RATE, 3.2e-6 of the compared elements (= 8 of the ~2.5 M of a batch-2 step); a kernel that mis-thresholds
# activations by more than rounding noise breaks it by orders of magnitude.
FLIP_RATE = 3.2e-6


rel_err = functools.partial(op_support.rel_err, floor=1e-12)
l2_err = functools.partial(op_support.l2_err, floor=1e-30)
EP_KEYS = {"layer1/conv_2": "conv1", "layer1/pool_2": "pool1", "layer2/conv_2": "conv2_0", "layer4/conv_2": "conv4",
           "layer5/conv_2": "conv5", "layer6/conv_2": "conv6", "layer7/conv_2": "conv7"}


def tf_adam_fp64(p, g, m, v, step, lr):
    """tf.train.AdamOptimizer update in float64"""
    p, g, m, v = p.double(), g.double(), m.double(), v.double()
    lr_t = lr * np.sqrt(1 - 0.999 ** step) / (1 - 0.9 ** step)
    m2 = 0.9 * m + 0.1 * g
    v2 = 0.999 * v + 0.001 * g * g
    return p - lr_t * m2 / (v2.sqrt() + 1e-8), m2, v2


@pytest.mark.parametrize("num_skip,embedding,precision", [(1, False, "f16x3"), (1, False, "f32"), (2, False, "f16x3"),
                                                         (0, True, "f32"), (0, False, "f16x3")])
def test_train_step_matches_oracle(device, num_skip, embedding, precision):
    """Three consecutive optimisation steps, each compared from IDENTICAL state (the HIP state is
    re-synchronised from the oracle before every step): forward tensors, loss terms, every gradient,
    BN moving statistics; and the optimiser itself against TF-1 Adam recomputed in fp64 from the
    gradients the HIP path produced.  (Free-running trajectories of two correct fp32 implementations
    drift: at step t=1 Adam's update is lr*g/(|g|+3.2e-7), which turns ~3e-8 of summation-order noise
    on near-zero gradient entries into ~0.1*lr weight differences — see the trajectory test below.)"""
    from oracle import trainer as otr

    B, lr = 2, 1e-3
    tr, orc, sess = build(device, num_skip, embedding, B, lr, precision)
    store = sess.store
    ac, mf, vid, eps = otr.synthetic_batch(B, seed=99)
    sd = store.state_dict()
    for k, v in orc.state_dict().items():   # lossless round trip through the padded internal layouts
        assert torch.equal(sd[k], v.detach()), k
    total_flips, total_elems, tie_mismatch = 0, 0, 0
    for step in range(3):
        store.load_state(orc.state_dict(), strict=True)
        store.load_slots(orc.m, orc.v)
        tr.global_step = orc.step
        before = store.state_dict()
        m0, v0 = store.slot_dict("m"), store.slot_dict("v")
        got = tr.train_step((ac, mf, vid), eps=eps)
        g = tr.primary
        acts = saved_activations(g)
        grads = store.grad_dict()
        # backward comparison: the oracle differentiates with the HIP run's ReLU on/off patterns
        masks = dict((k, v > 0) for k, v in acts.items())
        # ... and the argmin / argmax sets of the two per-sample min-max normalisations (a post-ReLU zero that is
        # 1e-7 on one side would otherwise become THE minimum there and take the whole reduce_min gradient)
        for key, src in (("minmax/conv2_0", acts["layer2/conv_2"]), ("minmax/feature", acts["conv_map"])):
            masks[key] = (src == src.amin(dim=(1, 2, 3), keepdim=True), src == src.amax(dim=(1, 2, 3), keepdim=True))
        ep = {}
        ref = orc.train_step(ac, mf, vid, eps, end_points=ep, keep_grads=True, relu_masks=masks)
        for k in ("mse", "huber", "latent", "reg", "loss"):
            assert abs(got[k] - ref[k]) <= TOL * max(abs(ref[k]), 1e-8), (step, k, got[k], ref[k])
        assert rel_err(acts["conv_map"], ep["resnet_v1_50/conv_map"]) < TOL, "resnet feature"
        assert rel_err(g.modelac.output, ref["output"]) < TOL, "generated image"
        assert rel_err(g.modelac.mean, ref["mean"]) < TOL, "mean"
        if not embedding:
            assert rel_err(g.modelac.std, ref["std"]) < TOL, "std"
        assert rel_err(g.modelac.network["features"], ep["features"]) < TOL, "145-ch feature map"
        for _, key in MASK_PAIRS:
            assert rel_err(acts[key], ep[EP_KEYS.get(key, key)].detach()) < TOL, "activation " + key
        if step == 0:  # how many ReLU outputs a free-running oracle would switch differently
            free = {}
            otr.Oracle(num_skip=num_skip, embedding=embedding, randomize=True).forward(vid, mf, eps, True, free)
            for _, key in MASK_PAIRS:
                total_flips += int(((acts[key] > 0) != (free[EP_KEYS.get(key, key)] > 0)).sum())
                total_elems += acts[key].numel()
            for src, oname in ((acts["layer2/conv_2"], "conv2_0"), (acts["conv_map"], "resnet_v1_50/conv_map")):
                o = free[oname].detach()
                for red in (torch.amin, torch.amax):
                    tie_mismatch += int(((src == red(src, dim=(1, 2, 3), keepdim=True)) !=
                                         (o == red(o, dim=(1, 2, 3), keepdim=True))).sum())
        worst, worst_l2 = ("", 0.0), ("", 0.0)
        for k, gr in ref["grads"].items():
            e = rel_err(grads[k], gr)
            if e > worst[1]:
                worst = (k, e)
            e = l2_err(grads[k], gr)
            if e > worst_l2[1]:
                worst_l2 = (k, e)
        assert worst[1] < TOL, "step %d gradient %s max-norm err %.3e" % ((step,) + worst)
        assert worst_l2[1] < TOL, "step %d gradient %s L2 err %.3e" % ((step,) + worst_l2)
        # optimiser: TF-1 Adam in fp64 applied to OUR gradients reproduces our new weights / slots
        after = store.state_dict()
        m1, v1 = store.slot_dict("m"), store.slot_dict("v")
        osd = orc.state_dict()
        for k in orc.train_names:
            p2, m2, v2 = tf_adam_fp64(before[k], grads[k], m0[k], v0[k], orc.step, lr)
            assert float((after[k].double() - p2).abs().max()) <= 2e-6 * max(float(p2.abs().max()), 1e-3), "adam p " + k
            assert rel_err(m1[k], m2) < 1e-4 and rel_err(v1[k], v2) < 1e-4, "adam slots " + k
            # and stays within a fraction of one step of the oracle's weights
            assert float((after[k].double() - osd[k].detach().double()).abs().max()) <= 0.5 * lr, "vs oracle " + k
        for k, v in osd.items():
            if "moving_" in k:
                assert rel_err(after[k], v) < 1e-4, "BN moving statistic " + k
            elif k not in orc.train_names:
                assert torch.equal(after[k], before[k]), "frozen variable changed: " + k
    print("ReLU outputs within rounding of zero (mask flips vs free-running oracle): %d of %d; min-max tie-set "
          "mismatches: %d" % (total_flips, total_elems, tie_mismatch))
    assert total_flips <= max(8, FLIP_RATE * total_elems), (total_flips, total_elems)
    assert tie_mismatch <= max(8, FLIP_RATE * total_elems), tie_mismatch
    # evaluation pass (BN inference mode) from synchronised state
    store.load_state(orc.state_dict(), strict=True)
    refe = orc.eval_step(ac, mf, vid, eps)
    gote = tr.eval_step((ac, mf, vid), eps=eps)
    for k in ("mse", "mse0", "mse1", "mse2", "mse3"):
        assert abs(gote[k] - refe[k]) <= TOL * refe[k], (k, gote[k], refe[k])
    assert rel_err(tr.primary.modelac.output, refe["output"]) < TOL


def test_free_running_trajectory(device):
    """5 un-synchronised steps at the reference's learning rate (1e-4, scripts/scriptacresn.bash): loss
    terms stay within 1e-3 relative of the oracle's trajectory and the loss goes down"""
    from oracle import trainer as otr

    tr, orc, sess = build(device, 1, False, 2, lr=1e-4)
    ac, mf, vid, eps = otr.synthetic_batch(2, seed=3)
    first = None
    for step in range(5):
        got = tr.train_step((ac, mf, vid), eps=eps)
        ref = orc.train_step(ac, mf, vid, eps)
        first = first or got
        for k in ("mse", "huber", "latent", "loss"):
            assert abs(got[k] - ref[k]) <= TOL * max(abs(ref[k]), 1e-8), (step, k, got[k], ref[k])
    assert got["mse"] < first["mse"]


def test_partial_batch_and_device_noise(device):
    """a smaller last batch gets its own plans over the same variables; eps=None samples on device"""
    tr, orc, sess = build(device, 1, False, 2)
    from oracle import trainer as otr

    ac, mf, vid, eps = otr.synthetic_batch(1, seed=5)
    ref = orc.eval_step(ac, mf, vid, eps)
    got = tr.eval_step((ac, mf, vid), eps=eps)
    assert abs(got["mse"] - ref["mse"]) <= TOL * ref["mse"]
    r1 = tr.train_step((ac, mf, vid))
    assert np.isfinite(r1["loss"])
    e = tr.graphs[1].eps.cpu()
    assert abs(float(e.mean())) < 0.5 and 0.5 < float(e.std()) < 1.5


def test_full_size_properties(device):
    """The bench configuration itself (batch 32, f16x3, 1 skip) through properties that need no oracle:
    (a) a train step replayed from the same state is bit-identical (losses, generated images, every gradient);
    (b) the inference pass is per-image: the batch of 32 equals its two halves run as batches of 16;
    (c) the reported MSE is the MSE of the generated images;
    (d) the gradient is the derivative of the reported loss: a central difference along the (normalised) gradient
        direction of all trained variables reproduces |g| (batch statistics and noise held fixed)."""
    from acimg.flags import FLAGS
    from acimg.session import Session
    from acimg.trainer import Trainer
    from acimg.unet_acresnet import UNetAc
    from acimg.vision import ResNet50Model
    from oracle import trainer as otr

    B = 32
    FLAGS.model, FLAGS.ae, FLAGS.latent_loss = "UNet", 0, 1e-6
    sess = Session(device)
    tr = Trainer(UNetAc(input_shape=[36, 48, 12], embedding=False, num_skip=1),
                 ResNet50Model(input_shape=[224, 298, 3], num_classes=None), learning_rate=1e-4, session=sess)
    g = tr._build_functions(batch_size=B)
    tr.modelimages.initialize(seed=1238)
    tr.modelac.initialize(seed=1239)
    ac, mf, vid, eps = otr.synthetic_batch(B, seed=41)
    st = sess.store
    w0 = st.flat["train"].clone()
    bn0 = st.flat["state"].clone()
    m0, v0 = st.adam_m.clone(), st.adam_v.clone()

    def restore(w=None):
        st.flat["train"].copy_(w0 if w is None else w)
        st.flat["state"].copy_(bn0)
        st.adam_m.copy_(m0)
        st.adam_v.copy_(v0)
        tr.global_step = 0

    # (a) determinism
    r1 = tr.train_step((ac, mf, vid), eps=eps)
    g1 = st.grad.clone()
    out1 = g.modelac.output.clone()
    restore()
    r2 = tr.train_step((ac, mf, vid), eps=eps)
    assert r1 == r2 and torch.equal(g1, st.grad) and torch.equal(out1, g.modelac.output)
    # (c) the reported MSE
    mse = float(((out1.double().cpu() - ac.double().reshape(B, 36, 48, 12)) ** 2).mean())
    assert abs(r1["mse"] - mse) <= 1e-5 * mse, (r1["mse"], mse)
    # (d) directional derivative along g (every trained variable: generator + conv_map)
    restore()
    gn = float(g1.double().norm())
    d = (g1.double() / gn).float()
    # step: the largest single weight moves by 2e-3 (weights are ~1e-2 ... 1e-1); the loss (~16, fp32: 2e-6 steps)
    # then changes by hundreds of its representable steps
    h = 2e-3 / max(float(d.abs().max()), 1e-12)
    fp, fm = [], []
    for sign, acc in ((+1.0, fp), (-1.0, fm)):
        restore(w0 + sign * h * d)
        acc.append(tr.train_step((ac, mf, vid), eps=eps)["loss"])
    restore()
    fd = (fp[0] - fm[0]) / (2 * h)
    assert abs(fd - gn) <= 3e-2 * gn, (fd, gn, h, fp[0] - fm[0])
    # (b) inference is per image
    full = tr.eval_step((ac, mf, vid), eps=eps)
    out_full = g.modelac.output.clone()
    halves = []
    for lo in (0, 16):
        tr.eval_step((ac[lo:lo + 16], mf[lo:lo + 16], vid[lo:lo + 16]), eps=eps[lo:lo + 16])
        halves.append(tr.graphs[16].modelac.output.clone())
    both = torch.cat(halves, 0)
    assert rel_err(both, out_full) < 1e-5, rel_err(both, out_full)
    assert np.isfinite(full["mse"])


def test_bench_configuration_matches_oracle(device):
    """The configuration bench.py times (batch 32, 1 skip, f16x3 trunk, default tile / split / tail-split paths,
    latent_loss 1e-6) against `oracle.trainer.Oracle` on identical weights, inputs and noise
    (trainer/mfcctrainer.py:28-82): loss terms, the ResNet `conv_map` feature, mean / std, the generated images and
    every gradient (max-norm and L2) within 1e-3; the ReLU patterns a free-running oracle would have chosen differ
    from the HIP run's in at most FLIP_RATE of the compared activations."""
    from oracle import trainer as otr

    B = 32
    tr, orc, sess = build(device, 1, False, B, lr=1e-4, bench_defaults=True)
    ac, mf, vid, eps = otr.synthetic_batch(B, seed=321)
    got = tr.train_step((ac, mf, vid), eps=eps)
    g = tr.primary
    acts = saved_activations(g)
    grads = sess.store.grad_dict()
    masks = dict((k, v > 0) for k, v in acts.items())
    for key, src in (("minmax/conv2_0", acts["layer2/conv_2"]), ("minmax/feature", acts["conv_map"])):
        masks[key] = (src == src.amin(dim=(1, 2, 3), keepdim=True), src == src.amax(dim=(1, 2, 3), keepdim=True))
    # free-running oracle forward first (its own ReLU decisions): forward parity + the flip census
    free = {}
    with torch.no_grad():
        fmean, fstd, fout, _ = otr.Oracle(num_skip=1, randomize=True, latent_loss=1e-6).forward(vid, mf, eps, True, free)
    assert rel_err(g.modelac.output, fout) < TOL, "generated image vs free-running oracle"
    assert rel_err(acts["conv_map"], free["resnet_v1_50/conv_map"]) < TOL, "resnet feature vs free-running oracle"
    flips = elems = 0
    for _, key in MASK_PAIRS:
        flips += int(((acts[key] > 0) != (free[EP_KEYS.get(key, key)] > 0)).sum())
        elems += acts[key].numel()
    print("batch 32: %d ReLU flips of %d activations" % (flips, elems))
    assert flips <= FLIP_RATE * elems, (flips, elems)
    del free
    ep = {}
    ref = orc.train_step(ac, mf, vid, eps, end_points=ep, keep_grads=True, relu_masks=masks)
    for k in ("mse", "huber", "latent", "reg", "loss"):
        assert abs(got[k] - ref[k]) <= TOL * max(abs(ref[k]), 1e-8), (k, got[k], ref[k])
    assert rel_err(acts["conv_map"], ep["resnet_v1_50/conv_map"]) < TOL
    assert rel_err(g.modelac.output, ref["output"]) < TOL
    assert rel_err(g.modelac.mean, ref["mean"]) < TOL and rel_err(g.modelac.std, ref["std"]) < TOL
    worst = max(((rel_err(grads[k], gr), l2_err(grads[k], gr), k) for k, gr in ref["grads"].items()))
    worst_l2 = max(((l2_err(grads[k], gr), k) for k, gr in ref["grads"].items()))
    print("batch 32 gradients: worst max-norm %.2e (%s), worst L2 %.2e (%s)" % (worst[0], worst[2], worst_l2[0], worst_l2[1]))
    assert worst[0] < TOL and worst_l2[0] < TOL, (worst, worst_l2)
    for k in ref["grads"]:    # per-variable gradient L2 norms
        n_ref = float(ref["grads"][k].double().norm())
        assert abs(float(grads[k].double().norm()) - n_ref) <= TOL * max(n_ref, 1e-12), k
    osd = orc.state_dict()
    after = sess.store.state_dict()
    for k, v in osd.items():
        if "moving_" in k:
            assert rel_err(after[k], v) < 1e-4, "BN moving statistic " + k


def test_configs2_two_skip_batch64(device):
    """BASELINE configs[2]: `unet_acresnet` 2-skip generator at batch 64 (models/unet_acresnet2skip.py:82-83 under
    trainer/mfcctrainer.py:28-82).  One whole oracle step at that size (loss terms, mean / std, generated images, the
    gradient of every trained variable: 1e-3), plus the size-independent properties: a replayed step is bit-identical, the reported MSE is the
    MSE of the generated images, and the step lowers the loss on a repeated batch."""
    from oracle import trainer as otr

    B = 64
    tr, orc, sess = build(device, 2, False, B, lr=1e-4, bench_defaults=True)
    ac, mf, vid, eps = otr.synthetic_batch(B, seed=77)
    st = sess.store
    w0, bn0 = st.flat["train"].clone(), st.flat["state"].clone()
    r1 = tr.train_step((ac, mf, vid), eps=eps)
    g = tr.primary
    out1, g1 = g.modelac.output.clone(), st.grad.clone()
    feat1 = g.modelimages.output.clone()
    # ONE oracle step (forward + backward) at this size: loss terms, feature, mean / std, images, and the gradient of
    # every trained variable (per-variable L2 norms and the L2 error), ReLU / tie patterns taken from the HIP run as
    # in the other train-step tests
    acts = saved_activations(g)
    masks = dict((k, v > 0) for k, v in acts.items())
    for key, src in (("minmax/conv2_0", acts["layer2/conv_2"]), ("minmax/feature", acts["conv_map"])):
        masks[key] = (src == src.amin(dim=(1, 2, 3), keepdim=True), src == src.amax(dim=(1, 2, 3), keepdim=True))
    ref = orc.train_step(ac, mf, vid, eps, keep_grads=True, relu_masks=masks)
    for k in ("mse", "huber", "latent", "reg", "loss"):
        assert abs(r1[k] - ref[k]) <= TOL * max(abs(ref[k]), 1e-8), (k, r1[k], ref[k])
    assert rel_err(out1, ref["output"]) < TOL and rel_err(g.modelac.mean, ref["mean"]) < TOL
    assert rel_err(g.modelac.std, ref["std"]) < TOL
    grads = st.grad_dict()
    worst_l2 = max(((l2_err(grads[k], gr), k) for k, gr in ref["grads"].items()))
    print("configs[2] batch 64 gradients: worst L2 error %.2e (%s)" % worst_l2)
    assert worst_l2[0] < TOL, worst_l2
    for k, gr in ref["grads"].items():
        n_ref = float(gr.double().norm())
        assert abs(float(grads[k].double().norm()) - n_ref) <= TOL * max(n_ref, 1e-12), k
    mse = float(((out1.double().cpu() - ac.double()) ** 2).mean())
    assert abs(r1["mse"] - mse) <= 1e-5 * mse
    # replay from the same state: bit-identical
    st.flat["train"].copy_(w0)
    st.flat["state"].copy_(bn0)
    st.adam_m.zero_()
    st.adam_v.zero_()
    tr.global_step = 0
    r2 = tr.train_step((ac, mf, vid), eps=eps)
    assert r1 == r2 and torch.equal(g1, st.grad) and torch.equal(out1, g.modelac.output)
    assert torch.equal(feat1, g.modelimages.output)
    for _ in range(3):
        r3 = tr.train_step(None, eps=eps)
    assert r3["mse"] < r1["mse"]


def test_sharded_step_pipelined_equals_one_stream(device):
    """`train_step_sharded(pipelined=True)` (bench.py --scaling strong): the shards of a strong-scaling step go through
    the pipeline's lanes (trunk of shard i + 1 beside the trained part of shard i; accumulation, the exchange and the
    one Adam update on the trained part's stream) - two steps of four shards, bit-identical to the one-stream form in
    weights, Adam moments, batch-norm moving statistics and the mean losses of each step."""
    from oracle import trainer as otr

    steps = [[otr.synthetic_batch(2, seed=700 + 10 * s_ + i) for i in range(4)] for s_ in range(2)]
    tr, orc, sess = build(device, 1, False, 2)
    seq = []
    for shards in steps:
        r = tr.train_step_sharded([b[:3] for b in shards], eps=[b[3] for b in shards])
        seq.append([r[k] for k in ("mse", "huber", "latent", "reg", "loss")])
    torch.cuda.synchronize()
    st = sess.store
    want = (st.flat["train"].clone(), st.flat["state"].clone(), st.adam_m.clone(), st.adam_v.clone())
    tr2, orc2, sess2 = build(device, 1, False, 2)
    for t, shards in enumerate(steps):
        assert tr2.train_step_sharded([b[:3] for b in shards], eps=[b[3] for b in shards], pipelined=True, tag=t) is None
    tr2.flush_pipeline()
    got = dict((t, [r[k] for k in ("mse", "huber", "latent", "reg", "loss")]) for t, r in tr2.pop_finished())
    torch.cuda.synchronize()
    assert tr2.global_step == 2 == tr.global_step
    st2 = sess2.store
    assert torch.equal(st2.flat["train"], want[0]), float((st2.flat["train"] - want[0]).abs().max())
    assert torch.equal(st2.flat["state"], want[1])
    assert torch.equal(st2.adam_m, want[2]) and torch.equal(st2.adam_v, want[3])
    for t in range(2):      # the one-stream form averages on the host in float32 tensors too: same bits
        assert got[t] == pytest.approx(seq[t], rel=1e-6, abs=0), (got[t], seq[t])


def test_pipelined_schedule_at_bench_size(device):
    """The schedule bench.py times, at the size it times it (batch 32, f16x3, three lanes): 8 DIFFERENT batches through
    `train_step_pipelined` - with a partial batch of 16 in the middle (another graph: the pipeline drains and refills)
    and an explicit `flush_pipeline()` between two full batches - against the same 8 batches through `train_step` on a
    second trainer: weights, Adam moments, batch-norm moving statistics and every batch's loss terms BIT-IDENTICAL.
    At this size a trunk stage is ~3 ms of kernels per lane, so the cross-stage hand-offs (boundary tensor / event "x",
    `xfinal` / event "b", per-stage arenas, statistics and tail workspaces) are exercised where they could race."""
    from oracle import trainer as otr

    B = 32
    sizes = [B, B, B, 16, B, B, B, B]
    batches = [otr.synthetic_batch(n, seed=900 + i) for i, n in enumerate(sizes)]
    tr, orc, sess = build(device, 1, False, B, lr=1e-4, bench_defaults=True)
    seq = []
    for ac, mf, vid, eps in batches:
        r = tr.train_step((ac, mf, vid), eps=eps)
        seq.append([r[k] for k in ("mse", "huber", "latent", "reg", "loss")])
    torch.cuda.synchronize()
    st = sess.store
    want = (st.flat["train"].clone(), st.flat["state"].clone(), st.adam_m.clone(), st.adam_v.clone())
    del tr, orc, sess
    torch.cuda.empty_cache()

    tr2, orc2, sess2 = build(device, 1, False, B, lr=1e-4, bench_defaults=True)
    got = {}
    for i, (ac, mf, vid, eps) in enumerate(batches):
        tr2.train_step_pipelined((ac, mf, vid), eps=eps, tag=i)
        if i == 5:
            tr2.flush_pipeline()                    # mid-stream drain: the next call refills the lanes
            assert tr2.global_step == 6
        for t, r in tr2.pop_finished():
            got[t] = [r[k] for k in ("mse", "huber", "latent", "reg", "loss")]
    assert tr2._pipe["lanes"] >= 2, "the lanes did not get streams of their own: nothing overlapped"
    tr2.flush_pipeline()
    for t, r in tr2.pop_finished():
        got[t] = [r[k] for k in ("mse", "huber", "latent", "reg", "loss")]
    torch.cuda.synchronize()
    assert tr2.global_step == len(batches) and sorted(got) == list(range(len(batches)))
    st2 = sess2.store
    assert torch.equal(st2.flat["train"], want[0]), float((st2.flat["train"] - want[0]).abs().max())
    assert torch.equal(st2.flat["state"], want[1]), "batch-norm moving statistics"
    assert torch.equal(st2.adam_m, want[2]) and torch.equal(st2.adam_v, want[3])
    assert [got[i] for i in range(len(batches))] == seq


def test_sharded_step_accumulates_like_data_parallel(device):
    """`Trainer.train_step_sharded` (bench.py --scaling strong): two shards of 2 images run one after the other with
    accumulated gradients and ONE Adam update = the update a 2-rank data-parallel step would make (each shard
    normalised with its own batch statistics, gradient = mean of the shard gradients): checked against TF-1 Adam in
    fp64 on the mean of the gradients of two separate single-shard steps from the same state."""
    from oracle import trainer as otr

    lr = 1e-3
    tr, orc, sess = build(device, 1, False, 2, lr=lr)
    st = sess.store
    shards = [otr.synthetic_batch(2, seed=200 + i) for i in range(2)]
    w0, bn0 = st.flat["train"].clone(), st.flat["state"].clone()
    grads = []
    for ac, mf, vid, eps in shards:          # per-shard gradients from the same weights (BN state restored each time)
        st.flat["train"].copy_(w0)
        st.flat["state"].copy_(bn0)
        st.adam_m.zero_()
        st.adam_v.zero_()
        tr.global_step = 0
        tr.train_step((ac, mf, vid), eps=eps)
        grads.append(st.grad.clone())
    st.flat["train"].copy_(w0)
    st.flat["state"].copy_(bn0)
    st.adam_m.zero_()
    st.adam_v.zero_()
    tr.global_step = 0
    out = tr.train_step_sharded([(s[0], s[1], s[2]) for s in shards], eps=[s[3] for s in shards])
    gmean = (grads[0].double() + grads[1].double()) / 2
    want, _, _ = tf_adam_fp64(w0, gmean.float(), torch.zeros_like(w0), torch.zeros_like(w0), 1, lr)
    got = st.flat["train"].double()
    assert float((got - want).abs().max()) <= 2e-6 * max(float(want.abs().max()), 1e-3)
    assert tr.global_step == 1 and np.isfinite(out["loss"])
    # the accumulated buffer is what Adam saw: sum of the shard gradients (scale 1/2 folded into the optimiser)
    assert float((st.grad.double() - (grads[0].double() + grads[1].double())).abs().max()) <= 1e-6 * float(gmean.abs().max() * 2 + 1e-12)


def test_side_lane_is_only_a_schedule(device, monkeypatch):
    """The generator's weight gradients run on the plan's SIDE LANE (a second HIP stream, forked per layer from the
    main stream's chain of data gradients, joined before anything reads a parameter gradient): the same kernels on
    the same operands, so gradients, losses and the updated weights are BIT-IDENTICAL to the single-stream plan;
    replaying the two-stream plan is bit-identical to itself (no race between the lanes)."""
    from oracle import trainer as otr

    ac, mf, vid, eps = otr.synthetic_batch(2, seed=77)
    res = {}
    for lane in (True, False):
        tr, orc, sess = build(device, 1, False, 2, side_lane=lane)      # a constructor argument of both models
        assert tr.modelac.side_lane == lane
        g = tr.graphs[2]
        assert bool(g.plan_train.side) == lane
        if lane:
            assert len(g.plan_train.side) >= 14          # every layer with a data gradient beside it
        out = tr.train_step((ac, mf, vid), eps=eps)
        torch.cuda.synchronize()
        res[lane] = (out, sess.store.grad.clone(), sess.store.flat["train"].clone())
        if lane:
            sess.store.load_state(orc.state_dict(), strict=True)
            sess.store.adam_m.zero_()
            sess.store.adam_v.zero_()
            tr.global_step = 0
            out2 = tr.train_step((ac, mf, vid), eps=eps)
            torch.cuda.synchronize()
            assert torch.equal(sess.store.grad, res[True][1]) and torch.equal(sess.store.flat["train"], res[True][2])
            assert out2["loss"] == out["loss"]
    assert torch.equal(res[True][1], res[False][1])
    assert torch.equal(res[True][2], res[False][2])
    assert res[True][0]["loss"] == res[False][0]["loss"]


def test_pipelined_steps_equal_sequential_steps(device):
    """`Trainer.train_step_pipelined` (bench.py's default): trunk stage 1 (units 1-8) of batch n, trunk stage 2 (units
    9-16) of batch n - 1 and conv_map + generator + backward + Adam of batch n - 2 run on three HIP streams.  The trunk
    reads no trained variable, so the arithmetic of every batch is the one-stream step's: after 4 different batches
    the weights, the Adam moments, the batch-norm moving statistics and every step's losses are BIT-IDENTICAL to 4
    calls of `train_step`; a sequential call after pipelined ones flushes the pipeline first."""
    from oracle import trainer as otr

    batches = [otr.synthetic_batch(2, seed=300 + i) for i in range(4)]
    tr, orc, sess = build(device, 1, False, 2)
    seq_losses = []
    for ac, mf, vid, eps in batches:
        r = tr.train_step((ac, mf, vid), eps=eps)
        seq_losses.append([r[k] for k in ("mse", "huber", "latent", "reg", "loss")])
    torch.cuda.synchronize()
    st = sess.store
    want = (st.flat["train"].clone(), st.flat["state"].clone(), st.adam_m.clone(), st.adam_v.clone())

    tr2, orc2, sess2 = build(device, 1, False, 2)
    got_losses = []
    for ac, mf, vid, eps in batches:
        out = tr2.train_step_pipelined((ac, mf, vid), eps=eps)
        if out is not None:
            torch.cuda.synchronize()
            got_losses.append(out[:5].tolist())
    depth = len(tr2._pipe["stages"])                             # trunk stages = batches in flight
    assert depth == tr2.modelimages.stages == 2
    assert len(got_losses) == 4 - depth and tr2.global_step == 4 - depth
    while tr2._pipe["inflight"]:
        out = tr2._advance(tr2._pipe, None)
        torch.cuda.synchronize()
        got_losses.append(out[:5].tolist())
    assert tr2.global_step == 4 and tr2.flush_pipeline() is None
    st2 = sess2.store
    assert torch.equal(st2.flat["train"], want[0]), float((st2.flat["train"] - want[0]).abs().max())
    assert torch.equal(st2.flat["state"], want[1])
    assert torch.equal(st2.adam_m, want[2]) and torch.equal(st2.adam_v, want[3])
    assert got_losses == seq_losses, (got_losses, seq_losses)
    # mixing the two entry points: a pending batch is finished before a one-stream step runs
    ac, mf, vid, eps = batches[0]
    tr2.train_step_pipelined((ac, mf, vid), eps=eps)
    r5 = tr2.train_step((batches[1][0], batches[1][1], batches[1][2]), eps=batches[1][3])
    r5s_a = tr.train_step((ac, mf, vid), eps=eps)
    r5s_b = tr.train_step((batches[1][0], batches[1][1], batches[1][2]), eps=batches[1][3])
    torch.cuda.synchronize()
    assert tr2.global_step == 6 and r5["loss"] == r5s_b["loss"]
    assert torch.equal(sess2.store.flat["train"], sess.store.flat["train"])
