"""The classification experiment on the device: `acimg_clip_eval` against the fp64 restatement (tests/classify_ref.py)
between guard bands, the loaders' clip mode against their frame mode on the same GZIP record files, the baseline
sources of `TrainerClass` against the CPU oracle, its train / test loops and Saver-V2 bundles, the `Trainer` bundle's bytes
across the extraction of the shared writer, and `python -m acimg.classify --mode compare` against the trainers."""
import functools
import json
import os
import re
from collections import OrderedDict

import numpy as np
import pytest
import torch

import classify_ref
from guard_arena import GuardArena
from data_support import write_outdoor_records
from model_support import make
from op_support import close_at, dyadic, rel_err, widen

pytestmark = pytest.mark.gpu

K10 = 10
close = close_at(2e-5)           # tests/test_ops_gpu.py RTOL


@pytest.fixture(autouse=True)
def flags_restored():
    """the tests below set the global FLAGS as a command line would: put every flag back afterwards"""
    from acimg.flags import FLAGS
    saved = dict(FLAGS.__dict__)
    yield
    FLAGS.__dict__.clear()
    FLAGS.__dict__.update(saved)


# ---- the kernel --------------------------------------------------------------------------------------------------------
# clips, F, K: one clip of one frame and one class; below / at the classes of the two data sets; every lane of the wave;
# 67 = one chunk of 64 clips and a tail; 130 = two chunks and a tail, all 64 classes
EVAL_CASES = [(1, 1, 1), (2, 12, 10), (5, 12, 14), (7, 1, 64), (67, 12, 10), (130, 12, 64)]


def _eval_inputs(clips, F_, K):
    """dyadic logits as test_clip_softmax_ce builds them (ties are exact; only the division by F rounds), an exact tie
    labelled low on clip 0 and high on clip 1, a wrong label on clip 2, labels -1 and K on clips 3 and 4"""
    g = torch.Generator().manual_seed(clips * 100 + F_ * 10 + K)
    base = dyadic(g, (clips, 1, K), 1 / 8, 76)
    logits = (base + dyadic(g, (clips, F_, K), 1 / 8, 4)).reshape(clips * F_, K)
    labels = torch.randint(0, K, (clips,), generator=g)
    if K > 1 and clips >= 2:
        lv = logits.view(clips, F_, K)
        top = lv.mean(1).argmax(1)
        for n, lab_low in ((0, True), (1, False)):
            a = int(top[n])
            b = (a + 1 + int(torch.randint(0, K - 1, (1,), generator=g))) % K
            lv[n, :, b] = lv[n, :, a]
            labels[n] = min(a, b) if lab_low else max(a, b)
        if clips >= 3:
            labels[2] = (int(lv[2].mean(0).argmax()) + 1) % K
    if clips >= 5:
        labels[3], labels[4] = -1, K
    return logits, labels


@pytest.mark.parametrize("case", EVAL_CASES, ids=lambda c: "clips%d_f%d_k%d" % c)
def test_clip_eval(device, case):
    from acimg import _lib
    lib = _lib.load()
    clips, F_, K = case
    logits, labels = _eval_inputs(clips, F_, K)
    ref = classify_ref.clip_eval(logits.numpy(), labels.numpy(), F_, K)
    if clips >= 5:
        assert ref["invalid"] == 2
    if K > 1 and clips >= 2:
        assert ref["clip_pred"][0] == labels[0] and ref["clip_pred"][1] < labels[1]      # the tie went to the lower index
    ldl = K + 3
    ld = widen(logits, ldl, fill=float("nan")).to(device)
    lab = labels.to(torch.int32).to(device)
    nstate = lib.acimg_clip_eval_state_bytes(K)
    assert nstate == 32 + 4 * K * K
    arena = GuardArena.for_sizes(device, [nstate, 4 * clips, 4 * clips])
    r_state = arena.region(nstate, fill=0, name="state")
    r_loss = arena.region(4 * clips, name="clip_loss")
    r_pred = arena.region(4 * clips, name="clip_pred")
    st = torch.cuda.current_stream(device).cuda_stream

    def call(loss_ptr, pred_ptr):
        _lib.check(lib.acimg_clip_eval(ld.data_ptr(), ldl, clips, F_, K, lab.data_ptr(), loss_ptr, pred_ptr, r_state.ptr,
                                       st), "clip_eval")

    def parse(raw):
        raw = raw.cpu().numpy()
        return (float(raw[:8].view(np.float64)[0]), [int(v) for v in raw[8:32].view(np.int64)],
                raw[32:].view(np.int32).reshape(K, K).astype(np.int64))

    def three_calls():
        """with both outputs, with neither, with both again: the state accumulates over the three"""
        r_state.fill(0)
        call(r_loss.ptr, r_pred.ptr)
        torch.cuda.synchronize(device)
        first = (r_loss.view(torch.float32, clips).cpu().clone(), r_pred.view(torch.int32, clips).cpu().clone())
        r_loss.fill(0x5A)
        r_pred.fill(0x5A)
        call(None, None)
        torch.cuda.synchronize(device)
        assert bool((r_loss.u8 == 0x5A).all()) and bool((r_pred.u8 == 0x5A).all()), "null outputs were written"
        call(r_loss.ptr, r_pred.ptr)
        torch.cuda.synchronize(device)
        arena.check("clip_eval %r" % (case,))
        third = (r_loss.view(torch.float32, clips).cpu().clone(), r_pred.view(torch.int32, clips).cpu().clone())
        assert torch.equal(first[0].view(torch.int32), third[0].view(torch.int32)) and torch.equal(first[1], third[1])
        return first, r_state.u8.clone()

    (loss, pred), state = three_calls()
    assert pred.tolist() == ref["clip_pred"].tolist()
    loss_ref = torch.from_numpy(ref["clip_loss"])
    print("clip_eval %r: clip_loss rel err %.2e" % (case, float((loss.double() - loss_ref).abs().max())
                                                     / max(float(loss_ref.abs().max()), 1e-12)))
    close(loss, loss_ref, what="clip_loss")
    valid = (labels >= 0) & (labels < K)
    assert not loss[~valid].any(), "an invalid clip's loss is not 0"
    loss_sum, (n_clips, n_correct, n_invalid), confusion = parse(state)
    assert (n_clips, n_correct, n_invalid) == (3 * ref["clips"], 3 * ref["correct"], 3 * ref["invalid"])
    assert np.array_equal(confusion, 3 * ref["confusion"])
    want = 0.0
    for _ in range(3):                      # the documented fold: clip order, onto the value already in the state
        want = classify_ref.fold(want, loss.numpy())
    assert loss_sum == want, (loss_sum, want)
    _, state2 = three_calls()
    assert torch.equal(state, state2), "two identical passes left different state"


def test_clip_evaluator(device):
    """the host wrapper: two updates, one read-back; accuracy from the integer counts"""
    from acimg.evaluate import ClipEvaluator
    clips, F_, K = 67, 12, 10
    logits, labels = _eval_inputs(clips, F_, K)
    ref = classify_ref.clip_eval(logits.numpy(), labels.numpy(), F_, K)
    ev = ClipEvaluator(device, K, F_)
    ld, lab = logits.float().to(device), labels.to(torch.int32).to(device)
    for _ in range(2):                      # a second pass after reset() starts from zero
        ev.reset()
        ev.update(None, ld, K, clips, lab)
        ev.update(None, ld[:24], K, 2, lab[:2])
        r = ev.result()
        first2 = classify_ref.clip_eval(logits.numpy()[:24], labels.numpy()[:2], F_, K)
        assert (r["clips"], r["correct"], r["invalid"]) == (ref["clips"] + 2, ref["correct"] + first2["correct"], 2)
        assert np.array_equal(r["confusion"], ref["confusion"] + first2["confusion"]) and r["confusion"].dtype == np.int64
        assert r["accuracy"] == r["correct"] / r["clips"] and r["loss"] == r["loss_sum"] / r["clips"]
        assert abs(r["loss_sum"] - (ref["loss_sum"] + first2["loss_sum"])) <= 2e-5 * ref["loss_sum"]


# ---- the loaders -------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def records(device, tmp_path_factory):
    """three GZIP files of one 12-frame record each (classes 2, 5, 8) and the 36 frames the frame-mode host loader makes
    of them (computed once, never written to)"""
    from acimg.data import TFRecordDataLoader
    paths = write_outdoor_records(tmp_path_factory.mktemp("clips"), 11, [(2 + 3 * r, 7 + r) for r in range(3)], wide=True)
    (frames,) = list(TFRecordDataLoader(paths, 64, device=device).data)
    assert frames[0].shape[0] == 36
    return paths, frames


def _clip_batch(frames, recs):
    """the clip batch of records `recs` cut from the frame-mode frames: one label row per clip"""
    rows = torch.cat([torch.arange(12) + 12 * r for r in recs])
    first = torch.tensor([12 * r for r in recs])
    return tuple(f[first] if k in (3, 4) else f[rows] for k, f in enumerate(frames))


def _equal(got, want, what):
    assert len(got) == 6 and len(want) == 6
    for k, (g, w) in enumerate(zip(got, want)):
        assert g.dtype == w.dtype and g.shape == w.shape, (what, k, g.shape, w.shape)
        assert torch.equal(g.cpu(), w.cpu()), (what, k)


def test_clip_mode_equals_frame_mode(device, records):
    from acimg.data import DeviceDataLoader, TFRecordDataLoader
    paths, frames = records
    host = TFRecordDataLoader(paths, 2, device=device, embedding=0)
    assert host.num_samples == 3 and host.total_batches == 2
    want = list(host.data)
    dl = DeviceDataLoader(paths, 2, device=device, embedding=0)
    assert dl.num_samples == 3 and dl.total_batches == 2
    got = [tuple(t.clone() for t in b) for b in dl.data]
    dl.close()
    assert [b[0].shape[0] for b in got] == [24, 12]                        # 2 + 1 clips
    for k, recs in enumerate(([0, 1], [2])):
        assert tuple(got[k][3].shape) == (len(recs), 10) and tuple(got[k][4].shape) == (len(recs), 61)
        assert all(t.device == device for t in got[k])
        _equal(got[k], want[k], "device against host loader, batch %d" % k)
        _equal(got[k], _clip_batch(frames, recs), "against the frame-mode frames, batch %d" % k)
    assert got[0][3].argmax(1).tolist() == [2, 5] and got[1][3].argmax(1).tolist() == [8]
    with pytest.raises(ValueError):
        DeviceDataLoader(paths, 2, device=device, embedding=2)


def test_clip_mode_shuffle(device, records):
    from acimg.data import DeviceDataLoader, epoch_files, epoch_rng, shuffle_order
    paths, frames = records

    def expected(seed, epoch, B):
        rng = epoch_rng(seed, epoch)
        files = epoch_files(paths, True, None, rng)                        # the file permutation comes first ...
        return [paths.index(files[i]) for i in shuffle_order(3, B, rng)]   # ... then the buffer, over records

    dl = DeviceDataLoader(paths, 2, shuffle=True, buffer_size=2, seed=4, device=device, embedding=0)
    orders = []
    for epoch in range(4):
        batches = [tuple(t.cpu() for t in b) for b in dl.data]
        order = expected(4, epoch, 2)
        assert sorted(order) == [0, 1, 2]                                  # each record once
        _equal(batches[0], _clip_batch(frames, order[:2]), "epoch %d, batch 0" % epoch)     # whole clips only
        _equal(batches[1], _clip_batch(frames, order[2:]), "epoch %d, batch 1" % epoch)
        orders.append(order)
    dl.close()
    assert len(set(map(tuple, orders))) > 1                                # reshuffle_each_iteration


def test_frame_mode_is_unchanged(device, records):
    """embedding=1, given or by default, yields today's tuples"""
    from acimg.data import DeviceDataLoader, TFRecordDataLoader
    paths, frames = records
    want = [tuple(f[i:i + 8] for f in frames) for i in range(0, 36, 8)]
    for kw in (dict(), dict(embedding=1)):
        host = list(TFRecordDataLoader(paths, 8, device=device, **kw).data)
        dl = DeviceDataLoader(paths, 8, device=device, **kw)
        assert dl.num_samples == 36 and dl.total_batches == 5
        got = [tuple(t.clone() for t in b) for b in dl.data]
        dl.close()
        assert len(got) == len(host) == len(want) == 5
        for g, h, w in zip(got, host, want):
            _equal(g, w, "device loader")
            _equal(h, w, "host loader")


# ---- the baseline sources ------------------------------------------------------------------------------------------------
rel = functools.partial(rel_err, floor=1e-30, same_shape=False)


def _baseline(device, source, lr=1e-3, epochs=1, K=K10):
    from acimg.dualcamnet import DualCamHybridModel
    from acimg.flags import FLAGS
    from acimg.session import Session
    from acimg.trainer_class import TrainerClass
    FLAGS.model = "DualCamNet"
    sess = Session(device)
    m = DualCamHybridModel(input_shape=[36, 48, 12], num_classes=K)
    tr = TrainerClass(m, None, None, learning_rate=lr, num_classes=K, num_epochs=epochs, session=sess, source=source)
    return tr, sess, m


@pytest.mark.parametrize("source", ["acoustic", "mfccmap"])
def test_baseline_step_against_the_oracle(device, source):
    """2 clips, K = 10, at the tolerances of test_dualcamnet_forward_backward: logits 1e-4, loss 1e-5, gradients 1e-3"""
    from oracle import dualcamnet as odc
    from oracle import tfsem
    lr = 1e-3
    tr, sess, m = _baseline(device, source, lr)
    tr._build_functions(batch_size=24)
    assert all(k.startswith("DualCamNet/") for k in sess.store.state_dict()) and len(sess.store.state_dict()) == 10
    params = odc.init_params(K10, seed=5, dtype=torch.float64, std=0.05, bias_std=0.05)
    m.initialize(state={k: v.float() for k, v in params.items()})
    gen = torch.Generator().manual_seed(6)
    labels = torch.tensor([3, 7])
    if source == "acoustic":
        x = torch.rand(24, 36, 48, 12, generator=gen, dtype=torch.float64)
        batch = (x.float().reshape(2, 12, 36, 48, 12), None, None, torch.nn.functional.one_hot(labels, K10).float())
    else:
        mfcc = torch.rand(24, 12, generator=gen, dtype=torch.float64).float()
        x = mfcc[:, None, None, :].expand(24, 36, 48, 12).double()
        batch = (None, mfcc, None, labels)
    before = sess.store.state_dict()
    got = tr.train_step(batch)
    g = tr.primary
    if source == "mfccmap":
        assert torch.equal(g.mfccmap.cpu(), x.float()), "the classifier's input is not tile(mfcc)"
    masks = {"conv1": (m.relu1.t > 0).cpu(), "conv2": (m.relu2.t > 0).cpu(), "conv3": (m.relu3.t > 0).cpu(),
             "full1": (m.relu4 > 0).cpu()}
    ref = odc.train_step_grads(params, x, labels, relu_masks=masks)
    assert rel(m.logits[:, :K10], ref["frame_logits"]) < 1e-4
    assert abs(got["loss"] - ref["loss"]) < 1e-5 * abs(ref["loss"]) + 1e-7, (got, ref["loss"])
    assert abs(got["accuracy"] - ref["accuracy"]) < 1e-6
    grads = sess.store.grad_dict()
    assert set(grads) == set(ref["grads"])
    for name, gref in ref["grads"].items():
        assert rel(grads[name].reshape(gref.shape), gref) < 1e-3, (name, rel(grads[name].reshape(gref.shape), gref))
    after = sess.store.state_dict()
    assert set(after) == set(before)
    for k in before:                        # TF-1 Adam, step 1, on every DualCamNet variable (there is nothing else)
        p2, _, _ = tfsem.adam_tf1(before[k].double(), grads[k].double().reshape(before[k].shape),
                                  torch.zeros_like(before[k]).double(), torch.zeros_like(before[k]).double(), 1, lr)
        assert float((after[k].double() - p2).abs().max()) <= 2e-6 * max(float(p2.abs().max()), 1e-3), k
        assert not torch.equal(before[k], after[k]), k
    ev = tr.eval_step(batch)                # the 4-tuple through the eval plan; weights have moved by one step
    assert np.isfinite(ev["loss"]) and ev["loss"] != got["loss"]


# ---- train() / test() ----------------------------------------------------------------------------------------------------
def _flags(tmp, exp="exp"):
    from acimg.flags import FLAGS
    FLAGS.model = "DualCamNet"
    FLAGS.checkpoint_dir, FLAGS.exp_name = str(tmp), exp
    FLAGS.restore_checkpoint = FLAGS.init_checkpoint = None
    FLAGS.acoustic_init_checkpoint = FLAGS.visual_init_checkpoint = None
    return FLAGS


def test_train_and_test_loops(device, records, tmp_path):
    from acimg import tfio
    from acimg.data import DeviceDataLoader
    from acimg.evaluate import ClipEvaluator
    from acimg.params import up4
    paths, _ = records
    FLAGS = _flags(tmp_path)
    tr, sess, m = _baseline(device, "acoustic", lr=1e-3, epochs=2)
    lines, passes = [], []
    tr.log = lines.append
    evaluate = tr._evaluate
    tr._evaluate = lambda *a: passes.append(evaluate(*a)) or passes[-1]
    train_data = DeviceDataLoader(paths, 2, shuffle=True, buffer_size=2, seed=1, device=device, embedding=0)
    valid_data = DeviceDataLoader(paths, 2, device=device, embedding=0)
    tr.train(train_data, valid_data)
    d = os.path.join(str(tmp_path), "exp")
    # --- log lines (:191-192, :205-209, :231-235): 2 iterations per epoch (2 + 1 clips), one validation line per epoch
    it = [ln for ln in lines if "Training_Loss" in ln]
    va = [ln for ln in lines if "- Epoch:" in ln]
    assert len(it) == 4 and len(va) == 2 and tr.global_step == 4 and len(passes) == 2
    assert re.search(r": exp - Iteration: \[  0\]\t Training_Loss: [0-9.]+\t Training_Accuracy: [0-9.]+$", it[0])
    assert re.search(r": exp - Iteration: \[  1\]\t Training_Loss: [0-9.]+\t Training_Accuracy: [0-9.]+$", it[3])
    for e, ln in enumerate(va):
        assert ln.endswith("exp - Epoch: {}\t Validation_Loss: {:6f}\t Validation_Accuracy: {:6f}".format(e, *passes[e]))
    assert tr.last_evaluation["clips"] == 3 and tr.last_evaluation["invalid"] == 0
    assert tr.last_evaluation["confusion"].sum() == 3 and set(np.nonzero(tr.last_evaluation["confusion"])[0]) <= {2, 5, 8}
    # --- best-epoch rule (:217): higher accuracy, or equal accuracy and lower-or-equal loss
    best_epoch, best_acc, best_loss, saved = -1, -1.0, 10000, {"epoch_random.ckpt"}
    for e, (loss, acc) in enumerate(passes):
        if acc > best_acc or (acc == best_acc and loss <= best_loss):
            best_epoch, best_acc, best_loss = e, acc, loss
            saved.add("epoch_%d.ckpt" % e)
    assert lines[-1].endswith("exp - Best Epoch: {}\t Validation_Loss: {:6f}\t Validation_Accuracy: {:6f}".format(
        best_epoch, best_loss, best_acc))
    txt = open(os.path.join(d, "model.txt")).read()
    assert txt.endswith(": exp\nBest Epoch: {}\nValidation_Loss: {:6f}\nValidation_Accuracy: {:6f}\n".format(
        best_epoch, best_loss, best_acc))
    assert set(f[:-6] for f in os.listdir(d) if f.endswith(".index")) == saved
    assert 'model_checkpoint_path: "epoch_%d.ckpt"' % best_epoch in open(os.path.join(d, "checkpoint")).read()
    # --- the bundle: the reference Saver's variable set, conv1 as the 5-D conv3d kernel
    ck = tfio.read_checkpoint(os.path.join(d, "epoch_%d.ckpt" % best_epoch), verify=True)
    names = list(sess.store.state_dict())
    assert set(ck) == set(names) | set(n + s for n in names for s in ("/Adam", "/Adam_1")) | {
        "beta1_power", "beta2_power", "global_step"}
    for sfx in ("", "/Adam", "/Adam_1"):
        assert ck["DualCamNet/conv1/weights" + sfx].shape == (12, 1, 1, 12, 12)
        assert ck["DualCamNet/full3/weights" + sfx].shape == (1000, 10)
    assert ck["global_step"].dtype == np.int64 and int(ck["global_step"]) == 2 * (best_epoch + 1)
    assert abs(float(ck["beta2_power"]) - 0.999 ** (2 * (best_epoch + 1) + 1)) < 1e-7
    assert float(np.abs(ck["DualCamNet/full1/weights/Adam"]).max()) > 0
    rnd = tfio.read_checkpoint(os.path.join(d, "epoch_random.ckpt"))
    assert int(rnd["global_step"]) == 0 and float(np.abs(rnd["DualCamNet/full1/weights/Adam"]).max()) == 0
    assert not np.array_equal(rnd["DualCamNet/conv1/weights"], ck["DualCamNet/conv1/weights"])
    # --- test(): both baseline sources restore the bundle and write their own file
    FLAGS.restore_checkpoint = os.path.join(d, "epoch_%d.ckpt" % best_epoch)
    test_data = DeviceDataLoader(paths, 2, device=device, embedding=0)
    for source, fname in (("acoustic", "test_accuracy_%d.txt"), ("mfccmap", "test_accuracy_mfccmap_%d.txt")):
        tr2, sess2, m2 = _baseline(device, source)
        out = []
        tr2.log = out.append
        got = tr2.test(test_data)
        for k, v in sess2.store.state_dict().items():
            assert np.array_equal(v.numpy().reshape(ck[k].shape), ck[k]), k
        r = tr2.last_evaluation
        assert got == r["loss"] and r["clips"] == 3
        text = open(os.path.join(d, fname % best_epoch)).read()
        assert text.endswith(": exp - Testing_Loss: {:6f}\nTesting_Accuracy: {:6f}".format(r["loss"], r["accuracy"]))
        assert out[-1] == text
        # the returned loss is that of a ClipEvaluator pass over the restored weights ...
        ev = ClipEvaluator(device, K10)
        loss_sum, acc_sum, size = 0.0, 0.0, 0
        for next_batch in test_data.data:
            batch = tr2._retrieve_batch(next_batch)
            step = tr2.eval_step(batch)                                     # ... and of the reference's per-batch form
            g = tr2._graph_for(tr2._clips_of(batch))
            ev.update(None, g.model.logits, up4(K10), g.clips, g.labels)
            n = batch[3].shape[0]
            size += n
            loss_sum += step["loss"] * n
            acc_sum += step["accuracy"] * n
        mine = ev.result()
        assert mine["loss"] == got and mine["correct"] == r["correct"] and np.array_equal(mine["confusion"], r["confusion"])
        print("%s: _evaluate loss %.9g, size-weighted mean of eval_step %.9g" % (source, got, loss_sum / size))
        # both sides run the same kernels: only the fp32 per-batch rounding of g.out separates them
        assert abs(got - loss_sum / size) <= 1e-6 * abs(loss_sum / size)
        assert abs(r["accuracy"] - acc_sum / size) <= 1e-6
    # --- Saver(max_to_keep=5): the oldest bundles are deleted
    for e in range(10, 16):
        tr._save_checkpoint(sess, e)
    left = [f for f in os.listdir(d) if f.endswith(".index")]
    assert len(left) == 5 and "epoch_random.ckpt.index" not in left and "epoch_15.ckpt.index" in left
    for loader in (train_data, valid_data, test_data):
        loader.close()


def test_frame_mode_loader_is_refused(device, records):
    from acimg.data import DeviceDataLoader
    paths, _ = records
    tr, sess, m = _baseline(device, "acoustic")
    tr._build_functions(batch_size=24)
    dl = DeviceDataLoader(paths, 24, device=device)
    with pytest.raises(ValueError, match="embedding=0"):
        tr._retrieve_batch(next(iter(dl.data)))
    dl.close()


# ---- the Trainer's bundle across the extraction of the shared writer ------------------------------------------------------
def _bundle_as_before(store, global_step, path, saved):
    """`Trainer._save_checkpoint`'s bundle-writing body as it stood before `write_saver_bundle` was cut out of it"""
    from acimg import tfio
    tensors = OrderedDict((k, v.numpy()) for k, v in store.state_dict().items())
    train = set(n for n in store.grad_dict())
    for which, sfx in (("m", "/Adam"), ("v", "/Adam_1")):
        for k, v in store.slot_dict(which).items():
            if k in train:
                tensors[k + sfx] = v.numpy()
    t = max(int(global_step), 0)
    tensors["beta1_power"] = np.float32(0.9 ** (t + 1))
    tensors["beta2_power"] = np.float32(0.999 ** (t + 1))
    tensors["global_step"] = np.int64(t)
    tfio.write_checkpoint(path, tensors)
    with open(os.path.join(os.path.dirname(path), "checkpoint"), "w") as f:
        f.write('model_checkpoint_path: "%s"\n' % os.path.basename(saved[-1]))
        for p in saved:
            f.write('all_model_checkpoint_paths: "%s"\n' % os.path.basename(p))


def test_trainer_checkpoint_bytes_are_unchanged(device, tmp_path):
    from oracle import trainer as otr
    _flags(tmp_path, "now")
    tr, sess = make(device)
    tr.log = lambda *a: None
    tr._build_functions(batch_size=2)
    tr.modelimages.initialize()
    tr.modelac.initialize()
    ac, mf, vid, eps = otr.synthetic_batch(2, seed=3)
    tr.train_step((ac, mf, vid), eps=eps)                # Adam slots and the step are no longer zero
    tr._save_checkpoint(sess, 0)
    path = tr._save_checkpoint(sess, 1)
    old = os.path.join(str(tmp_path), "before")
    os.makedirs(old)
    _bundle_as_before(sess.store, tr.global_step, os.path.join(old, "epoch_1.ckpt"), ["epoch_0.ckpt", "epoch_1.ckpt"])
    for name in ("epoch_1.ckpt.index", "epoch_1.ckpt.data-00000-of-00001", "checkpoint"):
        a = open(os.path.join(os.path.dirname(path), name), "rb").read()
        b = open(os.path.join(old, name), "rb").read()
        assert len(a) > 0 and a == b, name


# ---- compare ---------------------------------------------------------------------------------------------------------------
def test_compare_against_the_trainers(device, records, tmp_path):
    """one batch of 2 clips: `acc ac` is `TrainerClass(source="acoustic").test()`'s accuracy on the same checkpoint, `acc rec`
    that of `TrainerClass(source="generated")` on the same data and seed, or of source "mfccmap" under --mfccmap 1"""
    from acimg import classify
    from acimg.data import DeviceDataLoader
    from acimg.dualcamnet import DualCamHybridModel
    from acimg.session import Session
    from acimg.trainer_class import TrainerClass
    from acimg.unet_acresnet import UNetAc
    from acimg.vision import ResNet50Model
    from oracle import dualcamnet as odc
    paths, _ = records
    FLAGS = _flags(tmp_path, "gen")
    FLAGS.ae, FLAGS.num_skip_conn = 0, 1
    listing = str(tmp_path / "two.txt")
    with open(listing, "w") as f:
        f.write("\n".join(paths[:2]) + "\n")
    seed = 21
    # a generator + classifier checkpoint: every model at its initialisation, the classifier with weights that carry signal
    sess = Session(device)
    m = DualCamHybridModel(input_shape=[36, 48, 12], num_classes=K10)
    gen = TrainerClass(m, ResNet50Model(input_shape=[224, 298, 3], num_classes=None),
                       UNetAc(input_shape=[36, 48, 12], embedding=False, num_skip=1), num_classes=K10, session=sess,
                       source="generated")
    gen.log = lambda *a: None
    gen._build_functions(batch_size=24)
    gen._initialize()
    m.initialize(state=odc.init_params(K10, seed=8, dtype=torch.float32, std=0.05, bias_std=0.05))
    ckpt = gen._save_checkpoint(sess, 5)
    d = os.path.dirname(ckpt)
    data = DeviceDataLoader(listing, 2, device=device, embedding=0)
    gen.noise_seed, gen._noise_calls = seed, 0
    gen._evaluate(sess, "test", data)
    rec_want = gen.last_evaluation
    FLAGS.restore_checkpoint = ckpt
    want = {}
    for source in ("acoustic", "mfccmap"):
        tr, _, _ = _baseline(device, source)
        tr.log = lambda *a: None
        tr.test(data)
        want[source] = tr.last_evaluation
    data.close()
    assert rec_want["clips"] == want["acoustic"]["clips"] == 2
    for mfccmap, other, fname in ((0, rec_want, "test_unet5_dualcamnet5.txt"), (1, want["mfccmap"], "test_map_dualcamnet5.txt")):
        args = classify.build_compare_parser().parse_args(
            ["--mode", "compare", "--train_file", listing, "--init_checkpoint", ckpt, "--ac_checkpoint", ckpt,
             "--batch_size", "2", "--seed", str(seed), "--mfccmap", str(mfccmap), "--device", str(device)])
        doc = classify.run_compare(args, log=lambda *a: None)
        assert doc["files"] == (os.path.join(d, fname), os.path.join(d, "classification.json"))
        assert open(doc["files"][0]).read() == "acc rec {} acc ac {}".format(other["accuracy"], want["acoustic"]["accuracy"])
        saved = json.load(open(doc["files"][1]))
        assert saved == json.loads(json.dumps({k: v for k, v in doc.items() if k != "files"}))
        assert saved["scored"] == ("mfccmap" if mfccmap else "generated") and saved["seed"] == seed
        for part, ref in (("ac", want["acoustic"]), ("rec", other)):
            s = saved[part]
            assert s["confusion"] == ref["confusion"].tolist() and s["recall"] == classify_ref.per_class_recall(ref["confusion"])
            assert (s["clips"], s["correct"], s["invalid"]) == (ref["clips"], ref["correct"], ref["invalid"])
            assert s["accuracy"] == ref["correct"] / ref["clips"] and s["loss"] == ref["loss"]
            assert [k for k, v in enumerate(s["recall"]) if v is not None] == [2, 5]      # the two records' classes
    assert not [f for f in os.listdir(d) if f.endswith(".png")]
