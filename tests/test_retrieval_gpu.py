"""Latent-space evaluation on the device: `acimg_knn_topk` / `acimg_knn_vote` against the NumPy restatement (bit for bit
on integer-valued features, where every sum is exact in any order and ties are plentiful; to 1e-12 on random fp64),
against what the reference's knn.py / retrieve.py wrote (tests/golden/retrieval_golden.npz), run-to-run repeatability,
`Trainer.features` against the oracle's mean + std * eps, and the chain `acimg.features` -> `acimg.retrieval knn` ->
`acimg.retrieval retrieve` on records and a checkpoint."""
import json
import os
import sys
from collections import OrderedDict

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import retrieval_ref as ref  # noqa: E402
from data_support import outdoor_record  # noqa: E402
from retrieval_ref import int_features  # noqa: E402

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(HERE, "golden", "retrieval_golden.npz")


def run_topk(device, q, g, K, ldq=None, ldg=None):
    from acimg import ops
    Q, D = q.shape
    G = g.shape[0]
    ldq, ldg = ldq or D, ldg or D
    qb = torch.full((Q, ldq), float("nan"), dtype=torch.float64)   # pad columns must never be read
    gb = torch.full((G, ldg), float("nan"), dtype=torch.float64)
    qb[:, :D] = torch.from_numpy(q)
    gb[:, :D] = torch.from_numpy(g)
    qb, gb = qb.to(device), gb.to(device)
    dist2 = torch.full((Q, K), -5.0, dtype=torch.float64, device=device)
    idx = torch.full((Q, K), -7, dtype=torch.int32, device=device)
    plan = ops.Plan(device, eager=True)
    ops.knn_topk(plan, qb, ldq, Q, gb, ldg, G, D, K, dist2, idx)
    torch.cuda.synchronize(device)
    return dist2.cpu().numpy(), idx.cpu().numpy()


# (Q, G, D, K, ld pad): every Q, G, D and K of the plan, slab split and merge, -1 / +inf padding, ld > D
EXACT_CASES = [
    (1, 50000, 150, 64, 0), (63, 50000, 12, 30, 0), (700, 50000, 1, 15, 3), (1, 50000, 1031, 1, 0),
    (700, 1000, 1024, 15, 0), (63, 1000, 1031, 64, 5), (1, 1000, 12, 30, 1), (700, 1000, 150, 1, 0),
    (63, 61, 150, 64, 0), (700, 12, 1031, 15, 2), (1, 27, 1, 30, 0), (63, 1000, 150, 1, 7),
]


@pytest.mark.parametrize("Q,G,D,K,pad", EXACT_CASES)
def test_topk_exact_on_integer_features(device, Q, G, D, K, pad):
    rng = np.random.RandomState(Q * 7 + G + D + K)
    q, g = int_features(rng, Q, G, D)
    d2, idx = run_topk(device, q, g, K, ldq=D + pad if pad else None, ldg=D + 2 * pad if pad else None)
    want_d, want_i = ref.kneighbors(q, g, K)
    assert np.array_equal(idx, want_i)
    assert np.array_equal(d2, want_d)
    if K > G:
        assert (idx[:, G:] == -1).all() and np.isinf(d2[:, G:]).all()


def test_topk_random_fp64(device):
    rng = np.random.RandomState(3)
    q, g = rng.randn(200, 150) * 3.0, rng.randn(20000, 150) * 3.0 + 0.5
    d2, idx = run_topk(device, q, g, 30)
    want_d, want_i = ref.kneighbors(q, g, 30)
    np.testing.assert_allclose(d2, want_d, rtol=1e-12, atol=0)
    # indices agree except where the restatement's adjacent distances are within 1e-12 relative
    close = np.zeros_like(want_d, dtype=bool)
    near = np.abs(np.diff(want_d, axis=1)) <= 1e-12 * want_d[:, 1:]
    close[:, 1:] |= near
    close[:, :-1] |= near
    assert np.array_equal(idx[~close], want_i[~close])


def test_topk_is_repeatable(device):
    rng = np.random.RandomState(4)
    q, g = rng.randn(40, 150), rng.randn(30000, 150)
    a = run_topk(device, q, g, 64)
    b = run_topk(device, q, g, 64)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def test_vote_tie_rule_and_first_hit(device):
    from acimg import ops
    idx = np.array([[0, 1, 2, 3, -1], [4, 4, 5, 5, 6], [6, 6, 6, 0, 1], [-1, -1, 2, 3, 0]], np.int32)
    gl = np.array([3, 1, 3, 1, 7, 2, 0], np.int32)
    ql = np.array([1, 9, 3, 3], np.int32)
    t = [torch.from_numpy(v).to(device) for v in (idx, gl, ql)]
    pred = torch.full((4,), -9, dtype=torch.int32, device=device)
    hit = torch.full((4,), -9, dtype=torch.int32, device=device)
    plan = ops.Plan(device, eager=True)
    ops.knn_vote(plan, t[0], 5, 4, 4, t[1], t[2], 10, pred, hit)    # K = 4 of ldidx = 5
    torch.cuda.synchronize(device)
    assert pred.cpu().tolist() == [1, 2, 0, 1]
    assert hit.cpu().tolist() == [2, 0, 4, 3]
    assert list(ref.vote(idx[:, :4], gl, 10)) == [1, 2, 0, 1]
    assert list(ref.first_hit(idx[:, :4], gl, ql)) == [2, 0, 4, 3]


def test_knn_and_retrieve_match_the_reference_golden(device, tmp_path):
    from acimg import retrieval
    g = dict(np.load(GOLDEN))
    nn = retrieval.NearestNeighbours(device)
    pred = nn.knn_predict(g["train_x"], g["train_y"].astype(int), g["test_x"], k=15)
    assert np.array_equal(pred, g["sk_pred"])
    _, idx = nn.kneighbors(torch.from_numpy(g["test_x"].astype(np.float64)).to(device), g["train_x"], 15)
    assert np.array_equal(idx.cpu().numpy(), g["sk_kneighbors_idx"])
    # the tools on the dumps the reference scripts read
    ck = str(tmp_path / "ckpt" / "epoch_3.ckpt")

    def dump(dataset, enc, x, y):
        d = retrieval.dump_dir(ck, dataset, enc)
        os.makedirs(d)
        oh = np.zeros((len(y), 10), dtype=int)
        oh[np.arange(len(y)), y.astype(int)] = 1
        np.save("%s/%s_data.npy" % (d, dataset), x.astype(np.float64))
        np.save("%s/%s_labels.npy" % (d, dataset), oh)
        np.save("%s/%s_scenario.npy" % (d, dataset), np.zeros((len(y), 61), dtype=int))

    dump("training", "Video", g["train_x"], g["train_y"])
    dump("testing", "Video", g["test_x"], g["test_y"])
    dump("validation", "Audio", g["audio_x"], g["ret_y"])
    dump("validation", "Video", g["video_x"], g["ret_y"])
    quiet = dict(log=lambda *a: None)
    assert retrieval.main(["knn", ck, "Video", "testing"]) == 0
    with open(retrieval.knn_value_file(ck, "Video", "testing")) as f:
        assert f.read() == str(g["knn_text"])
    assert retrieval.main(["retrieve", ck, "Audio", "Video", "validation", "outdoor"]) == 0
    with open(retrieval.retrieval_file(ck, "Audio", "Video", "validation")) as f:
        assert f.read() == str(g["retrieval_text"])
    res = retrieval.run_retrieve(ck, "Audio", "Video", "validation", "outdoor", nn=nn, **quiet)
    y = g["ret_y"].astype(int)
    fh = np.array(res["first_hit"])
    assert (fh == 0).sum() == 1 and y[fh == 0][0] == 9
    text, ranks, cm1, cm5, cm10 = ref.retrieval(g["audio_x"], g["video_x"], y, 10)
    assert res["rank_counts"] == {str(r): n for r, n in ranks.items()}
    with open(os.path.join(retrieval.dump_dir(ck, "validation", "Video"), "retrieval.json")) as f:
        js = json.load(f)
    for name, m in (("confusion_matrix1", cm1), ("confusion_matrix5", cm5), ("confusion_matrix10", cm10)):
        assert js[name] == [None if np.isnan(r).all() else [float(v) for v in r] for r in m]
    with open(os.path.join(retrieval.dump_dir(ck, "testing", "Video"), "knn.json")) as f:
        kj = json.load(f)
    assert kj["predictions"] == [int(v) for v in g["sk_pred"]] and kj["k"] == 15


# ---- the extractor ---------------------------------------------------------------------------------------------------
def fresh_trainer_state(device, rng):
    from acimg.flags import FLAGS
    from acimg.session import Session
    from acimg.trainer import Trainer
    from acimg.unet_acresnet import UNetAc
    from acimg.vision import ResNet50Model
    FLAGS.model, FLAGS.ae, FLAGS.latent_loss = "UNet", 0, 1e-6
    src = Trainer(UNetAc(input_shape=[36, 48, 12], embedding=False, num_skip=1),
                  ResNet50Model(input_shape=[224, 298, 3], num_classes=None), session=Session(device))
    src._build_functions(batch_size=2)
    src.modelimages.initialize()
    src.modelac.initialize()
    state = OrderedDict((k, v.numpy()) for k, v in src.session.store.state_dict().items())
    for k in state:
        if k.endswith("/moving_mean"):
            state[k] = (rng.randn(*state[k].shape) * 0.05).astype(np.float32)
        elif k.endswith("/moving_variance"):
            state[k] = rng.uniform(0.5, 2.0, size=state[k].shape).astype(np.float32)
    return state


def test_trainer_features_match_the_oracle(device):
    from acimg.flags import FLAGS
    from acimg.session import Session
    from acimg.trainer import Trainer
    from acimg.unet_acresnet import UNetAc
    from acimg.vision import ResNet50Model
    from oracle import trainer as otr

    FLAGS.model, FLAGS.ae = "UNet", 0
    orc = otr.Oracle(num_skip=1, randomize=True)
    tr = Trainer(UNetAc(input_shape=[36, 48, 12], embedding=False, num_skip=1),
                 ResNet50Model(input_shape=[224, 298, 3], num_classes=None), session=Session(device))
    tr._build_functions(batch_size=2)
    tr.session.store.load_state(orc.state_dict(), strict=True)
    ac, mf, vid, eps = otr.synthetic_batch(2, seed=17)
    for n in (2, 1):                                   # the primary graph and a partial batch
        batch = (ac[:n], mf[:n], vid[:n])
        z = tr.features(batch, eps=eps[:n]).double().cpu()
        with torch.no_grad():
            mean, std, _, _ = orc.forward(vid[:n], mf[:n], eps[:n], False)
        want = (mean + std * eps[:n]).double()
        assert z.shape == (n, 150)
        assert float((z - want).abs().max() / want.abs().max()) < 1e-3, n
        # the z the decoder of the generate plan consumed: the same latent
        tr.generate(batch, eps=eps[:n])
        assert torch.equal(tr._graph_for(n).modelac.zbuf[:, :150].double().cpu(), z)


def test_extract_knn_retrieve_end_to_end(device, tmp_path):
    from acimg import features, localize, retrieval, tfio
    rng = np.random.RandomState(23)
    ckdir = tmp_path / "ckpt"
    ckdir.mkdir()
    ckpt = str(ckdir / "epoch_5.ckpt")
    tfio.write_checkpoint(ckpt, fresh_trainer_state(device, rng))
    recs = {"training": [(2, 7), (4, 60)], "testing": [(4, 1), (9, 0)]}
    for name, rr in recs.items():
        paths = []
        for i, (cls, loc) in enumerate(rr):
            p = str(tmp_path / ("%s%d.tfrecord" % (name, i)))
            tfio.write_tfrecord(p, [outdoor_record(rng, cls, loc, wide=False)], compression="GZIP")
            paths.append(p)
        (tmp_path / ("%s.txt" % name)).write_text("\n".join(paths) + "\n")
    quiet = dict(log=lambda *a: None)
    tr = None
    out = {}
    for name in ("training", "testing"):
        for enc in ("Video", "Audio"):
            a = features.parse_args(["--train_file", str(tmp_path / ("%s.txt" % name)), "--init_checkpoint", ckpt,
                                     "--encoder_type", enc, "--batch_size", "5", "--seed", "3"])
            tr = tr or localize.build_trainer(a, torch.device(device))
            out[name, enc] = features.run(a, trainer=tr, **quiet)
            d = "%s/%s_%s_5" % (ckdir, name, enc)
            assert out[name, enc]["files"] == tuple("%s/%s_%s.npy" % (d, name, k) for k in ("data", "labels", "scenario"))
            x, y, s = (np.load(f) for f in out[name, enc]["files"])
            assert x.shape == (24, 150) and x.dtype == np.float64 and np.isfinite(x).all()
            assert y.shape == (24, 10) and s.shape == (24, 61) and y.dtype.kind == "i" and s.dtype.kind == "i"
            cls = np.repeat([c for c, _ in recs[name]], 12)
            loc = np.repeat([l for _, l in recs[name]], 12)
            assert np.array_equal(y, np.eye(10, dtype=int)[cls]) and np.array_equal(s, np.eye(61, dtype=int)[loc])
    # same seed, same records: the two "encoders" extracted the same latents
    assert np.array_equal(out["testing", "Video"]["data"], out["testing", "Audio"]["data"])
    assert retrieval.main(["knn", ckpt, "Video", "testing"]) == 0
    ftr, fte = out["training", "Video"]["data"], out["testing", "Video"]["data"]
    ytr, yte = out["training", "Video"]["labels"].argmax(1), out["testing", "Video"]["labels"].argmax(1)
    pred = ref.vote(ref.kneighbors(fte, ftr, 15)[1], ytr, 10)
    with open(retrieval.knn_value_file(ckpt, "Video", "testing")) as f:
        assert f.read() == ref.knn_line(pred, yte, 15)
    with open("%s/testing_Video_5/knn.json" % ckdir) as f:
        assert json.load(f)["predictions"] == [int(v) for v in pred]
    assert retrieval.main(["retrieve", ckpt, "Audio", "Video", "testing", "outdoor"]) == 0
    text, ranks, cm1, _, cm10 = ref.retrieval(out["testing", "Audio"]["data"], fte, yte, 10)
    with open(retrieval.retrieval_file(ckpt, "Audio", "Video", "testing")) as f:
        assert f.read() == text
    with open("%s/testing_Video_5/retrieval.json" % ckdir) as f:
        js = json.load(f)
    assert js["rank_counts"] == {str(r): n for r, n in ranks.items()}
    assert js["confusion_matrix1"] == [None if np.isnan(r).all() else [float(v) for v in r] for r in cm1]
    assert js["confusion_matrix10"] == [None if np.isnan(r).all() else [float(v) for v in r] for r in cm10]
