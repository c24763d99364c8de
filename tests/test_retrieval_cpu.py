"""Latent-space evaluation, host side: the NumPy restatement against what the reference's knn.py / retrieve.py and
scikit-learn / SciPy computed (tests/golden/retrieval_golden.npz), the tools' paths and text formats, their refusals,
and the argument checks and workspace query of acimg_knn_topk / acimg_knn_vote (no device work)."""
import ctypes as C
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.dirname(os.path.abspath(__file__))
for p in (ROOT, os.path.join(ROOT, "acoustic-image-generation_amd"), HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

from acimg import _lib, features, retrieval  # noqa: E402
import retrieval_ref as ref  # noqa: E402

GOLDEN = os.path.join(HERE, "golden", "retrieval_golden.npz")
EINVAL, EWORKSPACE = -1, -2


@pytest.fixture(scope="module")
def golden():
    return dict(np.load(GOLDEN))


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def test_restatement_matches_sklearn_knn(golden):
    g = golden
    d2, idx = ref.kneighbors(g["test_x"], g["train_x"], 15)
    assert np.array_equal(idx, g["sk_kneighbors_idx"])
    np.testing.assert_allclose(np.sqrt(d2), g["sk_kneighbors_dist"], rtol=1e-9)
    pred = ref.vote(idx, g["train_y"].astype(int), 10)
    assert np.array_equal(pred, g["sk_pred"])
    assert ref.knn_line(pred, g["test_y"], 15) == str(g["knn_text"])
    assert int(g["vote_ties"]) > 0               # the tie rule decides some predictions


def test_vote_tie_goes_to_the_smallest_class():
    assert ref.vote(np.array([[0, 1, 2, 3]]), np.array([3, 1, 3, 1]), 4)[0] == 1
    assert ref.vote(np.array([[0, -1, 1]]), np.array([5, 2]), 6)[0] == 2


def test_restatement_matches_reference_retrieval(golden):
    g = golden
    y = g["ret_y"].astype(int)
    text, ranks, cm1, cm5, cm10 = ref.retrieval(g["audio_x"], g["video_x"], y, 10)
    assert text == str(g["retrieval_text"])
    _, idx = ref.kneighbors(g["audio_x"], g["video_x"], 31)
    assert np.array_equal(idx, g["cdist_order"])
    fh = ref.first_hit(idx[:, :30], y, y)
    assert (fh == 0).sum() == 1 and y[fh == 0][0] == 9   # the lone class-9 anchor
    for r in (1, 2, 5, 10, 30):
        assert ranks[r] == int(((fh >= 1) & (fh <= r)).sum())
    # the tool's own summary from first hits + neighbours reproduces the text and the matrices
    s = retrieval.retrieval_summary(fh, idx[:, :30], y, 10)
    assert s["text"] == str(g["retrieval_text"])
    for name, m in (("confusion_matrix1", cm1), ("confusion_matrix5", cm5), ("confusion_matrix10", cm10)):
        for i in range(10):
            assert s[name][i] == [float(v) for v in m[i]]


def test_retrieval_summary_null_rows_and_format():
    labels = np.array([0, 0, 2, 2, 2, 0, 2, 0, 2, 0, 0, 2])
    nb = np.tile(np.arange(12), (12, 1))
    fh = np.array([1, 0, 3, 30, 2, 5, 11, 10, 0, 1, 2, 6])
    s = retrieval.retrieval_summary(fh, nb, labels, 3)
    assert s["confusion_matrix1"][1] is None and s["num_samples_class"] == [6, 0, 6]
    assert s["rank_counts"] == {"1": 2, "2": 4, "5": 6, "10": 8, "30": 10}
    assert s["text"] == "Accuracy 0.166667 rank2 0.333333 rank5 0.500000 rank10 0.666667 rank30 0.833333"
    assert abs(sum(s["confusion_matrix10"][0]) - 1.0) < 1e-12
    assert retrieval.knn_accuracy_line([1, 2, 3], [1, 2, 0], 15) == "Accuracy=0.6666666666666666 k=15\n"


def test_tool_paths():
    ck = "/data/run/epoch_12.ckpt"
    assert retrieval.dump_dir(ck, "training", "Video") == "/data/run/training_Video_12"
    assert retrieval.knn_value_file(ck, "Video", "testing") == "/data/run/testing_Video_12_testing_knn_value.txt"
    assert (retrieval.retrieval_file(ck, "Audio", "Video", "testing") ==
            "/data/run/testing_Audio_12_Audio_Video_testing_retrieval.txt")
    a = features.parse_args(["--train_file", "/lists/testing.txt", "--init_checkpoint", ck, "--encoder_type", "Audio"])
    assert features.output_dir(a) == "/data/run/testing_Audio_12"
    assert features.output_files(a) == tuple("/data/run/testing_Audio_12/testing_%s.npy" % k
                                             for k in ("data", "labels", "scenario"))
    assert (a.batch_size, a.num_skip_conn, a.ae, a.datatype, a.seed) == (2, 1, 0, "outdoor", 0)
    assert [retrieval.num_classes(t) for t in ("outdoor", "music", "old")] == [10, 9, 14]
    r = retrieval.build_parser().parse_args(["retrieve", ck, "Audio", "Video", "testing", "music"])
    assert (r.tool, r.anchor, r.gallery, r.set, r.datatype) == ("retrieve", "Audio", "Video", "testing", "music")
    k = retrieval.build_parser().parse_args(["knn", ck, "Video", "testing"])
    assert (k.tool, k.encoder_type, k.set, k.k) == ("knn", "Video", "testing", 15)


def write_dump(d, name, x, y, ncls=10):
    os.makedirs(d, exist_ok=True)
    oh = np.zeros((len(y), ncls), dtype=int)
    oh[np.arange(len(y)), y] = 1
    np.save(os.path.join(d, name + "_data.npy"), np.asarray(x, np.float64))
    np.save(os.path.join(d, name + "_labels.npy"), oh)


def test_retrieve_refuses_different_label_arrays(tmp_path):
    rng = np.random.RandomState(0)
    ck = str(tmp_path / "epoch_1.ckpt")
    y = rng.randint(0, 10, 20)
    write_dump(retrieval.dump_dir(ck, "testing", "Audio"), "testing", rng.randn(20, 4), y)
    y2 = y.copy()
    y2[3] = (y2[3] + 1) % 10
    write_dump(retrieval.dump_dir(ck, "testing", "Video"), "testing", rng.randn(20, 4), y2)
    with pytest.raises(ValueError, match="label arrays differ"):
        retrieval.run_retrieve(ck, "Audio", "Video", "testing", "outdoor", log=lambda *a: None)
    write_dump(retrieval.dump_dir(ck, "testing", "Video"), "testing", rng.randn(21, 4), np.append(y, 1))
    with pytest.raises(ValueError, match="label arrays differ"):
        retrieval.run_retrieve(ck, "Audio", "Video", "testing", "outdoor", log=lambda *a: None)
    with pytest.raises(FileNotFoundError):
        retrieval.run_knn(ck, "Audio", "testing", log=lambda *a: None)


def test_features_refuses_old_datatype():
    a = features.parse_args(["--train_file", "x/testing.txt", "--init_checkpoint", "x/epoch_1.ckpt", "--datatype", "old"])
    with pytest.raises(ValueError, match="old"):
        features.run(a, trainer=SimpleNamespace())


def _topk(lib, Q=4, G=100, D=8, K=5, ldq=None, ldg=None, ws_bytes=0, null=False):
    fake = None if null else C.c_void_p(4096)
    return lib.acimg_knn_topk(fake, ldq if ldq is not None else D, Q, fake, ldg if ldg is not None else D, G, D, K, fake,
                              fake, fake, ws_bytes, None)


def test_knn_topk_argument_checks(lib):
    for kw in (dict(K=0), dict(K=65), dict(D=0), dict(ldq=7), dict(ldg=7), dict(G=0), dict(Q=-1)):
        assert _topk(lib, **kw) == EINVAL, kw
        assert _lib.last_error().startswith("knn_topk")
    assert "K = 65" in (_topk(lib, K=65), _lib.last_error())[1]
    assert _topk(lib, Q=0) == 0 and _topk(lib, Q=0, null=True) == 0      # a no-op
    assert _topk(lib, null=True) == EINVAL
    # small Q against a large gallery splits it into slabs: a workspace is needed, and a short one is refused
    need = lib.acimg_knn_topk_workspace(1, 50000, 150, 30)
    assert need > 0 and need % (30 * 12) == 0
    assert _topk(lib, Q=1, G=50000, D=150, K=30, ws_bytes=need - 1) == EWORKSPACE
    assert "workspace" in _lib.last_error()


def test_knn_topk_workspace_query(lib):
    ws = lib.acimg_knn_topk_workspace
    assert ws(0, 1000, 8, 5) == 0 and ws(4, 1000, 8, 0) == 0 and ws(4, 0, 8, 5) == 0 and ws(4, 10, 0, 5) == 0
    assert ws(100000, 100000, 1024, 30) == 0        # enough query blocks: one pass, written in place
    assert ws(1, 64, 8, 5) == 0                     # a single gallery tile: nothing to split
    assert ws(63, 50000, 150, 64) > ws(63, 50000, 150, 1) > 0
    assert ws(63, 50000, 12, 30) == ws(63, 50000, 1024, 30)      # D does not enter


def test_knn_vote_argument_checks(lib):
    fake = C.c_void_p(4096)
    v = lib.acimg_knn_vote
    assert v(fake, 5, 3, 0, fake, fake, 10, fake, fake, None) == EINVAL
    assert v(fake, 65, 3, 65, fake, fake, 10, fake, fake, None) == EINVAL
    assert v(fake, 4, 3, 5, fake, fake, 10, fake, fake, None) == EINVAL
    assert v(fake, 5, 3, 5, fake, fake, 0, fake, fake, None) == EINVAL
    assert v(fake, 5, 3, 5, fake, fake, 65, fake, fake, None) == EINVAL
    assert v(fake, 5, 3, 5, fake, None, 10, None, fake, None) == EINVAL     # first_hit needs query labels
    assert _lib.last_error().startswith("knn_vote")
    assert v(fake, 5, 0, 5, fake, fake, 10, fake, fake, None) == 0
    assert v(fake, 5, 3, 5, fake, None, 10, None, None, None) == 0          # nothing requested
