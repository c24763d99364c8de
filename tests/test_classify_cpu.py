"""The device-free half of the classification experiment: the fp64 restatement of the clip evaluation against hand-computed
cases and sklearn, the clip-mode ordering of the loaders' page logic on a fake pool, and the C ABI of `acimg_clip_eval`
(every refusal precedes the launch)."""
import math

import numpy as np
import pytest

import classify_ref
from data_support import FakePool


# ---- the restatement -------------------------------------------------------------------------------------------------
def test_restatement_on_hand_computed_cases():
    F, K = 2, 3
    # clip 0: means (1, 1, 0): exact tie at classes 0 and 1, labelled 0 -> predicted 0, correct
    # clip 1: the same tie labelled 1 -> predicted 0, wrong
    # clip 2: means (0, 0, 2), labelled 2 -> correct;  clip 3: label 3 = K, clip 4: label -1 -> invalid
    tie = [[2.0, 0.0, 0.0], [0.0, 2.0, 0.0]]
    top = [[0.0, 0.0, 1.0], [0.0, 0.0, 3.0]]
    logits = np.array(tie + tie + top + top + tie)
    r = classify_ref.clip_eval(logits, [0, 1, 2, 3, -1], F, K)
    l_tie = math.log(2 * math.e + 1) - 1.0                      # -log(e / (e + e + 1))
    l_top = math.log(2 + math.e ** 2) - 2.0
    assert r["clip_pred"].tolist() == [0, 0, 2, 2, 0]
    # fp64 on both sides; log-sum-exp minus the label's logit cancels a few units, so a few ulp of ~3 remain: 1e-14
    np.testing.assert_allclose(r["clip_loss"], [l_tie, l_tie, l_top, 0.0, 0.0], rtol=1e-14, atol=0)
    assert (r["clips"], r["correct"], r["invalid"]) == (3, 2, 2)
    assert r["confusion"].tolist() == [[1, 0, 0], [1, 0, 0], [0, 0, 1]]
    assert abs(r["loss_sum"] - (2 * l_tie + l_top)) < 1e-14
    assert classify_ref.per_class_recall(r["confusion"]) == [1.0, 0.0, 1.0]
    assert classify_ref.per_class_recall([[0, 0], [1, 3]]) == [None, 0.75]


def test_restatement_with_one_class():
    r = classify_ref.clip_eval(np.array([[3.0], [5.0], [-2.0], [-2.0]]), [0, 1], 2, 1)
    assert r["clip_pred"].tolist() == [0, 0] and r["clip_loss"].tolist() == [0.0, 0.0]
    assert (r["clips"], r["correct"], r["invalid"]) == (1, 1, 1) and r["confusion"].tolist() == [[1]]


def test_restatement_against_sklearn():
    metrics = pytest.importorskip("sklearn.metrics")
    rng = np.random.default_rng(5)
    clips, F, K = 200, 12, 10
    logits = rng.integers(-8, 9, (clips * F, K)) / 4.0           # dyadic: ties happen and are exact
    labels = rng.integers(0, K, clips)
    r = classify_ref.clip_eval(logits, labels, F, K)
    cm = metrics.confusion_matrix(labels, r["clip_pred"], labels=list(range(K)))
    assert np.array_equal(cm, r["confusion"])
    assert r["correct"] == int(round(metrics.accuracy_score(labels, r["clip_pred"]) * clips))
    m = classify_ref.clip_means(logits, clips, F)
    p = np.exp(m - m.max(1, keepdims=True))
    p /= p.sum(1, keepdims=True)
    assert abs(r["loss_sum"] / clips - metrics.log_loss(labels, p, labels=list(range(K)))) < 1e-12


def test_fold_is_sequential():
    vals = np.array([1e8, 1.0, -1e8, 1.0], dtype=np.float32)
    assert classify_ref.fold(0.5, vals) == ((((0.5 + 1e8) + 1.0) - 1e8) + 1.0)


# ---- clip-mode ordering ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_records,B", [(1, 1), (7, 1), (7, 3), (20, 3), (20, 50), (100, 16)])
@pytest.mark.parametrize("batch,prefetch,first", [(2, 2, 16), (5, 0, 1), (64, 1, 4)])
def test_clip_mode_page_bookkeeping_on_a_fake_pool(n_records, B, batch, prefetch, first):
    """whole records of 12 frames as the shuffle units: every batch consists of whole records with their frames in order,
    no page is uploaded into while one of its frames waits to be gathered (FakePool.upload asserts it), the records leave
    in `shuffle_order` over records, and buffer_size + prefetch + 2 pages - buffer_size counting records - are never
    exceeded"""
    from acimg.data import BatchFeeder, FramePages, epoch_rng, pool_pages, shuffle_order
    F = 12
    limit = pool_pages(B, prefetch)
    assert limit == B + prefetch + 2
    pool = FakePool(F)
    pages = FramePages(first, limit, F)
    grown = []
    feeder = BatchFeeder(iter([F] * n_records), pages, batch, B, prefetch, epoch_rng(3, 0), pool.upload, pool.gather,
                         grow=grown.append, units="records")
    sizes, seen = [], 0
    for got in feeder:
        sizes.append(got)
        assert not pages.pending
        covered = sorted(pool.rows)
        assert covered[0][0] == 0 and sum(c for _, c in covered) == got
        assert all(a[0] + a[1] == b[0] for a, b in zip(covered, covered[1:]))
        pool.rows = []
        rows = pool.emitted[seen:]
        seen = len(pool.emitted)
        assert len(rows) == got and got % F == 0
        for c in range(got // F):                               # a whole record, its frames consecutive and in order
            clip = rows[c * F:(c + 1) * F]
            assert clip[0] % F == 0 and clip == list(range(clip[0], clip[0] + F))
    assert sizes == [batch * F] * (n_records // batch) + ([(n_records % batch) * F] if n_records % batch else [])
    assert [f // F for f in pool.emitted[::F]] == shuffle_order(n_records, B, epoch_rng(3, 0))
    assert pages.size <= limit and len(pool.pages_seen) <= limit and max(pool.pages_seen) < pages.size
    assert all(g <= limit for g in grown) and grown == sorted(grown)
    assert not any(pool.resident.values()) and not any(pages.live)


def test_clip_mode_order_follows_the_permuted_file_list():
    """one record per file: the order of a pass = shuffle_order over records applied to the permuted file list, both
    drawn from the pass's one generator, file permutation first"""
    from acimg.data import BatchFeeder, FramePages, epoch_files, epoch_rng, pool_pages, shuffle_order
    files = ["f%d" % i for i in range(9)]
    rng = epoch_rng(11, 2)
    perm = epoch_files(files, True, None, rng)
    pool = FakePool(12)
    emitted_files = []
    uploaded = []

    def upload(page, rec):
        uploaded.append(rec)
        return pool.upload(page, 12)
    list(BatchFeeder(iter(perm), FramePages(16, pool_pages(4, 2), 12), 2, 4, 2, rng, upload, pool.gather, units="records"))
    emitted_files = [uploaded[f // 12] for f in pool.emitted[::12]]
    rng2 = epoch_rng(11, 2)
    perm2 = epoch_files(files, True, None, rng2)
    assert perm2 == perm and sorted(perm) == files
    assert emitted_files == [perm2[i] for i in shuffle_order(9, 4, rng2)]
    assert sorted(emitted_files) == files


def test_frame_mode_is_the_default_unit():
    from acimg.data import BatchFeeder, FramePages, epoch_rng, shuffle_order
    pool = FakePool(12)
    list(BatchFeeder(iter([12] * 4), FramePages(16, 9, 12), 5, 5, 2, epoch_rng(1, 0), pool.upload, pool.gather))
    assert pool.emitted == shuffle_order(48, 5, epoch_rng(1, 0))
    with pytest.raises(ValueError):
        BatchFeeder(iter([]), FramePages(1, 1, 12), 1, 1, 0, epoch_rng(0, 0), pool.upload, pool.gather, units="clips")


# ---- the C ABI without a GPU -------------------------------------------------------------------------------------------
def _eval(lib, ldl=13, clips=2, F=12, K=10, null=None, state=4096 * 6):
    """acimg_clip_eval on addresses that are never dereferenced: every case here is refused before the launch"""
    ptr = dict(logits=4096, labels=4096 * 2, clip_loss=4096 * 3, clip_pred=4096 * 4, state=state)
    if null is not None:
        ptr[null] = None
    return lib.acimg_clip_eval(ptr["logits"], ldl, clips, F, K, ptr["labels"], ptr["clip_loss"], ptr["clip_pred"],
                               ptr["state"], None)


def test_clip_eval_refusals_and_state_query():
    from acimg import _lib
    lib = _lib.load()
    EINVAL = -1
    assert lib.acimg_version() == 207
    # double loss_sum + int64 clips, correct, invalid + int32 confusion[K][K]
    for K in (1, 2, 10, 14, 63, 64):
        assert lib.acimg_clip_eval_state_bytes(K) == 8 + 3 * 8 + 4 * K * K
    for K in (0, -1, 65, 1 << 20):
        assert lib.acimg_clip_eval_state_bytes(K) == 0
        assert _eval(lib, K=K, ldl=1 << 21) == EINVAL and "1..64" in _lib.last_error()
    for kw in (dict(F=0), dict(F=-12), dict(clips=0), dict(clips=-1)):
        assert _eval(lib, **kw) == EINVAL, kw
    assert _eval(lib, ldl=9) == EINVAL and "stride" in _lib.last_error()
    for name in ("logits", "labels", "state"):
        assert _eval(lib, null=name) == EINVAL, name
    assert _eval(lib, state=4096 * 6 + 4) == EINVAL and "aligned" in _lib.last_error()


def test_clip_evaluator_refuses_a_class_count_the_kernel_does_not_take():
    from acimg.evaluate import ClipEvaluator
    for K in (0, 65):
        with pytest.raises(ValueError):
            ClipEvaluator("cpu", K)


# ---- the command line ----------------------------------------------------------------------------------------------------
def _compare_args(*extra):
    from acimg import classify
    return classify.build_compare_parser().parse_args(
        ["--mode", "compare", "--train_file", "lists/test.txt", "--init_checkpoint", "ckpt/unet/epoch_30.ckpt",
         "--ac_checkpoint", "ckpt/dualcam/epoch_7.ckpt"] + list(extra))


def test_compare_file_names():
    from acimg import classify
    a = _compare_args()
    assert classify.compare_file(a) == "ckpt/unet/test_unet30_dualcamnet7.txt"          # beside the generator checkpoint
    assert classify.compare_json_file(a) == "ckpt/unet/classification.json"
    b = _compare_args("--mfccmap", "1")
    assert classify.compare_file(b) == "ckpt/dualcam/test_map_dualcamnet7.txt"          # beside the classifier's
    assert classify.compare_json_file(b) == "ckpt/dualcam/classification.json"
    assert (a.batch_size, a.seed, a.num_skip_conn, a.ae, a.datatype) == (16, 0, 1, 0, "outdoor")
    c = classify.build_compare_parser().parse_args(["--train_file", "l.txt", "--ac_checkpoint", "d/epoch_2.ckpt"])
    with pytest.raises(ValueError):
        classify.compare_file(c)                                                        # no generator, no --mfccmap 1
    c.mfccmap = 1
    assert classify.compare_file(c) == "d/test_map_dualcamnet2.txt"


def test_datatype_old_is_refused_in_every_mode():
    from acimg import classify
    with pytest.raises(ValueError, match="actions_data_old"):
        classify.run_compare(_compare_args("--datatype", "old"))
    for mode in ("train", "test"):
        with pytest.raises(ValueError, match="actions_data_old"):
            classify.main(["--mode", mode, "--model", "DualCamNet", "--datatype", "old"])
    with pytest.raises(ValueError, match="mode"):
        classify.main(["--mode", "plot"])
    with pytest.raises(ValueError, match="mode"):
        classify.main([])


def test_classification_json_schema():
    import json

    from acimg import classify
    K = 3
    real = dict(loss=0.5, accuracy=0.75, clips=4, correct=3, invalid=1, loss_sum=2.0,
                confusion=np.array([[2, 0, 0], [1, 1, 0], [0, 0, 0]], dtype=np.int64))
    none = dict(loss=float("nan"), accuracy=float("nan"), clips=0, correct=0, invalid=5, loss_sum=0.0,
                confusion=np.zeros((K, K), dtype=np.int64))
    doc = json.loads(json.dumps(classify.compare_document(_compare_args("--seed", "9"), real, none, K)))
    assert set(doc) == {"train_file", "init_checkpoint", "ac_checkpoint", "mfccmap", "seed", "batch_size", "num_classes",
                        "scored", "ac", "rec"}
    assert doc["scored"] == "generated" and doc["seed"] == 9 and doc["num_classes"] == K
    for part in ("ac", "rec"):
        assert set(doc[part]) == {"loss", "accuracy", "clips", "correct", "invalid", "confusion", "recall"}
    assert doc["ac"]["confusion"] == [[2, 0, 0], [1, 1, 0], [0, 0, 0]]
    assert doc["ac"]["recall"] == [1.0, 0.5, None] == classify_ref.per_class_recall(real["confusion"])
    assert doc["ac"]["accuracy"] == 3 / 4 and doc["ac"]["invalid"] == 1 and doc["ac"]["loss"] == 0.5
    assert doc["rec"]["accuracy"] is None and doc["rec"]["loss"] is None and doc["rec"]["recall"] == [None] * K
    assert json.loads(json.dumps(classify.compare_document(_compare_args("--mfccmap", "1"), real, real, K)))["scored"] == \
        "mfccmap"


def test_source_follows_the_flags_when_not_given():
    from acimg.flags import FLAGS, _Flags
    from acimg.trainer_class import SOURCES, TrainerClass, source_from_flags
    saved = dict(FLAGS.__dict__)
    try:
        FLAGS.__dict__.update(_Flags().__dict__)
        assert source_from_flags() == "generated"
        FLAGS.mfccmap = 1
        assert source_from_flags() == "generated"              # --mfccmap alone does not select the baseline trainer
        FLAGS.mfcc = 1
        assert source_from_flags() == "mfccmap"
        FLAGS.mfccmap = 0
        assert source_from_flags() == "acoustic"
    finally:
        FLAGS.__dict__.update(saved)
    assert SOURCES == ("generated", "acoustic", "mfccmap")
    with pytest.raises(ValueError):
        TrainerClass(None, None, None, source="real")


def test_configuration_text_is_the_reference_layout():
    from acimg import classify
    from acimg.flags import _Flags
    f = _Flags()
    f.parse(["--mode", "train", "--model", "DualCamNet", "--exp_name", "e1", "--mfcc", "1"])
    text = classify.configuration_text(f, 10)
    assert text.startswith("Experiment: e1 \nBatch_size: 8\n Latent weight: 1e-06\nModel: DualCamNet \n")
    assert text.endswith("Mode: train \nInit_checkpoint: None \nRestore_checkpoint: None\n") and text.count("\n") == 22       # 3 + 3 + 3 + 3 + 3 + 4 + 3 lines
