"""CPU tests of the TensorBoard logging's host side: tags, TF's bucket limits and compression, the event file (round trip,
an independent google.protobuf decoder built from the public field numbers, PIL on the PNG, reproducible bytes), the
`python -m acimg.main` dispatch table and configuration.txt, and the host side of the two summary entry points."""
import ctypes as C
import io
import struct
import sys

import numpy as np
import pytest

import summary_ref as sref

DBL_MAX = sys.float_info.max


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge

    ge.build()
    from acimg import _lib

    return _lib.load()


# ---- tags -----------------------------------------------------------------------------------------------------------------
def test_sanitize_tag():
    from acimg.events import sanitize_tag
    assert sanitize_tag("l2 loss") == "l2_loss"
    assert sanitize_tag("l1 loss") == "l1_loss"
    assert sanitize_tag("UNetAcRes/layer1/conv_1/kernel:0") == "UNetAcRes/layer1/conv_1/kernel_0"
    assert sanitize_tag("/lead/slash") == "lead/slash"
    assert sanitize_tag("a-b.c_d/E9") == "a-b.c_d/E9"
    assert sanitize_tag("x[0]=é") == "x_0___"
    assert sanitize_tag("train_loss") == "train_loss"


def test_image_tags():
    from acimg.events import image_tags
    assert image_tags("mfcc0", 1) == ["mfcc0/image"]
    assert image_tags("mfcc0", 3) == ["mfcc0/image/0", "mfcc0/image/1", "mfcc0/image/2"]
    assert image_tags("reconstructed audio", 1) == ["reconstructed_audio/image"]


def test_logger_registers_tags(lib, tmp_path):
    from acimg.logger import Logger
    lg = Logger(str(tmp_path / "tags"), clock=lambda: 5.0, hostname="host")
    lg.log_scalar("l2 loss", "a")
    lg.log_image("mfcc1", "b", max_outputs=1)
    lg.log_image("many", "c", max_outputs=3)
    lg.log_histogram("scope/kernel:0", "d")
    lg.merge_summary()
    assert [(k, t) for k, t, _ in lg.summary_op] == [
        ("scalar", ["l2_loss"]), ("image", ["mfcc1/image"]), ("image", ["many/image/0", "many/image/1", "many/image/2"]),
        ("histogram", ["scope/kernel_0"])]
    lg.close()


# ---- limits ---------------------------------------------------------------------------------------------------------------
def test_default_bucket_limits():
    from acimg.events import default_bucket_limits
    lim = default_bucket_limits()
    assert len(lim) == 1551
    assert all(b > a for a, b in zip(lim, lim[1:]))
    assert lim[775] == 0.0 and lim[776] == 1e-12 and lim[774] == -1e-12
    assert lim[-1] == DBL_MAX and lim[0] == -DBL_MAX
    assert lim[-2] < 1e20 and lim[-2] >= 1e20 / 1.1
    assert [-x for x in reversed(lim)] == lim
    assert default_bucket_limits() is not lim                 # a fresh list: callers may not damage the table


# ---- compression ------------------------------------------------------------------------------------------------------
LIMS = [-3.0, -1.0, 0.0, 1.0, 3.0, DBL_MAX]


@pytest.mark.parametrize("counts,want", [
    ([0, 0, 0, 0, 0, 0], ([DBL_MAX], [0.0])),                                   # all empty: the run's last limit
    ([0, 0, 5, 0, 0, 0], ([-1.0, 0.0, DBL_MAX], [0.0, 5.0, 0.0])),              # one full bucket in the middle
    ([0, 2, 3, 4, 0, 0], ([-3.0, -1.0, 0.0, 1.0, DBL_MAX], [0.0, 2.0, 3.0, 4.0, 0.0])),   # adjacent full buckets
    ([0, 0, 1, 0, 7, 0], ([-1.0, 0.0, 1.0, 3.0, DBL_MAX], [0.0, 1.0, 0.0, 7.0, 0.0])),    # empty runs at both ends
    ([1, 0, 0, 0, 0, 2], ([-3.0, 3.0, DBL_MAX], [1.0, 0.0, 2.0])),               # no empty run at either end
])
def test_compress_buckets(counts, want):
    from acimg.events import compress_buckets
    assert compress_buckets(counts, LIMS) == want
    assert sref.compress(counts, LIMS) == want


def test_compress_nothing_emitted():
    from acimg.events import compress_buckets
    assert compress_buckets([], []) == ([DBL_MAX], [0.0])


def test_compress_random_counts_match_restatement():
    from acimg.events import compress_buckets, default_bucket_limits
    lim = default_bucket_limits()
    rng = np.random.RandomState(3)
    for _ in range(5):
        counts = np.zeros(len(lim), np.int64)
        idx = rng.randint(700, 850, size=40)
        counts[idx] = rng.randint(1, 100, size=40)
        assert compress_buckets(counts, lim) == sref.compress(counts, lim)


# ---- the file -----------------------------------------------------------------------------------------------------------
def _picture():
    rng = np.random.RandomState(1)
    return rng.randint(0, 256, size=(36, 48, 3)).astype(np.uint8)


def _write(logdir):
    from acimg import events
    lim = events.default_bucket_limits()
    counts = np.zeros(len(lim), np.int64)
    counts[[700, 701, 775, 900]] = [3, 1, 4, 2]
    t = [100.25]

    def clock():
        t[0] += 1.0
        return t[0]

    w = events.EventFileWriter(logdir, clock=clock, hostname="testhost")
    w.add_summary([events.scalar_value("l2_loss", 0.1), events.scalar_value("train_loss", np.float32(2.5))], 1)
    w.add_summary([events.image_value("mfcc0/image", _picture()),
                   events.histogram_value("scope/kernel_0", -0.5, 1.5, 10.0, 3.25, 7.5, counts, lim)], 2 ** 33 + 5)
    w.add_summary([events.scalar_value("valid_loss", 0.75)], 0)
    w.flush()
    w.close()
    return w.path, counts, lim


def _messages():
    """Event / Summary / HistogramProto classes built at run time from the public field numbers"""
    from google.protobuf import descriptor_pb2 as dpb
    from google.protobuf import descriptor_pool, message_factory
    F = dpb.FieldDescriptorProto
    fd = dpb.FileDescriptorProto(name="acimg_test_event.proto", package="acimgtest", syntax="proto3")

    def msg(parent, name, fields):
        m = parent.message_type.add() if isinstance(parent, dpb.FileDescriptorProto) else parent.nested_type.add()
        m.name = name
        for fname, num, typ, label, tname in fields:
            f = m.field.add(name=fname, number=num, type=typ, label=label)
            if tname:
                f.type_name = tname
        return m

    O, R = F.LABEL_OPTIONAL, F.LABEL_REPEATED
    msg(fd, "HistogramProto", [("min", 1, F.TYPE_DOUBLE, O, None), ("max", 2, F.TYPE_DOUBLE, O, None),
                               ("num", 3, F.TYPE_DOUBLE, O, None), ("sum", 4, F.TYPE_DOUBLE, O, None),
                               ("sum_squares", 5, F.TYPE_DOUBLE, O, None), ("bucket_limit", 6, F.TYPE_DOUBLE, R, None),
                               ("bucket", 7, F.TYPE_DOUBLE, R, None)])
    s = msg(fd, "Summary", [("value", 1, F.TYPE_MESSAGE, R, ".acimgtest.Summary.Value")])
    msg(s, "Image", [("height", 1, F.TYPE_INT32, O, None), ("width", 2, F.TYPE_INT32, O, None),
                     ("colorspace", 3, F.TYPE_INT32, O, None), ("encoded_image_string", 4, F.TYPE_BYTES, O, None)])
    msg(s, "Value", [("tag", 1, F.TYPE_STRING, O, None), ("simple_value", 2, F.TYPE_FLOAT, O, None),
                     ("image", 4, F.TYPE_MESSAGE, O, ".acimgtest.Summary.Image"),
                     ("histo", 5, F.TYPE_MESSAGE, O, ".acimgtest.HistogramProto")])
    msg(fd, "Event", [("wall_time", 1, F.TYPE_DOUBLE, O, None), ("step", 2, F.TYPE_INT64, O, None),
                      ("file_version", 3, F.TYPE_STRING, O, None), ("summary", 5, F.TYPE_MESSAGE, O, ".acimgtest.Summary")])
    pool = descriptor_pool.DescriptorPool()
    pool.Add(fd)
    return message_factory.GetMessageClass(pool.FindMessageTypeByName("acimgtest.Event"))


def test_event_file_round_trip(lib, tmp_path):
    from acimg import events, tfio
    path, counts, lim = _write(str(tmp_path / "log"))
    assert path.endswith("/log/events.out.tfevents.0000000101.testhost")
    recs = list(tfio.read_tfrecord(path, verify=True))
    assert len(recs) == 4
    ev = events.read_events(path)
    assert ev[0] == dict(wall_time=101.25, step=0, file_version="brain.Event:2")
    assert [e["step"] for e in ev] == [0, 1, 2 ** 33 + 5, 0]
    assert [e["wall_time"] for e in ev] == [101.25, 102.25, 103.25, 104.25]
    assert ev[1]["summary"] == [dict(tag="l2_loss", simple_value=float(np.float32(0.1))),
                                dict(tag="train_loss", simple_value=2.5)]
    img, hist = ev[2]["summary"]
    assert img["tag"] == "mfcc0/image"
    assert (img["image"]["height"], img["image"]["width"], img["image"]["colorspace"]) == (36, 48, 3)
    h = hist["histo"]
    assert hist["tag"] == "scope/kernel_0"
    assert (h["min"], h["max"], h["num"], h["sum"], h["sum_squares"]) == (-0.5, 1.5, 10.0, 3.25, 7.5)
    assert (h["bucket_limit"], h["bucket"]) == sref.compress(counts, lim)
    assert h["bucket"] == [0.0, 3.0, 1.0, 0.0, 4.0, 0.0, 2.0, 0.0]      # four runs of empty buckets, four full buckets
    assert ev[3]["summary"] == [dict(tag="valid_loss", simple_value=0.75)]


def test_event_file_decodes_with_an_independent_decoder(lib, tmp_path):
    from PIL import Image

    from acimg import tfio
    path, counts, lim = _write(str(tmp_path / "log"))
    Event = _messages()
    msgs = []
    for rec in tfio.read_tfrecord(path, verify=True):
        e = Event()
        e.ParseFromString(bytes(rec))
        assert e.SerializeToString(deterministic=True) == bytes(rec)      # nothing in the record the schema lacks
        msgs.append(e)
    assert msgs[0].file_version == "brain.Event:2" and msgs[0].wall_time == 101.25 and not msgs[0].HasField("summary")
    assert [m.step for m in msgs] == [0, 1, 2 ** 33 + 5, 0]
    v = msgs[1].summary.value
    assert [x.tag for x in v] == ["l2_loss", "train_loss"]
    assert struct.pack("<f", v[0].simple_value) == struct.pack("<f", np.float32(0.1)) and v[1].simple_value == 2.5
    im, hi = msgs[2].summary.value
    assert im.tag == "mfcc0/image" and (im.image.height, im.image.width, im.image.colorspace) == (36, 48, 3)
    pixels = np.asarray(Image.open(io.BytesIO(im.image.encoded_image_string)).convert("RGB"))
    assert np.array_equal(pixels, _picture())
    bl, bc = sref.compress(counts, lim)
    assert list(hi.histo.bucket_limit) == bl and list(hi.histo.bucket) == bc
    assert (hi.histo.min, hi.histo.max, hi.histo.num, hi.histo.sum, hi.histo.sum_squares) == (-0.5, 1.5, 10.0, 3.25, 7.5)
    assert msgs[3].summary.value[0].tag == "valid_loss" and msgs[3].summary.value[0].simple_value == 0.75


def test_event_file_is_reproducible(lib, tmp_path):
    a, _, _ = _write(str(tmp_path / "a"))
    b, _, _ = _write(str(tmp_path / "b"))
    assert a.split("/")[-1] == b.split("/")[-1] == "events.out.tfevents.0000000101.testhost"
    assert open(a, "rb").read() == open(b, "rb").read()


def test_writer_makes_the_directory_and_names_the_host(lib, tmp_path):
    import socket

    from acimg.events import EventFileWriter
    w = EventFileWriter(str(tmp_path / "x" / "y"), clock=lambda: 12.9)
    w.close()
    assert w.path == str(tmp_path / "x" / "y" / ("events.out.tfevents.0000000012." + socket.gethostname()))


# ---- acimg.main -----------------------------------------------------------------------------------------------------------
class _F(object):
    def __init__(self, **kw):
        from acimg.flags import _DEFS
        for name, _, default in _DEFS:
            setattr(self, name, default)
        for k, v in kw.items():
            setattr(self, k, v)


def test_dispatch_table():
    from acimg.main import dispatch
    for emb in (0, 1):
        for proxy in (0, 1):
            for project in (0, 1):
                for joint in (0, 1):
                    for mfcc in (0, 1):
                        for model in ("UNet", "DualCamNet", "Other"):
                            f = _F(embedding=emb, proxy=proxy, project=project, jointmvae=joint, mfcc=mfcc, model=model)
                            if emb:
                                want = ("TrainerNCAproxyanchor" if proxy else "TrainerAssociator" if project
                                        else "TrainerMulti" if joint else "generator" if mfcc else "TrainerLoss")
                            else:
                                want = {"UNet": "TrainerVAE", "DualCamNet": "classify", "Other": "Unknown model"}[model]
                            if want in ("generator", "classify"):
                                assert dispatch(f) == want
                            else:
                                with pytest.raises(ValueError, match=want):
                                    dispatch(f)
    for name in ("TrainerLoss", "TrainerNCAproxyanchor"):
        f = _F(embedding=1, proxy=int(name != "TrainerLoss"), mfcc=0)
        with pytest.raises(ValueError, match="not built"):
            dispatch(f)


def test_configuration_text_layout():
    from acimg.main import configuration_text
    f = _F(exp_name="E", model="UNet", learning_rate=0.001, num_epochs=3, total_length=30, sample_length=1,
           number_of_crops=30, margin=0.2, block_size=1, embedding=1, latent_loss=1e-06, train_file="t.txt",
           valid_file="v.txt", test_file=None, mode="train", visual_init_checkpoint=None, acoustic_init_checkpoint="a/b",
           restore_checkpoint=None, checkpoint_dir="ck", tensorboard="tb", batch_size=32, num_skip_conn=2, ae=0,
           huber_loss=1, MSE=0)
    assert configuration_text(f, 10) == (
        "Experiment: E \nModel: UNet \nLearning_rate: 0.001\n"
        "Num_epochs: 3 \nTotal_length: 30 \nSample_length: 1\n"
        "Number_of_crops: 30 \nMargin: 0.2\nNumber of classes: 10\n"
        "Block_size: 1 \nEmbedding: 1\nLatent weight: 1e-06\n"
        "Train_file: t.txt \nValid_file: v.txt \nTest_file: None\n"
        "Mode: train \nVisual_init_checkpoint: None \nAcoustic_init_checkpoint: a/b \nRestore_checkpoint: None\n"
        "Checkpoint_dir: ck \nLog dir: tb \nBatch_size: 32\n"
        "Number of skip connections: 2 \nAuto encoder: 0\nHuber: 1\nMSE: 0\n")


def test_main_refusals():
    from acimg.flags import _DEFS
    from acimg.main import parse, run_main
    defs = list(_DEFS)
    with pytest.raises(ValueError, match="--mode"):
        parse(["--exp_name", "e"])
    with pytest.raises(ValueError, match="--exp_name"):
        parse(["--mode", "train"])
    with pytest.raises(ValueError, match="Unknown execution mode"):
        parse(["--mode", "fly", "--exp_name", "e"])
    with pytest.raises(ValueError, match="actions_data_old"):
        parse(["--mode", "train", "--exp_name", "e", "--datatype", "old"])
    with pytest.raises(ValueError, match="TrainerMulti"):
        run_main(["--mode", "train", "--exp_name", "e", "--embedding", "1", "--jointmvae", "1"])
    flags, extra = parse(["--mode", "test", "--exp_name", "e", "--histograms", "1", "--seed", "4", "--device", "cpu"])
    assert (extra.histograms, extra.seed, extra.device, flags.mode) == (1, 4, "cpu", "test")
    assert parse(["--mode", "train", "--exp_name", "e"])[1].histograms == 0
    assert _DEFS == defs                                        # the flag table itself is left alone


# ---- host side of the entry points ------------------------------------------------------------------------------------------
def test_histogram_workspace_arithmetic(lib):
    q = lib.acimg_histogram_segments_workspace
    assert q(0, 1551, 100) == 0 and q(3, 0, 100) == 0 and q(3, 1551, 0) == 0 and q(-1, -1, -1) == 0
    # (V + 1) prefix words rounded up to 32 bytes + one 32-byte record per 8192-element chunk, at most total / 8192 + V
    assert q(1, 1, 1) == 32 + 32
    assert q(3, 1551, 8192 * 5 + 1) == 32 + 32 * (5 + 3)
    assert q(4, 1551, 8191) == 64 + 32 * 4
    assert q(100, 1551, 30000000) == 832 + 32 * (30000000 // 8192 + 100)
    assert q(3, 7, 100) == q(3, 1551, 100)                      # L takes no workspace
    assert lib.acimg_version() == 207                           # the entries were added without a bump


def test_entry_points_refuse_bad_arguments(lib):
    from acimg import _lib
    buf = (C.c_char * 4096)()
    p = C.addressof(buf)
    si = lib.acimg_summary_images
    for args in [(None, 12, 10, 0, 1, 1, p), (p, 12, 10, 0, 1, 1, None), (p, 12, 0, 0, 1, 1, p), (p, 12, -5, 0, 1, 1, p),
                 (p, 12, 10, 0, 0, 1, p), (p, 12, 10, 0, 1, 0, p), (p, 12, 10, -1, 1, 1, p), (p, 12, 10, 0, 5, 1, p),
                 (p, 16, 10, 3, 5, 1, p), (p, 0, 10, 0, 1, 1, p)]:
        assert si(*args, None) == -1, args
    assert "summary_images" in _lib.last_error()
    hs = lib.acimg_histogram_segments
    ok = [p, p, 2, p, 8, 100, p, p, p, p, 4096]
    for i, bad in [(0, None), (1, None), (3, None), (6, None), (7, None), (8, None), (9, None), (2, 0), (2, -1), (4, 0),
                   (4, 4097), (5, 0), (5, -7), (9, p + 4)]:
        args = list(ok)
        args[i] = bad
        assert hs(*args, None) == -1, (i, bad)
    assert "histogram_segments" in _lib.last_error()
    need = lib.acimg_histogram_segments_workspace(2, 8, 100)
    args = list(ok)
    args[10] = need - 1
    assert hs(*args, None) == -2 and "workspace" in _lib.last_error()
