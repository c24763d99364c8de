"""The correspondence pairs on the device: `acimg_batch_gather_pairs` between guard bands against the NumPy restatement of
tests/correspondence_ref.py (every element equal) and against `acimg_batch_gather` on the real rows (every bit equal);
both loaders with `correspondence=1` against the restatement applied to the plain loader's batches - without shuffling,
with the second shuffle stage, under page and ring reuse -; one epoch of `Trainer.train()` from the pair loader against
the same epoch from the restated batches; and `python -m acimg.main --correspondence 1`."""
from collections import OrderedDict

import numpy as np
import pytest
import torch

import correspondence_ref as cref
from data_support import write_outdoor_records
from guard_arena import GuardArena
from model_support import loss_lines, make

pytestmark = pytest.mark.gpu

A, L, NSLOTS = 10, 61, 5
CLASSES = [7, -1, A, A - 1, 0]           # per slot: in range, negative, one past the end, A - 1, 0
PLACES = [33, L, -1, 0, L - 1]
# row n takes MIXED[n % 9]: the last slot in both kinds side by side, a repeated silent row, a repeated real row, slot 0 as
# -1 (the code whose bits are all ones), every slot in some kind
MIXED = [4, ~4, ~2, 3, ~2, 0, ~0, 3, ~1]


def pair_pool(pixels, elems, stride, seed):
    rng = np.random.RandomState(seed)
    video = rng.randint(0, 256, size=(NSLOTS, stride)).astype(np.uint8)
    ac = (rng.rand(NSLOTS, elems) * 5 - 1).astype(np.float32)
    ac[3] = 3.25                                          # a constant frame: 0 / 0 in its real row
    ac[4, 0], ac[4, -1] = -100.0, 100.0
    mfcc = rng.rand(NSLOTS, 12).astype(np.float32)
    low = (rng.rand(NSLOTS, 12) * 3 - 1).astype(np.float32)      # not in [0, 1]: a silent row must not be normalised
    labels = np.stack([np.array(CLASSES), np.array(PLACES)], 1).astype(np.int32)
    return video, ac, mfcc, low, labels


def plain_frames(video, ac, mfcc, low, labels, pixels):
    """what the plain gather makes of every slot of the pool, in NumPy: the six tensors the restatement starts from"""
    v = video[:, :pixels * 3].reshape(NSLOTS, pixels, 3)[..., ::-1].astype(np.float32) * np.float32(1.0 / 255.0)
    a = ac - ac.min(axis=1, keepdims=True)
    with np.errstate(invalid="ignore", divide="ignore"):
        a = a / a.max(axis=1, keepdims=True)
    hot = []
    for col, width in ((0, A), (1, L)):
        h = np.zeros((NSLOTS, width), np.float32)
        for n, c in enumerate(labels[:, col]):
            if 0 <= c < width:
                h[n, c] = 1.0
        hot.append(h)
    return a, mfcc, v.reshape(NSLOTS, -1), hot[0], hot[1], low


def pairs_case(device, N, elems, kind, pixels=20, shift=0):
    """one call between guard bands.  shift: bytes by which the acoustic output is moved off its 16-byte boundary"""
    from acimg import _lib
    lib = _lib.load()
    stride = -(-pixels * 3 // 16) * 16
    video, ac, mfcc, low, labels = pair_pool(pixels, elems, stride, seed=N * 1000 + elems)
    codes = np.array([MIXED[n % 9] for n in range(N)], np.int32)
    if kind != "mixed":
        slot = np.where(codes < 0, ~codes, codes)
        codes = (slot if kind == "real" else ~slot).astype(np.int32)
    dv = [torch.from_numpy(x).to(device) for x in (video, ac, mfcc, low, labels, codes)]
    ws_bytes = lib.acimg_batch_gather_pairs_workspace(N, elems)
    assert ws_bytes == 16 * N
    sizes = OrderedDict([("video", N * pixels * 12), ("acoustic", N * elems * 4 + (16 if shift else 0)), ("mfcc", N * 48),
                         ("pair", N * 8), ("action", N * A * 4), ("location", N * L * 4), ("ws", ws_bytes)])
    arena = GuardArena.for_sizes(device, sizes.values())
    r = OrderedDict((k, arena.region(v, name=k)) for k, v in sizes.items())
    st = torch.cuda.current_stream(device).cuda_stream

    def call(nbytes):
        return lib.acimg_batch_gather_pairs(dv[0].data_ptr(), stride, dv[1].data_ptr(), dv[2].data_ptr(), dv[3].data_ptr(),
                                            dv[4].data_ptr(), dv[5].data_ptr(), N, pixels, elems, A, L, r["video"].ptr,
                                            r["acoustic"].ptr + shift, r["mfcc"].ptr, r["pair"].ptr, r["action"].ptr,
                                            r["location"].ptr, r["ws"].ptr, nbytes, st)
    assert call(ws_bytes - 16) == -2                       # a workspace 16 bytes short is refused ...
    torch.cuda.synchronize(device)
    assert bool((arena.buf == arena.canary).all())         # ... before anything is written
    _lib.check(call(ws_bytes), "batch_gather_pairs")
    torch.cuda.synchronize(device)
    arena.check("batch_gather_pairs N=%d elems=%d %s" % (N, elems, kind))
    raw = {k: r[k].u8.cpu().numpy() for k in sizes}
    if shift:                                              # the bytes around the shifted image are untouched as well
        assert (raw["acoustic"][:shift] == 0xA5).all() and (raw["acoustic"][shift + N * elems * 4:] == 0xA5).all()
        raw["acoustic"] = raw["acoustic"][shift:shift + N * elems * 4].copy()
    got = {k: v.view(np.float32) for k, v in raw.items()}
    want = cref.rows_of(plain_frames(video, ac, mfcc, low, labels, pixels), codes.tolist())
    for k, w in zip(("acoustic", "mfcc", "video", "action", "location", "pair"), want):
        assert np.array_equal(got[k], w.reshape(-1), equal_nan=True), k
    silent = codes < 0
    slot = np.where(silent, ~codes, codes)
    assert np.isnan(want[0]).any() == bool((~silent & (slot == 3)).any())       # only the constant frame's real row
    assert np.array_equal(got["pair"].reshape(N, 2), np.stack([silent, ~silent], 1).astype(np.float32))
    stats = got["ws"].reshape(N, 4)
    assert raw["ws"].reshape(N, 16)[silent].any() == 0                           # four zeros (all bits) for a silent row
    mn = ac[slot].min(axis=1)
    mx = (ac[slot] - mn[:, None]).max(axis=1)
    assert np.array_equal(stats[~silent, 0], mn[~silent]) and np.array_equal(stats[~silent, 1], mx[~silent])
    assert not stats[:, 2:].any()
    # the real rows against acimg_batch_gather on the same slots: every bit
    real = np.flatnonzero(~silent)
    if len(real):
        n = len(real)
        slots = torch.from_numpy(slot[real].astype(np.int32)).to(device)
        out = [torch.empty(n * w, device=device) for w in (pixels * 3, elems, 12, 12, A, L)]
        ws = torch.empty(4 * n, device=device)
        _lib.check(lib.acimg_batch_gather(dv[0].data_ptr(), stride, dv[1].data_ptr(), dv[2].data_ptr(), dv[3].data_ptr(),
                                          dv[4].data_ptr(), slots.data_ptr(), n, pixels, elems, A, L,
                                          *[t.data_ptr() for t in out], ws.data_ptr(), 16 * n, st), "batch_gather")
        torch.cuda.synchronize(device)
        for k, t, w in (("video", out[0], pixels * 3), ("acoustic", out[1], elems), ("mfcc", out[2], 12),
                        ("action", out[4], A), ("location", out[5], L), ("ws", ws, 4)):
            mine = torch.from_numpy(got[k].reshape(N, w)[real].copy()).view(torch.int32)
            assert torch.equal(mine, t.cpu().view(torch.int32).reshape(n, w)), k


@pytest.mark.parametrize("kind", ["real", "silent", "mixed"])
@pytest.mark.parametrize("elems", [12, 4104, 20736, 32760])
@pytest.mark.parametrize("N", [1, 7, 33])
def test_batch_gather_pairs(device, N, elems, kind):
    """12: fewer floats (and float4) than threads; 4104 = 1026 float4: two past one sweep of the 1024 threads, the second
    of a thread's three stores; 20736: the data set's 36 x 48 x 12 (5184 float4: two rounds of three); 32760: the largest
    multiple of 12 the LDS image admits.  N = 1: MIXED's first row alone; 7 and 33: more rows than MIXED's period"""
    pairs_case(device, N, elems, kind, pixels=4112 if elems == 20736 else 20)


@pytest.mark.parametrize("elems", [12, 4104, 20736])
def test_batch_gather_pairs_off_the_16_byte_boundary(device, elems):
    """the acoustic output 4 bytes past a 16-byte boundary: every multiple of 12 is a multiple of 4, so misalignment is the
    only way onto the float-by-float path"""
    pairs_case(device, 7, elems, "mixed", shift=4)


def test_batch_gather_pairs_is_repeatable(device):
    from acimg import ops
    video, ac, mfcc, low, labels = pair_pool(20, 20736, 64, seed=5)
    dv = [torch.from_numpy(x).to(device) for x in (video, ac, mfcc, low, labels, np.array(MIXED * 3, np.int32))]
    plan = ops.Plan(device, eager=True)
    runs = []
    for _ in range(2):
        out = [torch.empty(27, w, device=device) for w in (60, 20736, 12, 2, A, L)]
        ops.batch_gather_pairs(plan, dv[0], 64, dv[1], dv[2], dv[3], dv[4], dv[5], 27, 20, 20736, out[0], out[1], out[2],
                               out[3], out[4], A, out[5], L)
        torch.cuda.synchronize(device)
        runs.append([t.cpu().view(torch.int32) for t in out])
    assert all(torch.equal(a, b) for a, b in zip(*runs))


# ---- the loaders -------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def pair_records(device, tmp_path_factory):
    """three GZIP files of one 12-frame record each and the 36 plain frames `TFRecordDataLoader` makes of them (NumPy,
    computed once, never written to)"""
    from acimg.data import TFRecordDataLoader
    paths = write_outdoor_records(tmp_path_factory.mktemp("pairs"), 17, [(1 + 3 * r, 9 + r) for r in range(3)], wide=True)
    (frames,) = list(TFRecordDataLoader(paths, 64, device=device).data)
    assert frames[0].shape[0] == 36
    return paths, tuple(t.numpy() for t in frames)


def same_rows(got, want, what):
    assert len(got) == 6 and len(want) == 6
    for k, (g, w) in enumerate(zip(got, want)):
        w = torch.from_numpy(np.ascontiguousarray(w))
        assert g.dtype == w.dtype and g.shape == w.shape, (what, k, g.shape, w.shape)
        assert torch.equal(g.cpu(), w), (what, k)


@pytest.mark.parametrize("bs", [5, 8, 64])
def test_pair_loaders_without_shuffling(device, pair_records, bs):
    """5: a short last batch; 8: a batch boundary inside a record; 64: one batch larger than the data.  Every tensor of
    every batch of both loaders is the restated pair map of the plain loader's batch"""
    from acimg.data import DeviceDataLoader, TFRecordDataLoader
    paths, frames = pair_records
    want = [cref.pair_map(tuple(t[i:i + bs] for t in frames)) for i in range(0, 36, bs)]
    assert [w[0].shape[0] for w in want] == [2 * min(bs, 36 - i) for i in range(0, 36, bs)]
    host = TFRecordDataLoader(paths, bs, device=device, correspondence=1)
    assert (host.num_samples, host.total_batches, host.num_rows, host.num_batches) == (36, -(-36 // bs), 72, -(-36 // bs))
    got = list(host.data)
    assert len(got) == len(want)
    for k, (g, w) in enumerate(zip(got, want)):
        same_rows(g, w, "host loader, batch %d" % k)
    for workers in (1, 4):
        dl = DeviceDataLoader(paths, bs, workers=workers, device=device, correspondence=1)
        assert (dl.num_samples, dl.total_batches, dl.num_rows, dl.num_batches) == (36, -(-36 // bs), 72, -(-36 // bs))
        got = []
        for b in dl.data:
            assert all(t.device == device for t in b)
            got.append(tuple(t.clone() for t in b))
        dl.close()
        assert len(got) == len(want)
        for k, (g, w) in enumerate(zip(got, want)):
            same_rows(g, w, "device loader, batch %d, %d workers" % (k, workers))


def expected_pass(paths, frames, seed, epoch, bs, B, files=None):
    """the batches of one pass of the shuffling pair loader: file permutation and stage 1 from PCG64([seed, epoch]) as in
    the plain loader, stage 2 from PCG64([seed, epoch, 1]); every batch as rows of the restated pair map"""
    from acimg.data import epoch_files
    files = paths if files is None else files
    rng1 = np.random.Generator(np.random.PCG64([seed, epoch]))
    rng2 = np.random.Generator(np.random.PCG64([seed, epoch, 1]))
    base = np.concatenate([np.arange(12) + 12 * paths.index(p) for p in epoch_files(files, True, None, rng1)])
    out = []
    for codes in cref.pair_code_batches(len(base), bs, B, rng1, rng2):
        out.append(cref.rows_of(frames, [int(base[c]) if c >= 0 else -int(base[-c - 1]) - 1 for c in codes]))
    return out


@pytest.mark.parametrize("bs", [5, 8])
def test_pair_loader_shuffle(device, pair_records, bs):
    from acimg.data import DeviceDataLoader
    paths, frames = pair_records
    dl = DeviceDataLoader(paths, bs, shuffle=True, buffer_size=5, seed=3, device=device, correspondence=1)
    assert (dl.num_samples, dl.total_batches, dl.num_rows, dl.num_batches) == (36, -(-36 // bs), 72, -(-72 // bs))
    passes = [[tuple(t.cpu() for t in b) for b in dl.data] for _ in range(2)]
    dl.close()
    for epoch, got in enumerate(passes):
        want = expected_pass(paths, frames, 3, epoch, bs, 5)
        assert len(got) == len(want) == -(-72 // bs) and sum(b[0].shape[0] for b in got) == 72
        for k, (g, w) in enumerate(zip(got, want)):
            same_rows(g, w, "epoch %d, batch %d" % (epoch, k))
    assert not torch.equal(passes[0][0][2], passes[1][0][2])           # the second pass differs ...
    again = DeviceDataLoader(paths, bs, shuffle=True, buffer_size=5, seed=3, device=device, correspondence=1)
    for b, w in zip(again.data, passes[0]):                             # ... and the same seed gives the same pass
        assert all(torch.equal(x.cpu(), y) for x, y in zip(b, w))
    again.close()


def test_pair_loader_recycles_pages_and_ring(device, pair_records):
    """buffer_size 2, batch 4, no prefetch, ring 2: `pair_pages` = 8 pages for the nine records of the three files listed
    three times, and two output sets for 54 batches.  Every batch is right when yielded and still right one iteration
    later (ring - 1)"""
    from acimg.data import DeviceDataLoader, pair_pages
    paths, frames = pair_records
    files = paths * 3
    dl = DeviceDataLoader(files, 4, shuffle=True, buffer_size=2, seed=1, prefetch=0, ring=2, device=device, correspondence=1)
    dl.FIRST_PAGES = 2                                              # start below the bound: growth is exercised as well
    want = expected_pass(paths, frames, 1, 0, 4, 2, files=files)
    held = []
    for k, b in enumerate(dl.data):
        same_rows(b, want[k], "batch %d at yield" % k)
        held.append(b)
        if k >= 1:
            same_rows(held[k - 1], want[k - 1], "batch %d one iteration later" % (k - 1))
    assert len(held) == len(want) == 54
    assert dl._pool_pages <= pair_pages(2, 4, 0) == 8               # so the nine records shared pages
    dl.close()


class RestatedLoader(object):
    """the surface `Trainer.train()` reads, over batches computed in advance"""

    def __init__(self, batches, batch_size):
        self.data = [tuple(torch.from_numpy(np.ascontiguousarray(t)) for t in b) for b in batches]
        self.batch_size = batch_size


def test_pair_loader_feeds_the_trainer(device, pair_records):
    """one epoch of `Trainer.train()` - nine steps of 8 rows, validation on 16 + 8 rows of the first file - from the pair
    loaders and from the restated batches: both feed the same numbers, so the lines are the same"""
    from acimg.data import DeviceDataLoader
    from acimg.flags import FLAGS
    paths, frames = pair_records
    FLAGS.checkpoint_dir, FLAGS.exp_name = None, "pairs"
    FLAGS.restore_checkpoint = FLAGS.init_checkpoint = None
    FLAGS.acoustic_init_checkpoint = FLAGS.visual_init_checkpoint = None
    first = tuple(t[:12] for t in frames)
    keep = FLAGS.as_dict()
    feeds = [lambda: (DeviceDataLoader(paths, 8, shuffle=True, buffer_size=5, seed=2, device=device, correspondence=1),
                      DeviceDataLoader(paths[:1], 8, device=device, correspondence=1)),
             lambda: (RestatedLoader(expected_pass(paths, frames, 2, 0, 8, 5), 8),
                      RestatedLoader([cref.pair_map(tuple(t[i:i + 8] for t in first)) for i in (0, 8)], 8))]
    runs = []
    for feed in feeds:
        tr, sess = make(device, epochs=1)
        log = []
        tr.log = log.append
        train, valid = feed()
        best = tr.train(train, valid)
        for d in (train, valid):
            getattr(d, "close", lambda: None)()
        assert tr.global_step == 9 and np.isfinite(best)
        runs.append((loss_lines(log, validation=True), best))
    for k, v in keep.items():
        setattr(FLAGS, k, v)
    assert len(runs[0][0]) == 10 and runs[0] == runs[1]


@pytest.fixture(scope="module")
def cli_runs(device, pair_records, tmp_path_factory):
    """`python -m acimg.main` for one epoch at batch 8 on the 36 frames (validation: the first file), without and with
    `--correspondence 1`; the rows of every `eval_step` are noted"""
    from acimg.flags import FLAGS
    from acimg.main import run_main
    paths, _ = pair_records
    keep = FLAGS.as_dict()
    tmp = tmp_path_factory.mktemp("pairs_cli")
    train, valid = str(tmp / "train.txt"), str(tmp / "valid.txt")
    with open(train, "w") as f:
        f.write("\n".join(paths) + "\n")
    with open(valid, "w") as f:
        f.write(paths[0] + "\n")
    out = {}
    for flag in (0, 1):
        log, rows, box = [], [], {}

        def hook(tr, rows=rows, box=box):
            box["trainer"] = tr
            step = tr.eval_step

            def watched(batch=None, **kw):
                rows.append(int(batch[1].shape[0]))
                return step(batch, **kw)
            tr.eval_step = watched
        best = run_main(["--mode", "train", "--model", "UNet", "--embedding", "1", "--mfcc", "1", "--batch_size", "8",
                         "--num_epochs", "1", "--display_freq", "1", "--exp_name", "c%d" % flag, "--train_file", train,
                         "--valid_file", valid, "--checkpoint_dir", str(tmp / "ckpt"), "--buffer_size", "5", "--device",
                         str(device), "--correspondence", str(flag)], log=log.append, hooks=dict(trainer=hook))
        out[flag] = dict(log=log, rows=rows, best=best, steps=box["trainer"].global_step)
    for k, v in keep.items():                                       # the command line sets every flag: put them back
        setattr(FLAGS, k, v)
    return out


def test_command_line(cli_runs):
    plain, pairs = cli_runs[0], cli_runs[1]
    assert len(loss_lines(plain["log"], validation=False)) == 5 and plain["steps"] == 5
    assert len(loss_lines(pairs["log"], validation=False)) == 9 and pairs["steps"] == 9
    assert plain["rows"] == [8, 4] and pairs["rows"] == [16, 8]        # validation on the pair batches themselves
    assert np.isfinite(plain["best"]) and np.isfinite(pairs["best"])
