"""`acimg_batch_gather` against NumPy (every element equal, between guard bands) and `acimg.data.DeviceDataLoader`
against `TFRecordDataLoader` on the same GZIP record files: order without shuffle, the shuffle buffer's order with it,
page / ring recycling, and one epoch of `Trainer.train()` from either loader."""
from collections import OrderedDict

import numpy as np
import pytest
import torch

from guard_arena import GuardArena
from data_support import write_outdoor_records
from model_support import loss_lines, make

pytestmark = pytest.mark.gpu

A, L, NSLOTS = 10, 61, 5
# output n reads slot SLOTS[n % 7]: the pool's last slot first, a repeat, descending order
SLOTS = [4, 4, 3, 2, 1, 0, 2]
CLASSES = [7, -1, A, A - 1, 0]           # per slot: in range, negative, one past the end, A - 1, 0
PLACES = [33, L, -1, 0, L - 1]


def _pool(pixels, elems, stride, seed):
    rng = np.random.RandomState(seed)
    video = rng.randint(0, 256, size=(NSLOTS, stride)).astype(np.uint8)
    if pixels * 3 >= 256:
        video[4, :256] = np.arange(256)
    ac = (rng.rand(NSLOTS, elems) * 5 - 1).astype(np.float32)
    ac[3] = 3.25                                          # a constant frame: 0 / 0
    ac[4, 0], ac[4, -1] = -100.0, 100.0                   # minimum at element 0, maximum at the last one
    if elems > 2:
        ac[2, -1], ac[2, 0] = -50.0, 60.0                 # and the other way round
    mfcc = rng.rand(NSLOTS, 12).astype(np.float32)
    low = rng.rand(NSLOTS, 12).astype(np.float32)
    labels = np.stack([np.array(CLASSES), np.array(PLACES)], 1).astype(np.int32)
    return video, ac, mfcc, low, labels


def _one_hot(labels, width):
    out = np.zeros((len(labels), width), np.float32)
    for n, v in enumerate(labels):
        if 0 <= v < width:
            out[n, v] = 1.0
    return out


def _gather_case(device, N, pixels, elems, extra=0):
    from acimg import _lib
    lib = _lib.load()
    stride = -(-pixels * 3 // 16) * 16 + extra
    video, ac, mfcc, low, labels = _pool(pixels, elems, stride, seed=N * 1000 + pixels + elems)
    slots = np.array([SLOTS[n % 7] for n in range(N)], np.int32)
    dv = [torch.from_numpy(x).to(device) for x in (video, ac, mfcc, low, labels, slots)]
    ws_bytes = lib.acimg_batch_gather_workspace(N, elems)
    assert ws_bytes == 16 * N
    sizes = OrderedDict([("video", N * pixels * 12), ("acoustic", N * elems * 4), ("mfcc", N * 48), ("mfcc_low", N * 48),
                         ("action", N * A * 4), ("location", N * L * 4), ("ws", ws_bytes)])
    arena = GuardArena.for_sizes(device, sizes.values())
    r = OrderedDict((k, arena.region(v, name=k)) for k, v in sizes.items())
    st = torch.cuda.current_stream(device).cuda_stream

    def call(nbytes):
        return lib.acimg_batch_gather(dv[0].data_ptr(), stride, dv[1].data_ptr(), dv[2].data_ptr(), dv[3].data_ptr(),
                                      dv[4].data_ptr(), dv[5].data_ptr(), N, pixels, elems, A, L, r["video"].ptr,
                                      r["acoustic"].ptr, r["mfcc"].ptr, r["mfcc_low"].ptr, r["action"].ptr,
                                      r["location"].ptr, r["ws"].ptr, nbytes, st)
    assert call(ws_bytes - 16) == -2                       # a workspace 16 bytes short is refused ...
    torch.cuda.synchronize(device)
    assert bool((arena.buf == arena.canary).all())         # ... before anything is written
    _lib.check(call(ws_bytes), "batch_gather")
    torch.cuda.synchronize(device)
    arena.check("batch_gather N=%d pixels=%d elems=%d" % (N, pixels, elems))
    got = {k: r[k].view(torch.float32, v // 4).cpu().numpy() for k, v in sizes.items()}
    want_v = video[slots][:, :pixels * 3].reshape(N, pixels, 3)[..., ::-1].astype(np.float32) * np.float32(1.0 / 255.0)
    a = ac[slots]
    mn = a.min(axis=1, keepdims=True)
    a = a - mn
    mx = a.max(axis=1, keepdims=True)
    with np.errstate(invalid="ignore", divide="ignore"):
        want_a = a / mx
    assert np.array_equal(got["video"], want_v.reshape(-1))
    assert np.array_equal(got["acoustic"], want_a.reshape(-1), equal_nan=True)
    assert np.isnan(want_a).any() == bool((slots == 3).any() or elems == 1)       # the constant frame is NaN on both sides
    assert np.array_equal(got["mfcc"], mfcc[slots].reshape(-1)) and np.array_equal(got["mfcc_low"], low[slots].reshape(-1))
    assert np.array_equal(got["action"], _one_hot(labels[slots, 0], A).reshape(-1))
    assert np.array_equal(got["location"], _one_hot(labels[slots, 1], L).reshape(-1))
    stats = got["ws"].reshape(N, 4)
    assert np.array_equal(stats[:, 0], mn[:, 0]) and np.array_equal(stats[:, 1], mx[:, 0]) and not stats[:, 2:].any()
    return video, slots


@pytest.mark.parametrize("N", [1, 7, 33])
@pytest.mark.parametrize("pixels", [1, 15, 16, 17, 20, 4112, 66752])
def test_batch_gather_video_sizes(device, N, pixels):
    """1, 15, 17: the scalar path alone (rows of floats that are not 16-byte aligned); 16: one chunk; 20: a chunk and a
    tail; 4112 = 257 chunks: a whole tile and a tile of one chunk; 66752: the frame of the data set (4172 chunks)"""
    video, slots = _gather_case(device, N, pixels, elems=[5, 1000, 1][N % 3], extra=16 if N == 7 else 0)
    if pixels == 66752:
        assert len(np.unique(video[slots][:, :pixels * 3])) == 256           # every byte value went through


@pytest.mark.parametrize("N", [1, 7, 33])
@pytest.mark.parametrize("elems", [1, 4, 5, 1000, 1024, 1025, 4100, 16388, 20736, 32768])
def test_batch_gather_acoustic_sizes(device, N, elems):
    """float by float (1, 5, 1025: below and above one sweep of the 1024 threads) and as float4 (4, 1000; 4100 = one float4
    more than a sweep; 16388 = one more than four sweeps, the unrolled loads' second round); the data set's 36 x 48 x 12;
    the largest LDS image"""
    _gather_case(device, N, 16, elems)


# ---- the loader --------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def records(device, tmp_path_factory):
    """three GZIP files of one 12-frame record each, and the 36 frames `TFRecordDataLoader` makes of them (host tensors,
    computed once, never written to)"""
    from acimg.data import TFRecordDataLoader
    paths = write_outdoor_records(tmp_path_factory.mktemp("records"), 11, [(2 + 3 * r, 7 + r) for r in range(3)], wide=True)
    (frames,) = list(TFRecordDataLoader(paths, 64, device=device).data)
    assert frames[0].shape[0] == 36
    return paths, frames


def _same(got, want, what):
    assert len(got) == 6 and len(want) == 6
    for k, (g, w) in enumerate(zip(got, want)):
        assert g.dtype == w.dtype and g.shape == w.shape, (what, k, g.shape, w.shape)
        assert torch.equal(g.cpu(), w.cpu()), (what, k)


@pytest.mark.parametrize("bs", [5, 8, 64])
def test_loader_equals_the_host_loader(device, records, bs):
    """every tensor of every batch, `torch.equal` - the MFCC rows too: both loaders run the front end per record"""
    from acimg.data import DeviceDataLoader, TFRecordDataLoader
    paths, _ = records
    want = list(TFRecordDataLoader(paths, bs, device=device).data)
    seen = []
    for workers in (1, 4):
        dl = DeviceDataLoader(paths, bs, workers=workers, device=device)
        assert dl.num_samples == 36 and dl.total_batches == -(-36 // bs)
        got = []
        for b in dl.data:
            assert all(t.device == device for t in b)
            got.append(tuple(t.clone() for t in b))
        assert len(got) == len(want)
        for k, (g, w) in enumerate(zip(got, want)):
            _same(g, w, "batch %d, %d workers" % (k, workers))
        seen.append(got)
        dl.close()
    for g1, g4 in zip(*seen):
        _same(g1, g4, "1 worker against 4")


def _frames_of(loader):
    """the frames of one pass, copied out batch by batch (a yielded batch lives for `ring` iterations only)"""
    batches = [tuple(t.cpu() for t in b) for b in loader.data]
    return [torch.cat([b[k] for b in batches]) for k in range(6)]


def test_loader_shuffle(device, records):
    from acimg.data import DeviceDataLoader, epoch_files, epoch_rng, shuffle_order
    paths, frames = records

    def expected(seed, epoch, B):
        rng = epoch_rng(seed, epoch)
        files = epoch_files(paths, True, None, rng)                 # the file permutation comes first ...
        base = torch.cat([torch.arange(12) + 12 * paths.index(p) for p in files])
        return base[torch.tensor(shuffle_order(36, B, rng))]        # ... then the buffer, from the same generator

    dl = DeviceDataLoader(paths, 8, shuffle=True, buffer_size=5, seed=3, device=device)
    e0, e1 = _frames_of(dl), _frames_of(dl)
    for k in range(6):
        assert torch.equal(e0[k], frames[k][expected(3, 0, 5)]), k
        assert torch.equal(e1[k], frames[k][expected(3, 1, 5)]), k
    assert not torch.equal(e0[2], e1[2]) and not torch.equal(e0[2], frames[2])
    dl.close()
    again = DeviceDataLoader(paths, 8, shuffle=True, buffer_size=5, seed=3, device=device)
    for e in (e0, e1):
        for k, t in enumerate(_frames_of(again)):
            assert torch.equal(t, e[k]), k
    again.close()
    for B in (1, 1000):                                             # a buffer of one; a buffer larger than the data
        dl = DeviceDataLoader(paths, 8, shuffle=True, buffer_size=B, seed=5, device=device)
        got = _frames_of(dl)
        for k in range(6):
            assert torch.equal(got[k], frames[k][expected(5, 0, B)]), (B, k)
        assert dl._pool_pages <= 16                                 # the pool grows with need, not with buffer_size
        dl.close()


def test_loader_default_buffer_is_the_flag(device, records):
    from acimg.data import DeviceDataLoader
    from acimg.flags import FLAGS
    paths, _ = records
    assert DeviceDataLoader(paths, 8, shuffle=True, device=device).buffer_size == FLAGS.buffer_size
    assert DeviceDataLoader(paths, 8, device=device).buffer_size == 1
    assert DeviceDataLoader(paths, 8, workers=99, device=device).workers == 16


@pytest.mark.parametrize("repeat", [1, 3])
def test_loader_recycles_pages_and_ring(device, records, repeat):
    """buffer_size 3, prefetch 1, ring 2: six pages and two output sets.  Over the 36 frames the ring is reused; with the
    three files listed three times (nine records) the pages are too.  Every batch is right when yielded and still right
    one iteration later (ring - 1)."""
    from acimg.data import DeviceDataLoader, epoch_files, epoch_rng, shuffle_order
    paths, frames = records
    files = paths * repeat
    dl = DeviceDataLoader(files, 5, shuffle=True, buffer_size=3, seed=1, prefetch=1, ring=2, device=device)
    dl.FIRST_PAGES = 2                                              # start below the bound: growth is exercised as well
    rng = epoch_rng(1, 0)
    base = torch.cat([torch.arange(12) + 12 * paths.index(p) for p in epoch_files(files, True, None, rng)])
    order = base[torch.tensor(shuffle_order(36 * repeat, 3, rng))]
    held, k = [], 0
    for b in dl.data:
        rows = order[5 * k:5 * k + 5]
        _same(b, tuple(f[rows] for f in frames), "batch %d at yield" % k)
        held.append((b, rows))
        if k >= 1:
            old, old_rows = held[k - 1]
            _same(old, tuple(f[old_rows] for f in frames), "batch %d one iteration later" % (k - 1))
        k += 1
    assert k == -(-36 * repeat // 5)
    assert dl._pool_pages <= 6                                      # so the nine records of repeat = 3 shared pages
    dl.close()


def test_loader_feeds_the_trainer(device, records):
    """one epoch of `Trainer.train()` from each loader: the inputs are bit-equal and the step is deterministic, so the log
    lines and the validation loss are the same; then an epoch from the shuffled loader"""
    from acimg.data import DeviceDataLoader, TFRecordDataLoader
    from acimg.flags import FLAGS
    paths, _ = records
    FLAGS.checkpoint_dir, FLAGS.exp_name = None, "loader"
    FLAGS.restore_checkpoint = FLAGS.init_checkpoint = None
    FLAGS.acoustic_init_checkpoint = FLAGS.visual_init_checkpoint = None
    runs = []
    for kind in (TFRecordDataLoader, DeviceDataLoader):
        tr, sess = make(device, epochs=1)
        log = []
        tr.log = log.append
        best = tr.train(kind(paths, 8, device=device), kind(paths[:1], 8, device=device))
        assert tr.global_step == 5 and np.isfinite(best) and 0 < best < 1
        runs.append((loss_lines(log, validation=False), [ln.split("Validation_mse_Loss:")[1] for ln in log if "- Epoch:" in ln], best))
    assert len(runs[0][0]) == 5 and runs[0][0] == runs[1][0]
    assert len(runs[0][1]) == 1 and runs[0][1] == runs[1][1] and runs[0][2] == runs[1][2]
    log = []
    tr.log = log.append
    best = tr.train(DeviceDataLoader(paths, 8, shuffle=True, buffer_size=5, seed=2, device=device),
                    DeviceDataLoader(paths[:1], 8, device=device))
    assert tr.global_step == 10 and np.isfinite(best) and len(loss_lines(log, validation=False)) == 5
