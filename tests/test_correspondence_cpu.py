"""The device-free half of the correspondence pairs (`correspondence=1`): the order of the two shuffle stages against the
list-based restatement of tests/correspondence_ref.py, the page bookkeeping with two uses per frame on a fake pool, the
refusals of `acimg_batch_gather_pairs` (all of them precede the first launch) and of the loaders."""
import pytest

import correspondence_ref as cref
from data_support import FakePool

# (frames, batch, buffer): frames < batch; frames % batch != 0; buffer 1; buffer > 2 * frames; a whole number of batches
ORDERS = [(3, 8, 2), (24, 5, 4), (24, 5, 1), (7, 3, 1), (10, 4, 25), (36, 8, 5), (36, 12, 100), (1, 1, 1), (100, 7, 13)]


@pytest.mark.parametrize("n,batch,B", ORDERS)
def test_pair_order(n, batch, B):
    from acimg.data import epoch_rng, pair_order, pair_rng, shuffle_order
    flat = lambda batches: [c for b in batches for c in b]
    for seed in (0, 7):
        want = flat(cref.pair_code_batches(n, batch, B, epoch_rng(seed, 0), pair_rng(seed, 0)))
        order = pair_order(n, batch, B, epoch_rng(seed, 0), pair_rng(seed, 0))
        assert order == want
        assert sorted(order) == list(range(-n, n))                     # every frame exactly once real and once silent
        assert order == pair_order(n, batch, B, epoch_rng(seed, 0), pair_rng(seed, 0))
        # without stage 2: the pair batches, whose real halves are the plain loader's batches under the same seed
        plain = pair_order(n, batch, B, epoch_rng(seed, 0))
        assert plain == flat(cref.pair_code_batches(n, batch, B, epoch_rng(seed, 0)))
        stage1 = shuffle_order(n, B, epoch_rng(seed, 0))
        assert [c for c in plain if c >= 0] == stage1 and [~c for c in plain if c < 0] == stage1
        at = 0
        for b in cref.cut(stage1, batch):
            assert plain[at:at + 2 * len(b)] == b + [~f for f in b]
            at += 2 * len(b)
        if B == 1:                                                     # no shuffling at all: [0..n), ~[0..n) per batch
            assert order == plain == flat(list(r) + [~f for f in r] for r in cref.cut(range(n), batch))
    if B > 1 and n >= 24:
        a = pair_order(n, batch, B, epoch_rng(7, 0), pair_rng(7, 0))
        assert a != pair_order(n, batch, B, epoch_rng(7, 1), pair_rng(7, 1))      # reshuffle_each_iteration
        assert a != pair_order(n, batch, B, epoch_rng(7, 0), pair_rng(7, 1))      # stage 2 alone reshuffles too
        assert a != pair_order(n, batch, B, epoch_rng(7, 0))


def test_pair_order_refusals_and_the_second_generator():
    from acimg.data import epoch_rng, pair_order, pair_rng
    for bad in ((5, 0, 1), (5, 2, 0)):
        with pytest.raises(ValueError):
            pair_order(*bad, epoch_rng(0, 0))
    a, b = pair_rng(3, 2).integers(1 << 30, size=4), epoch_rng(3, 2).integers(1 << 30, size=4)
    assert list(a) != list(b) and list(a) == list(pair_rng(3, 2).integers(1 << 30, size=4))


class PairPool(FakePool):
    """`FakePool` with two rows per frame: (frame, 0) and (frame, 1) are resident from upload until gathered; `emitted`
    collects row codes in frame numbering"""

    def upload(self, page, nframes):
        n = FakePool.upload(self, page, nframes)
        self.resident[page] = set((f, kind) for f in self.resident[page] for kind in (0, 1))
        return n

    def gather(self, codes, offset):
        self.rows.append((offset, len(codes)))
        for c in codes:
            slot = ~c if c < 0 else c
            f = self.where[slot]
            self.resident[slot // self.frames].remove((f, int(c < 0)))       # KeyError: gathered twice, or page reused
            self.emitted.append(~f if c < 0 else f)


@pytest.mark.parametrize("n,B", [(1, 1), (24, 1), (24, 5), (24, 100), (200, 7)])
@pytest.mark.parametrize("batch,prefetch,first", [(5, 2, 16), (8, 0, 1), (64, 1, 4)])
@pytest.mark.parametrize("stage2", [False, True])
def test_pair_page_bookkeeping_on_a_fake_pool(n, B, batch, prefetch, first, stage2):
    """records of 12 frames (the last one shorter) through `BatchFeeder(pairs=True)`: `PairPool.upload` refuses a page
    that still holds an un-gathered row, so no page is released before both rows of each of its frames are gathered; the
    rows leave in `pair_order`; the gathers of a batch tile its rows; `pair_pages` pages are never exceeded"""
    from acimg.data import BatchFeeder, FramePages, epoch_rng, pair_order, pair_pages, pair_rng
    F = 12
    records = [min(F, n - r) for r in range(0, n, F)]
    limit = pair_pages(B, batch, prefetch)
    assert limit == 2 * B + batch + prefetch
    pool = PairPool(F)
    pages = FramePages(first, limit, F, uses=2)
    grown = []
    rng2 = pair_rng(3, 0) if stage2 else None
    feeder = BatchFeeder(iter(records), pages, batch, B, prefetch, epoch_rng(3, 0), pool.upload, pool.gather,
                         grow=grown.append, pairs=True, rng2=rng2)
    sizes = []
    for got in feeder:
        sizes.append(got)
        assert not pages.pending
        covered = sorted(pool.rows)
        assert covered[0][0] == 0 and sum(c for _, c in covered) == got
        assert all(a[0] + a[1] == b[0] for a, b in zip(covered, covered[1:]))
        if not stage2:
            assert covered == [(0, got)]                   # a pair batch is one gather: its size was known at its first row
        pool.rows = []
    want = cref.pair_code_batches(n, batch, B, epoch_rng(3, 0), pair_rng(3, 0) if stage2 else None)
    assert sizes == [len(b) for b in want]
    if stage2:
        assert sizes == [batch] * (2 * n // batch) + ([2 * n % batch] if 2 * n % batch else [])
    else:
        assert sizes == [2 * batch] * (n // batch) + ([2 * (n % batch)] if n % batch else [])
    assert pool.emitted == [c for b in want for c in b]
    assert pool.emitted == pair_order(n, batch, B, epoch_rng(3, 0), pair_rng(3, 0) if stage2 else None)
    assert pages.size <= limit and len(pool.pages_seen) <= limit and max(pool.pages_seen) < pages.size
    assert all(g <= limit for g in grown) and grown == sorted(grown)
    assert not any(pool.resident.values()) and not any(pages.live)


@pytest.mark.parametrize("B,batch", [(1, 1), (1, 2), (2, 3), (3, 5)])
def test_the_pair_page_bound_is_reached(B, batch):
    """records of ONE frame, no prefetch: every frame with a row to come pins a page of its own, and the stated worst case
    - 2 * buffer_size + batch_size - 1 of them and a page to upload into - occurs: the bound suffices and uses its last
    page, and one page fewer trips the feeder's assertion"""
    from acimg.data import BatchFeeder, FramePages, epoch_rng, pair_pages, pair_rng
    limit = pair_pages(B, batch, 0)

    def run(pages_limit):
        pool, pages = PairPool(12), FramePages(1, pages_limit, 12, uses=2)
        sizes = list(BatchFeeder(iter([1] * 60), pages, batch, B, 0, epoch_rng(1, 0), pool.upload, pool.gather, pairs=True,
                                 rng2=pair_rng(1, 0)))
        return sizes, pool, pages
    sizes, pool, pages = run(limit)
    assert sum(sizes) == 120 and sorted(pool.emitted) == list(range(-60, 60))
    assert pages.size == limit and len(pool.pages_seen) == limit         # 60 records shared them: pages were recycled
    with pytest.raises(AssertionError, match="frame pool exhausted"):
        run(limit - 1)


def test_a_small_bound_recycles_pages_and_gathers_in_pieces():
    """buffer 2, batch 30, prefetch 1: 35 pages bound the need, 6 hold 20 records of 12 frames here, and a batch of 30 rows
    that empties pages of its own is gathered in pieces when a page is wanted"""
    from acimg.data import BatchFeeder, FramePages, epoch_rng, pair_rng
    pool, pages = PairPool(12), FramePages(2, 6, 12, uses=2)
    calls = []

    def gather(codes, offset):
        calls.append(offset)
        pool.gather(codes, offset)
    sizes = list(BatchFeeder(iter([12] * 20), pages, 30, 2, 1, epoch_rng(0, 0), pool.upload, gather, pairs=True,
                             rng2=pair_rng(0, 0)))
    assert sizes == [30] * 16 and sorted(pool.emitted) == list(range(-240, 240))
    assert pages.size <= 6 and any(c > 0 for c in calls)


def test_feeder_and_pages_refuse_a_mismatched_pair_setup():
    from acimg.data import BatchFeeder, FramePages, epoch_rng
    pool = PairPool(12)
    with pytest.raises(ValueError):                                       # pages that count one use per frame
        BatchFeeder(iter([12]), FramePages(4, 8, 12), 4, 1, 0, epoch_rng(0, 0), pool.upload, pool.gather, pairs=True)
    with pytest.raises(ValueError):                                       # whole records as the units
        BatchFeeder(iter([12]), FramePages(4, 8, 12, uses=2), 4, 1, 0, epoch_rng(0, 0), pool.upload, pool.gather,
                    units="records", pairs=True)
    assert FramePages(4, 8, 12).uses == 1                                 # the default is today's behaviour


def pairs_call(lib, N=4, pixels=16, elems=24, stride=48, ws_bytes=None, null=None, A=10, L=61):
    """acimg_batch_gather_pairs on addresses that are never dereferenced: every case here is refused before a launch (there
    is no GPU: a launch attempted first would come back as ACIMG_ELAUNCH instead)"""
    names = ("pool_video", "pool_acoustic", "pool_mfcc", "pool_mfcc_low", "pool_labels", "rows", "video", "acoustic", "mfcc",
             "pair", "action", "location", "ws")
    ptr = {k: 4096 * (i + 1) for i, k in enumerate(names)}
    if null is not None:
        ptr[null] = None
    if ws_bytes is None:
        ws_bytes = lib.acimg_batch_gather_pairs_workspace(N, elems)
    return lib.acimg_batch_gather_pairs(ptr["pool_video"], stride, ptr["pool_acoustic"], ptr["pool_mfcc"], ptr["pool_mfcc_low"],
                                        ptr["pool_labels"], ptr["rows"], N, pixels, elems, A, L, ptr["video"], ptr["acoustic"],
                                        ptr["mfcc"], ptr["pair"], ptr["action"], ptr["location"], ptr["ws"], ws_bytes, None)


def test_batch_gather_pairs_refusals_and_workspace_query():
    from acimg import _lib
    lib = _lib.load()
    EINVAL, EWORKSPACE = -1, -2
    assert lib.acimg_version() == 207                                   # the entry was added without a bump
    assert lib.acimg_batch_gather_pairs_workspace(0, 20736) == 0 and lib.acimg_batch_gather_pairs_workspace(-3, 20736) == 0
    assert lib.acimg_batch_gather_pairs_workspace(1, 12) == 16 and lib.acimg_batch_gather_pairs_workspace(33, 20736) == 33 * 16
    for elems in (1, 8, 13, 20, 20735, 32764):                          # the tiling needs whole pixels of 12
        assert pairs_call(lib, elems=elems, ws_bytes=1 << 20) == EINVAL, elems
        assert "multiple of 12" in _lib.last_error()
    # ... and everything acimg_batch_gather refuses
    for stride in (47, 50, 56, 72):
        assert pairs_call(lib, stride=stride) == EINVAL and "multiple of 16" in _lib.last_error()
    assert pairs_call(lib, stride=32) == EINVAL
    assert pairs_call(lib, elems=32772) == EINVAL and "LDS" in _lib.last_error()
    assert pairs_call(lib, elems=12 << 20) == EINVAL
    for n in (0, -1, 65536):
        assert pairs_call(lib, N=n, ws_bytes=1 << 20) == EINVAL
    for kw in (dict(pixels=0), dict(elems=0), dict(A=0), dict(L=0)):
        assert pairs_call(lib, **kw) == EINVAL
    for name in ("pool_video", "pool_acoustic", "pool_mfcc", "pool_mfcc_low", "pool_labels", "rows", "video", "acoustic",
                 "mfcc", "pair", "action", "location", "ws"):
        assert pairs_call(lib, null=name) == EINVAL, name
        assert "null" in _lib.last_error()
    need = lib.acimg_batch_gather_pairs_workspace(4, 24)
    assert pairs_call(lib, ws_bytes=need - 16) == EWORKSPACE and pairs_call(lib, ws_bytes=0) == EWORKSPACE
    assert "batch_gather_pairs" in _lib.last_error()


def test_loaders_refuse_clips_and_bad_values():
    """checked before anything touches a device or a file"""
    from acimg.data import DeviceDataLoader, TFRecordDataLoader, _correspondence
    assert _correspondence(0, 1) == 0 and _correspondence(1, 1) == 1 and _correspondence(0, 0) == 0
    for bad in (2, -1, "1", None, 0.5):
        with pytest.raises(ValueError, match="correspondence is 0 or 1"):
            _correspondence(bad, 1)
    with pytest.raises(ValueError, match="embedding=1"):
        _correspondence(1, 0)
    for kind in (DeviceDataLoader, TFRecordDataLoader):
        with pytest.raises(ValueError, match="embedding=1"):
            kind(["no such file"], 8, embedding=0, correspondence=1)
        for bad in (2, -1, "1"):
            with pytest.raises(ValueError, match="correspondence is 0 or 1"):
                kind(["no such file"], 8, correspondence=bad)


def test_the_classification_route_refuses_the_flag():
    from acimg.flags import FLAGS
    from acimg.main import dispatch
    keep = FLAGS.as_dict()
    try:
        FLAGS.parse(["--embedding", "0", "--model", "DualCamNet", "--correspondence", "1"])
        with pytest.raises(ValueError, match="--correspondence 1"):
            dispatch(FLAGS)
        FLAGS.parse(["--embedding", "0", "--model", "DualCamNet"])
        assert dispatch(FLAGS) == "classify"
        FLAGS.parse(["--embedding", "1", "--mfcc", "1", "--correspondence", "1"])
        assert dispatch(FLAGS) == "generator" and FLAGS.correspondence == 1
    finally:
        for k, v in keep.items():
            setattr(FLAGS, k, v)
