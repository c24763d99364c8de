"""The device-free half of `acimg.data.DeviceDataLoader`: the shuffle buffer's emission order, the page bookkeeping of the
frame pool on a fake pool, sharding, and the refusals of `acimg_batch_gather` (all of them precede the first launch)."""
import ctypes as C

import numpy as np
import pytest

from data_support import FakePool

SIZES = [(1, 1), (24, 1), (24, 5), (24, 24), (24, 100), (1000, 100)]


def restated_order(n, B, rng):
    """tf.data's shuffle buffer, list-based: fill to B, emit a uniformly drawn occupied position, refill it with the next
    input, and close the hole with the last entry once the input is over"""
    todo = list(range(n))
    buf, todo = todo[:B], todo[B:]
    out = []
    while buf:
        j = int(rng.integers(len(buf)))
        out.append(buf[j])
        if todo:
            buf[j] = todo.pop(0)
        else:
            buf[j] = buf[-1]
            del buf[-1]
    return out


@pytest.mark.parametrize("n,B", SIZES)
def test_shuffle_order(n, B):
    from acimg.data import epoch_rng, shuffle_order
    order = shuffle_order(n, B, epoch_rng(7, 0))
    assert order == restated_order(n, B, epoch_rng(7, 0))
    assert sorted(order) == list(range(n))                                   # a permutation
    assert all(v <= k + B - 1 for k, v in enumerate(order))                  # output k was in the buffer by then
    assert order == shuffle_order(n, B, epoch_rng(7, 0))                     # (seed, epoch) decides it
    if B == 1:
        assert order == list(range(n))
    if B > 1 and n >= 24:
        assert order != shuffle_order(n, B, epoch_rng(7, 1))                 # reshuffle_each_iteration
        assert order != shuffle_order(n, B, epoch_rng(8, 0))


def test_shuffle_order_refuses_an_empty_buffer():
    from acimg.data import epoch_rng, shuffle_order
    with pytest.raises(ValueError):
        shuffle_order(5, 0, epoch_rng(0, 0))


@pytest.mark.parametrize("n,B", SIZES)
@pytest.mark.parametrize("batch,prefetch,first", [(5, 2, 16), (8, 0, 1), (64, 1, 4)])
def test_page_bookkeeping_on_a_fake_pool(n, B, batch, prefetch, first):
    """records of 12 frames (the last one shorter when n is no multiple) through `BatchFeeder`: no page is uploaded into
    while a frame of it waits to be gathered, the frames leave in `shuffle_order`, batches are dense, and
    buffer_size + prefetch + 2 pages are never exceeded"""
    from acimg.data import BatchFeeder, FramePages, epoch_rng, pool_pages, shuffle_order
    F = 12
    records = [min(F, n - r) for r in range(0, n, F)]
    limit = pool_pages(B, prefetch)
    assert limit == B + prefetch + 2
    pool = FakePool(F)
    pages = FramePages(first, limit, F)
    grown = []
    feeder = BatchFeeder(iter(records), pages, batch, B, prefetch, epoch_rng(3, 0), pool.upload, pool.gather,
                         grow=grown.append)
    sizes = []
    for got in feeder:
        sizes.append(got)
        assert not pages.pending                           # everything emitted so far has been gathered
        covered = sorted(pool.rows)                        # the gather calls of this batch tile rows 0 .. got
        assert covered[0][0] == 0 and sum(c for _, c in covered) == got
        assert all(a[0] + a[1] == b[0] for a, b in zip(covered, covered[1:]))
        pool.rows = []
    assert sizes == [batch] * (n // batch) + ([n % batch] if n % batch else [])
    assert pool.emitted == shuffle_order(n, B, epoch_rng(3, 0))
    assert pages.size <= limit and len(pool.pages_seen) <= limit and max(pool.pages_seen) < pages.size
    assert all(g <= limit for g in grown) and grown == sorted(grown)
    assert not any(pool.resident.values()) and not any(pages.live)


def test_the_page_bound_is_tight_enough_to_force_reuse():
    """buffer 3, prefetch 1: six pages for 20 records, so pages are recycled - and a batch of 64 frames, which empties
    five pages by itself, is gathered in pieces"""
    from acimg.data import BatchFeeder, FramePages, epoch_rng
    pool = FakePool(12)
    pages = FramePages(16, 6, 12)
    calls = []

    def gather(slots, offset):
        calls.append(offset)
        pool.gather(slots, offset)
    sizes = list(BatchFeeder(iter([12] * 20), pages, 64, 3, 1, epoch_rng(0, 0), pool.upload, gather))
    assert sizes == [64, 64, 64, 48] and pages.size == 6 and len(pool.pages_seen) == 6
    assert sorted(pool.emitted) == list(range(240))
    assert len(calls) > 4 and any(c > 0 for c in calls)


def test_shard_partitions_the_record_list():
    from acimg.data import epoch_files, epoch_rng
    files = ["f%02d" % i for i in range(11)]
    for world in (1, 2, 3, 4):
        parts = [epoch_files(files, False, (r, world), None) for r in range(world)]
        assert sorted(sum(parts, [])) == files
        assert all(p == files[r::world] for r, p in enumerate(parts))
        perm = epoch_files(files, True, None, epoch_rng(5, 2))
        assert sorted(perm) == files and perm != files
        shuffled = [epoch_files(files, True, (r, world), epoch_rng(5, 2)) for r in range(world)]
        assert all(p == perm[r::world] for r, p in enumerate(shuffled))       # every rank permutes alike, then takes its part
    assert epoch_files(files, True, None, epoch_rng(5, 3)) != perm
    for bad in ((2, 2), (-1, 2), (0, 0)):
        with pytest.raises(ValueError):
            epoch_files(files, False, bad, None)


def _call(lib, N=4, pixels=16, elems=8, stride=48, ws_bytes=None, null=None, A=10, L=61):
    """acimg_batch_gather on addresses that are never dereferenced: every case here is refused before a launch"""
    ptr = {k: 4096 * (i + 1) for i, k in enumerate(("pool_video", "pool_acoustic", "pool_mfcc", "pool_mfcc_low", "pool_labels",
                                                    "slots", "video", "acoustic", "mfcc", "mfcc_low", "action", "location",
                                                    "ws"))}
    if null is not None:
        ptr[null] = None
    if ws_bytes is None:
        ws_bytes = lib.acimg_batch_gather_workspace(N, elems)
    return lib.acimg_batch_gather(ptr["pool_video"], stride, ptr["pool_acoustic"], ptr["pool_mfcc"], ptr["pool_mfcc_low"],
                                  ptr["pool_labels"], ptr["slots"], N, pixels, elems, A, L, ptr["video"], ptr["acoustic"],
                                  ptr["mfcc"], ptr["mfcc_low"], ptr["action"], ptr["location"], ptr["ws"], ws_bytes, None)


def test_batch_gather_refusals_and_workspace_query():
    from acimg import _lib
    lib = _lib.load()
    EINVAL, EWORKSPACE = -1, -2
    assert lib.acimg_version() == 207                                   # the entry was added without a bump
    # the workspace: 16 bytes per frame, nothing for an empty batch
    assert lib.acimg_batch_gather_workspace(0, 20736) == 0 and lib.acimg_batch_gather_workspace(-3, 20736) == 0
    assert lib.acimg_batch_gather_workspace(1, 1) == 16 and lib.acimg_batch_gather_workspace(33, 20736) == 33 * 16
    for stride in (47, 50, 56, 72):                                     # not a multiple of 16
        assert _call(lib, stride=stride) == EINVAL
        assert "multiple of 16" in _lib.last_error()
    assert _call(lib, stride=32) == EINVAL                              # a multiple, but 16 pixels need 48 bytes
    assert _call(lib, elems=32769) == EINVAL and "LDS" in _lib.last_error()
    assert _call(lib, elems=1 << 30) == EINVAL
    for n in (0, -1, 65536):
        assert _call(lib, N=n, ws_bytes=1 << 20) == EINVAL
    for kw in (dict(pixels=0), dict(elems=0), dict(A=0), dict(L=0)):
        assert _call(lib, **kw) == EINVAL
    for name in ("pool_video", "pool_acoustic", "pool_mfcc", "pool_mfcc_low", "pool_labels", "slots", "video", "acoustic",
                 "mfcc", "mfcc_low", "action", "location", "ws"):
        assert _call(lib, null=name) == EINVAL, name
        assert "null" in _lib.last_error()
    need = lib.acimg_batch_gather_workspace(4, 8)
    assert _call(lib, ws_bytes=need - 16) == EWORKSPACE and _call(lib, ws_bytes=0) == EWORKSPACE


def test_workers_are_capped_without_asking_the_machine():
    import inspect

    from acimg import data
    src = inspect.getsource(data.DeviceDataLoader)
    assert "cpu_count" not in src and data.DeviceDataLoader.MAX_WORKERS == 16
