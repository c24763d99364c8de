"""Loaders with the surface of the reference's (dataloader/outdoor_data_mfcc.py): `.data` (iterable of 6-tuples
(acoustic [n,36,48,12], mfcc [n,12], video [n,224,298,3], action one-hot, location one-hot, mfcc of the low-passed
audio [n,12])), `.num_samples`, `.total_batches` (:117,214,973-976).

* `SyntheticDataLoader`: seeded synthetic tensors at the reference's shapes and value ranges (every tensor
  entering the hot path is float32 in [0,1]; acoustic image and MFCC vector min-max normalised per sample).
* `TFRecordDataLoader` (round 3): the reference's ON-DISK format end to end - GZIP TFRecords of `SequenceExample`s
  (convert_data.py:247-279) through the native reader behind the C ABI (`acimg_gzip_inflate`, `acimg_tfrecord_index`,
  `acimg_sequence_example_decode`: `_parse_sequence`, :263-343, with its LR + UD flip), the audio front end on the
  device (`acimg_filtfilt` = `butter_lowpass_filter`, :558-575; `acimg_mfcc_frontend` = `_build_spectrograms_function`,
  :796-876, with `_normalize_mfcc`, :696-703), the per-frame maps of :634-703 on the host, unbatch to frames and batch
  (:99-104): a plain Python generator, one record at a time, `shuffle=False`.
* `DeviceDataLoader` (round 5): the same files through the tf.data machinery the reference wraps around the parser -
  parallel map (`num_parallel_calls=4`), prefetch, and the shuffle buffer of :104-105 (`shuffle=True,
  buffer_size=FLAGS.buffer_size`, main.py:112-116) with `reshuffle_each_iteration`.  Decoded frames stay on the device
  in their raw form (video as bytes); a batch is assembled by `acimg_batch_gather`, which applies the per-frame maps
  while it gathers, and is handed out as device tensors.
* `correspondence=1` on either of the two (the published training recipe, `--correspondence 1`): the pair map of
  :108-113, 888-928 - every frame a second time with the MFCC of the low-passed sound, tiled, as its acoustic image -
  and, for a shuffling `DeviceDataLoader`, the second shuffle stage; the sixth tensor is then the one-hot
  correspondence label [n,2].
* `BoxRecordLoader`: the box-annotated Flickr-SoundNet records of dataloader/frames.py (`ActionsDataLoader(...,
  embedding=1, nr_frames=1, sample_length=1, shuffle=False)`, written by convert_data2.py:200-307): 8-tuples (acoustic
  zeros [n,36,48,12], mfcc [n,12], video [n,224,298,3], xmin, xmax, ymin, ymax, typescene [n,3] int32) that
  showimages_bb.py:86-93 indexes.  Records through `acimg_box_sequence_example_decode`; the MFCC of the whole clip is
  `box_mfcc` on the host (the [1, L] reading of `_build_spectrograms_function`).
* `ClassRecordLoader`: the two-object test set of dataloader/framesclass.py (records written by convert_data4.py, here
  `python -m acimg.convert_collected`): 4-tuples (acoustic zeros, mfcc [n,12], video [n,224,298,3], classnumber [n,1]
  int32), parsed with `tfio.parse_sequence_example`; the same `box_mfcc`."""
import collections
import concurrent.futures
import ctypes
import time

import numpy as np
import torch


class SyntheticDataLoader(object):
    def __init__(self, num_samples, batch_size, num_actions=10, num_locations=61, seed=1234, device="cpu"):
        self.num_samples = int(num_samples)
        self.batch_size = int(batch_size)
        self.total_batches = -(-self.num_samples // self.batch_size)
        self.num_actions, self.num_locations = num_actions, num_locations
        self.seed = seed
        self.device = device
        self.data = self

    def _batch(self, n, seed):
        g = torch.Generator().manual_seed(seed)
        video = torch.rand(n, 224, 298, 3, generator=g)
        mfcc = torch.rand(n, 12, generator=g)
        mfcc = mfcc - mfcc.amin(1, keepdim=True)
        mfcc = mfcc / mfcc.amax(1, keepdim=True)
        ac = torch.rand(n, 36, 48, 12, generator=g)
        ac = ac - ac.amin((1, 2, 3), keepdim=True)
        ac = ac / ac.amax((1, 2, 3), keepdim=True)
        labels = torch.nn.functional.one_hot(torch.randint(0, self.num_actions, (n,), generator=g), self.num_actions)
        scen = torch.nn.functional.one_hot(torch.randint(0, self.num_locations, (n,), generator=g), self.num_locations)
        return ac, mfcc, video, labels.float(), scen.float(), mfcc.clone()

    def __iter__(self):
        left = self.num_samples
        i = 0
        while left > 0:
            n = min(self.batch_size, left)
            yield self._batch(n, self.seed + i)
            left -= n
            i += 1


class TFRecordDataLoader(object):
    """`ActionsDataLoader(txt_file, mode, batch_size, ..., embedding=1, normalize=..., shuffle=False)` of the reference for
    the MFCC path (FLAGS.mfcc): one record = one second = 12 frames; frames are unbatched and re-batched to
    `batch_size` (:99-104).  `files`: a list of TFRecord paths, or the path of a text file listing them (:214-236).
    device: where the audio front end runs (a GPU: there is no CPU fallback); tensors are returned on the host, like the
    reference's session.run results, and `Trainer._feed` copies them up.
    embedding=0 is the path without `unbatch` (:102-107): `batch_size` counts records (clips); the frame tensors come out
    as [B*12, ...] with each clip's frames consecutive and in record order, the two label tensors as ONE row per clip
    ([B, num_actions], [B, num_locations]); `num_samples` / `total_batches` count clips.
    raw_audio=True: every batch carries a seventh tensor, the records' int32 [n,1024] audio samples as stored, batched
    like the other frame tensors (the sound track of `python -m acimg.show video --avi 1`).
    modalities: None = all three, every record must carry `audio/image`.  (1, 2) = audio data + video, the reference's
    `modalities=[1, 2]` (showvideo.py:72-75, outdoor_data_mfcc.py:35-37,316-317): records with or without `audio/image`
    - `python -m acimg.convert` writes none - are read, and the acoustic slot holds zeros [n,36,48,12] as :316 builds
    them; the other tensors are unchanged.  Other subsets are refused.  (Given by keyword, like `raw_audio`, which stays
    the last parameter.)
    correspondence=1 (given by keyword as well): the pair map of :108-109, 888-928 on every batch, in the form of a
    loader that does not shuffle (this one never does): a batch of n frames becomes 2n rows, the n real rows followed by the n silent
    rows of the same frames - acoustic image = the low-passed MFCC row tiled over the pixels (not normalised), mfcc =
    that row, video and labels (and raw audio) the frame's - and the sixth tensor is the one-hot correspondence label
    [2n, 2], [0, 1] real / [1, 0] silent.  `num_samples` / `total_batches` keep the reference's formulas (:973-976),
    which know nothing of the doubling; `num_rows` / `num_batches` are the counts of a pass.  Refused with
    embedding=0."""

    def __init__(self, files, batch_size, num_actions=10, num_locations=61, device="cuda:0", frames_per_record=12,
                 compression_verify=True, embedding=1, modalities=None, correspondence=0, raw_audio=False):
        if modalities is not None:
            if sorted(modalities) != [1, 2]:
                raise ValueError("modalities is None (acoustic image, audio, video) or (1, 2) (audio, video), got %r"
                                 % (modalities,))
            modalities = (1, 2)
        self.modalities = modalities
        from .frontend import FrontEnd
        if isinstance(files, str):
            with open(files) as f:
                files = [ln.strip() for ln in f if ln.strip()]
        self.files = list(files)
        self.batch_size = int(batch_size)
        self.num_actions, self.num_locations = int(num_actions), int(num_locations)
        self.frames = int(frames_per_record)
        self.verify = bool(compression_verify)
        self.embedding = _embedding(embedding)
        self.correspondence = _correspondence(correspondence, self.embedding)
        self.tensors = 7 if raw_audio else 6
        self.device = torch.device(device)
        self.fe = FrontEnd(self.device)
        self.data = self
        self._num_samples = None

    # ---- :117, :973-976 ---------------------------------------------------------------------------------------------
    @property
    def num_samples(self):
        """frames in the data set (every record is `frames_per_record` frames), clips with embedding=0: counted once
        from the record index"""
        if self._num_samples is None:
            from . import tfio
            records = sum(len(tfio.read_tfrecord_native(p, verify=False)) for p in self.files)
            self._num_samples = records * (self.frames if self.embedding else 1)
        return self._num_samples

    @property
    def total_batches(self):
        return -(-self.num_samples // self.batch_size)

    @property
    def num_rows(self):
        """rows (embedding=0: clips) of one pass: `num_samples`, twice that with correspondence=1"""
        return self.num_samples * (2 if self.correspondence else 1)

    @property
    def num_batches(self):
        """batches of one pass (the pair map doubles the rows of a batch, not the batches)"""
        return self.total_batches

    # ---- one record -> 12 frames (:263-343, :434-476, :558-575, :634-703) ---------------------------------------------
    def _record(self, rec):
        from . import tfio
        d = tfio.decode_sequence_example_native(rec)
        ai, sa, vi = d["audio_images"], d["audio_samples"], d["video_images"]
        n = vi.shape[0]
        if self.modalities is not None:      # audio + video: the acoustic image, if the record has one, is not read
            ai = np.zeros((n, 36, 48, 12), np.float32)
        if not (ai.shape[0] == n and sa.shape[0] == n and sa.shape[1] == 1024):
            raise ValueError("record with %d video / %d acoustic / %d audio steps" % (n, ai.shape[0], sa.shape[0]))
        # audio: raw frames -> device; low-passed copy (`filtered_wav`, :562) and the two MFCC vectors, each min-max
        # normalised per frame (`_normalize_mfcc`)
        frames = torch.from_numpy(np.ascontiguousarray(sa)).to(self.device)
        mfcc = self.fe._build_spectrograms_function(frames, normalize=True)
        low = self.fe.butter_lowpass_filter(frames)
        mfcc_low = self.fe._build_spectrograms_function(low, normalize=True)
        # acoustic images: per-frame min-max (`_normalize_acoustic_images_rescaled`, :672-679)
        a = ai.astype(np.float32)
        if self.modalities is None:
            a = a - a.min(axis=(1, 2, 3), keepdims=True)
            a = a / a.max(axis=(1, 2, 3), keepdims=True)
        # video: float, channel order reversed, 1/255 (`_normalize_images_rescaled`, :649-655)
        v = vi[..., ::-1].astype(np.float32) * np.float32(1.0 / 255.0)
        act = np.zeros((n, self.num_actions), np.float32)
        act[:, d["action"]] = 1.0
        loc = np.zeros((n, self.num_locations), np.float32)
        loc[:, d["location"]] = 1.0
        out = (torch.from_numpy(a), mfcc.cpu(), torch.from_numpy(np.ascontiguousarray(v)), torch.from_numpy(act),
               torch.from_numpy(loc), mfcc_low.cpu())
        if self.tensors == 7:
            out += (torch.from_numpy(np.ascontiguousarray(sa, dtype=np.int32)),)
        return out

    def _clip_batch(self, pend):
        """whole records -> one clip batch: frames concatenated, the two label tensors cut to one row per record"""
        for p_ in pend:
            if p_[0].shape[0] != self.frames:
                raise ValueError("clip mode wants records of %d frames, got one of %d" % (self.frames, p_[0].shape[0]))
        return tuple(torch.cat([(p_[k][:1] if k in (3, 4) else p_[k]) for p_ in pend], 0) for k in range(self.tensors))

    def _iter_clips(self):
        from . import tfio
        pend = []
        for path in self.files:
            for rec in tfio.read_tfrecord_native(path, verify=self.verify):
                if len(rec) == 0:
                    continue
                pend.append(self._record(rec))
                if len(pend) == self.batch_size:
                    yield self._clip_batch(pend)
                    pend = []
        if pend:
            yield self._clip_batch(pend)

    def _pairs(self, b):
        """`_map_func_correspondence` (:888-928) on one batch"""
        ac, mfcc, video, act, loc, low = b[:6]
        n = ac.shape[0]
        silent = low.reshape((n,) + (1,) * (ac.dim() - 2) + (12,)).expand_as(ac)
        label = torch.zeros(2 * n, 2)
        label[:n, 1] = 1.0
        label[n:, 0] = 1.0
        out = (torch.cat([ac, silent]), torch.cat([mfcc, low]), torch.cat([video, video]), torch.cat([act, act]),
               torch.cat([loc, loc]), label)
        return out + tuple(torch.cat([t, t]) for t in b[6:])

    def __iter__(self):
        batches = self._iter_clips() if not self.embedding else self._iter_frames()
        for b in batches:
            yield self._pairs(b) if self.correspondence else b

    def _iter_frames(self):
        from . import tfio
        pend, have = [], 0
        for path in self.files:
            for rec in tfio.read_tfrecord_native(path, verify=self.verify):
                if len(rec) == 0:
                    continue
                pend.append(self._record(rec))
                have += pend[-1][0].shape[0]
                while have >= self.batch_size:
                    cat = [torch.cat([p_[k] for p_ in pend], 0) for k in range(self.tensors)]
                    yield tuple(c[:self.batch_size] for c in cat)
                    rest = tuple(c[self.batch_size:] for c in cat)
                    have = rest[0].shape[0]
                    pend = [rest] if have else []
        if have:
            yield tuple(torch.cat([p_[k] for p_ in pend], 0) for k in range(self.tensors))


# ---- the tf.data machinery of dataloader/outdoor_data_mfcc.py:99-105 -------------------------------------------------
_END = object()


def _embedding(embedding):
    """the reference's `embedding` argument: 1 un-batches records to frames, 0 keeps records whole (clips)"""
    if embedding not in (0, 1, False, True):
        raise ValueError("embedding is 1 (frames) or 0 (clips), got %r" % (embedding,))
    return int(embedding)


def _correspondence(correspondence, embedding):
    """the reference's `correspondence` argument: 1 adds the pair map of :108-113 (frames only)"""
    if correspondence not in (0, 1, False, True):
        raise ValueError("correspondence is 0 or 1, got %r" % (correspondence,))
    if correspondence and not embedding:
        raise ValueError("correspondence=1 needs embedding=1: the pair map's reshape(-1, 1, 12) of a clip batch has no defined "
                         "meaning in main.py's dispatch")
    return int(correspondence)


def epoch_rng(seed, epoch):
    """the generator of one pass over the data: `reshuffle_each_iteration` is a new `epoch`"""
    return np.random.Generator(np.random.PCG64([int(seed), int(epoch)]))


def pair_rng(seed, epoch):
    """the generator of a pass's SECOND shuffle stage (the one behind the pair map): one of its own, so that stage 1 draws
    from `epoch_rng(seed, epoch)` exactly what it draws in a loader without the pair map"""
    return np.random.Generator(np.random.PCG64([int(seed), int(epoch), 1]))


def shuffle_stream(inputs, buffer_size, rng):
    """tf.data's shuffle buffer over an iterator: fill to `buffer_size`; every output takes a uniformly drawn occupied
    position, which is refilled with the next input; when the input ends the buffer drains (the last occupied position
    moves into the hole).  Only the procedure is TensorFlow's: its random stream cannot be reproduced and is not claimed."""
    inputs = iter(inputs)
    buf = []
    while len(buf) < buffer_size:
        x = next(inputs, _END)
        if x is _END:
            break
        buf.append(x)
    while buf:
        j = int(rng.integers(len(buf)))
        out = buf[j]
        x = next(inputs, _END)
        if x is _END:
            buf[j] = buf[-1]
            buf.pop()
        else:
            buf[j] = x
        yield out


def shuffle_order(n_frames, buffer_size, rng):
    """emission order of `n_frames` inputs 0, 1, ... through a shuffle buffer of `buffer_size` (1: the identity)"""
    if buffer_size < 1:
        raise ValueError("buffer_size must be at least 1, got %r" % (buffer_size,))
    return list(shuffle_stream(range(int(n_frames)), int(buffer_size), rng))


def pair_batches(inputs, batch_size, buffer_size, rng1):
    """stage 1 and the pair map of :104-109 over an iterator of non-negative ints: shuffle buffer, batches of
    `batch_size` (the last may be short), and every batch [x0 .. xn-1] expanded to the ROW CODES [x0 .. xn-1, ~x0 ..
    ~xn-1]: x is the real row of x, ~x (negative) its silent row.  A batch is expanded once stage 1 has completed it."""
    batch = []
    for x in shuffle_stream(inputs, buffer_size, rng1):
        batch.append(x)
        if len(batch) == batch_size:
            yield batch + [~v for v in batch]
            batch = []
    if batch:
        yield batch + [~v for v in batch]


def pair_stream(inputs, batch_size, buffer_size, rng1, rng2):
    """stage 2 (:110-112): the rows of the pair batches, in order, through a second shuffle buffer of `buffer_size` rows
    drawing from `rng2`"""
    return shuffle_stream((code for b in pair_batches(inputs, batch_size, buffer_size, rng1) for code in b), buffer_size,
                          rng2)


def pair_order(n_frames, batch_size, buffer_size, rng1, rng2=None):
    """row codes, in frame numbering, of one pass over `n_frames` frames with the pair map: the pair batches one after
    the other (rng2 None: a loader that does not shuffle; cut them at the batches of `shuffle_order` to get its batches),
    or those rows through stage 2 (a shuffling loader, which re-batches them to `batch_size` rows)"""
    if batch_size < 1 or buffer_size < 1:
        raise ValueError("batch_size and buffer_size must be at least 1, got %r, %r" % (batch_size, buffer_size))
    frames = range(int(n_frames))
    if rng2 is None:
        return [code for b in pair_batches(frames, int(batch_size), int(buffer_size), rng1) for code in b]
    return list(pair_stream(frames, int(batch_size), int(buffer_size), rng1, rng2))


def epoch_files(files, shuffle, shard, rng):
    """the record files of one pass: permuted with the pass's generator when shuffling (`_shuffle_and_repeat_lists`,
    :218-225), then entries i % world == rank of that list for shard = (rank, world)"""
    files = list(files)
    if shuffle:
        files = [files[i] for i in rng.permutation(len(files))]
    if shard is not None:
        rank, world = int(shard[0]), int(shard[1])
        if not 0 <= rank < world:
            raise ValueError("shard = (rank, world) with 0 <= rank < world, got %r" % (shard,))
        files = files[rank::world]
    return files


def pool_pages(buffer_size, prefetch):
    """pages that always suffice: at most `buffer_size` un-emitted frames sit in the shuffle buffer and one frame can
    pin a page; one record is being fed into the buffer; `prefetch` records are uploaded ahead; one page to upload into.
    With whole records as the units (`BatchFeeder(..., units="records")`) `buffer_size` counts records: an un-emitted
    record pins exactly its own page, so the same `buffer_size + prefetch + 2` holds (the pages emptied by the batch
    being assembled come back at its gather, which `_admit` forces when it finds no free page)."""
    return int(buffer_size) + int(prefetch) + 2


def pair_pages(buffer_size, batch_size, prefetch):
    """pages that always suffice with the pair map (`BatchFeeder(..., pairs=True)`), where a frame pins its page until
    BOTH of its rows are emitted.  When a record is admitted, the frames with a row to come are: at most `buffer_size`
    in the stage-1 buffer (the one just drawn included), at most `batch_size - 1` in the pair batch that stage 1 is
    completing (stage 1 is only asked for more once stage 2 has taken every row of the batch before), and at most
    `buffer_size` with a row in the stage-2 buffer (the row just drawn included): 2 * buffer_size + batch_size - 1
    frames, one page each at the worst, and one page to upload into.  That is 2 * buffer_size + batch_size, reached by
    records of one frame; `prefetch` more let records be uploaded ahead at that moment too (uploading ahead only ever
    takes a free page, so it adds nothing to the need).  Without stage 2 (a loader that does not shuffle) the third term
    is absent and the bound, kept as it is, is `buffer_size` pages loose."""
    return 2 * int(buffer_size) + int(batch_size) + int(prefetch)


class FramePages(object):
    """Bookkeeping of the frame pool, no device in sight: pages of `frames` slots; a page is taken for one record, counts
    that record's un-emitted frames, and comes back once its last frame's gather has been enqueued (`release`).  The pool
    starts with `size` pages and may grow to `limit`.  uses: how often every frame is emitted before it is done with (2 with
    the pair map: its real and its silent row)."""

    def __init__(self, size, limit, frames, uses=1):
        self.frames, self.limit, self.size = int(frames), int(limit), min(int(size), int(limit))
        self.uses = int(uses)
        self.live = [0] * self.size
        self.free = list(range(self.size - 1, -1, -1))
        self.pending = []

    def acquire(self):
        """a page that holds no un-emitted frame, or None"""
        if not self.free:
            return None
        page = self.free.pop()
        assert self.live[page] == 0, "page %d handed out with %d live frames" % (page, self.live[page])
        return page

    def fill(self, page, n):
        assert 0 < n <= self.frames and self.live[page] == 0
        self.live[page] = n * self.uses

    def emit(self, slot):
        page = slot // self.frames
        assert self.live[page] > 0
        self.live[page] -= 1
        if self.live[page] == 0:
            self.pending.append(page)

    def release(self):
        """every emitted frame's gather is enqueued: the emptied pages may be uploaded into again (stream order)"""
        self.free.extend(reversed(self.pending))
        self.pending = []

    def grow(self):
        """double the pool up to `limit`; returns the new size (unchanged at the limit)"""
        new = min(self.limit, max(2 * self.size, 1))
        self.free = list(range(new - 1, self.size - 1, -1)) + self.free
        self.live += [0] * (new - self.size)
        self.size = new
        return new


class BatchFeeder(object):
    """One pass: records -> pages -> shuffle buffer -> batches of slots.  Everything that touches a device is a callback,
    so the page logic runs on a fake pool in the tests:
      records      iterator of decoded records, in file order (`next` may block on a worker)
      ready()      True when `next(records)` would not block (only such records are uploaded ahead of need)
      upload(page, record) -> frames in the record (enqueues the copies and the audio front end)
      gather(slots, offset) enqueues the gather of these slots into rows offset.. of the batch being assembled
      grow(pages)  the pool now has `pages` pages
    A batch is gathered in one call unless a page is wanted while the only candidates are pages emptied by THIS batch:
    then the rows chosen so far are gathered first, which frees them.
    units="records" (the loaders' embedding=0): the shuffle buffer holds whole records and `batch_size` counts them; a
    record's slots enter the batch together, in record order.
    pairs=True (the loaders' correspondence=1; `pages` must count two uses per frame): what `gather` receives are ROW
    CODES, slot or ~slot (`pair_batches`).  rng2 None: a batch is one pair batch, up to 2 * batch_size rows; its rows are
    chosen only once stage 1 has completed it, so its size is known at its first row, no record is admitted between its
    rows, and it is gathered in one call at offset 0.  With rng2 the rows pass stage 2 (`pair_stream`) and leave in
    batches of `batch_size` rows.  `pair_pages` is the page bound."""

    def __init__(self, records, pages, batch_size, buffer_size, prefetch, rng, upload, gather, grow=None, ready=None,
                 units="frames", pairs=False, rng2=None):
        if units not in ("frames", "records"):
            raise ValueError("units is 'frames' or 'records', got %r" % (units,))
        self.by_record = units == "records"
        self.pairs, self.rng2 = bool(pairs), rng2
        if self.pairs and (self.by_record or pages.uses != 2):
            raise ValueError("the pair map wants frames as the units and pages that count two uses per frame")
        self.records, self.pages = iter(records), pages
        self.batch_size, self.buffer_size, self.prefetch, self.rng = int(batch_size), int(buffer_size), int(prefetch), rng
        self.upload, self.gather, self.grow_cb, self.ready = upload, gather, grow, ready or (lambda: True)
        self.ahead = collections.deque()      # (page, frames) uploaded, not yet fed into the shuffle buffer
        self.done = False
        self.batch, self.flushed = [], 0

    def _admit(self):
        rec = next(self.records, None)
        if rec is None:
            self.done = True
            return False
        page = self.pages.acquire()
        if page is None and self.pages.pending:
            self._flush()
            page = self.pages.acquire()
        if page is None and self.pages.size < self.pages.limit:
            size = self.pages.grow()
            if self.grow_cb is not None:
                self.grow_cb(size)
            page = self.pages.acquire()
        assert page is not None, "frame pool exhausted: %d pages (%s) must suffice" % (
            self.pages.limit, "2 * buffer_size + batch_size + prefetch" if self.pairs else "buffer_size + prefetch + 2")
        n = self.upload(page, rec)
        self.pages.fill(page, n)
        self.ahead.append((page, n))
        return True

    def _slots(self):
        """the shuffle buffer's inputs: single slots, or one tuple of slots per record"""
        while self.ahead or (not self.done and self._admit()):
            page, n = self.ahead.popleft()
            if self.by_record:
                yield tuple(page * self.pages.frames + i for i in range(n))
                continue
            for i in range(n):
                yield page * self.pages.frames + i

    def _flush(self):
        if self.flushed < len(self.batch):
            self.gather(self.batch[self.flushed:], self.flushed)
            self.flushed = len(self.batch)
        self.pages.release()

    def _top_up(self):
        while (len(self.ahead) < self.prefetch and not self.done and self.ready()
               and (self.pages.free or self.pages.size < self.pages.limit)):
            self._admit()

    def _rows(self):
        """(rows, last): the rows that enter the batch together, and whether they complete it"""
        if self.pairs and self.rng2 is None:
            for b in pair_batches(self._slots(), self.batch_size, self.buffer_size, self.rng):
                for k, code in enumerate(b):
                    yield (code,), k == len(b) - 1
            return
        if self.pairs:
            stream = pair_stream(self._slots(), self.batch_size, self.buffer_size, self.rng, self.rng2)
        else:
            stream = shuffle_stream(self._slots(), self.buffer_size, self.rng)
        for k, unit in enumerate(stream):
            yield (unit if self.by_record else (unit,)), (k + 1) % self.batch_size == 0

    def __iter__(self):
        """yields the size of each batch once its gather is enqueued"""
        for rows, last in self._rows():
            for row in rows:
                self.batch.append(row)
                self.pages.emit(~row if row < 0 else row)
            if last:
                self._flush()
                self._top_up()
                yield len(self.batch)
                self.batch, self.flushed = [], 0
        if self.batch:
            self._flush()
            yield len(self.batch)
            self.batch, self.flushed = [], 0


def _inflate_file(path, verify):
    """worker stage 1: file -> (inflated image, record offsets, record lengths, seconds spent inflating / indexing)"""
    from . import _lib
    lib = _lib.load()
    t0 = time.perf_counter()
    raw = np.fromfile(path, dtype=np.uint8)
    gz = raw.size >= 18 and raw[0] == 0x1f and raw[1] == 0x8b
    # a GZIP member ends with its inflated size mod 2^32: the first guess, so that most files are inflated once
    guess = int(raw[-4:].view("<u4")[0]) if gz else raw.size
    produced = ctypes.c_size_t(0)
    buf = np.empty(max(guess, 1), dtype=np.uint8)
    rc = lib.acimg_gzip_inflate(raw.ctypes.data, raw.size, buf.ctypes.data, buf.size, ctypes.byref(produced))
    if rc == -2:
        buf = np.empty(max(produced.value, 1), dtype=np.uint8)
        rc = lib.acimg_gzip_inflate(raw.ctypes.data, raw.size, buf.ctypes.data, buf.size, ctypes.byref(produced))
    _lib.check(rc, "gzip_inflate")
    t1 = time.perf_counter()
    n = produced.value
    count = lib.acimg_tfrecord_index(buf.ctypes.data, n, None, None, 0, int(bool(verify)))
    if count < 0:
        raise IOError("%s: %s" % (path, _lib.last_error()))
    off = np.zeros(max(count, 1), dtype=np.uint64)
    ln = np.zeros(max(count, 1), dtype=np.uint64)
    lib.acimg_tfrecord_index(buf.ctypes.data, n, off.ctypes.data, ln.ctypes.data, count, 0)
    keep = [i for i in range(count) if ln[i]]
    return buf, [int(off[i]) for i in keep], [int(ln[i]) for i in keep], t1 - t0, time.perf_counter() - t1


def _read_file(path):
    """worker stage 0 of the device path: file -> (file image, its gzip plan or None, seconds)"""
    from . import inflate as _inflate
    t0 = time.perf_counter()
    raw = np.fromfile(path, dtype=np.uint8)
    return raw, _inflate.gzip_plan(raw), time.perf_counter() - t0


def _index_file(path, raw, plan, data, status, end_bits, verify):
    """worker stage 1 of the device path: the device's result for a file is checked against its container (CRC-32, ISIZE,
    where the stream ends; the host's reader takes the file otherwise), then indexed as `_inflate_file` does"""
    from . import _lib
    from . import inflate as _inflate
    lib = _lib.load()
    t0 = time.perf_counter()
    buf = _inflate.gzip_verify(raw, plan, data, status, end_bits)
    t1 = time.perf_counter()
    n = buf.size
    count = lib.acimg_tfrecord_index(buf.ctypes.data, n, None, None, 0, int(bool(verify)))
    if count < 0:
        raise IOError("%s: %s" % (path, _lib.last_error()))
    off = np.zeros(max(count, 1), dtype=np.uint64)
    ln = np.zeros(max(count, 1), dtype=np.uint64)
    lib.acimg_tfrecord_index(buf.ctypes.data, n, off.ctypes.data, ln.ctypes.data, count, 0)
    keep = [i for i in range(count) if ln[i]]
    return buf, [int(off[i]) for i in keep], [int(ln[i]) for i in keep], t1 - t0, time.perf_counter() - t1


def _record_dims(buf, off, ln):
    """AcimgSequenceDims of the serialized SequenceExample at buf[off:off + ln] (sizes only)"""
    from . import _lib
    dims = _lib.SequenceDims()
    _lib.check(_lib.load().acimg_sequence_example_decode(buf.ctypes.data + off, ln, ctypes.byref(dims), None, 0, None, 0,
                                                         None, 0), "sequence_example_decode")
    return dims


class _Staging(object):
    """pinned host buffers of one record (video bytes, acoustic floats, audio samples, labels) + the event behind the
    uploads that read them"""

    def __init__(self, frames, pixels3, elems):
        self.video = torch.empty(frames, pixels3, dtype=torch.uint8).pin_memory()
        self.acoustic = torch.empty(frames, elems, dtype=torch.float32).pin_memory()
        self.audio = torch.empty(frames, 1024, dtype=torch.int32).pin_memory()
        self.labels = torch.empty(frames, 2, dtype=torch.int32).pin_memory()
        self.event = None
        self.n = 0


def _decode_record(buf, off, ln, st, dims0):
    """worker stage 2: one serialized SequenceExample -> the pinned buffers of `st`; returns seconds spent"""
    from . import _lib
    lib = _lib.load()
    t0 = time.perf_counter()
    base = buf.ctypes.data + off
    dims = _record_dims(buf, off, ln)
    n = int(dims.video_steps)
    shape = (int(dims.audio_height), int(dims.audio_width), int(dims.audio_depth), int(dims.video_height),
             int(dims.video_width), int(dims.video_depth))
    if not (dims.audio_image_steps == n and dims.audio_data_values == n * 1024 and dims.samples == 1024):
        raise ValueError("record with %d video / %d acoustic steps, %d audio values of %d samples"
                         % (n, dims.audio_image_steps, dims.audio_data_values, dims.samples))
    if shape != dims0 or not 0 < n <= st.video.shape[0]:
        raise ValueError("record of %d frames with dimensions %r in a data set of <= %d frames with %r"
                         % (n, shape, st.video.shape[0], dims0))
    _lib.check(lib.acimg_sequence_example_decode(base, ln, ctypes.byref(dims), st.acoustic.data_ptr(), st.acoustic.numel(),
                                                 st.audio.data_ptr(), st.audio.numel(), st.video.data_ptr(),
                                                 st.video.numel()), "sequence_example_decode")
    st.labels[:n, 0] = int(dims.classes)
    st.labels[:n, 1] = int(dims.location)
    st.n = n
    return time.perf_counter() - t0


class DeviceDataLoader(object):
    """`ActionsDataLoader(txt_file, mode, batch_size, ..., embedding=1, shuffle=..., buffer_size=...)` of the reference for
    the MFCC path, with the tf.data stages around the record parser: the same 6-tuples as `TFRecordDataLoader`, same
    order, shapes and dtypes, ON `device`.

    * workers: `workers` (<= 16) threads read, inflate, index and decode records into pinned staging buffers through the
      C ABI (ctypes drops the GIL); records are consumed in file order whatever order the workers finish in; a staging
      buffer is written again only after the event behind its upload has completed.
    * pool: decoded records live on the device in pages of `frames_per_record` slots (video as stored bytes, the
      acoustic image as decoded, the raw audio, the two MFCC rows, the labels): one upload per modality and record.  The
      audio front end (`FrontEnd`, per record as in `TFRecordDataLoader`) fills the MFCC rows in place.  Uploads, front
      end and gathers share ONE stream, so a page emptied by a gather may be uploaded into right away.
      `pool_pages(buffer_size, prefetch)` pages suffice (asserted); the pool starts small and doubles up to that.
    * shuffle: frames leave in `shuffle_order` (tf.data's shuffle buffer, un-batched frames, :104-105) drawn from
      `epoch_rng(seed, epoch)`, epoch = the number of `__iter__` calls before this one; with `shuffle=True` the file list
      is permuted first with the same generator.  `shuffle=False` is a buffer of one.
    * batches are gathered (`acimg_batch_gather`) into one of `ring` output sets: a yielded batch stays valid until the
      iterator has advanced `ring` more times.  The consumer's current stream waits for the gather's event on the GPU;
      nothing synchronises the host.  One pass at a time: starting a new one ends the previous iterator.
    * shard = (rank, world): files i % world == rank of the (permuted) list.
    * embedding=0 (the path without `unbatch`, :102-107): `batch_size` counts records (clips) and the shuffle buffer
      holds whole records - same procedure, seeding and file permutation, records as the units.  A clip batch is only
      another slot list for the same gather: frame tensors [B*12, ...] with each clip's frames consecutive and in record
      order; the label tensors are the strided view of the gathered rows that keeps one row per clip ([B, num_actions],
      [B, num_locations]).  `num_samples` / `total_batches` count clips; every record must hold `frames_per_record`
      frames.  `pool_pages` states why the page bound is the same with records as the units.
    * correspondence=1 (`--correspondence 1`, the published recipe; :108-113, 888-928; embedding=1 only): stage 1 is all of
      the above, unchanged.  A stage-1 batch of n frames becomes a pair batch of 2n rows: the n real rows - today's
      tensors - then the n silent rows of the same frames in the same order: acoustic image = the frame's low-passed
      MFCC row tiled over the pixels (not normalised), mfcc = that row, video and labels the frame's.  The sixth tensor
      is no longer `mfcc_low` but the one-hot correspondence label [rows, 2], [0, 1] real / [1, 0] silent.
      STAGE 2 RUNS ONLY FOR A SHUFFLING LOADER: the reference un-batches, shuffles again and re-batches under `mode ==
      'training'` (:110), and `acimg.main` passes shuffle=True exactly for that mode.  Then the rows of the pair batches,
      in order, pass a second shuffle buffer of `buffer_size` rows that draws from `pair_rng(seed, epoch)` - a generator
      of its own, so stage 1 emits the order the plain loader emits under the same seed - and leave in batches of
      `batch_size` rows: 2 * num_samples rows in ceil(2 * num_samples / batch_size) batches.  As with `shuffle_stream`,
      the procedure is tf.data's, the random stream is not.  A loader that does not shuffle yields the pair batches
      themselves: ceil(num_samples / batch_size) batches of up to 2 * batch_size rows, for which the output ring is
      sized.  The silent half of such a batch starts at the batch's final size: the rows of a pair batch are chosen only
      once stage 1 has completed it (`BatchFeeder`), so that size is known at the first row and the batch is one gather.
      A frame stays resident until both of its rows are gathered (`FramePages(uses=2)`); `pair_pages` is the page bound
      (asserted).  A batch is one `acimg_batch_gather_pairs` over row codes, still one int32 list uploaded per gather.
      `num_samples` / `total_batches` keep the reference's formulas (:973-976), which know nothing of the doubling;
      `num_rows` / `num_batches` are the true counts of a pass.
    * inflate="device" (default "zlib": the workers' `acimg_gzip_inflate`, nothing changes): the workers read the files and
      parse the gzip headers; the files of the look-ahead, up to `workers` of them, are inflated in ONE
      `acimg.inflate.DeviceInflater.gunzip_device` call on the loader's stream and copied to pinned host memory; the workers
      check each against its container (end of the stream, ISIZE, CRC-32) and index it, and hand whatever the device path
      does not take - a second member, a failed stream, a mismatch - to `acimg_gzip_inflate`, which raises what it always
      raised.  Everything after the inflated image is the same code.  `times["inflate"]` is then the host's share and
      `times["inflate_device"]` the consuming thread's seconds in the grouped calls.
    `times` accumulates the host seconds of the stages (inflate, index, decode in the workers; upload, wait on the
    consuming thread)."""

    MAX_WORKERS = 16
    FIRST_PAGES = 16

    def __init__(self, files, batch_size, shuffle=False, buffer_size=None, seed=0, workers=4, prefetch=2, ring=4,
                 shard=None, num_actions=10, num_locations=61, device="cuda:0", compression_verify=True,
                 frames_per_record=12, embedding=1, correspondence=0, inflate="zlib"):
        from . import ops
        from .flags import FLAGS
        from .frontend import FrontEnd
        if inflate not in ("zlib", "device"):
            raise ValueError("inflate is 'zlib' or 'device', got %r" % (inflate,))
        self.inflate = inflate
        if isinstance(files, str):
            with open(files) as f:
                files = [ln.strip() for ln in f if ln.strip()]
        self.files = list(files)
        self.batch_size = int(batch_size)
        self.shuffle = bool(shuffle)
        self.buffer_size = (int(FLAGS.buffer_size if buffer_size is None else buffer_size)) if self.shuffle else 1
        self.seed, self.shard = int(seed), shard
        self.workers = max(1, min(int(workers), self.MAX_WORKERS))
        self.prefetch, self.ring = max(0, int(prefetch)), int(ring)
        if self.batch_size < 1 or self.buffer_size < 1 or self.ring < 1:
            raise ValueError("batch_size, buffer_size and ring must be at least 1")
        epoch_files(self.files, False, shard, None)      # validates `shard`
        self.num_actions, self.num_locations = int(num_actions), int(num_locations)
        self.frames = int(frames_per_record)
        self.embedding = _embedding(embedding)
        self.correspondence = _correspondence(correspondence, self.embedding)
        frames = self.batch_size * (1 if self.embedding else self.frames)      # frames behind a full batch
        # rows of a full batch: its frames, or a whole pair batch where stage 2 does not re-batch
        self._rows = frames * (2 if self.correspondence and not self.shuffle else 1)
        self.verify = bool(compression_verify)
        self.device = torch.device(device)
        self.fe = FrontEnd(self.device)
        self.plan = ops.Plan(self.device, eager=True)
        self.stream = torch.cuda.Stream(device=self.device)
        self.data = self
        self.times = dict(inflate=0.0, index=0.0, decode=0.0, upload=0.0, wait=0.0)
        self._inflater = None
        if self.inflate == "device":
            from .inflate import DeviceInflater
            self._inflater = DeviceInflater(self.device)
            self.times["inflate_device"] = 0.0       # the consumer's seconds in the grouped device calls, copy back included
        # decode window: enough records in the workers' hands to cover a batch while the consumer is away
        self._window = max(self.workers + self.prefetch, -(-frames // self.frames) + self.workers)
        self._num_samples = None
        self._epoch = 0
        self._pass = 0            # the pass whose iterator may touch the pool
        self._exec = None
        self._dims = None
        self._pool, self._pool_pages = None, 0
        self._outs = None

    # ---- :117, :973-976 ---------------------------------------------------------------------------------------------
    @property
    def num_samples(self):
        """frames (embedding=0: clips) this loader yields per pass (its shard of the files), counted once from the
        decoded dimensions"""
        if self._num_samples is None:
            total = 0
            files = epoch_files(self.files, False, self.shard, None)
            for buf, offs, lens, _, _ in self._executor().map(lambda p: _inflate_file(p, False), files):
                if not self.embedding:
                    total += len(offs)
                    continue
                total += sum(int(_record_dims(buf, off, ln).video_steps) for off, ln in zip(offs, lens))
            self._num_samples = total
        return self._num_samples

    @property
    def total_batches(self):
        return -(-self.num_samples // self.batch_size)

    @property
    def num_rows(self):
        """rows (embedding=0: clips) of one pass: `num_samples`, twice that with correspondence=1"""
        return self.num_samples * (2 if self.correspondence else 1)

    @property
    def num_batches(self):
        """batches of one pass: stage 2 re-batches the doubled rows; without it the pair map doubles the rows of a batch"""
        if self.correspondence and self.shuffle:
            return -(-self.num_rows // self.batch_size)
        return self.total_batches

    def _executor(self):
        if self._exec is None:
            self._exec = concurrent.futures.ThreadPoolExecutor(max_workers=self.workers, thread_name_prefix="acimg-loader")
        return self._exec

    def close(self):
        """end the current pass and stop the worker threads"""
        self._pass += 1
        if self._exec is not None:
            self._exec.shutdown(wait=True)
            self._exec = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- device buffers -----------------------------------------------------------------------------------------------
    def _setup(self, dims):
        """pool, output ring, staging and slot buffers for records of these dimensions (known from the first record)"""
        ah, aw, ad, vh, vw, vd = dims
        if vd != 3:
            raise ValueError("video depth %d: the gather reverses three channels" % vd)
        self._dims = dims
        self.pixels, self.elems = vh * vw, ah * aw * ad
        self.vstride = -(-self.pixels * 3 // 16) * 16
        dev, bs = self.device, self._rows
        self._slot_rows = 8                      # slot lists in flight between the host and the gathers that read them
        with torch.cuda.stream(self.stream):     # every device buffer of the loader belongs to its stream
            self._outs = [(torch.empty(bs, ah, aw, ad, device=dev), torch.empty(bs, 12, device=dev),
                           torch.empty(bs, vh, vw, 3, device=dev), torch.empty(bs, self.num_actions, device=dev),
                           torch.empty(bs, self.num_locations, device=dev),
                           torch.empty(bs, 2 if self.correspondence else 12, device=dev))
                          for _ in range(self.ring)]
            self._slots_dev = torch.empty(self._slot_rows, bs, dtype=torch.int32, device=dev)
        self._staging = collections.deque(_Staging(self.frames, self.pixels * 3, self.elems)
                                          for _ in range(self._window + 2))
        self._slots_host = torch.empty(self._slot_rows, bs, dtype=torch.int32).pin_memory()
        self._slot_events = [None] * self._slot_rows
        self._slot_next = 0
        self._pool, self._pool_pages = None, 0

    def _alloc_pool(self, pages):
        """(re)allocate the pool at `pages` pages on the loader's stream, keeping the pages it holds"""
        n, dev = pages * self.frames, self.device
        with torch.cuda.stream(self.stream):
            new = dict(video=torch.empty(n, self.vstride, dtype=torch.uint8, device=dev),
                       acoustic=torch.empty(n, self.elems, device=dev),
                       audio=torch.empty(n, 1024, dtype=torch.int32, device=dev), low=torch.empty(n, 1024, device=dev),
                       mfcc=torch.empty(n, 12, device=dev), mfcc_low=torch.empty(n, 12, device=dev),
                       labels=torch.empty(n, 2, dtype=torch.int32, device=dev))
            if self._pool is not None:
                old = self._pool_pages * self.frames
                for k, t in new.items():
                    t[:old].copy_(self._pool[k])
            self._pool, self._pool_pages = new, pages

    # ---- one pass -------------------------------------------------------------------------------------------------------
    def _records(self, files, alive):
        """decoded records in file order: (staging set) per record; files are inflated `workers` ahead, records decoded
        `_window` ahead, each into a staging set taken - in record order - once its last upload has completed"""
        ex = self._executor()
        file_q, rec_q = collections.deque(), collections.deque()
        files = iter(files)
        state = dict(cur=None, files_done=False)

        read_q = collections.deque()             # the device path: files being read, ahead of the group being inflated

        def more_files(block=True, group=True):
            if self._inflater is not None:
                return more_files_device(block, group)
            while not state["files_done"] and len(file_q) < self.workers:
                p = next(files, None)
                if p is None:
                    state["files_done"] = True
                else:
                    file_q.append(ex.submit(_inflate_file, p, self.verify))

        def more_files_device(block, group):
            """reads run up to two groups ahead; when a file is wanted and no inflated one is left, the files of the
            look-ahead, up to `workers` of them, are inflated in ONE call on the loader's stream and handed back to the
            workers (not block: only if their reads have finished)"""
            while not state["files_done"] and len(read_q) + len(file_q) < 2 * self.workers:
                p = next(files, None)
                if p is None:
                    state["files_done"] = True
                else:
                    read_q.append((p, ex.submit(_read_file, p)))
            if not group or file_q or not read_q:
                return
            if not block and not all(f.done() for _, f in list(read_q)[:self.workers]):
                return
            group = [read_q.popleft() for _ in range(min(self.workers, len(read_q)))]
            t0 = time.perf_counter()
            read = [f.result() for _, f in group]
            self.times["wait"] += time.perf_counter() - t0
            self.times["inflate"] += sum(r[2] for r in read)
            t0 = time.perf_counter()
            with torch.cuda.stream(self.stream):
                got = self._inflater.gunzip_device([r[0] for r in read], [r[1] for r in read])
            self.times["inflate_device"] += time.perf_counter() - t0
            for (p, _), (raw, plan, _), (data, status, end_bits) in zip(group, read, got):
                file_q.append(ex.submit(_index_file, p, raw, plan, data, status, end_bits, self.verify))

        def more_records(block=True):
            while len(rec_q) < self._window:
                if state["cur"] is None:
                    more_files(block)
                    if not file_q or not (block or file_q[0].done()):
                        return
                    t0 = time.perf_counter()
                    buf, offs, lens, t_inf, t_idx = file_q.popleft().result()
                    self.times["wait"] += time.perf_counter() - t0
                    self.times["inflate"] += t_inf
                    self.times["index"] += t_idx
                    more_files(group=False)
                    state["cur"] = (buf, collections.deque(zip(offs, lens)))
                buf, todo = state["cur"]
                if not todo:
                    state["cur"] = None
                    continue
                off, ln = todo.popleft()
                if self._dims is None:           # the first record of the first pass sizes every buffer
                    d = _record_dims(buf, off, ln)
                    self._setup((int(d.audio_height), int(d.audio_width), int(d.audio_depth), int(d.video_height),
                                 int(d.video_width), int(d.video_depth)))
                st = (self._staging.popleft() if self._staging
                      else _Staging(self.frames, self.pixels * 3, self.elems))
                if st.event is not None:
                    st.event.synchronize()
                    st.event = None
                rec_q.append((st, ex.submit(_decode_record, buf, off, ln, st, self._dims)))

        self._more_records = more_records
        self._rec_q = rec_q
        try:
            while alive():
                more_records(block=not rec_q)
                if not rec_q:
                    return
                st, fut = rec_q.popleft()
                t0 = time.perf_counter()
                self.times["decode"] += fut.result()
                self.times["wait"] += time.perf_counter() - t0
                yield st
        finally:
            for fut in file_q:
                fut.cancel()
            for _, fut in read_q:
                fut.cancel()
            for st, fut in rec_q:
                fut.cancel()
            concurrent.futures.wait([f for f in file_q] + [f for _, f in read_q] + [f for _, f in rec_q])
            for st, _ in rec_q:
                self._staging.append(st)

    def _ready(self):
        self._more_records(block=False)
        return bool(self._rec_q) and self._rec_q[0][1].done()

    def _upload(self, page, st):
        t0 = time.perf_counter()
        n, lo = st.n, page * self.frames
        if not self.embedding and n != self.frames:
            raise ValueError("clip mode wants records of %d frames, got one of %d" % (self.frames, n))
        pool = self._pool
        with torch.cuda.stream(self.stream):
            pool["video"][lo:lo + n, :self.pixels * 3].copy_(st.video[:n], non_blocking=True)
            pool["acoustic"][lo:lo + n].copy_(st.acoustic[:n], non_blocking=True)
            pool["audio"][lo:lo + n].copy_(st.audio[:n], non_blocking=True)
            pool["labels"][lo:lo + n].copy_(st.labels[:n], non_blocking=True)
            st.event = torch.cuda.Event()
            st.event.record(self.stream)
            frames = pool["audio"][lo:lo + n]
            self.fe._build_spectrograms_function(frames, normalize=True, out=pool["mfcc"][lo:lo + n])
            low = self.fe.butter_lowpass_filter(frames, out=pool["low"][lo:lo + n])
            self.fe._build_spectrograms_function(low, normalize=True, out=pool["mfcc_low"][lo:lo + n])
        self._staging.append(st)
        self.times["upload"] += time.perf_counter() - t0
        return n

    def _gather(self, slots, offset, out, wait):
        """enqueue the gather of `slots` into rows offset.. of the output set `out`; the first gather into a set waits
        (on the GPU) for what its consumer had enqueued when the iterator was advanced"""
        from . import ops
        n, row = len(slots), self._slot_next
        self._slot_next = (row + 1) % self._slot_rows
        if self._slot_events[row] is not None:
            self._slot_events[row].synchronize()
        self._slots_host[row, :n] = torch.tensor(slots, dtype=torch.int32)
        pool = self._pool
        with torch.cuda.stream(self.stream):
            self._slots_dev[row, :n].copy_(self._slots_host[row, :n], non_blocking=True)
            ev = torch.cuda.Event()
            ev.record(self.stream)
            self._slot_events[row] = ev
            if wait is not None:
                self.stream.wait_event(wait)
            ac, mf, vid, act, loc, mfl = (t[offset:offset + n] for t in out)
            gather = ops.batch_gather_pairs if self.correspondence else ops.batch_gather      # mfl: then the pair rows
            gather(self.plan, pool["video"], self.vstride, pool["acoustic"], pool["mfcc"], pool["mfcc_low"], pool["labels"],
                   self._slots_dev[row], n, self.pixels, self.elems, vid, ac, mf, mfl, act, self.num_actions, loc,
                   self.num_locations)

    def __iter__(self):
        epoch, self._epoch = self._epoch, self._epoch + 1
        self._pass += 1
        me = self._pass
        rng = epoch_rng(self.seed, epoch)
        files = epoch_files(self.files, self.shuffle, self.shard, rng)
        rng2 = pair_rng(self.seed, epoch) if self.correspondence and self.shuffle else None
        return self._iterate(files, rng, me, rng2)

    def _iterate(self, files, rng, me, rng2=None):
        def alive():
            if self._pass != me:
                raise RuntimeError("DeviceDataLoader: this iterator was ended by a later pass over the same loader")
            return True

        records = self._records(files, alive)
        first = next(records, None)          # sizes the buffers on the first pass
        if first is None:
            return
        pairs = bool(self.correspondence)
        limit = (pair_pages(self.buffer_size, self.batch_size, self.prefetch) if pairs
                 else pool_pages(self.buffer_size, self.prefetch))
        # (a pool grown by an earlier pass is kept)
        pages = FramePages(min(limit, max(self.FIRST_PAGES, self._pool_pages)), limit, self.frames, uses=2 if pairs else 1)
        if self._pool_pages < pages.size:
            self._alloc_pool(pages.size)

        def chain():
            yield first
            for st in records:
                yield st

        state = dict(k=0, wait=None)

        def gather(slots, offset):
            self._gather(slots, offset, self._outs[state["k"] % self.ring], state["wait"])
            state["wait"] = None

        feeder = BatchFeeder(chain(), pages, self.batch_size, self.buffer_size, self.prefetch, rng, self._upload, gather,
                             grow=self._alloc_pool, ready=self._ready, units="frames" if self.embedding else "records",
                             pairs=pairs, rng2=rng2)
        try:
            for n in feeder:
                done = torch.cuda.Event()
                done.record(self.stream)
                cur = torch.cuda.current_stream(self.device)
                cur.wait_event(done)
                out = tuple(t[:n] for t in self._outs[state["k"] % self.ring])
                if not self.embedding:           # one label row per clip: the first of its 12 identical gathered rows
                    out = out[:3] + (out[3][::self.frames], out[4][::self.frames]) + out[5:]
                yield out
                alive()
                # the consumer may have enqueued reads of every batch yielded so far: the next gather into the set that
                # is `ring` batches old starts behind them
                cur = torch.cuda.current_stream(self.device)
                consumed = torch.cuda.Event()
                consumed.record(cur)
                state["k"] += 1
                state["wait"] = consumed
        finally:
            records.close()


def box_mfcc(audio):
    """float64 NumPy restatement of dataloader/frames.py `_build_spectrograms_function` (:659-688, with `createfilters`
    and `get_feats`) + `_normalize_mfcc` (:559-566) on the [rows, L] array the function evidently means: ONE
    un-windowed rfft over the whole clip, power of the first L // 2 bins, a mel bank built for fft_len = L // 2, the
    1e-3 floor, log, DCT, * mfnorm, * lifter, NaN / inf -> 0, float32; then per row (x - min) / max in float32.
    audio: int32 [rows, L] -> float32 [rows, 12].  (On the [1, 1, L] array the TF pipeline actually hands it the
    function degenerates to an audio-independent vector; DESIGN §8 records why that is not reproduced.)"""
    from .frontend import FILTER_NUM, HI_FREQ, LIFTER_NUM, LO_FREQ, MFCC_NUM, createfilters
    x = np.asarray(audio)
    if x.ndim != 2 or x.shape[1] < 4:
        raise ValueError("box_mfcc wants [rows, L >= 4] audio, got %s" % (x.shape,))
    length = x.shape[1]
    fft_len = length // 2
    power = np.abs(np.fft.rfft(x, length, axis=1))[:, :-1] ** 2
    power = power.reshape(x.shape[0], fft_len)
    dct_base = np.zeros((FILTER_NUM, MFCC_NUM))
    for m in range(MFCC_NUM):
        dct_base[:, m] = np.cos((m + 1) * np.pi / FILTER_NUM * (np.arange(FILTER_NUM) + 0.5))
    lifter = 1 + (LIFTER_NUM / 2) * np.sin(np.pi * (1 + np.arange(MFCC_NUM)) / LIFTER_NUM)
    mel = power.dot(createfilters(fft_len, FILTER_NUM, LO_FREQ, HI_FREQ, 2 * HI_FREQ))
    mel[mel < 0.001] = 0.001
    c = np.log(mel).dot(dct_base)
    c *= np.sqrt(2.0 / FILTER_NUM)
    c *= lifter
    c[~np.isfinite(c)] = 0
    c = c.astype(np.float32)
    c = c - c.min(axis=1, keepdims=True)
    return c / c.max(axis=1, keepdims=True)


class BoxRecordLoader(object):
    """`ActionsDataLoader(txt_file, 'testing', batch_size, ..., embedding=1, nr_frames=1, sample_length=1,
    shuffle=False)` of dataloader/frames.py with modalities [1, 2] (audio data + video; no acoustic image in these
    records, so the acoustic slot holds zeros as :316 builds them).  `files`: a list of TFRecord paths or the path of a
    text file listing them.  Everything runs on the host (the MFCC is one clip-length rfft per record, loader work like
    the per-frame maps of `TFRecordDataLoader`); tensors are returned on the host."""

    def __init__(self, files, batch_size, compression_verify=True):
        if isinstance(files, str):
            with open(files) as f:
                files = [ln.strip() for ln in f if ln.strip()]
        self.files = list(files)
        self.batch_size = int(batch_size)
        self.verify = bool(compression_verify)
        self.data = self
        self._num_samples = None

    @property
    def num_samples(self):
        """frames in the data set, counted from the decoded records (one frame per record in convert_data2.py files)"""
        if self._num_samples is None:
            from . import tfio
            self._num_samples = sum(int(tfio.decode_box_sequence_example_native(r)["dims"].video_steps)
                                    for p in self.files for r in tfio.read_tfrecord_native(p, verify=False) if len(r))
        return self._num_samples

    @property
    def total_batches(self):
        return -(-self.num_samples // self.batch_size)

    def _record(self, rec):
        from . import tfio
        d = tfio.decode_box_sequence_example_native(rec)
        boxes, vi, sa = d["boxes"], d["video_images"], d["audio_samples"]
        n = vi.shape[0]
        if not (boxes.shape[0] == n and sa.shape[0] == n and n > 0):
            raise ValueError("record with %d video frames, %d box rows, %d audio rows" % (n, boxes.shape[0], sa.shape[0]))
        mfcc = box_mfcc(sa)
        # video: float, channel order reversed, 1/255 (`_normalize_images_rescaled`, :640-646)
        v = vi[..., ::-1].astype(np.float32) * np.float32(1.0 / 255.0)
        out = [np.zeros((n, 36, 48, 12), np.float32), mfcc, np.ascontiguousarray(v)]
        out += [np.ascontiguousarray(boxes[:, k]) for k in range(4)] + [d["typescene"]]
        return tuple(torch.from_numpy(a) for a in out)

    def __iter__(self):
        from . import tfio
        pend, have = [], 0
        for path in self.files:
            for rec in tfio.read_tfrecord_native(path, verify=self.verify):
                if len(rec) == 0:
                    continue
                pend.append(self._record(rec))
                have += pend[-1][0].shape[0]
                while have >= self.batch_size:
                    cat = [torch.cat([p_[k] for p_ in pend], 0) for k in range(8)]
                    yield tuple(c[:self.batch_size] for c in cat)
                    rest = tuple(c[self.batch_size:] for c in cat)
                    have = rest[0].shape[0]
                    pend = [rest] if have else []
        if have:
            yield tuple(torch.cat([p_[k] for p_ in pend], 0) for k in range(8))


class ClassRecordLoader(object):
    """`ActionsDataLoader(txt_file, 'testing', batch_size, ..., embedding=1, nr_frames=1, sample_length=1, shuffle=False,
    modalities=[1, 2])` of dataloader/framesclass.py on the records `python -m acimg.convert_collected` writes (the
    two-object test set): a sibling of `BoxRecordLoader`, sharing `box_mfcc`.  Batches are (acoustic zeros [n,36,48,12]
    as :284 builds them, mfcc float32 [n,12], video float32 R G B / 255 [n,224,298,3], classnumber int32 [n,1]).  Records
    are parsed with `tfio.parse_sequence_example`; a frame that is not 224 x 298 x 3 is refused by name, because the
    reference's reshape (:333) fails there.  The reference's fifth output, the MFCC of the low-passed clip (:392-408), is
    NOT produced: `showimages_collected.py` never reads it.  `files`: a list of TFRecord paths or the path of a text
    file listing them.  Everything runs on the host; tensors are returned on the host."""

    FRAME = (224, 298, 3)

    def __init__(self, files, batch_size, compression_verify=True):
        if isinstance(files, str):
            with open(files) as f:
                files = [ln.strip() for ln in f if ln.strip()]
        self.files = list(files)
        self.batch_size = int(batch_size)
        self.verify = bool(compression_verify)
        self.data = self
        self._num_samples = None

    @property
    def num_samples(self):
        """frames in the data set (one per record in convert_collected's files)"""
        if self._num_samples is None:
            from . import tfio
            self._num_samples = sum(len(tfio.parse_sequence_example(r)[1].get("video/image", ()))
                                    for p in self.files for r in tfio.read_tfrecord_native(p, verify=False) if len(r))
        return self._num_samples

    @property
    def total_batches(self):
        return -(-self.num_samples // self.batch_size)

    def _record(self, rec, path):
        from . import tfio
        ctx, lists = tfio.parse_sequence_example(rec)
        for key in ("audio_data/mics", "audio_data/samples", "classnumber", "video/height", "video/width", "video/depth"):
            if key not in ctx:
                raise ValueError("%s: a record without the context feature %r" % (path, key))
        for key in ("audio/data", "video/image"):
            if key not in lists:
                raise ValueError("%s: a record without the feature list %r" % (path, key))
        shape = tuple(int(np.asarray(ctx[k]).reshape(-1)[0]) for k in ("video/height", "video/width", "video/depth"))
        if shape != self.FRAME:
            raise ValueError("%s: a frame of %d x %d x %d: only 224 x 298 x 3 frames are loaded" % ((path,) + shape))
        samples = int(np.asarray(ctx["audio_data/samples"]).reshape(-1)[0])
        sa = np.frombuffer(b"".join(v for step in lists["audio/data"] for v in step), "<i4").reshape(-1, samples)
        vi = np.frombuffer(b"".join(v for step in lists["video/image"] for v in step), np.uint8).reshape((-1,) + self.FRAME)
        n = vi.shape[0]
        if not (sa.shape[0] == n and n > 0):
            raise ValueError("%s: a record with %d video frames and %d audio rows" % (path, n, sa.shape[0]))
        # video: float, channel order reversed, 1/255 (`_normalize_images_rescaled`)
        v = vi[..., ::-1].astype(np.float32) * np.float32(1.0 / 255.0)
        label = np.full((n, 1), int(np.asarray(ctx["classnumber"]).reshape(-1)[0]), np.int32)
        out = [np.zeros((n, 36, 48, 12), np.float32), box_mfcc(sa), np.ascontiguousarray(v), label]
        return tuple(torch.from_numpy(a) for a in out)

    def __iter__(self):
        from . import tfio
        pend, have = [], 0
        for path in self.files:
            for rec in tfio.read_tfrecord_native(path, verify=self.verify):
                if len(rec) == 0:
                    continue
                pend.append(self._record(rec, path))
                have += pend[-1][0].shape[0]
                while have >= self.batch_size:
                    cat = [torch.cat([p_[k] for p_ in pend], 0) for k in range(4)]
                    yield tuple(c[:self.batch_size] for c in cat)
                    rest = tuple(c[self.batch_size:] for c in cat)
                    have = rest[0].shape[0]
                    pend = [rest] if have else []
        if have:
            yield tuple(torch.cat([p_[k] for p_ in pend], 0) for k in range(4))
