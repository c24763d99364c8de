"""NumPy restatement of the correspondence pairs (`--correspondence 1`; dataloader/outdoor_data_mfcc.py:102-113, 888-928)
for the tests of `acimg_batch_gather_pairs` and of the loaders' `correspondence=1`, written from the semantics alone:

* the pair map works from the plain 6-tuples of a pass (acoustic, mfcc, video, action, location, mfcc_low): concatenate
  every tensor with itself, except that the second half of the acoustic images is the low-passed MFCC row tiled over
  the pixels (not normalised) and the second half of the MFCC rows is that row; the sixth tensor becomes the one-hot
  label, [0, 1] for the first (real) half and [1, 0] for the second (silent) half;
* the order: frames -> shuffle buffer -> batches -> pair map -> (a shuffling loader only) rows -> second shuffle
  buffer -> batches.  The shuffle buffer here is a list-based one of its own, independent of `acimg.data`.

Row codes, as the C ABI defines them: code >= 0 is the real row of frame (slot) code, code < 0 the silent row of ~code."""
import numpy as np


def buffer_order(items, B, rng):
    """tf.data's shuffle buffer over a list: fill to B, emit a uniformly drawn occupied position, refill it with the next
    item, and close the hole with the last entry once the items are used up"""
    todo = list(items)
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


def cut(items, size):
    """consecutive batches of `size`, the last one possibly short"""
    return [items[i:i + size] for i in range(0, len(items), size)]


def pair_code_batches(n_frames, batch, B, rng1, rng2=None):
    """the batches of one pass as lists of row codes in frame numbering.  rng2 None (a loader that does not shuffle): the
    pair batches themselves; else their rows, in order, through the second buffer, in batches of `batch` rows"""
    pairs = [b + [-f - 1 for f in b] for b in cut(buffer_order(range(n_frames), B, rng1), batch)]
    if rng2 is None:
        return pairs
    return cut(buffer_order([c for b in pairs for c in b], B, rng2), batch)


def pair_map(batch):
    """one plain batch (six arrays, n rows each) -> the pair batch of 2n rows"""
    ac, mfcc, video, action, location, low = [np.asarray(t) for t in batch]
    n = ac.shape[0]
    pixels = int(np.prod(ac.shape[1:])) // 12
    silent = np.tile(low.reshape(n, 1, 12), (1, pixels, 1)).reshape(ac.shape)
    label = np.zeros((2 * n, 2), np.float32)
    label[:n, 1] = 1.0
    label[n:, 0] = 1.0
    return (np.concatenate([ac, silent]), np.concatenate([mfcc, low]), np.concatenate([video, video]),
            np.concatenate([action, action]), np.concatenate([location, location]), label)


def rows_of(frames, codes):
    """the rows `codes` (frame numbering) of a pass whose plain frames are `frames` (six arrays, one row per frame): the
    pair map over ALL frames, then real row f is row f and silent row f is row n + f"""
    full = pair_map(frames)
    n = np.asarray(frames[0]).shape[0]
    idx = np.array([c if c >= 0 else n + (-c - 1) for c in codes], np.int64)
    return tuple(t[idx] for t in full)
