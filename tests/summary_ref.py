"""NumPy restatements of the two summary rules include/acimg.h states (TF 1.x's, from its documented behaviour; there is
no TensorFlow here to pin them against) and of the histogram compression of acimg/events.py."""
import sys

import numpy as np

DBL_MAX = sys.float_info.max


def normalize_image(s):
    """tf.summary.image on one float [H,W,3] slice, in np.float32 arithmetic: min / max over the finite values; negative
    minimum -> scale 127 / max(|min|, |max|) and offset 128, else scale 255 / max and offset 0 (scale 0 below 1e-6);
    a pixel with a non-finite channel -> (255, 0, 0); every other value -> uint8(trunc(v * scale + offset)), the product
    rounded to fp32 before the sum"""
    s = np.asarray(s, np.float32)
    assert s.ndim == 3 and s.shape[2] == 3
    fin = np.isfinite(s)
    image_min = np.float32(s[fin].min()) if fin.any() else np.float32(np.inf)
    image_max = np.float32(s[fin].max()) if fin.any() else np.float32(-np.inf)
    eps = np.float32(1e-6)
    with np.errstate(all="ignore"):
        if image_min < 0:
            m = np.maximum(np.abs(image_min), np.abs(image_max))
            scale = np.float32(0) if m < eps else np.float32(127) / m
            offset = np.float32(128)
        else:
            scale = np.float32(0) if image_max < eps else np.float32(255) / image_max
            offset = np.float32(0)
        scale = np.float32(scale)
        prod = (np.where(fin, s, np.float32(0)) * scale).astype(np.float32)
        val = (prod + offset).astype(np.float32)
    out = np.clip(np.trunc(val), 0, 255).astype(np.uint8)
    bad = ~fin.all(axis=2)
    out[bad] = (255, 0, 0)
    return out


def summary_images(x, c0, G, n_images):
    """x [N,H,W,ldc] float32 -> uint8 [n_images,G,H,W,3]"""
    x = np.asarray(x, np.float32)
    return np.stack([np.stack([normalize_image(x[n, :, :, c0 + 3 * g:c0 + 3 * g + 3]) for g in range(G)])
                     for n in range(n_images)])


def histogram(values, limits):
    """values: the counted fp32 values (any shape) -> (counts int64 [L], dict(min, max, num, sum, sum_squares),
    nonfinite): bucket = searchsorted(limits, float64(v), 'right'), non-finite values left out, fp64 statistics"""
    v = np.asarray(values, np.float32).reshape(-1)
    fin = np.isfinite(v)
    d = v[fin].astype(np.float64)
    limits = np.asarray(limits, np.float64)
    b = np.minimum(np.searchsorted(limits, d, side="right"), len(limits) - 1)
    counts = np.bincount(b, minlength=len(limits)).astype(np.int64)
    stats = dict(min=float(d.min()) if d.size else float("inf"), max=float(d.max()) if d.size else float("-inf"),
                 num=float(d.size), sum=float(d.sum()), sum_squares=float((d * d).sum()))
    return counts, stats, int((~fin).sum())


def compress(counts, limits):
    """TF's EncodeToProto, written from its description: emitted entries are every non-empty bucket, and - for every
    maximal run of empty buckets - one entry with the run's LAST limit and count 0; nothing at all -> (DBL_MAX, 0)"""
    counts = [float(c) for c in counts]
    out = []
    run_end = None
    for c, lim in zip(counts, limits):
        if c > 0:
            if run_end is not None:
                out.append((run_end, 0.0))
                run_end = None
            out.append((float(lim), c))
        else:
            run_end = float(lim)
    if run_end is not None:
        out.append((run_end, 0.0))
    if not out:
        out = [(DBL_MAX, 0.0)]
    return [a for a, _ in out], [b for _, b in out]
