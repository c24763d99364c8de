"""NumPy restatement of the Flickr-SoundNet box metric (showimages_bb.py:286-320) for the localisation tests: the
mean-threshold mask of a [36,48] energy map, cv2.resize(m2 * 1.0, (298, 224)) with INTER_LINEAR on a float64 image
(half-pixel mapping, float32 weights clamped at the borders, float64 products and sums), > 0.5, and the weighted IoU
against the consensus of up to three annotators' boxes (0.5 per filled rectangle, capped at 1)."""
import numpy as np

FRAME_H, FRAME_W = 224, 298


def linear_coefs(n_in, n_out):
    """source index s, s1 and float32 weights (w0, w1) of every output coordinate"""
    scale = 1.0 / (float(n_out) / n_in)
    d = np.arange(n_out, dtype=np.float64)
    f = ((d + 0.5) * scale - 0.5).astype(np.float32)
    s = np.floor(f).astype(np.int64)
    f = (f - s.astype(np.float32)).astype(np.float32)
    lo, hi = s < 0, s >= n_in - 1
    s[lo], f[lo] = 0, 0
    s[hi], f[hi] = n_in - 1, 0
    s1 = np.minimum(s + 1, n_in - 1)
    return s, s1, (np.float32(1) - f).astype(np.float32), f


def energy_mask(energy):
    """map > mean(map) on a float32 map (mean in float64, like acimg_mask_iou)"""
    e = np.asarray(energy, dtype=np.float32).reshape(36, 48)
    return (e.astype(np.float64) > e.astype(np.float64).mean()).astype(np.float64)


def resize_mask(m):
    """cv2.resize(m * 1.0, (298, 224)) > 0.5 for a [36,48] 0/1 array -> bool [224,298]"""
    sx, sx1, wx0, wx1 = linear_coefs(48, FRAME_W)
    sy, sy1, wy0, wy1 = linear_coefs(36, FRAME_H)
    m = np.asarray(m, dtype=np.float64)
    h = wx0.astype(np.float64)[None, :] * m[:, sx] + wx1.astype(np.float64)[None, :] * m[:, sx1]
    v = wy0.astype(np.float64)[:, None] * h[sy, :] + wy1.astype(np.float64)[:, None] * h[sy1, :]
    return v > 0.5


def consensus(boxes):
    """boxes [4,3] = xmin, xmax, ymin, ymax of three annotators -> mtot [224,298] in {0, 0.5, 1}"""
    b = np.asarray(boxes).reshape(4, 3)
    m = np.zeros((3, FRAME_H, FRAME_W), np.float32)
    for k in range(3):
        if b[1, k] == 0:
            continue
        x0, x1 = sorted((int(b[0, k]), int(b[1, k])))
        y0, y1 = sorted((int(b[2, k]), int(b[3, k])))
        x0, y0, x1, y1 = max(x0, 0), max(y0, 0), min(x1, FRAME_W - 1), min(y1, FRAME_H - 1)
        if x0 <= x1 and y0 <= y1:
            m[k, y0:y1 + 1, x0:x1 + 1] = 0.5
    mtot = m.sum(0)
    mtot[mtot > 1.0] = 1.0
    return mtot


def score(m2, boxes):
    """(numerator, denominator, iou) of showimages_bb.py:311-320 for a resized bool mask and one box record; numerator
    and denominator in half-units (integers)"""
    mtot = consensus(boxes)
    m2 = np.asarray(m2, dtype=np.float64)
    intersection = np.logical_and(mtot, m2) * mtot
    union = np.logical_or(mtot, m2)
    box = 1 * (mtot > 0)
    unionbig = union + (mtot - box)
    num, den = float(np.sum(intersection)), float(np.sum(unionbig))
    with np.errstate(invalid="ignore", divide="ignore"):
        iou = np.float64(num) / np.float64(den)
    return int(round(2 * num)), int(round(2 * den)), float(iou)


def box_iou(energy, boxes):
    """the whole metric of one sample: energy [36,48] float32, boxes [4,3] -> (num, den, iou, resized mask)"""
    m2 = resize_mask(energy_mask(energy))
    num, den, iou = score(m2, boxes)
    return num, den, iou, m2


def boxes_of(*quads):
    """(xmin, xmax, ymin, ymax) per annotator -> [4,3] int32"""
    b = np.zeros((4, 3), np.int32)
    for k, q in enumerate(quads):
        b[:, k] = q
    return b


def random_boxes(rng, N):
    """[N,4,3] int32 boxes that reach past the frame, some with reversed corners, some annotators absent"""
    b = rng.randint(-30, 330, size=(N, 4, 3)).astype(np.int32)
    b[:, 2:] = rng.randint(-30, 250, size=(N, 2, 3))
    rev = rng.rand(N, 3) < 0.2                           # reversed corners
    b[:, 0][rev], b[:, 1][rev] = b[:, 1][rev], b[:, 0][rev].copy()
    off = rng.rand(N, 3) < 0.25
    b[:, 1][off] = 0                                     # xmax == 0: that annotator is absent
    return b
