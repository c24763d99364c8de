"""NumPy restatement of the overlay rule of `acimg_overlay_render` (include/acimg.h) for the visualisation tests: grey of
the frame in float32 with every product and sum rounded on its own, the 3-pixel box outlines painted as 1, the energy map
resized to the frame in float64 (`localize_ref.linear_coefs`: cv2.resize's INTER_LINEAR), each layer autoscaled, indexed
as matplotlib indexes a colormap (trunc(t * 256), 256 -> 255, a flat layer -> 0) and blended in integer arithmetic."""
import struct
import zlib

import numpy as np

from localize_ref import FRAME_H, FRAME_W, linear_coefs


def grey(frame):
    """[224,298,>=3] -> float32 [224,298]: (F0 * 0.114 + F1 * 0.587) + F2 * 0.299, float32 throughout"""
    f = np.asarray(frame, dtype=np.float32)
    a = f[..., 0] * np.float32(0.114)
    b = f[..., 1] * np.float32(0.587)
    c = f[..., 2] * np.float32(0.299)
    return ((a + b).astype(np.float32) + c).astype(np.float32)


def outline_mask(boxes):
    """boxes [4,3] = xmin, xmax, ymin, ymax of three annotators -> bool [224,298]: the pixels the outlines cover"""
    b = np.asarray(boxes).reshape(4, 3)
    y, x = np.mgrid[0:FRAME_H, 0:FRAME_W]
    m = np.zeros((FRAME_H, FRAME_W), bool)
    for k in range(3):
        if b[1, k] == 0:
            continue
        x0, x1 = sorted((int(b[0, k]), int(b[1, k])))
        y0, y1 = sorted((int(b[2, k]), int(b[3, k])))
        outer = (x >= x0 - 1) & (x <= x1 + 1) & (y >= y0 - 1) & (y <= y1 + 1)
        inner = (x >= x0 + 2) & (x <= x1 - 2) & (y >= y0 + 2) & (y <= y1 - 2)
        m |= outer & ~inner
    return m


def resize_map(energy):
    """cv2.resize(map, (298, 224)) of a [36,48] map promoted to float64 -> float64 [224,298]"""
    sx, sx1, wx0, wx1 = linear_coefs(48, FRAME_W)
    sy, sy1, wy0, wy1 = linear_coefs(36, FRAME_H)
    m = np.asarray(energy, dtype=np.float32).reshape(36, 48).astype(np.float64)
    h = wx0.astype(np.float64)[None, :] * m[:, sx] + wx1.astype(np.float64)[None, :] * m[:, sx1]
    return wy0.astype(np.float64)[:, None] * h[sy, :] + wy1.astype(np.float64)[:, None] * h[sy1, :]


def lut_index(a):
    """table index of every value of `a` (float32 or float64, arithmetic in that type) over the array's own range"""
    a = np.asarray(a)
    assert a.dtype in (np.float32, np.float64)
    lo, hi = a.min(), a.max()
    if hi == lo:
        return np.zeros(a.shape, np.int64)
    t = (a - lo) / (hi - lo)
    s = t * a.dtype.type(256)
    i = np.trunc(s).astype(np.int64)
    i[s == 256] = 255
    return np.clip(i, 0, 255)


def colorize(a, table):
    """table[lut_index(a)]: what `cmap(Normalize()(a), bytes=True)[..., :3]` gives for a float32 / float64 image"""
    return np.asarray(table, np.uint8)[lut_index(a)]


def blend(base_rgb, over_rgb, alpha=(7, 10)):
    num, den = int(alpha[0]), int(alpha[1])
    b, o = base_rgb.astype(np.int64), over_rgb.astype(np.int64)
    return ((num * o + (den - num) * b + den // 2) // den).astype(np.uint8)


def render(frame, energy, lut_base, lut_over, boxes=None, alpha=(7, 10)):
    """one sample: frame [224,298,>=3] float32, energy [36,48] float32, two [256,3] uint8 tables -> uint8 [224,298,3]"""
    g = grey(frame)
    if boxes is not None:
        g[outline_mask(boxes)] = np.float32(1.0)
    v = resize_map(energy)
    return blend(colorize(g, lut_base), colorize(v, lut_over), alpha)


def read_png(data):
    """a reader for what write_png promises: signature, chunk CRCs, IHDR 8-bit RGB, one IDAT, filter 0 on every line"""
    assert data[:8] == b"\x89PNG\r\n\x1a\n"
    pos, chunks = 8, []
    while pos < len(data):
        n, kind = struct.unpack(">I4s", data[pos:pos + 8])
        body = data[pos + 8:pos + 8 + n]
        (crc,) = struct.unpack(">I", data[pos + 8 + n:pos + 12 + n])
        assert crc == zlib.crc32(kind + body) & 0xFFFFFFFF, kind
        chunks.append((kind, body))
        pos += 12 + n
    assert pos == len(data)
    assert [k for k, _ in chunks] == [b"IHDR", b"IDAT", b"IEND"] and chunks[2][1] == b""
    w, h, depth, ctype, comp, flt, lace = struct.unpack(">IIBBBBB", chunks[0][1])
    assert (depth, ctype, comp, flt, lace) == (8, 2, 0, 0, 0)
    raw = zlib.decompress(chunks[1][1])
    assert len(raw) == h * (1 + 3 * w)
    rows = np.frombuffer(raw, np.uint8).reshape(h, 1 + 3 * w)
    assert not rows[:, 0].any()
    return rows[:, 1:].reshape(h, w, 3)
