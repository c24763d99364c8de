"""What the converter tests measure against, written independently of csrc/resize_cubic.* and acimg/convert.py:

* the NumPy restatement of OpenCV's scalar fixed-point `cv2.resize(..., INTER_CUBIC)` for 8-bit frames (tap tables in
  float32 -> int16, the horizontal then the vertical int32 pass, (v + 2^21) >> 22, clamp) - DESIGN section 8;
* the fp64 cubic convolution (a = -0.75) it is held against;
* writers of the fixture files: 24-bit BMP (and headers of the kinds that are refused), PCM WAV, a raw recording tree."""
import os
import struct

import numpy as np

CROP_H, CROP_W = 224, 298


# ---- the restatement ------------------------------------------------------------------------------------------------------
def cubic_tables(n_in, n_out, first=0, count=None):
    """(idx int32 [count,4], coef int16 [count,4]) of output coordinates first .. first + count - 1"""
    count = n_out - first if count is None else count
    f32 = np.float32
    scale = 1.0 / (float(n_out) / float(n_in))                               # fp64, as cv::resize forms it
    d = np.arange(first, first + count, dtype=np.float64)
    f = ((d + 0.5) * scale - 0.5).astype(f32)
    s = np.floor(f)
    f = (f - s).astype(f32)
    A, one = f32(-0.75), f32(1)
    x = f + one
    c0 = ((A * x - f32(5) * A) * x + f32(8) * A) * x - f32(4) * A
    c1 = ((A + f32(2)) * f - (A + f32(3))) * f * f + one
    y = one - f
    c2 = ((A + f32(2)) * y - (A + f32(3))) * y * y + one
    c3 = one - c0 - c1 - c2
    c = np.stack([c0, c1, c2, c3], 1)
    assert c.dtype == np.float32
    coef = np.clip(np.rint(c * f32(2048)), -32768, 32767).astype(np.int16)   # rint: half to even
    idx = np.clip(s.astype(np.int64)[:, None] - 1 + np.arange(4)[None, :], 0, n_in - 1).astype(np.int32)
    return idx, coef


def resize_with_tables(frame, idx_y, coef_y, idx_x, coef_x):
    """uint8 [H,W,C] -> uint8 [len(idx_y), len(idx_x), C]"""
    src = np.asarray(frame).astype(np.int64)
    h = np.zeros((src.shape[0], idx_x.shape[0], src.shape[2]), np.int64)
    for k in range(4):
        h += src[:, idx_x[:, k], :] * coef_x[:, k].astype(np.int64)[None, :, None]
    v = np.zeros((idx_y.shape[0],) + h.shape[1:], np.int64)
    for k in range(4):
        v += h[idx_y[:, k]] * coef_y[:, k].astype(np.int64)[:, None, None]
    assert np.abs(h).max() < 2 ** 31 and np.abs(v).max() < 2 ** 31 - 2 ** 21     # the int32 of the definition holds them
    return np.clip((v + (1 << 21)) >> 22, 0, 255).astype(np.uint8)


def resize_cubic(frame, new_h, new_w, window=None):
    """cv2.resize(frame, (new_w, new_h), interpolation=cv2.INTER_CUBIC)[y0:y0 + oh, x0:x0 + ow]; window = (y0, x0, oh, ow)"""
    H, W = frame.shape[:2]
    y0, x0, oh, ow = window if window is not None else (0, 0, new_h, new_w)
    return resize_with_tables(frame, *(cubic_tables(H, new_h, y0, oh) + cubic_tables(W, new_w, x0, ow)))


def smallest_size_at_least(height, width, side=224):
    scale = float(side) / float(width) if height > width else float(side) / float(height)
    return int(float(height) * scale), int(float(width) * scale)


def convert_frame(frame):
    """`_read_video_frame` of convert_data.py after the imread: resize to smallest side 224, central 224 x 298 crop"""
    nh, nw = smallest_size_at_least(frame.shape[0], frame.shape[1])
    return resize_cubic(frame, nh, nw, ((nh - CROP_H) // 2, (nw - CROP_W) // 2, CROP_H, CROP_W))


# ---- the yardstick: cubic convolution in fp64 -------------------------------------------------------------------------
def cubic_weights_f64(f, a=-0.75):
    f = np.asarray(f, np.float64)

    def near(t):      # |t| <= 1
        return ((a + 2) * t - (a + 3)) * t * t + 1

    def far(t):       # 1 < |t| < 2
        return ((a * t - 5 * a) * t + 8 * a) * t - 4 * a
    return np.stack([far(f + 1), near(f), near(1 - f), far(2 - f)], 1)


def resize_cubic_f64(frame, new_h, new_w):
    """the same sampling positions and border rule in fp64, no rounding, clipped to [0, 255]"""
    def axis(n_in, n_out):
        pos = (np.arange(n_out) + 0.5) * (float(n_in) / n_out) - 0.5
        s = np.floor(pos)
        return (np.clip(s.astype(np.int64)[:, None] - 1 + np.arange(4)[None, :], 0, n_in - 1), cubic_weights_f64(pos - s))
    src = np.asarray(frame, np.float64)
    iy, wy = axis(src.shape[0], new_h)
    ix, wx = axis(src.shape[1], new_w)
    h = sum(src[:, ix[:, k], :] * wx[:, k][None, :, None] for k in range(4))
    v = sum(h[iy[:, k]] * wy[:, k][:, None, None] for k in range(4))
    return np.clip(v, 0.0, 255.0)


# ---- fixture files ----------------------------------------------------------------------------------------------------------
def bmp_bytes(bgr, bottom_up=True, bpp=24, compression=0, offset=54):
    """a BMP file holding uint8 [H,W,3] `bgr`; bpp / compression other than 24 / 0 give a header of that kind over the
    same body (for the refusals)"""
    H, W = bgr.shape[:2]
    pitch = (3 * W + 3) // 4 * 4
    rows = np.zeros((H, pitch), np.uint8)
    rows[:, :3 * W] = np.asarray(bgr, np.uint8).reshape(H, 3 * W)
    body = (rows[::-1] if bottom_up else rows).tobytes()
    head = b"BM" + struct.pack("<IHHI", offset + len(body), 0, 0, offset)
    head += struct.pack("<IiiHHIIiiII", 40, W, H if bottom_up else -H, 1, bpp, compression, len(body), 2835, 2835, 0, 0)
    return head + b"\0" * (offset - 54) + body


def wav_bytes(samples, rate=12288, bits=16, channels=1):
    """a PCM RIFF/WAVE file of `samples` (interleaved if channels > 1)"""
    dt = {8: "u1", 16: "<i2", 32: "<i4"}[bits]
    body = np.asarray(samples).astype(dt).tobytes()
    block = channels * bits // 8
    fmt = struct.pack("<HHIIHH", 1, channels, rate, rate * block, block, bits)
    return (b"RIFF" + struct.pack("<I", 4 + 8 + len(fmt) + 8 + len(body)) + b"WAVE" + b"fmt " + struct.pack("<I", len(fmt))
            + fmt + b"data" + struct.pack("<I", len(body)) + body)


def write_recording(root, cls, loc, video_time, frames, samples, bits=16, rate=12288, bottom_up=True, time_text=None):
    """ROOT/class_<cls>/data_<loc:03d>/{video_time.txt, video/I_%06d.bmp, audio/output_audio2.wav} -> its directory;
    frames: uint8 [n,H,W,3] (BGR, as stored), samples: the WAV's samples"""
    d = os.path.join(str(root), "class_%d" % cls, "data_%03d" % loc)
    os.makedirs(os.path.join(d, "video"))
    os.makedirs(os.path.join(d, "audio"))
    with open(os.path.join(d, "video_time.txt"), "w") as f:
        f.write(time_text if time_text is not None else "video_time: %d\nframes: %d\n" % (video_time, len(frames)))
    for i, fr in enumerate(frames):
        with open(os.path.join(d, "video", "I_%06d.bmp" % (i + 1)), "wb") as f:
            f.write(bmp_bytes(fr, bottom_up=bottom_up))
    with open(os.path.join(d, "audio", "output_audio2.wav"), "wb") as f:
        f.write(wav_bytes(samples, rate=rate, bits=bits))
    return d
