#!/usr/bin/env python3
"""Writes tests/golden/jpeg_decode_golden.npz: baseline JPEG files encoded by Pillow and what Pillow (libjpeg-turbo) decodes
them to - the yardstick of the device decoder (csrc/jpeg_decode.hip) and of its restatement (tests/jpeg_decode_ref.py).
Data only: `names`, and per name `jpeg_<name>` (the file's bytes) and `pixels_<name>` (uint8 [3][H][W]: the R, G and B
planes, which deflate better than interleaved pixels; [H][W] for greyscale).  Run on a CPU machine that has Pillow; no
test imports Pillow.  The asserts below state what the fixture must hold, so that a change of the cases or of the encoder
cannot leave a softer fixture behind unnoticed.  (37 x 53 pixels at 4:2:0 are 3 x 4 MCUs, so an interval of 3 MCUs gives
four full intervals; the short last interval is the case with an interval of 5.)

    python tests/golden/make_jpeg_decode_golden.py
"""
import io
import os
import struct
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "jpeg_decode_golden.npz")
MAX_BYTES = 200 * 1000


def smooth(h, w, seed, lo=0.02, hi=0.09):
    rng = np.random.RandomState(seed)
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    img = np.zeros((h, w, 3))
    for c in range(3):
        a, b, p, q = rng.uniform(lo, hi, 4)
        img[..., c] = 128 + 70 * np.sin(a * x + p * 20) * np.cos(b * y + q * 20) + 50 * np.sin(0.013 * (x + y) * (c + 1))
    return np.clip(np.rint(img), 0, 255).astype(np.uint8)


def noise(h, w, seed):
    return np.random.RandomState(seed).randint(0, 256, size=(h, w, 3)).astype(np.uint8)


def harsh(h, w, seed):
    """noise of 0 and 255 only: what a coarse quantiser throws past both ends of the range"""
    return (np.random.RandomState(seed).randint(0, 2, size=(h, w, 3)) * 255).astype(np.uint8)


def segments(data):
    """[(marker, payload)] of the header up to and including SOS, and the offset of the scan"""
    out, pos = [], 2
    while True:
        marker, length = data[pos + 1], struct.unpack_from(">H", data, pos + 2)[0]
        out.append((marker, data[pos + 4:pos + 2 + length]))
        pos += 2 + length
        if marker == 0xDA:
            return out, pos


def facts(data):
    segs, scan = segments(data)
    sof = [p for m, p in segs if m == 0xC0]
    assert len(sof) == 1, "baseline (SOF0) only"
    comps = sof[0][5]
    sampling = (sof[0][7] >> 4, sof[0][7] & 15) if comps == 3 else (0, 0)
    dri = [struct.unpack(">H", p)[0] for m, p in segs if m == 0xDD]
    body = np.frombuffer(data[scan:-2], np.uint8)
    ff = np.flatnonzero(body[:-1] == 0xFF)
    nxt = body[ff + 1]
    dht = b"".join(p for m, p in segs if m == 0xC4)
    return dict(comps=comps, sampling=sampling, restart=dri[0] if dri else 0, stuffed=int((nxt == 0).sum()),
                markers=[int(v) for v in nxt[(nxt >= 0xD0) & (nxt <= 0xD7)]], dht=dht)


def main():
    from PIL import Image
    cases = []

    def add(name, img, **kw):
        buf = io.BytesIO()
        Image.fromarray(img).save(buf, "JPEG", **kw)
        data = buf.getvalue()
        px = np.asarray(Image.open(io.BytesIO(data)))
        assert px.shape == img.shape and px.dtype == np.uint8
        cases.append((name, data, px, facts(data)))
        return cases[-1]

    for sub, tag in ((0, "444"), (1, "422"), (2, "420")):
        for (w, h) in ((1, 1), (17, 9), (16, 16)):
            add("smooth_%s_%dx%d" % (tag, w, h), smooth(h, w, 3 + sub), quality=90, subsampling=sub)
            add("noise_%s_%dx%d" % (tag, w, h), noise(h, w, 7 + sub), quality=75, subsampling=sub)
    add("grey_17x9", smooth(9, 17, 1)[..., 0], quality=85)
    add("grey_noise_37x53", noise(53, 37, 2)[..., 0], quality=60)
    add("optimize_420_37x53", noise(53, 37, 3), quality=80, subsampling=2, optimize=True)
    add("noise_420_37x53", noise(53, 37, 11), quality=95, subsampling=2)
    add("smooth_420_37x53", smooth(53, 37, 12), quality=30, subsampling=2)
    add("q5_noise_420_40x72", harsh(72, 40, 4), quality=5, subsampling=2)
    add("q5_noise_444_17x9", harsh(9, 17, 5), quality=5, subsampling=0)
    add("q100_noise_422_37x53", noise(53, 37, 6), quality=100, subsampling=1)
    add("restart3_420_37x53", noise(53, 37, 8), quality=70, subsampling=2, restart_marker_blocks=3)
    add("restart5_420_37x53", noise(53, 37, 8), quality=70, subsampling=2, restart_marker_blocks=5)
    add("restart1_420_40x72", smooth(72, 40, 9), quality=92, subsampling=2, restart_marker_blocks=1)
    add("smooth_420_256x256", smooth(256, 256, 10, 0.01, 0.03), quality=90, subsampling=2)

    by = {c[0]: c for c in cases}
    f = {name: c[3] for name, c in by.items()}
    # what the fixture must hold
    assert {c[3]["sampling"] for c in cases} >= {(1, 1), (2, 1), (2, 2)} and any(c[3]["comps"] == 1 for c in cases)
    standard = f["smooth_420_16x16"]["dht"]
    assert f["optimize_420_37x53"]["dht"] != standard and f["noise_420_16x16"]["dht"] == standard, "own Huffman tables"
    for name in ("q5_noise_420_40x72", "q5_noise_444_17x9"):
        px = by[name][2]
        assert px.min() == 0 and px.max() == 255, "%s: both clamps (%d..%d)" % (name, px.min(), px.max())
    r3 = f["restart3_420_37x53"]            # 3 x 4 MCUs of 16 x 16: intervals of 3, 3, 3, 3 MCUs
    assert r3["sampling"] == (2, 2) and r3["restart"] == 3 and r3["markers"] == [0xD0, 0xD1, 0xD2]
    r5 = f["restart5_420_37x53"]            # 12 MCUs in intervals of 5, 5 and 2: the last one is short
    assert r5["restart"] == 5 and r5["markers"] == [0xD0, 0xD1]
    r1 = f["restart1_420_40x72"]            # 3 x 5 MCUs, one each: 15 intervals, the markers wrap past RST7
    assert r1["sampling"] == (2, 2) and r1["restart"] == 1 and r1["markers"] == [0xD0 + (i & 7) for i in range(14)]
    assert any(c[3]["stuffed"] > 0 for c in cases), "a stuffed FF 00"
    shapes = {c[2].shape[:2] for c in cases}
    assert {(1, 1), (9, 17), (16, 16), (256, 256)} <= shapes
    assert by["smooth_420_256x256"][3]["sampling"] == (2, 2)

    arrays = {"names": np.array([c[0] for c in cases])}
    for name, data, px, _ in cases:
        arrays["jpeg_" + name] = np.frombuffer(data, np.uint8)
        arrays["pixels_" + name] = np.ascontiguousarray(px.transpose(2, 0, 1)) if px.ndim == 3 else px
    np.savez_compressed(OUT, **arrays)
    size = os.path.getsize(OUT)
    assert size <= MAX_BYTES, "%d bytes exceed %d" % (size, MAX_BYTES)
    print("%s: %d streams, %d bytes; stuffed FF 00 in %d of them" % (OUT, len(cases), size,
                                                                    sum(c[3]["stuffed"] > 0 for c in cases)))
    return 0


if __name__ == "__main__":
    sys.exit(main())
