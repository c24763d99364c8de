#!/usr/bin/env python3
"""Writes tests/golden/jpeg_decode_extreme_golden.npz: baseline JPEG files of FULL-SWING images encoded by Pillow at quality
100, and what Pillow (libjpeg-turbo) decodes them to.  The streams of jpeg_decode_golden.npz come from mild inputs and stop
at DC category 8, AC size 9 and coefficients below 300; these reach what 8-bit input can reach: DC differences of
category 11, AC magnitudes of size 10, |DC| = 1024, 16-bit AC codes and DC codes of 9 bits and more, and a restart marker
between every two MCUs while the DC swings from end to end.  Same layout as jpeg_decode_golden.npz (`names`, `jpeg_<name>`,
`pixels_<name>` as uint8 [3][H][W] R G B planes, [H][W] for greyscale); tests/jpeg_decode_ref.py `load_golden` reads both
files.  Run on a CPU machine that has Pillow; no test imports Pillow.  The asserts state, from each file's own bytes (walked by
the restatement tests/jpeg_decode_ref.py), what the fixture must hold, so that a change of encoder cannot soften it unnoticed.

    python tests/golden/make_jpeg_decode_extreme_golden.py
"""
import io
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import jpeg_decode_ref as jref  # noqa: E402
from make_jpeg_decode_golden import facts, harsh  # noqa: E402

OUT = os.path.join(HERE, "jpeg_decode_extreme_golden.npz")
MAX_BYTES = 200 * 1000


def blocks(h, w):
    """8 x 8 blocks of 0 and 255 in turn: every block's DC at one end of the range, the difference at the other"""
    y, x = np.mgrid[0:h, 0:w]
    return ((((y // 8) + (x // 8)) & 1) * 255).astype(np.uint8)


def checker(h, w):
    """pixels of 0 and 255 in turn: all of a block's energy in its highest frequency"""
    y, x = np.mgrid[0:h, 0:w]
    return (((y + x) & 1) * 255).astype(np.uint8)


def reached(data):
    r = {}
    coef, status, _ = jref.entropy(jref.parse_stream(data), reached=r)
    assert status == 0
    return r


def main():
    from PIL import Image
    cases = []

    def add(name, img, **kw):
        buf = io.BytesIO()
        Image.fromarray(img).save(buf, "JPEG", quality=100, **kw)
        data = buf.getvalue()
        px = np.asarray(Image.open(io.BytesIO(data)))
        assert px.shape == img.shape and px.dtype == np.uint8
        cases.append((name, data, px, facts(data), reached(data)))

    h, w = 48, 32
    rgb = lambda p: np.stack([p] * 3, -1)       # noqa: E731
    add("blocks_444", rgb(blocks(h, w)), subsampling=0)
    add("blocks_420", rgb(blocks(h, w)), subsampling=2)
    add("checker_444", rgb(checker(h, w)), subsampling=0)
    add("checker_grey", checker(h, w))
    add("colour_blocks_444", np.stack([blocks(h, w), 255 - blocks(h, w), checker(h, w)], -1), subsampling=0)
    add("harsh_420_optimize", harsh(h, w, 21), subsampling=2, optimize=True)
    add("restart1_blocks_420", rgb(blocks(96, 64)), subsampling=2, restart_marker_blocks=1)

    by = {c[0]: c for c in cases}
    r = {name: c[4] for name, c in by.items()}
    for name, c in by.items():
        print("%-22s %5d bytes  %s" % (name, len(c[1]), "  ".join("%s %d" % kv for kv in sorted(c[4].items()))))
    # what the fixture must hold
    for name in ("blocks_444", "blocks_420", "restart1_blocks_420"):
        assert r[name]["dc_category"] == 11 and r[name]["dc_abs"] == 1024 and r[name]["dc_code_bits"] >= 9, (name, r[name])
    assert r["colour_blocks_444"]["dc_category"] == 11 and r["colour_blocks_444"]["dc_code_bits"] == 11      # the chroma table's
    for name in ("checker_444", "checker_grey"):
        assert r[name]["ac_size"] == 10 and r[name]["ac_abs"] >= 800 and r[name]["ac_code_bits"] == 16, (name, r[name])
    assert r["colour_blocks_444"]["ac_code_bits"] == 16 and r["colour_blocks_444"]["ac_size"] >= 9
    standard = by["blocks_420"][3]["dht"]
    assert by["harsh_420_optimize"][3]["dht"] != standard and by["blocks_444"][3]["dht"] == standard, "own Huffman tables"
    r1 = by["restart1_blocks_420"][3]           # 4 x 6 MCUs, one each: 24 intervals, the marker index wraps twice
    assert r1["sampling"] == (2, 2) and r1["restart"] == 1 and r1["markers"] == [0xD0 + (i & 7) for i in range(23)]
    assert len(r1["markers"]) >= 17
    assert all(c[2].min() == 0 and c[2].max() == 255 for c in cases), "both clamps"
    assert max(c[2].shape[0] for c in cases) <= 96 and max(c[2].shape[1] for c in cases) <= 64

    arrays = {"names": np.array([c[0] for c in cases])}
    for name, data, px, _, _ in cases:
        arrays["jpeg_" + name] = np.frombuffer(data, np.uint8)
        arrays["pixels_" + name] = np.ascontiguousarray(px.transpose(2, 0, 1)) if px.ndim == 3 else px
    np.savez_compressed(OUT, **arrays)
    size = os.path.getsize(OUT)
    assert size <= MAX_BYTES, "%d bytes exceed %d" % (size, MAX_BYTES)
    print("%s: %d streams, %d bytes" % (OUT, len(cases), size))
    return 0


if __name__ == "__main__":
    sys.exit(main())
