#!/usr/bin/env python3
"""Writes tests/golden/png_decode_golden.npz: PNG files written by Pillow, files written by tests/png_writer.py (the cases
of tests/png_cases.py that Pillow cannot write: Adam7, forced filters, every form), and what Pillow (libpng's rules,
Pillow's own decoder) reads BOTH kinds as - the independent yardstick of the device decoder (csrc/png_decode.hip) and of
its restatement (tests/png_decode_ref.py).  Data only: `names`, `origins` ('pillow' or 'writer'), and per name
`png_<name>` (the file's bytes) and `pixels_<name>` (uint8 [3][H][W]: the R, G and B planes of the 8-bit pixels
`cv2.imread` would return: Pillow's pixels with alpha dropped, a 16-bit grey image (`I;16`, exact samples) cut to its
high byte and grey replicated).  Run on a CPU machine that has Pillow; no test imports Pillow.  The asserts state what
the fixture must hold.

    python tests/golden/make_png_decode_golden.py
"""
import io
import os
import sys
import zlib

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
OUT = os.path.join(HERE, "png_decode_golden.npz")
MAX_BYTES = 200 * 1000
WRITER_CASES = ("planted", "rows65_random", "rows129_filter3", "rows64_filter4", "bpp8_w65", "bpp6_w3", "sub_c0d1_w9",
                "sub_c3d2_w7", "palette_short", "adam7_53x37_rgb8", "adam7_9x65_p2", "adam7_5x3_c0d16", "adam7_3x5_c2d8", "adam7_8x8_c2d16",
                "adam7_4x64_c6d16")


def pillow_pixels(data):
    """the file through Pillow -> uint8 [H, W, 3] R G B by the pixel rule, and Pillow's mode"""
    from PIL import Image
    im = Image.open(io.BytesIO(data))
    im.load()
    if im.mode.startswith("I;16"):
        grey = (np.asarray(im).astype(np.uint16) >> 8).astype(np.uint8)
        return np.repeat(grey[..., None], 3, axis=2), im.mode
    return np.asarray(im.convert("RGB")), im.mode


def filter_bytes(data):
    """the set of filter types of a non-interlaced file"""
    import png_decode_ref as ref
    hdr = ref.png_header(data)
    raw = zlib.decompress(hdr.idat)
    (p,) = ref.passes(hdr.height, hdr.width, hdr.colour_type, hdr.bit_depth, 0)
    return set(np.frombuffer(raw, np.uint8).reshape(p.rows, p.row_bytes + 1)[:, 0].tolist())


def main():
    from PIL import Image

    import png_cases
    cases = []

    def add(name, image, **kw):
        buf = io.BytesIO()
        image.save(buf, "PNG", **kw)
        data = buf.getvalue()
        px, mode = pillow_pixels(data)
        cases.append((name, "pillow", data, px, mode))
        return data

    rgb = png_cases.photo(96, 130, 3)
    used = filter_bytes(add("pillow_rgb_130x96", Image.fromarray(rgb)))
    assert {1, 4} <= used, "Pillow's smooth-image file uses filters 1 and 4, got %s" % sorted(used)
    add("pillow_rgba_37x53", Image.fromarray(png_cases.smooth(53, 37, 6, 8, 4).astype(np.uint8), "RGBA"))
    add("pillow_grey_65x9", Image.fromarray(png_cases.smooth(9, 65, 0, 8, 5).astype(np.uint8)[..., 0]))
    add("pillow_la_9x17", Image.fromarray(png_cases.smooth(17, 9, 4, 8, 6).astype(np.uint8), "LA"))
    add("pillow_grey16_21x11", Image.fromarray(png_cases.smooth(11, 21, 0, 16, 7)[..., 0]))
    add("pillow_bilevel_19x7", Image.fromarray(png_cases.smooth(7, 19, 0, 8, 8).astype(np.uint8)[..., 0]).convert("1"))
    pal = Image.fromarray(rgb[:40, :50]).quantize(13)
    add("pillow_palette13_50x40", pal)
    add("pillow_palette13_trns_50x40", pal, transparency=3)
    modes = {c[4] for c in cases}
    assert modes >= {"RGB", "RGBA", "L", "LA", "1", "P"} and any(m.startswith("I;16") for m in modes), modes
    written = png_cases.files()
    for name in WRITER_CASES:
        px, mode = pillow_pixels(written[name])
        want = png_cases.expected_pixels(png_cases.named_cases()[name])[..., ::-1]
        assert np.array_equal(px, want), "%s: Pillow does not read the writer's file to the samples given" % name
        cases.append((name, "writer", written[name], px, mode))

    arrays = {"names": np.array([c[0] for c in cases]), "origins": np.array([c[1] for c in cases])}
    for name, _, data, px, _ in cases:
        arrays["png_" + name] = np.frombuffer(data, np.uint8)
        arrays["pixels_" + name] = np.ascontiguousarray(px.transpose(2, 0, 1))
    np.savez_compressed(OUT, **arrays)
    size = os.path.getsize(OUT)
    assert size <= MAX_BYTES, "%d bytes exceed %d" % (size, MAX_BYTES)
    print("%s: %d files (%d by Pillow), %d bytes" % (OUT, len(cases), sum(c[1] == "pillow" for c in cases), size))
    return 0


if __name__ == "__main__":
    sys.exit(main())
