#!/usr/bin/env python3
"""Writes tests/golden/jpeg_progressive_golden.npz: progressive JPEG files (SOF2) encoded by Pillow and what Pillow
(libjpeg-turbo) decodes them to - the yardstick of the progressive entropy stage (csrc/jpeg_decode.hip) and of its
restatement (tests/jpeg_progressive_ref.py).  Same form as make_jpeg_decode_golden.py: data only - `names`, and per name
`jpeg_<name>` (the file's bytes) and `pixels_<name>` (uint8 [3][H][W] R, G, B planes; [H][W] for greyscale; a name listed
in `pixels_in_baseline_fixture` has the pixels of the same name in jpeg_decode_golden.npz).  Run on a CPU machine that has
Pillow; no test imports Pillow.  The asserts state what the fixture must hold.

It also checks the writer (tests/jpeg_progressive_writer.py) against Pillow: every writer case of
tests/jpeg_progressive_cases.py is decoded by Pillow, and the pixels must equal the restatement's - the writer's files are
real JPEG, not a private dialect.  Nothing of that is stored: the cases are rebuilt by the tests.

    python tests/golden/make_jpeg_progressive_golden.py
"""
import io
import os
import struct
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
OUT = os.path.join(HERE, "jpeg_progressive_golden.npz")
MAX_BYTES = 200 * 1000

from make_jpeg_decode_golden import harsh, noise, smooth  # noqa: E402


def facts(data):
    """the markers of a file: SOF, per scan (components, Ss, Se, Ah, Al), the DRI values, the RSTn markers of each scan"""
    pos, sof, scans, dri, rst = 2, [], [], [], []
    while pos + 4 <= len(data):
        assert data[pos] == 0xFF, pos
        marker, length = data[pos + 1], struct.unpack_from(">H", data, pos + 2)[0]
        body = data[pos + 4:pos + 2 + length]
        pos += 2 + length
        if marker in (0xC0, 0xC1, 0xC2):
            sof.append((marker, body[5], (body[7] >> 4, body[7] & 15) if body[5] == 3 else (0, 0)))
        elif marker == 0xDD:
            dri.append(struct.unpack(">H", body)[0])
        elif marker == 0xDA:
            ns = body[0]
            scans.append((ns, body[1 + 2 * ns], body[2 + 2 * ns], body[3 + 2 * ns] >> 4, body[3 + 2 * ns] & 15))
            marks = []
            while not (data[pos] == 0xFF and data[pos + 1] not in (0, 0xFF) and not 0xD0 <= data[pos + 1] <= 0xD7):
                if data[pos] == 0xFF and 0xD0 <= data[pos + 1] <= 0xD7:
                    marks.append(data[pos + 1])
                pos += 1
            rst.append(marks)
        elif marker == 0xD9:
            break
    return dict(sof=sof, scans=scans, dri=dri, rst=rst)


def main():
    from PIL import Image
    cases = []

    def add(name, img, **kw):
        buf = io.BytesIO()
        Image.fromarray(img).save(buf, "JPEG", progressive=True, **kw)
        data = buf.getvalue()
        px = np.asarray(Image.open(io.BytesIO(data)))
        assert px.shape == img.shape and px.dtype == np.uint8
        # a complete progressive file holds the coefficients of its baseline twin: libjpeg smooths nothing
        twin = io.BytesIO()
        Image.fromarray(img).save(twin, "JPEG", **kw)
        assert np.array_equal(px, np.asarray(Image.open(io.BytesIO(twin.getvalue())))), name
        cases.append((name, data, px, facts(data)))

    for sub, tag in ((0, "444"), (1, "422"), (2, "420")):
        for (w, h) in ((1, 1), (17, 9), (16, 16), (24, 24), (37, 53)):
            add("smooth_%s_%dx%d" % (tag, w, h), smooth(h, w, 3 + sub), quality=90, subsampling=sub)
            add("noise_%s_%dx%d" % (tag, w, h), noise(h, w, 7 + sub), quality=75, subsampling=sub)
    add("noise_420_8x24", noise(24, 8, 21), quality=80, subsampling=2)
    add("grey_17x9", smooth(9, 17, 1)[..., 0], quality=85)
    add("grey_noise_37x53", noise(53, 37, 2)[..., 0], quality=60)
    add("q5_noise_420_40x72", harsh(72, 40, 4), quality=5, subsampling=2)
    add("q100_noise_422_37x53", noise(53, 37, 6), quality=100, subsampling=1)
    for r in (1, 3, 5):
        add("restart%d_420_37x53" % r, noise(53, 37, 8), quality=70, subsampling=2, restart_marker_blocks=r)
    add("smooth_420_256x256", smooth(256, 256, 10, 0.01, 0.03), quality=90, subsampling=2)

    by = {c[0]: c for c in cases}
    f = {name: c[3] for name, c in by.items()}
    # what the fixture must hold
    assert all(len(c[3]["sof"]) == 1 and c[3]["sof"][0][0] == 0xC2 for c in cases), "progressive (SOF2) only"
    assert {c[3]["sof"][0][2] for c in cases} >= {(1, 1), (2, 1), (2, 2)} and any(c[3]["sof"][0][1] == 1 for c in cases)
    ten = [(3, 0, 0, 0, 1), (1, 1, 5, 0, 2), (1, 1, 63, 0, 1), (1, 1, 63, 0, 1), (1, 6, 63, 0, 2), (1, 1, 63, 2, 1),
           (3, 0, 0, 1, 0), (1, 1, 63, 1, 0), (1, 1, 63, 1, 0), (1, 1, 63, 1, 0)]
    assert f["noise_420_24x24"]["scans"] == ten, f["noise_420_24x24"]["scans"]
    assert len(f["grey_17x9"]["scans"]) == 6
    px = by["q5_noise_420_40x72"][2]
    assert px.min() == 0 and px.max() == 255, "both clamps (%d..%d)" % (px.min(), px.max())
    for r in (1, 3, 5):
        fr = f["restart%d_420_37x53" % r]
        assert fr["dri"] == [r] and fr["sof"][0][2] == (2, 2)
        # 3 x 4 MCUs in the DC scans; 5 x 7 luma and 3 x 4 chroma blocks in the AC scans: the interval counts each scan's own
        for (ns, ss, _, _, _), marks in zip(fr["scans"], fr["rst"]):
            units = 12 if ss == 0 else None
            if units is not None:
                assert len(marks) == -(-units // r) - 1, (r, ns, ss, len(marks))
            assert marks == [0xD0 + (i & 7) for i in range(len(marks))]
        assert {len(m) for m in fr["rst"]} >= {-(-35 // r) - 1, -(-12 // r) - 1}
    assert max(len(m) for m in f["restart1_420_37x53"]["rst"]) == 34, "RSTn wraps past 7 four times"
    shapes = {c[2].shape[:2] for c in cases}
    assert {(1, 1), (9, 17), (16, 16), (24, 24), (53, 37), (24, 8), (256, 256)} <= shapes

    # the writer against Pillow, through the restatement
    import jpeg_progressive_cases as pc
    import jpeg_progressive_ref as pref
    for name, case in pc.cases().items():
        px = np.asarray(Image.open(io.BytesIO(case.data)))
        bgr = px[..., ::-1] if px.ndim == 3 else np.repeat(px[..., None], 3, 2)
        got = pref.decode_progressive(case.data)
        assert got.shape == bgr.shape and np.array_equal(got, bgr), "%s: Pillow and the restatement differ" % name
        print("writer case %s: %d bytes, Pillow's pixels equal the restatement's" % (name, len(case.data)))

    # the 256 x 256 picture is the baseline fixture's: same input, quality and sampling, hence (asserted here) the same
    # pixels, which are therefore not stored twice - jpeg_progressive_ref.load_golden takes them from there
    base = np.load(os.path.join(HERE, "jpeg_decode_golden.npz"))
    arrays = {"names": np.array([c[0] for c in cases]), "pixels_in_baseline_fixture": np.array(["smooth_420_256x256"])}
    for name, data, px, _ in cases:
        arrays["jpeg_" + name] = np.frombuffer(data, np.uint8)
        planes = np.ascontiguousarray(px.transpose(2, 0, 1)) if px.ndim == 3 else px
        if name in arrays["pixels_in_baseline_fixture"].tolist():
            assert np.array_equal(base["pixels_" + name], planes), name
        else:
            arrays["pixels_" + name] = planes
    np.savez_compressed(OUT, **arrays)
    size = os.path.getsize(OUT)
    assert size <= MAX_BYTES, "%d bytes exceed %d" % (size, MAX_BYTES)
    print("%s: %d streams, %d bytes" % (OUT, len(cases), size))
    return 0


if __name__ == "__main__":
    sys.exit(main())
