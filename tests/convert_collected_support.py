"""Fake trees of the two-object test set for the converter's tests: ROOT/test_list.txt, ROOT/<id>.png (written by
tests/png_writer.py) and ROOT/<id>.wav (tests/convert_ref.py)."""
import numpy as np

import convert_ref
import png_cases
import png_writer

# id -> (height, width, colour type, depth, interlace, filters), (rate, bits, samples)
RECORDINGS = {
    7: ((224, 298, 2, 8, 0, (1, 4, 2, 3, 0)), (22050, 16, 2500)),          # the data set's own size
    1: ((224, 298, 2, 16, 1, (4, 1, 3)), (44100, 32, 3000)),               # 16-bit, Adam7
    23: ((224, 298, 3, 8, 0, (0, 2, 4)), (12288, 16, 1500)),               # palette; the rate that passes through
    12: ((37, 53, 6, 8, 0, (3, 4)), (22050, 16, 900)),                     # another size: logged, still written
}
LISTED = ("7.png", "23.png", "1.png", "12.png")
CLASS_OF_ID = (9, 9, 9, 9, 9, 9, 2, 9, 9, 4, 6, 7, 6, 1, 1, 8, 8, 2, 2, 0, 2, 3, 5)


def picture(ident):
    """-> (the file's bytes, the B G R pixels its samples stand for)"""
    h, w, ct, depth, lace, filters = RECORDINGS[ident][0]
    rng = np.random.RandomState(ident)
    if ct == 3:
        palette = rng.randint(0, 256, size=(200, 3)).astype(np.uint8).tobytes()
        samples = (png_cases.photo(h, w, ident)[..., :1].astype(np.uint16) * 199) // 255
    else:
        palette = None
        base = png_cases.photo(h, w, ident).astype(np.uint16)
        if png_writer.CHANNELS[ct] == 4:
            base = np.concatenate([base, rng.randint(0, 256, size=(h, w, 1)).astype(np.uint16)], axis=2)
        if depth == 16:                               # a low byte that the pixel rule must drop
            base = (base << 8) | rng.randint(0, 256, size=base.shape).astype(np.uint16)
        samples = base
    case = png_cases.Case(samples, ct, depth, filters, lace, palette)
    return png_cases.file_of(case), png_cases.expected_pixels(case)


def sound(ident):
    rate, bits, n = RECORDINGS[ident][1]
    amp = 2 ** (bits - 2)
    wave = np.random.RandomState(100 + ident).randn(n) * amp / 8 + amp * np.sin(2 * np.pi * 700.0 * np.arange(n) / rate)
    return np.clip(wave, -2 * amp, 2 * amp - 1).astype(np.int32)


def write_tree(root, idents=tuple(RECORDINGS), listed=LISTED):
    """-> {id: (pixels, samples)}"""
    out = {}
    for ident in idents:
        data, bgr = picture(ident)
        (root / ("%d.png" % ident)).write_bytes(data)
        rate, bits, _ = RECORDINGS[ident][1]
        (root / ("%d.wav" % ident)).write_bytes(convert_ref.wav_bytes(sound(ident), rate=rate, bits=bits))
        out[ident] = (bgr, sound(ident))
    (root / "test_list.txt").write_text("".join(n + "\n" for n in listed))
    return out
