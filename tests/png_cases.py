"""The named PNG cases of the decoder's tests: what tests/png_writer.py is asked to write.  A case is its samples (uint16
[H, W, channels]) with colour type, depth, the filter of every row, the interlace flag and the palette; `named_cases()`
builds them once, `file_of(case)` writes the file.  tests/png_census.py counts what they reach."""
import collections
import functools

import numpy as np

import png_writer

Case = collections.namedtuple("Case", "samples colour_type depth filters interlace palette")
FORMS = [(0, 1), (0, 2), (0, 4), (0, 8), (0, 16), (2, 8), (2, 16), (3, 1), (3, 2), (3, 4), (3, 8), (4, 8), (4, 16), (6, 8), (6, 16)]
BPP_FORMS = {1: (0, 8), 2: (4, 8), 3: (2, 8), 4: (6, 8), 6: (2, 16), 8: (6, 16)}       # one form per filter unit
ADAM7_SIZES = ((1, 1), (1, 9), (9, 1), (2, 2), (3, 5), (5, 3), (8, 8), (9, 9), (53, 37), (9, 65), (65, 3), (129, 2), (2, 65),
               (63, 1), (64, 4))                  # height, width


def palette_of(depth, rng, entries=None):
    n = entries or (1 << depth)
    return rng.randint(0, 256, size=(n, 3)).astype(np.uint8).tobytes()


def noise(rng, h, w, colour_type, depth, entries=None):
    hi = (entries or (1 << depth)) if colour_type == 3 else (1 << depth)
    return rng.randint(0, hi, size=(h, w, png_writer.CHANNELS[colour_type])).astype(np.uint16)


def smooth(h, w, colour_type, depth, seed):
    """a smooth image: neighbours are close, so Average and Paeth meet their ties and the filters' sums stay small"""
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    top = (1 << depth) - 1
    ch = [0.5 + 0.5 * np.sin(0.07 * (c + 1 + seed) * x + 0.05 * (c + 2) * y) for c in range(png_writer.CHANNELS[colour_type])]
    return np.clip(np.rint(np.stack(ch, axis=-1) * top), 0, top).astype(np.uint16)


def photo(h, w, seed):
    """uint8 [h, w, 3]: products of slow waves per channel, the kind of image for which an encoder's filter heuristic
    picks Sub on the first row and Paeth below it"""
    rng = np.random.RandomState(seed)
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    img = np.zeros((h, w, 3))
    for c in range(3):
        a, b, p, q = rng.uniform(0.02, 0.09, 4)
        img[..., c] = 128 + 70 * np.sin(a * x + p * 20) * np.cos(b * y + q * 20) + 50 * np.sin(0.013 * (x + y) * (c + 1))
    return np.clip(np.rint(img), 0, 255).astype(np.uint8)


def planted():
    """RGB8, rows of Paeth, Paeth and Average around chosen neighbours (left a, up b, upleft c), e.g. a 0, b 3, c 2 (the
    a = c tie), a 3, b 0, c 2 (b = c), equal triples, a 10, b 20, c 15 (upleft wins), Average over 255 + 255.  On its own
    it reaches Paeth choosing left, up and upleft, all four ties and an Average sum of 256 or more
    (tests/test_png_decode_cpu.py holds it to that), whatever the noise of the other cases does."""
    rows = np.zeros((3, 8, 3), np.uint16)
    rows[0, :, :] = np.array([2, 3, 2, 0, 9, 5, 7, 7])[:, None]           # c, b pairs for the row below
    rows[1, :, :] = np.array([0, 250, 3, 255, 5, 255, 7, 200])[:, None]
    rows[0, :, 1] = np.array([15, 20, 10, 200, 255, 255, 100, 100])
    rows[1, :, 1] = np.array([10, 251, 0, 199, 255, 254, 200, 1])
    rows[2, :, :] = np.array([255, 0, 128, 255, 1, 254, 3, 250])[:, None]
    return Case(rows, 2, 8, (4, 4, 3), 0, None)


@functools.lru_cache(maxsize=None)
def named_cases():
    """name -> Case, in a fixed order"""
    rng = np.random.RandomState(2083)
    out = collections.OrderedDict()

    def add(name, h, w, ct, depth, filters, interlace=0, kind="noise", entries=None):
        assert name not in out, name
        s = noise(rng, h, w, ct, depth, entries) if kind == "noise" else smooth(h, w, ct, depth, len(out))
        if not isinstance(filters, int):
            filters = tuple(int(v) for v in filters)
        out[name] = Case(s, ct, depth, filters, interlace, palette_of(depth, rng, entries) if ct == 3 else None)

    def random_filters(n):
        return rng.randint(0, 5, size=n)

    # widths 1, 2, 3 and 65 at every filter unit; 5 rows so that every row has a row above with every filter
    for bpp, (ct, depth) in BPP_FORMS.items():
        for w in (1, 2, 3, 65):
            add("bpp%d_w%d" % (bpp, w), 6, w, ct, depth, (4, 3, 1, 2, 4, 3))
    # row padding below 8 bits
    for ct, depth in ((0, 1), (0, 2), (0, 4), (3, 1), (3, 2), (3, 4)):
        for w in (1, 7, 8, 9):
            add("sub_c%dd%d_w%d" % (ct, depth, w), 5, w, ct, depth, (0, 1, 2, 3, 4))
    # band edges and the hand-over row: every filter forced on all rows, and random filters, at every height
    for h in (1, 2, 63, 64, 65, 129):
        add("rows%d_random" % h, h, 5, 2, 8, random_filters(h))
        for ft in range(5):
            add("rows%d_filter%d" % (h, ft), h, 3, (2, 6, 0, 4, 2)[ft], 8, ft, kind="noise" if ft % 2 else "smooth")
    add("rows129_w65_rgba16", 129, 65, 6, 16, random_filters(129))
    # all 15 forms, wider than a chunk of any filter unit
    for ct, depth in FORMS:
        add("form_c%dd%d" % (ct, depth), 7, 37, ct, depth, random_filters(7), kind="smooth" if depth >= 8 and ct != 3 else "noise")
    add("palette_short", 4, 9, 3, 8, (0, 1, 2, 4), entries=5)
    # Adam7: every pass present and absent, the forms in turn
    for k, (h, w) in enumerate(ADAM7_SIZES):
        ct, depth = FORMS[k % len(FORMS)]
        add("adam7_%dx%d_c%dd%d" % (w, h, ct, depth), h, w, ct, depth, random_filters(11), interlace=1)
    add("adam7_53x37_rgb8", 37, 53, 2, 8, random_filters(13), interlace=1)
    add("adam7_9x65_p2", 65, 9, 3, 2, random_filters(7), interlace=1)
    add("adam7_65x129_ga8", 129, 65, 4, 8, random_filters(17), interlace=1)
    out["planted"] = planted()
    return out


def file_of(case, **kw):
    return png_writer.write_png(case.samples, case.colour_type, case.depth, case.filters, case.interlace, case.palette, **kw)


@functools.lru_cache(maxsize=None)
def files():
    """name -> the file's bytes, written once"""
    return collections.OrderedDict((name, file_of(c)) for name, c in named_cases().items())


def expected_pixels(case):
    """the B G R pixels the pixel rule gives the case's samples: from what went INTO the writer, no decoder involved"""
    s, ct, depth = case.samples.astype(np.int64), case.colour_type, case.depth
    if ct == 3:
        pal = np.frombuffer(case.palette, np.uint8).reshape(-1, 3)
        rgb = pal[s[..., 0]]
    else:
        v = s >> 8 if depth == 16 else s * {1: 255, 2: 85, 4: 17, 8: 1}[depth]
        rgb = np.repeat(v[..., :1], 3, axis=2) if ct in (0, 4) else v[..., :3]
    return np.ascontiguousarray(rgb[..., ::-1].astype(np.uint8))
