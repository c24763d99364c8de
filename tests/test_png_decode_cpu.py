"""The PNG reader's host side: the restatement (tests/png_decode_ref.py) against Pillow's pixels of the committed fixture,
the test writer against Pillow, every refusal of `acimg.png.parse_png` by name, the census of the cases, the size queries
of the library and the job tables of interlaced images.  No GPU."""
import collections
import os
import struct
import sys
import zlib

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import png_cases  # noqa: E402
import png_census  # noqa: E402
import png_decode_ref as ref  # noqa: E402
import png_writer  # noqa: E402


@pytest.fixture(scope="module")
def golden():
    return ref.load_png_golden()


def test_restatement_equals_pillow_on_every_golden_file(golden):
    assert {o for _, _, o in golden.values()} == {"pillow", "writer"}
    for name, (data, pillow, _) in golden.items():
        _, bgr, status = ref.decode_png(data)
        assert status == 0 and bgr.shape == pillow.shape and np.array_equal(bgr, pillow), name


def test_pillow_reads_the_writers_files_to_the_samples_given(golden):
    """the fixture's pixels of a writer file are Pillow's; the expectation is formed from what went into the writer"""
    seen = 0
    for name, (data, pillow, origin) in golden.items():
        if origin == "writer":
            case = png_cases.named_cases()[name]
            assert np.array_equal(pillow, png_cases.expected_pixels(case)), name
            hdr = ref.png_header(data)
            assert (hdr.height, hdr.width, hdr.colour_type, hdr.bit_depth, hdr.interlace) == (
                case.samples.shape[0], case.samples.shape[1], case.colour_type, case.depth, case.interlace), name
            # today's writer still writes those scanlines (the deflated bytes may differ with the zlib at hand)
            assert ref.inflate_idat(hdr) == png_writer.scanlines(case.samples, case.colour_type, case.depth, case.filters, case.interlace)
            seen += 1
    assert seen >= 10


def test_restatement_gives_every_case_the_pixels_of_its_samples():
    for name, data in png_cases.files().items():
        case = png_cases.named_cases()[name]
        samples, bgr, status = ref.decode_png(data)
        assert status == 0 and np.array_equal(bgr, png_cases.expected_pixels(case)), name
        assert np.array_equal(ref.gather(samples, ref.png_header(data)), case.samples), name


def test_census_of_the_cases():
    assert png_census.missing() == []
    count = collections.Counter()
    hdr = ref.png_header(png_cases.files()["planted"])
    ref.unfilter(ref.inflate_idat(hdr), hdr, count)
    for key in ["paeth chooses " + w for w in "abc"] + ["paeth tie " + t for t in ("a=b=c", "a=b", "a=c", "b=c")] + [
            "average with a sum of 256 or more", "sum wraps"]:
        assert count[key], "the planted case no longer reaches: " + key


# ---- parse_png ------------------------------------------------------------------------------------------------------------
def small_png(**kw):
    s = np.arange(12, dtype=np.uint16).reshape(2, 2, 3) * 20
    return png_writer.write_png(s, 2, 8, (1, 4), **kw)


def rebuilt(data, edit):
    """the file with its chunk list passed through `edit` ([(kind, body)] -> the same), CRCs made anew"""
    return png_writer.SIGNATURE + b"".join(png_writer.chunk(k, b) for k, b in edit(ref.chunks(data)))


def with_ihdr(data, **fields):
    def edit(ch):
        names = ("width", "height", "depth", "ctype", "compression", "filter", "interlace")
        v = dict(zip(names, struct.unpack(">IIBBBBB", ch[0][1])))
        v.update(fields)
        return [(b"IHDR", struct.pack(">IIBBBBB", *[v[n] for n in names]))] + ch[1:]
    return rebuilt(data, edit)


def with_stream(data, change):
    def edit(ch):
        z = bytearray(b"".join(b for k, b in ch if k == b"IDAT"))
        z = change(z)
        return [c for c in ch if c[0] not in (b"IDAT", b"IEND")] + [(b"IDAT", bytes(z)), (b"IEND", b"")]
    return rebuilt(data, edit)


def fdict(z):
    z[1] |= 0x20
    z[1] = (z[1] & 0xE0) | ((31 - ((z[0] << 8) | (z[1] & 0xE0)) % 31) % 31)
    return z


def big_window(z):
    z[0] = 0x88                                     # CINFO 8: a window of 64 KiB
    z[1] = (z[1] & 0xE0)
    z[1] |= (31 - ((z[0] << 8) | z[1]) % 31) % 31
    return z


def flipped_crc(data):
    at = data.index(b"IDAT") + 5
    return data[:at] + bytes([data[at] ^ 0x10]) + data[at + 1:]


PALETTE = png_writer.write_png(np.array([[0, 1], [1, 0]], np.uint16)[..., None], 3, 1, 0, palette=bytes(6))
REFUSALS = collections.OrderedDict([
    ("bad signature", (lambda: b"\x89PNG\r\n\x1a\r" + small_png()[8:], "not a PNG file")),
    ("truncated chunk", (lambda: small_png()[:-20], "truncated PNG file")),
    ("truncated chunk header", (lambda: small_png()[:-6], "end inside a chunk header")),
    ("flipped CRC bit", (lambda: flipped_crc(small_png()), "CRC mismatch in chunk IDAT")),
    ("no IHDR", (lambda: rebuilt(small_png(), lambda ch: ch[1:]), "the first chunk is IDAT, not IHDR")),
    ("no IDAT", (lambda: rebuilt(small_png(), lambda ch: [c for c in ch if c[0] != b"IDAT"]), "no IDAT chunk")),
    ("no IEND", (lambda: rebuilt(small_png(), lambda ch: ch[:-1]), "no IEND chunk")),
    ("IDAT after IEND", (lambda: rebuilt(small_png(), lambda ch: ch + [ch[1]]), "after IEND")),
    ("IDAT not consecutive", (lambda: small_png(idat_splits=(5,), between_idat=[(b"tEXt", b"a\x00b")]), "IDAT chunks are not consecutive")),
    ("PLTE after IDAT", (lambda: rebuilt(PALETTE, lambda ch: [ch[0], ch[2], ch[1], ch[3]]), "PLTE after the first IDAT")),
    ("illegal colour type", (lambda: with_ihdr(small_png(), ctype=5), "colour type 5 with bit depth 8")),
    ("illegal depth", (lambda: with_ihdr(small_png(), depth=4), "colour type 2 with bit depth 4")),
    ("compression method", (lambda: with_ihdr(small_png(), compression=1), "compression method 1")),
    ("filter method", (lambda: with_ihdr(small_png(), filter=1), "filter method 1")),
    ("interlace method", (lambda: with_ihdr(small_png(), interlace=2), "interlace method 2")),
    ("zero width", (lambda: with_ihdr(small_png(), width=0), "0 x 2 pixels")),
    ("zero height", (lambda: with_ihdr(small_png(), height=0), "2 x 0 pixels")),
    ("PLTE missing", (lambda: rebuilt(PALETTE, lambda ch: [c for c in ch if c[0] != b"PLTE"]), "colour type 3 without a PLTE")),
    ("PLTE not a multiple of 3", (lambda: rebuilt(PALETTE, lambda ch: [ch[0], (b"PLTE", bytes(7))] + ch[2:]), "no multiple of 3")),
    ("PLTE too long", (lambda: rebuilt(PALETTE, lambda ch: [ch[0], (b"PLTE", bytes(9))] + ch[2:]), "PLTE of 3 entries for a bit depth of 1")),
    ("unknown critical chunk", (lambda: small_png(before_idat=[(b"CgBI", b"\x00" * 4)]), "unknown critical chunk CgBI")),
    ("zlib method", (lambda: with_stream(small_png(), lambda z: bytearray(b"\x79\x01") + z[2:]), "zlib header 79 01")),
    ("zlib window", (lambda: with_stream(small_png(), big_window), "is not deflate with a window of at most 32 KiB")),
    ("zlib check bits", (lambda: with_stream(small_png(), lambda z: bytearray([z[0], z[1] ^ 1]) + z[2:]), "zlib header")),
    ("zlib FDICT", (lambda: with_stream(small_png(), fdict), "preset dictionary")),
])


@pytest.mark.parametrize("what", list(REFUSALS))
def test_parse_png_refuses_by_name(what):
    from acimg import png
    from acimg.convert import ConvertError
    make, text = REFUSALS[what]
    with pytest.raises(ConvertError) as e:
        png.parse_png(make(), "dir/%s.png" % what)
    assert str(e.value).startswith("dir/%s.png: " % what) and text in str(e.value), str(e.value)


def test_parse_png_reads_what_is_legal():
    from acimg import png
    info = png.parse_png(small_png(), "a.png")
    assert (info.height, info.width, info.colour_type, info.bit_depth, info.interlace, info.bpp) == (2, 2, 2, 8, 0, 3)
    assert (info.inflated_bytes, info.sample_bytes, info.palette) == (14, 12, b"") and zlib.decompress(info.idat)[0] == 1
    # several IDAT chunks, zero-length ones included, ancillary chunks everywhere, PLTE in a truecolour file
    cut = small_png(idat_splits=(0, 1, 1, 7), before_idat=[(b"gAMA", struct.pack(">I", 45455)), (b"PLTE", bytes(12)),
                                                        (b"tRNS", bytes(6))], after_idat=[(b"tEXt", b"k\x00v")])
    assert [k for k, _ in ref.chunks(cut)].count(b"IDAT") == 5
    assert png.parse_png(cut, "b.png") == info
    pal = png.parse_png(PALETTE, "c.png")
    assert (pal.colour_type, pal.bit_depth, pal.palette, pal.bpp) == (3, 1, bytes(6), 1)
    assert png.inflate_host(info, "a.png") == zlib.decompress(info.idat)
    from acimg.convert import ConvertError
    short = with_ihdr(small_png(), height=3)
    with pytest.raises(ConvertError, match=r"tall.png: the IDAT stream inflates to 14 bytes, IHDR implies 21"):
        png.inflate_host(png.parse_png(short, "tall.png"), "tall.png")


def test_parse_png_agrees_with_the_restatement_on_every_case():
    from acimg import _lib, png
    L = _lib.load()
    for name, data in png_cases.files().items():
        info, hdr = png.parse_png(data, name), ref.png_header(data)
        geo = (hdr.height, hdr.width, hdr.colour_type, hdr.bit_depth, hdr.interlace)
        assert (info.height, info.width, info.colour_type, info.bit_depth, info.interlace) == geo, name
        assert info.idat == hdr.idat and info.palette == hdr.palette
        assert (info.inflated_bytes, info.sample_bytes, 3 * info.height * info.width) == ref.sizes(*geo), name
        assert info.inflated_bytes == len(zlib.decompress(info.idat)), name
        assert [tuple(r[:5]) for r in png.job_rows(info)] == ref.job_table(*geo), name
        assert int(L.acimg_png_inflated_bytes(*geo)) == info.inflated_bytes, name
        assert int(L.acimg_png_sample_bytes(*geo)) == info.sample_bytes, name


@pytest.mark.parametrize("h,w", [(1, 1), (1, 9), (9, 1), (2, 2), (3, 5), (5, 3), (8, 8), (9, 9)])
def test_job_tables_of_interlaced_images(h, w):
    """height x width; passes without a row or a column are omitted (1 x 1 is one job), for all 15 forms"""
    from acimg import png
    present = {(1, 1): [0], (1, 9): [0, 1, 3, 5], (9, 1): [0, 2, 4, 6], (2, 2): [0, 5, 6], (3, 5): [0, 1, 3, 4, 5, 6],
               (5, 3): [0, 2, 3, 4, 5, 6], (8, 8): list(range(7)), (9, 9): list(range(7))}[(h, w)]
    for ct, depth in ref.FORMS:
        s = np.zeros((h, w, png_writer.CHANNELS[ct]), np.uint16)
        info = png.parse_png(png_writer.write_png(s, ct, depth, 0, 1, palette=bytes(3) if ct == 3 else None), "x.png")
        assert [p.index for p in info.passes] == present
        rows = png.job_rows(info, file_index=4, src_base=1000, dst_base=500)
        want = ref.job_table(h, w, ct, depth, 1)
        assert rows == [[1000 + s_, 500 + d, r, rb, bpp, 4] for s_, d, r, rb, bpp in want]
        assert sum(p.rows * p.cols for p in info.passes) == h * w               # every pixel lies in exactly one pass
        assert all(rb % bpp == 0 for _, _, _, rb, bpp in want)


def test_size_queries_and_their_refusals():
    from acimg import _lib
    L = _lib.load()
    assert int(L.acimg_png_inflated_bytes(224, 298, 2, 8, 0)) == 224 * (1 + 894)
    assert int(L.acimg_png_sample_bytes(224, 298, 2, 8, 0)) == 224 * 894
    assert int(L.acimg_png_pixel_bytes(224, 298)) == 224 * 298 * 3
    assert int(L.acimg_png_inflated_bytes(3, 5, 0, 1, 1)) == 2 + 2 + 2 + 2 + 4 + 2       # passes 0, 1, 3, 4, 5, 6 of 5 wide, 3 high
    assert int(L.acimg_png_sample_bytes(1, 9, 6, 16, 0)) == 72 and int(L.acimg_png_sample_bytes(1, 9, 0, 1, 0)) == 2
    for ct, depth in ref.FORMS:
        for lace in (0, 1):
            for h, w in ((1, 1), (7, 9), (65, 3)):
                want = ref.sizes(h, w, ct, depth, lace)
                got = (int(L.acimg_png_inflated_bytes(h, w, ct, depth, lace)), int(L.acimg_png_sample_bytes(h, w, ct, depth, lace)),
                       int(L.acimg_png_pixel_bytes(h, w)))
                assert got == want, (h, w, ct, depth, lace)
    for bad in ((0, 8, 2, 8, 0), (8, 0, 2, 8, 0), (-1, 8, 2, 8, 0), (8, 8, 1, 8, 0), (8, 8, 5, 8, 0), (8, 8, 2, 4, 0),
                (8, 8, 3, 16, 0), (8, 8, 4, 4, 0), (8, 8, 0, 3, 0), (8, 8, 2, 8, 2), (8, 8, 2, 8, -1), (65536, 65536, 2, 8, 0),
                (46341, 46341, 0, 8, 1)):
        assert int(L.acimg_png_inflated_bytes(*bad)) == 0 and int(L.acimg_png_sample_bytes(*bad)) == 0, bad
    assert int(L.acimg_png_inflated_bytes(46340, 46340, 0, 8, 0)) == 46340 * 46341
    assert int(L.acimg_png_pixel_bytes(0, 8)) == 0 and int(L.acimg_png_pixel_bytes(8, -2)) == 0
    assert int(L.acimg_png_pixel_bytes(26755, 26755)) == 0 and int(L.acimg_png_pixel_bytes(26754, 26754)) == 3 * 26754 ** 2
    assert int(L.acimg_png_unfilter_workspace(0)) == 0 and int(L.acimg_png_unfilter_workspace(3)) == 144
    assert int(L.acimg_png_pixels_workspace(0)) == 0 and int(L.acimg_png_pixels_workspace(3)) == 224
