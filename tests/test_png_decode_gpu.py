"""PNG decoding on the device: `acimg_png_unfilter` and `acimg_png_pixels` through the raw C ABI with every operand inside
guard bands, outputs pre-filled with a sentinel, inputs checked unchanged; each stage against the restatement
(tests/png_decode_ref.py), the pixels against what went into the writer and against Pillow's pixels of the committed
fixture.  One launch of many files of different geometry; a filter byte of 5 and a palette index beyond PLTE in one file
of a launch; `PngDecoder` with the inflate on the device against the host's, and the fallback to zlib."""
import ctypes as C
import os
import sys
import zlib

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import png_cases  # noqa: E402
import png_decode_ref as ref  # noqa: E402
import png_writer  # noqa: E402
from guard_arena import GuardArena  # noqa: E402

pytestmark = pytest.mark.gpu

SENT = 0x7B


@pytest.fixture(scope="module")
def golden():
    return ref.load_png_golden()


@pytest.fixture(scope="module")
def restated():
    """name -> (reconstructed bytes, B G R pixels) of the restatement for every case; never modified"""
    out = {}
    for name, data in png_cases.files().items():
        samples, bgr, status = ref.decode_png(data)
        assert status == 0
        samples.setflags(write=False)
        bgr.setflags(write=False)
        out[name] = (samples, bgr)
    return out


def device_png(device, files, what="", raws=None):
    """ONE launch of each kernel on `files` (any geometries) -> ([reconstructed bytes per file], [B G R pixels per file],
    status after the first stage, status after the second) as host arrays.  raws: the inflated streams when they are not
    what zlib gives.  Inputs and outputs lie in one guard arena, the outputs are pre-filled with a sentinel, the bands are
    checked after each stage and the inputs compared with what was uploaded."""
    from acimg import _lib, ops, png
    L = _lib.load()
    infos = [png.parse_png(f, "%s[%d]" % (what, i)) for i, f in enumerate(files)]
    raws = raws or [zlib.decompress(g.idat) for g in infos]
    n = len(files)
    jobs, table, s_at, d_at, o_at, p_at = [], [], 0, 0, 0, 0
    for i, g in enumerate(infos):
        geo = (g.height, g.width, g.colour_type, g.bit_depth, g.interlace)
        assert len(raws[i]) == int(L.acimg_png_inflated_bytes(*geo)) == g.inflated_bytes
        assert int(L.acimg_png_sample_bytes(*geo)) == g.sample_bytes
        assert int(L.acimg_png_pixel_bytes(g.height, g.width)) == 3 * g.height * g.width
        jobs += png.job_rows(g, i, s_at, d_at)
        table.append([d_at, g.height, g.width, g.colour_type, g.bit_depth, g.interlace, p_at, len(g.palette) // 3, o_at])
        s_at, d_at, o_at, p_at = s_at + g.inflated_bytes, d_at + g.sample_bytes, o_at + 3 * g.height * g.width, p_at + len(g.palette)
    src = np.frombuffer(b"".join(raws), np.uint8)
    pal = np.frombuffer(b"".join(g.palette for g in infos), np.uint8)
    ws_bytes = max(int(L.acimg_png_unfilter_workspace(len(jobs))), int(L.acimg_png_pixels_workspace(n)))
    arena = GuardArena.for_sizes(device, [src.nbytes, pal.nbytes, d_at, o_at, 4 * n, ws_bytes])
    r_src, r_pal = arena.region(src.nbytes, name="src"), arena.region(pal.nbytes, name="palette")
    r_src.u8.copy_(torch.from_numpy(src.copy()))
    if pal.nbytes:
        r_pal.u8.copy_(torch.from_numpy(pal.copy()))
    r_samples = arena.region(d_at, fill=SENT, name="samples")
    r_pixels = arena.region(o_at, fill=SENT, name="pixels")
    r_status = arena.region(4 * n, fill=SENT, name="status")
    r_ws = arena.region(ws_bytes, fill=SENT, name="ws")
    st = ops.current_stream_handle(device)
    flat = [int(v) for row in jobs for v in row]
    rc = L.acimg_png_unfilter(r_src.ptr, src.nbytes, (C.c_long * len(flat))(*flat), len(jobs), n, r_samples.ptr, d_at, r_status.ptr,
                              r_ws.ptr, ws_bytes, st)
    assert rc == 0, _lib.last_error()
    torch.cuda.synchronize(device)
    arena.check(what + " unfilter")
    assert (r_pixels.u8 == SENT).all(), what
    status1 = r_status.u8.cpu().numpy().view(np.int32).copy()
    samples = r_samples.u8.cpu().numpy()
    flat = [int(v) for row in table for v in row]
    rc = L.acimg_png_pixels(r_samples.ptr, d_at, (C.c_long * len(flat))(*flat), n, r_pal.ptr if pal.nbytes else None, pal.nbytes,
                            r_pixels.ptr, o_at, r_status.ptr, r_ws.ptr, ws_bytes, st)
    assert rc == 0, _lib.last_error()
    torch.cuda.synchronize(device)
    arena.check(what + " pixels")
    assert np.array_equal(r_samples.u8.cpu().numpy(), samples), "%s: the samples were written by the pixel stage" % what
    assert np.array_equal(r_src.u8.cpu().numpy(), src), "%s: the inflated streams were written" % what
    assert np.array_equal(r_pal.u8.cpu().numpy(), pal), "%s: the palettes were written" % what
    pixels = r_pixels.u8.cpu().numpy()
    status2 = r_status.u8.cpu().numpy().view(np.int32).copy()
    per_s, per_p, d_at, o_at = [], [], 0, 0
    for g in infos:
        per_s.append(samples[d_at:d_at + g.sample_bytes])
        per_p.append(pixels[o_at:o_at + 3 * g.height * g.width].reshape(g.height, g.width, 3))
        d_at, o_at = d_at + g.sample_bytes, o_at + 3 * g.height * g.width
    return per_s, per_p, status1, status2


def assert_file(got, k, want_samples, want_pixels, name, others=()):
    per_s, per_p, status1, status2 = got
    assert status1[k] == 0 and status2[k] == 0, "%s: status %d, %d" % (name, status1[k], status2[k])
    pairs = [("reconstructed bytes", per_s[k], want_samples), ("pixels", per_p[k], want_pixels)] + [
        ("pixels against " + label, per_p[k], w) for label, w in others]
    for stage, g, w in pairs:
        bad = np.flatnonzero(np.asarray(g).reshape(-1) != np.asarray(w).reshape(-1)) if g.shape == w.shape else None
        assert bad is not None and bad.size == 0, "%s: %s differ at %s of %d places, first at %s" % (
            name, stage, "all" if bad is None else bad.size, w.size, None if bad is None else bad[0])


# ---- the two stages ---------------------------------------------------------------------------------------------------------
def test_every_case_alone_stage_by_stage(device, restated):
    """every width, height, filter, form and Adam7 size of tests/png_cases.py, one file per launch"""
    for name, data in png_cases.files().items():
        got = device_png(device, [data], name)
        assert_file(got, 0, restated[name][0], restated[name][1], name,
                    [("the samples the writer was given", png_cases.expected_pixels(png_cases.named_cases()[name]))])


def test_every_case_in_one_launch_and_twice_the_same(device, restated):
    names = list(png_cases.files())
    files = [png_cases.files()[n] for n in names]
    a = device_png(device, files, "all cases")
    for k, name in enumerate(names):
        assert_file(a, k, restated[name][0], restated[name][1], name)
    b = device_png(device, files, "all cases again")
    assert all(np.array_equal(x, y) for x, y in zip(a[0] + a[1], b[0] + b[1]))


def test_every_fixture_file_against_pillow(device, golden):
    names = list(golden)
    got = device_png(device, [golden[n][0] for n in names], "fixture")
    for k, name in enumerate(names):
        samples, bgr, status = ref.decode_png(golden[name][0])
        assert status == 0
        assert_file(got, k, samples, bgr, name, [("Pillow", golden[name][1])])


FIVE = ("rows65_random", "adam7_53x37_rgb8", "rows129_w65_rgba16", "sub_c3d2_w9", "form_c0d16")


def test_filter_byte_of_5_in_the_third_file_of_five(device, restated):
    """five files of different geometry in one launch; row 70 of the third's 129 holds filter byte 5: its status is set,
    nothing leaves its extent (the files beside it are exact, the bands clean), every other file is exact"""
    from acimg import png
    files = [png_cases.files()[n] for n in FIVE]
    raws = [zlib.decompress(png.parse_png(f).idat) for f in files]
    info = png.parse_png(files[2])
    bad = bytearray(raws[2])
    bad[70 * (info.passes[0].row_bytes + 1)] = 5
    raws[2] = bytes(bad)
    got = device_png(device, files, "filter 5", raws=raws)
    print("status after unfilter %s, after pixels %s" % (got[2].tolist(), got[3].tolist()))
    assert got[2].tolist() == [0, 0, ref.BAD_FILTER, 0, 0] and got[3].tolist() == got[2].tolist()
    for k, name in enumerate(FIVE):
        if k != 2:
            assert_file(got, k, restated[name][0], restated[name][1], name)
    above = 70 * info.passes[0].row_bytes                     # the rows above the bad one do not depend on it
    assert np.array_equal(got[0][2][:above], restated[FIVE[2]][0][:above])
    hdr = ref.png_header(files[2])
    want, st = ref.unfilter(raws[2], hdr)
    assert st == ref.BAD_FILTER and np.array_equal(got[0][2], want), "the stated choice: such a row is taken as filter 0"


def test_palette_index_beyond_plte_sets_the_status_of_that_file_alone(device, restated):
    case = png_cases.named_cases()["palette_short"]                # 5 entries at depth 8
    s = case.samples.copy()
    s[1, 3, 0], s[3, 8, 0] = 5, 255                          # the first index beyond PLTE, and the last there is
    bad = png_writer.write_png(s, 3, 8, case.filters, 0, case.palette)
    lace = png_writer.write_png(s, 3, 8, case.filters, 1, case.palette)
    names = ["palette_short", "form_c3d1", None, "sub_c3d4_w9", None]
    files = [png_cases.files()[n] if n else (bad if k == 2 else lace) for k, n in enumerate(names)]
    got = device_png(device, files, "bad index")
    assert got[2].tolist() == [0] * 5 and got[3].tolist() == [0, 0, ref.BAD_INDEX, 0, ref.BAD_INDEX]
    for k, name in enumerate(names):
        if name:
            assert_file(got, k, restated[name][0], restated[name][1], name)
        else:
            _, want, st = ref.decode_png(files[k])
            assert st == ref.BAD_INDEX and np.array_equal(got[1][k], want)
            assert got[1][k][1, 3].tolist() == [0, 0, 0] and got[1][k][3, 8].tolist() == [0, 0, 0]


def test_the_pixel_stage_keeps_the_first_stages_verdict(device):
    """status is in / out for acimg_png_pixels: it stores ACIMG_PNG_BAD_INDEX and nothing else"""
    s = np.zeros((3, 4, 3), np.uint16)
    data = png_writer.write_png(s, 2, 8, (0, 5, 0))
    got = device_png(device, [data, png_cases.files()["planted"]], "verdict kept")
    assert got[2].tolist() == [ref.BAD_FILTER, 0] and got[3].tolist() == [ref.BAD_FILTER, 0]


def test_refusals_before_any_launch(device):
    from acimg import _lib
    L = _lib.load()
    buf = torch.zeros(65536, dtype=torch.uint8, device=device)
    p = buf.data_ptr()

    def unfilter(job, src=p, src_bytes=4096, njobs=1, nfiles=1, dst_bytes=4096, ws=p + 32768, ws_bytes=4096):
        return L.acimg_png_unfilter(src, src_bytes, (C.c_long * 6)(*job), njobs, nfiles, p + 8192, dst_bytes, p + 16384, ws, ws_bytes, None)

    good = (0, 0, 4, 12, 3, 0)
    assert unfilter(good, src=None) == -1 and "null" in _lib.last_error()
    assert unfilter(good, njobs=0) == -1 and unfilter(good, nfiles=0) == -1
    assert unfilter(good, ws=p + 32772) == -1 and "aligned" in _lib.last_error()
    assert unfilter(good, ws_bytes=47) == -2
    for job, text in (((0, 0, 4, 12, 5, 0), "filter unit of 5"), ((0, 0, 4, 12, 0, 0), "filter unit of 0"),
                      ((0, 0, 0, 12, 3, 0), "0 rows"), ((0, 0, 4, 0, 3, 0), "rows of 0 bytes"), ((0, 0, 4, 13, 3, 0), "unit 3"),
                      ((0, 0, 4, 12, 3, 1), "names file 1 of 1"), ((0, 0, 4, 12, 3, -1), "names file -1"),
                      ((4045, 0, 4, 12, 3, 0), "reads 52 bytes at 4045 of 4096"), ((-1, 0, 4, 12, 3, 0), "reads"),
                      ((0, 4049, 4, 12, 3, 0), "writes 48 bytes at 4049 of 4096"), ((0, -1, 4, 12, 3, 0), "writes")):
        assert unfilter(job) == -1 and text in _lib.last_error(), (job, _lib.last_error())
    assert unfilter((4044, 4048, 4, 12, 3, 0)) == 0                       # the last job that fits

    def pixels(row, samples=p, sample_bytes=4096, nfiles=1, pal=p + 4096, pal_bytes=768, out_bytes=4096, ws_bytes=4096):
        return L.acimg_png_pixels(samples, sample_bytes, (C.c_long * 9)(*row), nfiles, pal, pal_bytes, p + 8192, out_bytes, p + 16384,
                                  p + 32768, ws_bytes, None)

    fine = (0, 4, 4, 2, 8, 0, 0, 0, 0)
    assert pixels(fine, samples=None) == -1 and pixels(fine, nfiles=0) == -1 and pixels(fine, nfiles=65536) == -1
    assert pixels(fine, ws_bytes=71) == -2
    for row, text in (((0, 0, 4, 2, 8, 0, 0, 0, 0), "is 0 x 4"), ((0, 4, 4, 2, 4, 0, 0, 0, 0), "no PNG form"),
                      ((0, 4, 4, 5, 8, 0, 0, 0, 0), "no PNG form"), ((0, 4, 4, 2, 8, 2, 0, 0, 0), "no PNG form"),
                      ((4049, 4, 4, 2, 8, 0, 0, 0, 0), "reads 48 bytes at 4049"), ((0, 4, 4, 2, 8, 0, 0, 0, 4049), "writes 48 bytes at 4049"),
                      ((0, 4, 4, 3, 8, 0, 0, 0, 0), "palette of 0 entries"), ((0, 4, 4, 3, 8, 0, 0, 257, 0), "palette of 257 entries"),
                      ((0, 4, 4, 3, 8, 0, 1, 256, 0), "palette of 256 entries at 1 of 768")):
        assert pixels(row) == -1 and text in _lib.last_error(), (row, _lib.last_error())
    assert pixels((0, 4, 4, 3, 8, 0, 0, 0, 0), pal=None) == -1
    assert pixels((4048, 4, 4, 2, 8, 0, 0, 0, 4048)) == 0
    torch.cuda.synchronize(device)
    assert not buf[:32768].any()                          # only the two calls that fit ran, on zeros; their tables lie behind


# ---- PngDecoder -----------------------------------------------------------------------------------------------------------
MIXED = ("form_c6d16", "adam7_53x37_rgb8", "rows129_random", "sub_c0d1_w9", "adam7_9x65_p2", "planted", "bpp6_w65")


def test_decoder_with_the_inflate_on_the_device_gives_the_pixels_of_zlib(device, golden, restated):
    from acimg import png
    files = [png_cases.files()[n] for n in MIXED] + [golden[n][0] for n in golden]
    want = [restated[n][1] for n in MIXED] + [golden[n][1] for n in golden]
    host, dev = png.PngDecoder(device), png.PngDecoder(device, inflate="device")
    infos = [png.parse_png(f) for f in files]
    a, sa = host.decode_many(files, infos, inflated=[png.inflate_host(g) for g in infos])
    b, sb = dev.decode_many(files)
    assert sa.dtype == np.int32 and not sa.any() and not sb.any() and dev.fallbacks == 0
    for x, y, w in zip(a, b, want):
        assert x.device.type == "cuda" and x.dtype == torch.uint8 and tuple(x.shape) == w.shape
        assert np.array_equal(x.cpu().numpy(), w) and np.array_equal(y.cpu().numpy(), w)
    assert np.array_equal(png.decode_png(golden["pillow_rgba_37x53"][0], device), golden["pillow_rgba_37x53"][1])
    assert host.decode_many([])[0] == []


def test_corrupt_adler_trailer_ends_in_zlibs_own_error_through_the_fallback(device, restated):
    from acimg import png
    from acimg.convert import ConvertError
    good = png_cases.files()["rows65_random"]
    hdr = ref.png_header(good)
    z = bytearray(hdr.idat)
    z[-1] ^= 1
    case = png_cases.named_cases()["rows65_random"]
    bad = png_writer.assemble(b"", 65, 5, 2, 8, stream=bytes(z))
    dev = png.PngDecoder(device, inflate="device")
    with pytest.raises(zlib.error, match="incorrect data check"):
        dev.decode_many([png_cases.files()["planted"], bad])
    assert dev.fallbacks == 1
    with pytest.raises(zlib.error, match="incorrect data check"):
        png.PngDecoder(device).decode_many([bad])
    # a stream that is whole but of another size than IHDR implies: refused by name in both modes
    tall = png_writer.assemble(b"", 66, 5, 2, 8, stream=hdr.idat)
    for mode in png.INFLATE_CHOICES:
        with pytest.raises(ConvertError, match=r"tall.png: the IDAT stream inflates to 1040 bytes, IHDR implies 1056"):
            png.PngDecoder(device, inflate=mode).decode_many([tall], names=["tall.png"])
    # a stream with a full flush in its middle (an empty stored block, a byte-aligned restart) decodes as any other
    co = zlib.compressobj(6)
    raw = png_writer.scanlines(case.samples, 2, 8, case.filters)
    stream = co.compress(raw[:300]) + co.flush(zlib.Z_FULL_FLUSH) + co.compress(raw[300:]) + co.flush()
    flushed = png_writer.assemble(b"", 65, 5, 2, 8, stream=stream)
    pixels, status = dev.decode_many([flushed])
    assert not status.any() and np.array_equal(pixels[0].cpu().numpy(), restated["rows65_random"][1])
    with pytest.raises(ConvertError, match=r"five.png: corrupt PNG: a filter byte above 4"):
        png.decode_png(png_writer.write_png(np.zeros((3, 4, 3), np.uint16), 2, 8, (0, 5, 0)), device, "five.png")
