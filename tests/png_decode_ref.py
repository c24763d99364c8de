"""NumPy restatement of the PNG reader (acimg/png.py, csrc/png_decode.hip), the stages separate: the chunk walk, inflate
by zlib, the scanline filters of RFC 2083 section 6 undone byte by byte, the Adam7 gather into a sample array, and the
pixel rule of `cv2.imread` (libpng's transforms as OpenCV sets them for IMREAD_COLOR): palette through PLTE, grey of 1 /
2 / 4 bits times 255 / 85 / 17, the high byte of 16-bit samples, grey replicated, alpha dropped, B G R.  Written from the
specification, it shares no code with acimg/png.py.  `unfilter` can count what it meets (tests/png_census.py)."""
import collections
import os
import struct
import zlib

import numpy as np

SIGNATURE = b"\x89PNG\r\n\x1a\n"
CHANNELS = {0: 1, 2: 3, 3: 1, 4: 2, 6: 4}
FORMS = [(0, d) for d in (1, 2, 4, 8, 16)] + [(2, 8), (2, 16)] + [(3, d) for d in (1, 2, 4, 8)] + [(4, 8), (4, 16), (6, 8), (6, 16)]
ADAM7_X = ((0, 8), (4, 8), (0, 4), (2, 4), (0, 2), (1, 2), (0, 1))        # origin, step per pass
ADAM7_Y = ((0, 8), (0, 8), (4, 8), (0, 4), (2, 4), (0, 2), (1, 2))
BAD_FILTER, BAD_INDEX = 1, 2
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "png_decode_golden.npz")

Header = collections.namedtuple("Header", "height width colour_type bit_depth interlace palette idat chunks")
Pass = collections.namedtuple("Pass", "index rows cols row_bytes")


def chunks(data):
    """[(kind, body)] of a file whose CRCs hold"""
    assert data[:8] == SIGNATURE
    out, pos = [], 8
    while pos < len(data):
        length, kind = struct.unpack_from(">I4s", data, pos)
        body = data[pos + 8:pos + 8 + length]
        assert zlib.crc32(kind + body) & 0xFFFFFFFF == struct.unpack_from(">I", data, pos + 8 + length)[0], kind
        out.append((kind, body))
        pos += 12 + length
    return out


def png_header(data):
    ch = chunks(data)
    w, h, depth, ctype, comp, filt, lace = struct.unpack(">IIBBBBB", ch[0][1])
    assert ch[0][0] == b"IHDR" and comp == 0 and filt == 0 and (ctype, depth) in FORMS
    plte = [b for k, b in ch if k == b"PLTE"]
    return Header(h, w, ctype, depth, lace, plte[0] if plte else b"", b"".join(b for k, b in ch if k == b"IDAT"), ch)


def bpp_of(colour_type, bit_depth):
    return max(1, CHANNELS[colour_type] * bit_depth // 8)


def passes(height, width, colour_type, bit_depth, interlace):
    """the passes that have a row and a column, in stream order"""
    bits = CHANNELS[colour_type] * bit_depth
    out = []
    if not interlace:
        return [Pass(0, height, width, (width * bits + 7) // 8)]
    for p in range(7):
        (x0, dx), (y0, dy) = ADAM7_X[p], ADAM7_Y[p]
        cols = len(range(x0, width, dx))
        rows = len(range(y0, height, dy))
        if rows and cols:
            out.append(Pass(p, rows, cols, (cols * bits + 7) // 8))
    return out


def sizes(height, width, colour_type, bit_depth, interlace):
    """(inflated bytes, reconstructed bytes, pixel bytes)"""
    ps = passes(height, width, colour_type, bit_depth, interlace)
    return sum(p.rows * (p.row_bytes + 1) for p in ps), sum(p.rows * p.row_bytes for p in ps), 3 * height * width


def job_table(height, width, colour_type, bit_depth, interlace):
    """[(src_off, dst_off, rows, row_bytes, bpp)] per pass: what acimg_png_unfilter's job rows hold for one file"""
    out, src, dst = [], 0, 0
    for p in passes(height, width, colour_type, bit_depth, interlace):
        out.append((src, dst, p.rows, p.row_bytes, bpp_of(colour_type, bit_depth)))
        src += p.rows * (p.row_bytes + 1)
        dst += p.rows * p.row_bytes
    return out


def inflate_idat(hdr):
    raw = zlib.decompress(hdr.idat)
    assert len(raw) == sizes(hdr.height, hdr.width, hdr.colour_type, hdr.bit_depth, hdr.interlace)[0]
    return raw


def paeth(a, b, c):
    """-> (the predictor, which of 'a', 'b', 'c' it is, the tie that was broken or None)"""
    p = a + b - c
    pa, pb, pc = abs(p - a), abs(p - b), abs(p - c)
    if pa <= pb and pa <= pc:
        tie = "a=b=c" if pa == pb == pc else "a=b" if pa == pb else "a=c" if pa == pc else None
        return a, "a", tie
    if pb <= pc:
        return b, "b", "b=c" if pb == pc else None
    return c, "c", None


def unfilter_rows(raw, rows, row_bytes, bpp, census=None, band=64):
    """the rows * (1 + row_bytes) bytes of one pass -> (uint8 [rows, row_bytes], status).  A filter byte above 4 gives
    BAD_FILTER and that row is taken as filter 0."""
    src = np.frombuffer(raw, np.uint8).reshape(rows, row_bytes + 1)
    out = np.zeros((rows, row_bytes), np.int64)
    status = 0
    for r in range(rows):
        ft = int(src[r, 0])
        line = src[r, 1:].astype(np.int64)
        up = out[r - 1] if r else np.zeros(row_bytes, np.int64)
        if census is not None:
            census["filter %d on a %s row" % (ft, "first" if r == 0 else "later")] += 1
            if r and r % band == 0:
                census["band edge crossed with filter %d" % ft] += 1
        if ft > 4:
            status, ft = BAD_FILTER, 0
        if ft == 0:
            out[r] = line
        elif ft == 2:
            out[r] = (line + up) & 255
        else:
            cur = out[r]
            for x in range(row_bytes):
                a = int(cur[x - bpp]) if x >= bpp else 0
                b = int(up[x])
                c = int(up[x - bpp]) if x >= bpp and r else 0
                if ft == 1:
                    pred = a
                elif ft == 3:
                    pred = (a + b) >> 1
                    if census is not None and a + b >= 256:
                        census["average with a sum of 256 or more"] += 1
                else:
                    pred, which, tie = paeth(a, b, c)
                    if census is not None:
                        census["paeth chooses " + which] += 1
                        if tie:
                            census["paeth tie " + tie] += 1
                if census is not None and line[x] + pred >= 256:
                    census["sum wraps"] += 1
                cur[x] = (int(line[x]) + pred) & 255
    return out.astype(np.uint8), status


def unfilter(raw, hdr, census=None):
    """the inflated stream -> (the reconstructed bytes of every pass, back to back; status)"""
    out, at, status = [], 0, 0
    bpp = bpp_of(hdr.colour_type, hdr.bit_depth)
    for p in passes(hdr.height, hdr.width, hdr.colour_type, hdr.bit_depth, hdr.interlace):
        n = p.rows * (p.row_bytes + 1)
        rows, st = unfilter_rows(raw[at:at + n], p.rows, p.row_bytes, bpp, census)
        out.append(rows.reshape(-1))
        status = status or st
        at += n
    assert at == len(raw)
    return np.concatenate(out), status


def unpack_row_samples(rows, cols, channels, depth):
    """uint8 [rows, row_bytes] -> uint16 [rows, cols, channels]"""
    if depth == 8:
        return rows.reshape(rows.shape[0], cols, channels).astype(np.uint16)
    if depth == 16:
        b = rows.reshape(rows.shape[0], cols, channels, 2).astype(np.uint16)
        return (b[..., 0] << 8) | b[..., 1]
    bits = np.unpackbits(rows, axis=1)[:, :cols * depth].reshape(rows.shape[0], cols, depth)       # MSB first
    weights = (1 << np.arange(depth - 1, -1, -1)).astype(np.uint16)
    return (bits * weights).sum(axis=2).astype(np.uint16)[..., None]


def gather(samples, hdr):
    """the reconstructed bytes -> uint16 [H, W, channels], Adam7 passes put back in place"""
    ch = CHANNELS[hdr.colour_type]
    img = np.zeros((hdr.height, hdr.width, ch), np.uint16)
    at = 0
    for p in passes(hdr.height, hdr.width, hdr.colour_type, hdr.bit_depth, hdr.interlace):
        n = p.rows * p.row_bytes
        part = unpack_row_samples(np.asarray(samples[at:at + n]).reshape(p.rows, p.row_bytes), p.cols, ch, hdr.bit_depth)
        at += n
        if hdr.interlace:
            (x0, dx), (y0, dy) = ADAM7_X[p.index], ADAM7_Y[p.index]
            img[y0::dy, x0::dx] = part
        else:
            img[:] = part
    assert at == len(samples)
    return img


def pixels(img, hdr):
    """uint16 [H, W, channels] -> (uint8 [H, W, 3] B G R, status)"""
    ct, depth = hdr.colour_type, hdr.bit_depth
    status = 0
    if ct == 3:
        pal = np.frombuffer(hdr.palette, np.uint8).reshape(-1, 3)
        idx = img[..., 0].astype(np.int64)
        bad = idx >= len(pal)
        if bad.any():
            status = BAD_INDEX
        rgb = np.concatenate([pal, np.zeros((1, 3), np.uint8)])[np.where(bad, len(pal), idx)]
    else:
        v = img
        if depth == 16:
            v = v >> 8
        elif depth < 8:
            v = v * {1: 255, 2: 85, 4: 17}[depth]
        v = v.astype(np.uint8)
        rgb = np.repeat(v[..., :1], 3, axis=2) if ct in (0, 4) else v[..., :3]
    return np.ascontiguousarray(rgb[..., ::-1]), status


def decode_png(data, census=None):
    """a whole file -> (reconstructed bytes, B G R pixels, status), stage after stage"""
    hdr = png_header(data)
    samples, st = unfilter(inflate_idat(hdr), hdr, census)
    bgr, st2 = pixels(gather(samples, hdr), hdr)
    return samples, bgr, st or st2


def load_png_golden():
    """tests/golden/png_decode_golden.npz -> {name: (file bytes, Pillow's pixels as uint8 [H, W, 3] B G R, written by:
    'pillow' or 'writer')}, in file order; read-only"""
    z = np.load(GOLDEN)
    out = collections.OrderedDict()
    for name, origin in zip(z["names"].tolist(), z["origins"].tolist()):
        px = z["pixels_" + name]
        bgr = np.ascontiguousarray(px[::-1].transpose(1, 2, 0))
        bgr.setflags(write=False)
        out[name] = (z["png_" + name].tobytes(), bgr, origin)
    return out
