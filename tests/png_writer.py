"""A PNG writer for the tests: any of the 15 colour-type / bit-depth forms, a filter chosen per row, Adam7, the IDAT payload
cut at given points (zero-length chunks included) and extra chunks - what Pillow cannot write (it never interlaces and
picks its own filters).  The samples are given, so a decoder is held to what went in, not to another decoder."""
import struct
import zlib

import numpy as np

SIGNATURE = b"\x89PNG\r\n\x1a\n"
CHANNELS = {0: 1, 2: 3, 3: 1, 4: 2, 6: 4}
ADAM7 = ((0, 0, 8, 8), (4, 0, 8, 8), (0, 4, 4, 8), (2, 0, 4, 4), (0, 2, 2, 4), (1, 0, 2, 2), (0, 1, 1, 2))     # x0, y0, dx, dy


def chunk(kind, body=b""):
    return struct.pack(">I", len(body)) + kind + body + struct.pack(">I", zlib.crc32(kind + body) & 0xFFFFFFFF)


def pack_rows(samples, depth):
    """uint16 [rows, cols, channels] -> uint8 [rows, row_bytes]: MSB first, rows padded to a byte, 16 bits big-endian"""
    s = np.asarray(samples, np.uint16)
    rows = s.shape[0]
    if depth == 16:
        return np.stack([s >> 8, s & 255], axis=-1).astype(np.uint8).reshape(rows, -1)
    if depth == 8:
        return s.astype(np.uint8).reshape(rows, -1)
    flat = s.reshape(rows, -1)
    bits = ((flat[..., None] >> np.arange(depth - 1, -1, -1)) & 1).astype(np.uint8).reshape(rows, -1)
    return np.packbits(bits, axis=1)


def filter_row(ft, line, up, bpp):
    """the filtered bytes of one row (RFC 2083 section 6.2); a type above 4 is written with the bytes of type 0"""
    line, up = line.astype(np.int64), up.astype(np.int64)
    left = np.concatenate([np.zeros(bpp, np.int64), line[:-bpp]])[:line.size]
    upleft = np.concatenate([np.zeros(bpp, np.int64), up[:-bpp]])[:line.size]
    if ft == 1:
        pred = left
    elif ft == 2:
        pred = up
    elif ft == 3:
        pred = (left + up) >> 1
    elif ft == 4:
        p = left + up - upleft
        pa, pb, pc = np.abs(p - left), np.abs(p - up), np.abs(p - upleft)
        pred = np.where((pa <= pb) & (pa <= pc), left, np.where(pb <= pc, up, upleft))
    else:
        pred = np.zeros_like(line)
    return ((line - pred) & 255).astype(np.uint8)


def scanlines(samples, colour_type, depth, filters=0, interlace=0):
    """-> the bytes the IDAT stream inflates to.  filters: one type, or a sequence indexed by the running row number over
    all passes (cycled)."""
    s = np.asarray(samples, np.uint16)
    if s.ndim == 2:
        s = s[..., None]
    assert s.shape[2] == CHANNELS[colour_type], (s.shape, colour_type)
    bpp = max(1, CHANNELS[colour_type] * depth // 8)
    kinds = [filters] if isinstance(filters, int) else list(filters)
    out, n = [], 0
    for x0, y0, dx, dy in (ADAM7 if interlace else ((0, 0, 1, 1),)):
        part = s[y0::dy, x0::dx]
        if part.shape[0] == 0 or part.shape[1] == 0:
            continue
        rows = pack_rows(part, depth)
        up = np.zeros(rows.shape[1], np.uint8)
        for line in rows:
            ft = kinds[n % len(kinds)]
            out.append(bytes([ft]) + filter_row(ft, line, up, bpp).tobytes())
            up, n = line, n + 1
    return b"".join(out)


def assemble(raw, height, width, colour_type, depth, interlace=0, palette=None, idat_splits=(), before_idat=(), after_idat=(),
             between_idat=(), level=6, stream=None):
    """the file around the scanline bytes `raw` (or around the zlib stream `stream`, taken as it is)"""
    z = zlib.compress(raw, level) if stream is None else stream
    cuts = [0] + sorted(idat_splits) + [len(z)]
    parts = [SIGNATURE, chunk(b"IHDR", struct.pack(">IIBBBBB", width, height, depth, colour_type, 0, 0, interlace))]
    if palette is not None:
        parts.append(chunk(b"PLTE", bytes(palette)))
    parts += [chunk(k, b) for k, b in before_idat]
    for i, (a, b) in enumerate(zip(cuts[:-1], cuts[1:])):
        parts.append(chunk(b"IDAT", z[a:b]))
        if i == 0:
            parts += [chunk(k, body) for k, body in between_idat]
    parts += [chunk(k, b) for k, b in after_idat]
    parts.append(chunk(b"IEND"))
    return b"".join(parts)


def write_png(samples, colour_type, depth, filters=0, interlace=0, palette=None, **kw):
    s = np.asarray(samples)
    return assemble(scanlines(s, colour_type, depth, filters, interlace), s.shape[0], s.shape[1], colour_type, depth, interlace,
                    palette, **kw)
