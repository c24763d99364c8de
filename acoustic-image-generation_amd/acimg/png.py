"""A PNG writer on the standard library alone (zlib + struct): 8-bit RGB, colour type 2, no interlace, every scanline
with filter 0, one IDAT chunk.  It is what `python -m acimg.show` saves its frames with - no PIL, imageio or cv2."""
import struct
import zlib

import numpy as np

SIGNATURE = b"\x89PNG\r\n\x1a\n"


def _chunk(kind, data):
    return struct.pack(">I", len(data)) + kind + data + struct.pack(">I", zlib.crc32(kind + data) & 0xFFFFFFFF)


def encode_png(rgb_uint8, level=6, deflater=None):
    """[H,W,3] uint8 -> the bytes of a PNG file; `deflater` (an acimg.deflate.DeviceDeflater) compresses the scanlines on
    the device instead of zlib at `level`"""
    a = np.asarray(rgb_uint8)
    if a.dtype != np.uint8 or a.ndim != 3 or a.shape[2] != 3 or a.shape[0] < 1 or a.shape[1] < 1:
        raise ValueError("write_png wants a [H,W,3] uint8 array, got %s %s" % (a.dtype, a.shape))
    h, w = a.shape[:2]
    rows = np.zeros((h, 1 + 3 * w), np.uint8)            # filter byte 0 in front of every scanline
    rows[:, 1:] = a.reshape(h, 3 * w)
    ihdr = struct.pack(">IIBBBBB", w, h, 8, 2, 0, 0, 0)
    idat = deflater.zlib(rows.tobytes()) if deflater is not None else zlib.compress(rows.tobytes(), int(level))
    return SIGNATURE + _chunk(b"IHDR", ihdr) + _chunk(b"IDAT", idat) + _chunk(b"IEND", b"")


def encode_png_many(frames, deflater):
    """uint8 [n,H,W,3] (a device tensor, or an array) -> the bytes of n PNG files, each what
    `encode_png(frame, deflater=deflater)` gives.  The filter-0 scanlines are formed on the device, every frame is
    deflated in ONE call and its Adler-32 comes from the device (`DeviceDeflater.zlib_many`); the chunk CRCs over the
    small compressed streams are the host's."""
    import torch
    f = torch.as_tensor(frames)
    if f.dtype != torch.uint8 or f.dim() != 4 or f.shape[3] != 3 or f.shape[1] < 1 or f.shape[2] < 1:
        raise ValueError("encode_png_many wants a [n,H,W,3] uint8 tensor, got %s %s" % (f.dtype, tuple(f.shape)))
    n, h, w = int(f.shape[0]), int(f.shape[1]), int(f.shape[2])
    if n == 0:
        return []
    rows = torch.zeros(n, h, 1 + 3 * w, dtype=torch.uint8, device=deflater.device)     # filter byte 0, then the scanline
    rows[:, :, 1:] = f.to(deflater.device).reshape(n, h, 3 * w)
    ihdr = _chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, 2, 0, 0, 0))
    return [SIGNATURE + ihdr + _chunk(b"IDAT", idat) + _chunk(b"IEND", b"") for idat in deflater.zlib_many(list(rows))]


def write_png(path, rgb_uint8, level=6, deflater=None):
    data = encode_png(rgb_uint8, level, deflater)
    with open(path, "wb") as f:
        f.write(data)
    return len(data)
