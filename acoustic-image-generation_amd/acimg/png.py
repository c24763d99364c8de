"""A PNG writer on the standard library alone (zlib + struct): 8-bit RGB, colour type 2, no interlace, every scanline
with filter 0, one IDAT chunk.  It is what `python -m acimg.show` saves its frames with - no PIL, imageio or cv2.

And a PNG reader (below the writer): `parse_png` walks a file's chunks on the host, `PngDecoder` takes a batch of files of
any legal form - 15 colour-type / depth pairs, Adam7, any filters - through the kernels of csrc/png_decode.hip to the
B, G, R pixels `cv2.imread` returns; what `python -m acimg.convert_collected` reads its frames with."""
import collections
import ctypes as C
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


# ---- the reader ---------------------------------------------------------------------------------------------------------------
# Host: `parse_png` walks the chunks; the zlib stream is inflated by the callers' workers (zlib) or on the device
# (acimg.inflate).  Device: csrc/png_decode.hip undoes the filters and forms the B, G, R pixels `cv2.imread` returns.
OK, BAD_FILTER, BAD_INDEX = 0, 1, 2                   # ACIMG_PNG_* of include/acimg.h
STATUS_TEXT = {BAD_FILTER: "a filter byte above 4", BAD_INDEX: "a palette index beyond PLTE"}
JOB_FIELDS, FILE_FIELDS = 6, 9                        # ACIMG_PNG_JOB_FIELDS, ACIMG_PNG_FILE_FIELDS
CHANNELS = {0: 1, 2: 3, 3: 1, 4: 2, 6: 4}
DEPTHS = {0: (1, 2, 4, 8, 16), 2: (8, 16), 3: (1, 2, 4, 8), 4: (8, 16), 6: (8, 16)}
ADAM7 = ((0, 0, 8, 8), (4, 0, 8, 8), (0, 4, 4, 8), (2, 0, 4, 4), (0, 2, 2, 4), (1, 0, 2, 2), (0, 1, 1, 2))   # x0, y0, dx, dy
INFLATE_CHOICES = ("zlib", "device")

PngPass = collections.namedtuple("PngPass", "index rows cols row_bytes src_off dst_off")
PngInfo = collections.namedtuple(
    "PngInfo", "height width colour_type bit_depth interlace palette idat passes bpp inflated_bytes sample_bytes")


def pass_geometry(height, width, colour_type, bit_depth, interlace):
    """-> ([PngPass]: the passes that have a row and a column, with their offsets in the inflated stream (first filter byte)
    and in the reconstructed samples; inflated bytes; sample bytes)"""
    bits = CHANNELS[colour_type] * bit_depth
    passes, src, dst = [], 0, 0
    for p, (x0, y0, dx, dy) in enumerate(ADAM7 if interlace else ((0, 0, 1, 1),)):
        rows, cols = -(-(height - y0) // dy), -(-(width - x0) // dx)
        if rows < 1 or cols < 1:
            continue
        row_bytes = (cols * bits + 7) // 8
        passes.append(PngPass(p, rows, cols, row_bytes, src, dst))
        src += rows * (row_bytes + 1)
        dst += rows * row_bytes
    return passes, src, dst


def parse_png(data, name="<png>"):
    """a whole PNG file -> PngInfo: geometry, colour type, depth, interlace, the palette (bytes, R G B per entry), the
    concatenated IDAT payload (the zlib stream), the per-pass job geometry and the inflated size IHDR implies.  Checks the
    signature, every chunk's CRC-32 and the chunk order; ancillary chunks are skipped.  ConvertError names the file and
    the reason for everything that is no legal file of PNG 1.2's critical chunks."""
    from .convert import ConvertError
    buf = bytes(data)
    if buf[:8] != SIGNATURE:
        raise ConvertError("%s: not a PNG file (bad signature)" % name)
    pos, size = 8, len(buf)
    ihdr = palette = None
    idat, state, ended = [], "start", False           # state: start, header, idat, after
    while pos < size:
        if ended:
            raise ConvertError("%s: %d bytes after IEND" % (name, size - pos))
        if pos + 8 > size:
            raise ConvertError("%s: truncated PNG file: %d bytes end inside a chunk header" % (name, size))
        length, kind = struct.unpack_from(">I4s", buf, pos)
        if length > 2 ** 31 - 1 or pos + 12 + length > size:
            raise ConvertError("%s: truncated PNG file: %d bytes end inside chunk %s of %d bytes"
                               % (name, size, kind.decode("latin-1"), length))
        body = buf[pos + 8:pos + 8 + length]
        crc = struct.unpack_from(">I", buf, pos + 8 + length)[0]
        if zlib.crc32(buf[pos + 4:pos + 8 + length]) & 0xFFFFFFFF != crc:
            raise ConvertError("%s: CRC mismatch in chunk %s at byte %d" % (name, kind.decode("latin-1"), pos))
        pos += 12 + length
        if state == "start" and kind != b"IHDR":
            raise ConvertError("%s: the first chunk is %s, not IHDR" % (name, kind.decode("latin-1")))
        if kind == b"IHDR":
            if state != "start":
                raise ConvertError("%s: a second IHDR chunk" % name)
            if length != 13:
                raise ConvertError("%s: IHDR of %d bytes" % (name, length))
            ihdr = struct.unpack(">IIBBBBB", body)
            state = "header"
        elif kind == b"PLTE":
            if state != "header":
                raise ConvertError("%s: PLTE after the first IDAT" % name)
            if palette is not None:
                raise ConvertError("%s: a second PLTE chunk" % name)
            palette = body
        elif kind == b"IDAT":
            if state == "after":
                raise ConvertError("%s: IDAT chunks are not consecutive" % name)
            state = "idat"
            idat.append(body)
        elif kind == b"IEND":
            ended = True
        elif not kind[0] & 0x20:
            raise ConvertError("%s: unknown critical chunk %s" % (name, kind.decode("latin-1")))
        if kind != b"IDAT" and state == "idat":       # any other chunk ends the run of IDAT chunks
            state = "after"
    if ihdr is None:
        raise ConvertError("%s: no IHDR chunk" % name)
    if not idat:
        raise ConvertError("%s: no IDAT chunk" % name)
    if not ended:
        raise ConvertError("%s: no IEND chunk" % name)
    width, height, depth, ctype, compression, filt, interlace = ihdr
    if width < 1 or height < 1 or width > 2 ** 31 - 1 or height > 2 ** 31 - 1:
        raise ConvertError("%s: a PNG of %d x %d pixels" % (name, width, height))
    if ctype not in DEPTHS or depth not in DEPTHS[ctype]:
        raise ConvertError("%s: colour type %d with bit depth %d is no PNG form" % (name, ctype, depth))
    if compression != 0:
        raise ConvertError("%s: compression method %d (only 0, deflate, is defined)" % (name, compression))
    if filt != 0:
        raise ConvertError("%s: filter method %d (only 0 is defined)" % (name, filt))
    if interlace > 1:
        raise ConvertError("%s: interlace method %d (0 and 1, Adam7, are defined)" % (name, interlace))
    if ctype == 3 and palette is None:
        raise ConvertError("%s: colour type 3 without a PLTE chunk" % name)
    if palette is not None:
        if len(palette) % 3 or not palette:
            raise ConvertError("%s: PLTE of %d bytes is no multiple of 3" % (name, len(palette)))
        if len(palette) // 3 > (1 << depth if ctype == 3 else 256):
            raise ConvertError("%s: PLTE of %d entries for a bit depth of %d" % (name, len(palette) // 3, depth))
    stream = b"".join(idat)
    if len(stream) < 6:
        raise ConvertError("%s: a zlib stream of %d bytes" % (name, len(stream)))
    cmf, flg = stream[0], stream[1]
    if (cmf & 15) != 8 or (cmf >> 4) > 7 or ((cmf << 8) | flg) % 31:
        raise ConvertError("%s: zlib header %02x %02x is not deflate with a window of at most 32 KiB" % (name, cmf, flg))
    if flg & 0x20:
        raise ConvertError("%s: zlib stream with a preset dictionary" % name)
    passes, inflated, samples = pass_geometry(height, width, ctype, depth, interlace)
    if inflated > 2 ** 31 - 1:
        raise ConvertError("%s: %d x %d pixels inflate to %d bytes, 2^31 - 1 are decoded" % (name, width, height, inflated))
    return PngInfo(height, width, ctype, depth, interlace, palette if ctype == 3 else b"", stream, tuple(passes),
                   max(1, CHANNELS[ctype] * depth // 8), inflated, samples)


def job_rows(info, file_index=0, src_base=0, dst_base=0):
    """the rows of `acimg_png_unfilter`'s job table for one file: [src_off, dst_off, rows, row_bytes, bpp, file]"""
    return [[src_base + p.src_off, dst_base + p.dst_off, p.rows, p.row_bytes, info.bpp, file_index] for p in info.passes]


def inflate_host(info, name="<png>"):
    """worker: the file's scanlines through `zlib.decompress` (which checks the Adler-32) -> bytes of exactly the size IHDR
    implies; a stream zlib refuses raises zlib's own error, another size is refused by name"""
    from .convert import ConvertError
    raw = zlib.decompress(info.idat)
    if len(raw) != info.inflated_bytes:
        raise ConvertError("%s: the IDAT stream inflates to %d bytes, IHDR implies %d" % (name, len(raw), info.inflated_bytes))
    return raw


class PngDecoder(object):
    """PNG files -> B, G, R pixels on `device`: `decode_many` takes a batch of files of any geometries through ONE
    `acimg_png_unfilter` and ONE `acimg_png_pixels`.  inflate="zlib": the scanlines are inflated on the host (by the
    caller's workers when it hands `inflated` in, else here) and uploaded once, packed.  inflate="device": the zlib bodies
    go through `DeviceInflater.inflate_launch` with the sizes IHDR implies and `DeviceChecksum`'s Adler-32 is held against
    each trailer, so the inflated bytes never reach the host; a stream whose status is not 0, whose end is not where the
    trailer begins or whose Adler-32 differs is inflated by zlib on the host instead, which decides and raises."""

    def __init__(self, device, inflate="zlib"):
        import torch

        from . import _lib
        from .convert import ConvertError
        if inflate not in INFLATE_CHOICES:
            raise ConvertError("--inflate is one of %s, got %r" % (", ".join(INFLATE_CHOICES), inflate))
        self.device, self.inflate = torch.device(device), inflate
        self.lib = _lib.load()
        self._inflater = self._checksum = None
        self.fallbacks = 0                              # streams the device path handed to zlib

    def _inflate_device(self, infos, names):
        """-> the inflated streams packed in one uint8 device tensor"""
        import torch

        from .checksum import ADLER32, DeviceChecksum
        from .inflate import OK as INFLATE_OK
        from .inflate import DeviceInflater
        if self._inflater is None:
            self._inflater, self._checksum = DeviceInflater(self.device), DeviceChecksum(self.device)
        sizes = [g.inflated_bytes for g in infos]
        bodies = [np.frombuffer(g.idat, np.uint8)[2:-4] for g in infos]
        out, status, end_bits = self._inflater.inflate_launch(bodies, sizes)
        adler = self._checksum.values(self._checksum.packed(out, sizes, ADLER32))
        status, end_bits = status.cpu().tolist(), end_bits.cpu().tolist()
        at = 0
        for g, nm, body, st, end, a in zip(infos, names, bodies, status, end_bits, adler):
            if st != INFLATE_OK or (end + 7) // 8 != body.size or a != struct.unpack(">I", g.idat[-4:])[0]:
                self.fallbacks += 1
                raw = inflate_host(g, nm)                # zlib decides: its own error, or the size refused by name
                out[at:at + g.inflated_bytes] = torch.from_numpy(np.frombuffer(raw, np.uint8).copy()).to(self.device)
            at += g.inflated_bytes
        return out

    def stages(self, src, infos):
        """the packed inflated streams (uint8 device tensor) of `infos` through the two kernels ->
        (samples uint8 packed, pixels uint8 packed, status int32 [n] on the device)"""
        import torch

        from . import _lib, ops
        L, dev, n = self.lib, self.device, len(infos)
        jobs, files, palettes, s_at, d_at, o_at, p_at = [], [], [], 0, 0, 0, 0
        for i, g in enumerate(infos):
            jobs += job_rows(g, i, s_at, d_at)
            files.append([d_at, g.height, g.width, g.colour_type, g.bit_depth, g.interlace, p_at, len(g.palette) // 3, o_at])
            palettes.append(g.palette)
            s_at, d_at, o_at, p_at = s_at + g.inflated_bytes, d_at + g.sample_bytes, o_at + 3 * g.height * g.width, p_at + len(g.palette)
        if src.numel() != s_at:
            raise ValueError("%d inflated bytes for files that imply %d" % (src.numel(), s_at))
        samples = torch.empty(d_at, dtype=torch.uint8, device=dev)
        pixels = torch.empty(o_at, dtype=torch.uint8, device=dev)
        status = torch.empty(n, dtype=torch.int32, device=dev)
        palette = torch.from_numpy(np.frombuffer(b"".join(palettes), np.uint8).copy()).to(dev) if p_at else None
        ws_bytes = max(int(L.acimg_png_unfilter_workspace(len(jobs))), int(L.acimg_png_pixels_workspace(n)))
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
        st = ops.current_stream_handle(dev)
        flat = [int(v) for row in jobs for v in row]
        _lib.check(L.acimg_png_unfilter(src.data_ptr(), src.numel(), (C.c_long * len(flat))(*flat), len(jobs), n,
                                        samples.data_ptr(), samples.numel(), status.data_ptr(), ws.data_ptr(), ws_bytes, st),
                   "png_unfilter")
        flat = [int(v) for row in files for v in row]
        _lib.check(L.acimg_png_pixels(samples.data_ptr(), samples.numel(), (C.c_long * len(flat))(*flat), n,
                                      palette.data_ptr() if palette is not None else None, p_at, pixels.data_ptr(),
                                      pixels.numel(), status.data_ptr(), ws.data_ptr(), ws_bytes, st), "png_pixels")
        return samples, pixels, status

    def decode_many(self, files, infos=None, inflated=None, names=None):
        """files: whole files (bytes); infos: their `parse_png` records; inflated (inflate="zlib" only): their scanlines as
        the workers' `inflate_host` gave them -> ([uint8 [H,W,3] device tensor per file, views of one tensor], int32
        [files] status on the host: 0, BAD_FILTER or BAD_INDEX)"""
        import torch
        names = names or ["<png %d>" % i for i in range(len(files))]
        infos = infos or [parse_png(f, nm) for f, nm in zip(files, names)]
        if not infos:
            return [], np.zeros(0, np.int32)
        if self.inflate == "device":
            src = self._inflate_device(infos, names)
        else:
            inflated = inflated or [inflate_host(g, nm) for g, nm in zip(infos, names)]
            src = torch.from_numpy(np.frombuffer(b"".join(inflated), np.uint8).copy()).to(self.device)
        _, pixels, status = self.stages(src, infos)
        out, at = [], 0
        for g in infos:
            n = 3 * g.height * g.width
            out.append(pixels[at:at + n].view(g.height, g.width, 3))
            at += n
        return out, status.cpu().numpy()


def decode_png(data, device="cuda:0", name="<png>"):
    """one file -> uint8 [H,W,3] B, G, R on the host; a device status other than 0 is a ConvertError"""
    from .convert import ConvertError
    pixels, status = PngDecoder(device).decode_many([data], names=[name])
    if status[0]:
        raise ConvertError("%s: corrupt PNG: %s" % (name, STATUS_TEXT.get(int(status[0]), status[0])))
    return pixels[0].cpu().numpy()
