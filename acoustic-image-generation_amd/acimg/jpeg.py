"""Baseline JPEG files (JFIF, 4:2:0) of RGB8 device tensors: the two kernels of csrc/jpeg.hip (`acimg_jpeg_blocks`,
`acimg_jpeg_scan`) produce each frame's entropy-coded segment on the device; the header segments, which depend on the
size, the quality and the restart interval alone, are built here once per encoder and size.  Per `encode` call two
transfers come back: the frames' byte counts and their packed bytes.  No imaging library is involved."""
import ctypes as C
import struct

import numpy as np
import torch

from . import _lib, ops

# zig-zag position -> natural (row-major) index: the order a DQT segment stores a table in
ZIGZAG = (0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
          35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55,
          62, 63)

# ITU-T T.81 Annex K.3: (table class << 4 | destination, BITS, HUFFVAL) of the four typical tables, in file order
_DC_VALS = bytes(range(12))
_AC_LUMA_VALS = bytes.fromhex(
    "01020300041105122131410613516107227114328191a1082342b1c11552d1f02433627282090a161718191a25262728292a3435363738393a"
    "434445464748494a535455565758595a636465666768696a737475767778797a838485868788898a92939495969798999aa2a3a4a5a6a7a8a9"
    "aab2b3b4b5b6b7b8b9bac2c3c4c5c6c7c8c9cad2d3d4d5d6d7d8d9dae1e2e3e4e5e6e7e8e9eaf1f2f3f4f5f6f7f8f9fa")
_AC_CHROMA_VALS = bytes.fromhex(
    "0001020311040521310612415107617113223281081442 91a1b1c109233352f0156272d10a162434e125f11718191a262728292a353637"
    "38393a434445464748494a535455565758595a636465666768696a737475767778797a82838485868788898a92939495969798999aa2a3a4"
    "a5a6a7a8a9aab2b3b4b5b6b7b8b9bac2c3c4c5c6c7c8c9cad2d3d4d5d6d7d8d9dae2e3e4e5e6e7e8e9eaf2f3f4f5f6f7f8f9fa")
HUFFMAN_TABLES = (
    (0x00, bytes((0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0)), _DC_VALS),
    (0x10, bytes((0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7D)), _AC_LUMA_VALS),
    (0x01, bytes((0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0)), _DC_VALS),
    (0x11, bytes((0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77)), _AC_CHROMA_VALS),
)
EOI = b"\xFF\xD9"


def quant_tables(quality):
    """uint8 [2,64], natural order, luma then chroma (`acimg_jpeg_quant_tables`)"""
    out = np.zeros(128, np.uint8)
    _lib.check(_lib.load().acimg_jpeg_quant_tables(int(quality), out.ctypes.data_as(C.c_void_p)), "jpeg_quant_tables")
    return out.reshape(2, 64)


def _segment(marker, payload):
    return struct.pack(">BBH", 0xFF, marker, len(payload) + 2) + payload


def jfif_header(height, width, qtables, restart_mcus):
    """SOI, APP0, two DQT, SOF0 (Y 2x2, Cb 1x1, Cr 1x1), four DHT, DRI, SOS: everything in front of the scan"""
    qt = np.asarray(qtables, np.uint8).reshape(2, 64)
    zz = list(ZIGZAG)
    h = b"\xFF\xD8" + _segment(0xE0, b"JFIF\x00" + struct.pack(">BBBHHBB", 1, 1, 0, 1, 1, 0, 0))
    for i in range(2):
        h += _segment(0xDB, bytes((i,)) + qt[i][zz].tobytes())
    h += _segment(0xC0, struct.pack(">BHHB", 8, height, width, 3) + bytes((1, 0x22, 0, 2, 0x11, 1, 3, 0x11, 1)))
    for tc_th, bits, vals in HUFFMAN_TABLES:
        h += _segment(0xC4, bytes((tc_th,)) + bits + vals)
    h += _segment(0xDD, struct.pack(">H", restart_mcus))
    return h + _segment(0xDA, bytes((3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0)))


class JpegEncoder(object):
    """quality 1..100 (the libjpeg scaling of the Annex K tables); restart_mcus: MCUs (16 x 16 pixels) per restart
    interval, None = one MCU row.  The intervals are what the device codes in parallel."""

    def __init__(self, device, quality=90, restart_mcus=None):
        self.device = torch.device(device)
        self.lib = _lib.load()
        self.quality = int(quality)
        if restart_mcus is not None and not 1 <= int(restart_mcus) <= 65535:
            raise ValueError("restart_mcus is 1..65535 or None, got %r" % (restart_mcus,))
        self._restart = None if restart_mcus is None else int(restart_mcus)
        self.qtables = quant_tables(self.quality)
        self._qt_dev = torch.from_numpy(self.qtables.reshape(128).copy()).to(self.device)
        self._headers = {}

    def restart_mcus(self, width):
        return self._restart if self._restart is not None else -(-int(width) // 16)

    def header(self, height, width):
        key = (int(height), int(width))
        if key not in self._headers:
            self._headers[key] = jfif_header(key[0], key[1], self.qtables, self.restart_mcus(width))
        return self._headers[key]

    def scan(self, frames):
        """uint8 [n,H,W,3] -> (scan uint8 [n,stride] on the device, scan_bytes int32 [n] on the device)"""
        f = frames.to(self.device)
        if f.dtype != torch.uint8 or f.dim() != 4 or f.shape[3] != 3 or f.shape[0] < 1:
            raise ValueError("frames are uint8 [n,H,W,3], got %s %s" % (frames.dtype, tuple(frames.shape)))
        f = f.contiguous()
        n, H, W = int(f.shape[0]), int(f.shape[1]), int(f.shape[2])
        L, r = self.lib, self.restart_mcus(W)
        stride = int(L.acimg_jpeg_scan_capacity(H, W, r))
        if stride == 0:
            raise ValueError("a JPEG frame is 1..65535 pixels wide and high, got %d x %d" % (H, W))
        stride = -(-stride // 16) * 16
        coef = torch.empty(int(L.acimg_jpeg_coef_bytes(n, H, W)) // 2, dtype=torch.int16, device=self.device)
        ws_bytes = int(L.acimg_jpeg_scan_workspace(n, H, W, r))
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=self.device)
        out = torch.empty(n, stride, dtype=torch.uint8, device=self.device)
        nbytes = torch.empty(n, dtype=torch.int32, device=self.device)
        st = ops.current_stream_handle(self.device)
        _lib.check(L.acimg_jpeg_blocks(f.data_ptr(), n, H, W, self._qt_dev.data_ptr(), coef.data_ptr(), st), "jpeg_blocks")
        _lib.check(L.acimg_jpeg_scan(coef.data_ptr(), n, H, W, r, out.data_ptr(), stride, nbytes.data_ptr(), ws.data_ptr(),
                                     ws_bytes, st), "jpeg_scan")
        return out, nbytes

    def encode(self, frames):
        """uint8 [n,H,W,3] (device or host tensor) -> a list of n complete JFIF files as bytes"""
        out, nbytes = self.scan(frames)
        counts = nbytes.cpu().tolist()                                       # read-back 1: n int32
        packed = torch.cat([out[i, :c] for i, c in enumerate(counts)]).cpu().numpy().tobytes()    # read-back 2
        head = self.header(frames.shape[1], frames.shape[2])
        files, at = [], 0
        for c in counts:
            files.append(head + packed[at:at + c] + EOI)
            at += c
        return files


def encode_jpeg(rgb_uint8, quality=90, restart_mcus=None, device="cuda:0"):
    """[H,W,3] uint8 (array or tensor) -> the bytes of a JFIF file, encoded on `device`"""
    a = torch.as_tensor(rgb_uint8)
    if a.dtype != torch.uint8 or a.dim() != 3 or a.shape[2] != 3:
        raise ValueError("write_jpeg wants a [H,W,3] uint8 image, got %s %s" % (a.dtype, tuple(a.shape)))
    return JpegEncoder(device, quality, restart_mcus).encode(a.unsqueeze(0))[0]


def write_jpeg(path, rgb_uint8, quality=90, restart_mcus=None, device="cuda:0"):
    data = encode_jpeg(rgb_uint8, quality, restart_mcus, device)
    with open(path, "wb") as f:
        f.write(data)
    return len(data)
