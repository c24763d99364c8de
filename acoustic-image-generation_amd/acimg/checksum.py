"""The containers' checksums on the device (csrc/checksum.hip, `acimg_checksum`) and the gather that assembles framed
records there (`acimg_record_gather`): what `DeviceDeflater.gzip_many` / `zlib_many`, `--assemble device` of
`python -m acimg.convert` and `png.encode_png_many` finish their files with, without the payload reaching the host.

Every value equals `zlib.crc32`, `tfio.crc32c` (`acimg_crc32c`), `tfio.mask_crc` of it, or `zlib.adler32` bit for bit.
tests/checksum_ref.py restates the algebra of the segment combine."""
import ctypes as C

import numpy as np
import torch

from . import _lib, ops
from .deflate import _as_u8

CRC32, CRC32C, CRC32C_MASKED, ADLER32 = 0, 1, 2, 3       # ACIMG_CHECKSUM_* of include/acimg.h
SEGMENT = 16384                                          # ACIMG_CHECKSUM_SEGMENT
MASK_OF_ZERO = 0xa282ead8                                # tfio.mask_crc(0)
EMPTY = {CRC32: 0, CRC32C: 0, CRC32C_MASKED: MASK_OF_ZERO, ADLER32: 1}


def _longs(values):
    return (C.c_long * len(values))(*[int(v) for v in values])


class DeviceChecksum(object):
    def __init__(self, device):
        self.device = torch.device(device)
        self.lib = _lib.load()

    def packed(self, data, lengths, kind, store_base=None, store_at=None):
        """ONE `acimg_checksum` on the current stream.  data: uint8 on the device, the payloads of `lengths` one behind
        the other from its first byte -> int32 [count] on the device (the values' bits; `values` reads them).  store_at
        (with store_base, a uint8 device tensor): byte offsets in store_base that also receive the values, little-endian;
        negative = none."""
        if data.dtype != torch.uint8 or data.device != self.device or not data.is_contiguous():
            raise ValueError("data is a contiguous uint8 tensor on %s" % self.device)
        count, total = len(lengths), sum(int(n) for n in lengths)
        if count < 1 or total > data.numel():
            raise ValueError("%d payloads of %d bytes together in a buffer of %d" % (count, total, data.numel()))
        if store_at is not None and (store_base is None or len(store_at) != count
                                     or any(int(o) + 4 > store_base.numel() for o in store_at)):
            raise ValueError("store_at names %d offsets inside store_base" % count)
        L = self.lib
        ws_bytes = int(L.acimg_checksum_workspace(total, count))
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=self.device)
        out = torch.empty(count, dtype=torch.int32, device=self.device)
        _lib.check(L.acimg_checksum(data.data_ptr() if data.numel() else ws.data_ptr(), _longs(lengths), count, int(kind),
                                    out.data_ptr(), store_base.data_ptr() if store_at is not None else None,
                                    _longs(store_at) if store_at is not None else None, ws.data_ptr(), ws_bytes,
                                    ops.current_stream_handle(self.device)), "checksum")
        return out

    @staticmethod
    def values(out):
        """the int32 tensor of `packed` -> list of ints 0 .. 2^32 - 1"""
        return [int(v) for v in out.cpu().numpy().view(np.uint32)]

    def many(self, payloads, kind, store=None):
        """payloads (bytes-like or uint8 tensors, on the host or the device) -> their checksums of `kind`, a list of
        ints.  store: (uint8 device tensor, [offset or a negative number, per payload])"""
        tensors = [_as_u8(p) for p in payloads]
        if not tensors:
            return []
        parts = [t.to(self.device) for t in tensors if t.numel()]
        data = torch.cat(parts) if len(parts) > 1 else (parts[0].contiguous() if parts else
                                                        torch.empty(0, dtype=torch.uint8, device=self.device))
        base, at = store if store is not None else (None, None)
        return self.values(self.packed(data, [t.numel() for t in tensors], kind, base, at))

    def crc32(self, data):
        return self.many([data], CRC32)[0]

    def crc32c(self, data, masked=False):
        return self.many([data], CRC32C_MASKED if masked else CRC32C)[0]

    def adler32(self, data):
        return self.many([data], ADLER32)[0]

    def gather(self, src0, src1, segments, dst):
        """ONE `acimg_record_gather` on the current stream: rows {dst_off, src_off, len, which} of `segments` copy bytes
        of src0 (which = 0) or src1 (which = 1), uint8 device tensors or None, into the uint8 device tensor `dst`"""
        for t in (src0, src1, dst):
            if t is not None and (t.dtype != torch.uint8 or t.device != self.device or not t.is_contiguous()):
                raise ValueError("sources and dst are contiguous uint8 tensors on %s" % self.device)
        rows = [[int(v) for v in row] for row in segments]
        for d, s, n, which in rows:
            src = src1 if which else src0
            if which not in (0, 1) or src is None or s < 0 or n < 0 or s + n > src.numel():
                raise ValueError("segment {dst %d, src %d, len %d, which %d} leaves its source" % (d, s, n, which))
        L = self.lib
        nseg = len(rows)
        ws_bytes = int(L.acimg_record_gather_workspace(nseg))
        ws = torch.empty(max(ws_bytes, 16), dtype=torch.uint8, device=self.device)
        _lib.check(L.acimg_record_gather(src0.data_ptr() if src0 is not None else None,
                                         src1.data_ptr() if src1 is not None else None,
                                         _longs([v for row in rows for v in row]), nseg, dst.data_ptr(), dst.numel(),
                                         ws.data_ptr(), ws_bytes, ops.current_stream_handle(self.device)), "record_gather")
        return dst
