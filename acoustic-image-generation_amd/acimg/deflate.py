"""DEFLATE on the device (csrc/deflate.hip, `acimg_deflate`): raw RFC 1951 streams of byte payloads, and the gzip and
zlib containers around them - what `--deflate device` of `python -m acimg.convert` / `acimg.convert_boxes` and
`--png_deflate device` of `python -m acimg.show` compress with instead of the host's zlib.

A payload is cut into blocks of BLOCK bytes that are coded independently; `compress_many` codes all blocks of all its
payloads in ONE `acimg_deflate` call and brings back two transfers: the streams' byte counts and their packed bytes.
The containers' checksums (CRC-32, Adler-32) are the host's `zlib.crc32` / `zlib.adler32`: the payload is host memory
where the tools call this.  tests/deflate_ref.py restates the streams bit for bit."""
import ctypes as C
import struct
import zlib

import numpy as np
import torch

from . import _lib, ops

BLOCK = 16384                                   # ACIMG_DEFLATE_BLOCK of include/acimg.h
EMPTY_STREAM = b"\x01\x00\x00\xff\xff"          # a payload of 0 bytes: one final empty stored block, no launch
GZIP_HEADER = b"\x1f\x8b\x08\x00\x00\x00\x00\x00\x00\xff"   # deflate, no flags, mtime 0, no extra flags, OS unknown
ZLIB_HEADER = b"\x78\x01"                       # 32 KiB window, no dictionary, fastest-compression hint


def bound(n):
    """the most bytes the raw stream of an n-byte payload has (acimg_deflate_bound)"""
    return int(n) + 10 * (-(-int(n) // BLOCK)) + 5


def gzip_container(stream, payload):
    """RFC 1952 member around a raw stream of `payload`"""
    return GZIP_HEADER + stream + struct.pack("<II", zlib.crc32(payload) & 0xFFFFFFFF, len(payload) & 0xFFFFFFFF)


def zlib_container(stream, payload):
    """RFC 1950 stream around a raw stream of `payload`"""
    return ZLIB_HEADER + stream + struct.pack(">I", zlib.adler32(payload) & 0xFFFFFFFF)


def write_gzip_files(deflater, items):
    """[(path, bytes)] -> one gzip file each, all compressed in ONE `compress_many` (the converters' device path)"""
    streams = deflater.compress_many([buf for _, buf in items])
    for (path, buf), stream in zip(items, streams):
        with open(path, "wb") as f:
            f.write(gzip_container(stream, buf))


def _as_u8(data):
    if isinstance(data, torch.Tensor):
        if data.dtype != torch.uint8:
            raise ValueError("a payload tensor is uint8, got %s" % data.dtype)
        return data.reshape(-1)
    return torch.from_numpy(np.frombuffer(data, np.uint8).copy())      # a copy: torch wants writable memory


class DeviceDeflater(object):
    def __init__(self, device):
        self.device = torch.device(device)
        self.lib = _lib.load()
        if int(self.lib.acimg_deflate_bound(BLOCK)) != bound(BLOCK):
            raise _lib.AcimgError("libacimg.so codes blocks of another size than acimg.deflate.BLOCK = %d" % BLOCK)

    def compress_many(self, payloads):
        """payloads (bytes-like or uint8 tensors, on the host or the device) -> their raw streams as bytes, in order"""
        tensors = [_as_u8(p) for p in payloads]
        out = [EMPTY_STREAM if t.numel() == 0 else None for t in tensors]
        work = [i for i, t in enumerate(tensors) if t.numel()]
        if not work:
            return out
        L = self.lib
        lengths = [int(tensors[i].numel()) for i in work]
        total, count = sum(lengths), len(work)
        data = torch.cat([tensors[i].to(self.device) for i in work]) if count > 1 else tensors[work[0]].to(self.device).contiguous()
        out_bytes = sum(int(L.acimg_deflate_bound(n)) for n in lengths)
        ws_bytes = int(L.acimg_deflate_workspace(total, count))
        if ws_bytes == 0:
            raise ValueError("deflate: %d payloads of %d bytes together are outside the encoder's range" % (count, total))
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=self.device)
        packed = torch.empty(out_bytes, dtype=torch.uint8, device=self.device)
        sizes = torch.empty(count, dtype=torch.int64, device=self.device)
        _lib.check(L.acimg_deflate(data.data_ptr(), (C.c_long * count)(*lengths), count, packed.data_ptr(), out_bytes,
                                   sizes.data_ptr(), ws.data_ptr(), ws_bytes, ops.current_stream_handle(self.device)), "deflate")
        sizes = sizes.cpu().tolist()
        host = packed[:sum(sizes)].cpu().numpy()
        at = 0
        for i, n in zip(work, sizes):
            out[i] = host[at:at + n].tobytes()
            at += n
        return out

    def deflate(self, data):
        """-> the raw RFC 1951 stream of `data`"""
        return self.compress_many([data])[0]

    def gzip(self, data):
        """-> a gzip member (10-byte header with mtime 0, the stream, CRC-32, ISIZE) that `gzip.decompress` reads"""
        data = bytes(data)
        return gzip_container(self.deflate(data), data)

    def zlib(self, data):
        """-> a zlib stream (78 01, the stream, Adler-32) that `zlib.decompress` reads"""
        data = bytes(data)
        return zlib_container(self.deflate(data), data)

    def huffman_lengths(self, freq, limit):
        """int32 [n][nsym] histograms -> uint8 [n][nsym] code lengths of at most `limit` bits (acimg_huffman_lengths)"""
        f = torch.as_tensor(freq, dtype=torch.int32).to(self.device).contiguous()
        if f.dim() != 2 or f.shape[0] < 1:
            raise ValueError("histograms are int32 [n][nsym], got %s" % (tuple(f.shape),))
        out = torch.empty(f.shape, dtype=torch.uint8, device=self.device)
        _lib.check(self.lib.acimg_huffman_lengths(f.data_ptr(), int(f.shape[0]), int(f.shape[1]), int(limit), out.data_ptr(),
                                                  ops.current_stream_handle(self.device)), "huffman_lengths")
        return out.cpu()
