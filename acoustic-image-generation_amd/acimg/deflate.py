"""DEFLATE on the device (csrc/deflate.hip, `acimg_deflate`): raw RFC 1951 streams of byte payloads, and the gzip and
zlib containers around them - what `--deflate device` of `python -m acimg.convert` / `acimg.convert_boxes` and
`--png_deflate device` of `python -m acimg.show` compress with instead of the host's zlib.

A payload is cut into blocks of BLOCK bytes that are coded independently; `compress_many` codes all blocks of all its
payloads in ONE `acimg_deflate` call and brings back two transfers: the streams' byte counts and their packed bytes.
The containers' checksums (CRC-32, Adler-32) of `gzip` / `zlib` are the host's `zlib.crc32` / `zlib.adler32`: the payload
is host memory there.  `gzip_many` / `zlib_many` take payloads that live on the device and get their checksums from
`acimg_checksum` (acimg/checksum.py) in the same stream.  tests/deflate_ref.py restates the streams bit for bit."""
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

    def _launch(self, data, lengths):
        """ONE `acimg_deflate` on the current stream: data uint8 on the device, payloads of `lengths` (each >= 1) one behind
        the other -> (packed streams, their int64 byte counts), both on the device"""
        L = self.lib
        total, count = sum(lengths), len(lengths)
        out_bytes = sum(int(L.acimg_deflate_bound(n)) for n in lengths)
        ws_bytes = int(L.acimg_deflate_workspace(total, count))
        if ws_bytes == 0:
            raise ValueError("deflate: %d payloads of %d bytes together are outside the encoder's range" % (count, total))
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=self.device)
        packed = torch.empty(out_bytes, dtype=torch.uint8, device=self.device)
        sizes = torch.empty(count, dtype=torch.int64, device=self.device)
        _lib.check(L.acimg_deflate(data.data_ptr(), (C.c_long * count)(*lengths), count, packed.data_ptr(), out_bytes,
                                   sizes.data_ptr(), ws.data_ptr(), ws_bytes, ops.current_stream_handle(self.device)), "deflate")
        return packed, sizes

    @staticmethod
    def _download(packed, sizes, sums=None):
        """-> ([stream bytes], [checksum] or None): the byte counts (and the int32 checksums with them, in the same small
        transfer), then the streams' bytes alone"""
        count = sizes.numel()
        head = sizes.view(torch.uint8) if sums is None else torch.cat([sizes.view(torch.uint8), sums.view(torch.uint8)])
        head = head.cpu().numpy()
        n = head[:8 * count].view(np.int64).tolist()
        values = None if sums is None else [int(v) for v in head[8 * count:].view(np.uint32)]
        host = packed[:sum(n)].cpu().numpy()
        ends = np.cumsum(n).tolist()
        return [host[e - k:e].tobytes() for e, k in zip(ends, n)], values

    def _gather_payloads(self, payloads):
        tensors = [_as_u8(p) for p in payloads]
        work = [i for i, t in enumerate(tensors) if t.numel()]
        lengths = [int(tensors[i].numel()) for i in work]
        data = None
        if work:
            data = (torch.cat([tensors[i].to(self.device) for i in work]) if len(work) > 1
                    else tensors[work[0]].to(self.device).contiguous())
        return tensors, work, lengths, data

    def compress_many(self, payloads):
        """payloads (bytes-like or uint8 tensors, on the host or the device) -> their raw streams as bytes, in order"""
        tensors, work, lengths, data = self._gather_payloads(payloads)
        out = [EMPTY_STREAM if t.numel() == 0 else None for t in tensors]
        if not work:
            return out
        streams, _ = self._download(*self._launch(data, lengths))
        for i, s in zip(work, streams):
            out[i] = s
        return out

    def _containers(self, payloads, kind, host_sum, wrap):
        from . import checksum
        tensors, work, lengths, data = self._gather_payloads(payloads)
        on_device = [isinstance(p, torch.Tensor) and p.device.type != "cpu" for p in payloads]
        sums = [None if dev else host_sum(t.numpy()) & 0xFFFFFFFF for t, dev in zip(tensors, on_device)]
        streams = [EMPTY_STREAM] * len(tensors)
        device_sums = None
        if work:
            if any(on_device[i] for i in work):      # same stream, before the deflate launches: the payload stays where it is
                device_sums = checksum.DeviceChecksum(self.device).packed(data, lengths, kind)
            got, values = self._download(*self._launch(data, lengths), sums=device_sums)
            for k, i in enumerate(work):
                streams[i] = got[k]
                if on_device[i]:
                    sums[i] = values[k]
        return [wrap(s, checksum.EMPTY[kind] if v is None else v, int(t.numel())) for s, v, t in zip(streams, sums, tensors)]

    def gzip_many(self, payloads):
        """payloads -> complete gzip members, in order.  A payload that is a device tensor never reaches the host: its
        CRC-32 comes from `acimg_checksum` in the stream of `acimg_deflate`, and the download carries byte counts and
        checksums together, then the streams.  Host bytes keep `zlib.crc32`; the result is the same either way."""
        return self._containers(payloads, 0, zlib.crc32, lambda s, v, n: GZIP_HEADER + s + struct.pack("<II", v, n & 0xFFFFFFFF))

    def zlib_many(self, payloads):
        """payloads -> complete zlib streams, in order; the Adler-32 of a device tensor comes from the device"""
        return self._containers(payloads, 3, zlib.adler32, lambda s, v, n: ZLIB_HEADER + s + struct.pack(">I", v))

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
