"""INFLATE on the device (csrc/inflate.hip, `acimg_inflate`): raw RFC 1951 streams, and the gzip and zlib containers around
them - what `DeviceDataLoader(inflate="device")` and `--inflate device` of `python -m acimg.main` read GZIP records with
instead of the workers' zlib.

`inflate_many` decodes every chunk of every stream in ONE `acimg_inflate` call (a call of one file leaves most of the
card idle) and returns device tensors.  The `gunzip*` front ends strip the RFC 1952 container on the host, and check what
zlib checks: the stream ends where the 8-byte trailer begins, ISIZE, and the member's CRC-32 (the host's `zlib.crc32`,
once the bytes are on the host).  Whatever the device path does not take - a second member, a status other than 0, a
size of 0 or of 2^31 and more, any mismatch - goes to the host's `acimg_gzip_inflate` as before, which decides and raises
what it always raised.  tests/inflate_ref.py restates the decoder's plan."""
import ctypes as C
import struct
import zlib as _zlib

import numpy as np
import torch

from . import _lib, ops

DEFAULT_CHUNK_BYTES = 16384                     # compressed bytes per chunk: DESIGN section 8 has the measurement
OK, CORRUPT, SIZE, TRUNCATED = 0, 1, 2, 3       # ACIMG_INFLATE_* of include/acimg.h
STATUS_NAMES = {OK: "ok", CORRUPT: "corrupt", SIZE: "size mismatch", TRUNCATED: "truncated"}
FTEXT, FHCRC, FEXTRA, FNAME, FCOMMENT = 1, 2, 4, 8, 16
MAX_SIZE = 2 ** 31 - 1

# the debug view of the workspace: AcimgInflateChunk of include/acimg.h
CHUNK_DTYPE = np.dtype([("src_off", "<i8"), ("src_len", "<i8"), ("out_off", "<i8"), ("out_len", "<i8"), ("stream", "<i4"),
                        ("index", "<i4"), ("first", "<i4"), ("nchunks", "<i4"), ("start", "<i8"), ("end", "<i8"),
                        ("length", "<i8"), ("offset", "<i8"), ("next", "<i4"), ("status", "<i4"), ("live", "<i4"),
                        ("reserved", "<i4")])
assert CHUNK_DTYPE.itemsize == 96


def parse_gzip(raw):
    """the first member of a gzip file -> (body_offset, body_length, crc32, isize): the raw deflate stream is
    raw[body_offset:body_offset + body_length] IF the file holds this one member (the caller checks where the stream ends),
    crc32 and isize are the file's last 8 bytes.  FEXTRA, FNAME, FCOMMENT and FHCRC are skipped.  ValueError for anything
    that is no such header."""
    raw = memoryview(raw).cast("B") if not isinstance(raw, (bytes, bytearray)) else raw
    n = len(raw)
    if n < 18 or raw[0] != 0x1F or raw[1] != 0x8B:
        raise ValueError("no gzip member: %d bytes, magic %s" % (n, bytes(raw[:2]).hex()))
    if raw[2] != 8:
        raise ValueError("gzip compression method %d is not deflate" % raw[2])
    flags = raw[3]
    if flags & 0xE0:
        raise ValueError("gzip header with reserved flag bits 0x%02x" % flags)
    at = 10
    if flags & FEXTRA:
        if at + 2 > n:
            raise ValueError("gzip header ends in FEXTRA")
        at += 2 + (raw[at] | raw[at + 1] << 8)
    for bit in (FNAME, FCOMMENT):
        if flags & bit:
            while at < n and raw[at] != 0:
                at += 1
            at += 1
    if flags & FHCRC:
        at += 2
    if at + 8 >= n:
        raise ValueError("gzip header of %d bytes leaves no stream in %d" % (at, n))
    crc, isize = struct.unpack("<II", bytes(raw[n - 8:n]))
    return at, n - 8 - at, crc, isize


def host_gunzip(raw):
    """the host's reader (`acimg_gzip_inflate`: every member, every check) -> uint8 array; raises what it always raised"""
    lib = _lib.load()
    raw = np.frombuffer(raw, np.uint8) if not isinstance(raw, np.ndarray) else raw
    gz = raw.size >= 18 and raw[0] == 0x1f and raw[1] == 0x8b
    # a GZIP member ends with its inflated size mod 2^32: the first guess, so that most files are inflated once
    guess = int(raw[-4:].view("<u4")[0]) if gz else raw.size
    produced = C.c_size_t(0)
    buf = np.empty(max(guess, 1), dtype=np.uint8)
    rc = lib.acimg_gzip_inflate(raw.ctypes.data, raw.size, buf.ctypes.data, buf.size, C.byref(produced))
    if rc == -2:
        buf = np.empty(max(produced.value, 1), dtype=np.uint8)
        rc = lib.acimg_gzip_inflate(raw.ctypes.data, raw.size, buf.ctypes.data, buf.size, C.byref(produced))
    _lib.check(rc, "gzip_inflate")
    return buf[:produced.value]


def gzip_plan(raw):
    """(body_offset, body_length, crc32, isize) when the device path may try this file, else None (the host decides)"""
    try:
        off, length, crc, isize = parse_gzip(raw)
    except ValueError:
        return None
    if not 0 < isize <= MAX_SIZE:
        return None
    return off, length, crc, isize


def gzip_verify(raw, plan, data, status, end_bits):
    """the device's result for one file against the container -> the inflated bytes: `data` when the stream ended where
    the trailer begins and ISIZE and CRC-32 hold, else whatever `host_gunzip` returns or raises"""
    if plan is not None and data is not None and status == OK:
        off, length, crc, isize = plan
        if (end_bits + 7) // 8 == length and len(data) == isize and (_zlib.crc32(data) & 0xFFFFFFFF) == crc:
            return data
    return host_gunzip(raw)


def _as_u8(data):
    if isinstance(data, torch.Tensor):
        if data.dtype != torch.uint8:
            raise ValueError("a stream tensor is uint8, got %s" % data.dtype)
        return data.reshape(-1)
    if isinstance(data, np.ndarray):
        return torch.from_numpy(np.require(data, np.uint8, ["C", "W"]).reshape(-1))      # a copy only if read-only
    return torch.from_numpy(np.frombuffer(data, np.uint8).copy())      # a copy: torch wants writable memory


class DeviceInflater(object):
    def __init__(self, device, chunk_bytes=DEFAULT_CHUNK_BYTES):
        self.device = torch.device(device)
        self.chunk_bytes = int(chunk_bytes)
        self.lib = _lib.load()
        if self.lib.acimg_inflate_workspace(self.chunk_bytes, 1, 1, self.chunk_bytes) == 0:
            raise ValueError("chunk_bytes = %d is no power of two in 256..2^24" % self.chunk_bytes)
        self.last_workspace = None              # the workspace of the last call: tests read its debug view

    def inflate_launch(self, streams, sizes):
        """enqueue ONE acimg_inflate call on the current stream -> (out: one uint8 device tensor, the outputs one behind the
        other, status int32 [count] and end_bits int64 [count] ON THE DEVICE); nothing is read back"""
        tensors = [_as_u8(s) for s in streams]
        sizes = [int(n) for n in sizes]
        count = len(tensors)
        if count < 1 or len(sizes) != count:
            raise ValueError("inflate: %d streams with %d sizes" % (count, len(sizes)))
        if any(t.numel() < 1 for t in tensors) or any(not 0 < n <= MAX_SIZE for n in sizes):
            raise ValueError("inflate: every stream has bytes and an expected size in 1..2^31 - 1")
        L = self.lib
        lengths = [int(t.numel()) for t in tensors]
        total_src, total_out = sum(lengths), sum(sizes)
        if all(t.device.type == "cpu" for t in tensors):
            src = torch.cat(tensors).to(self.device) if count > 1 else tensors[0].to(self.device)
        else:
            src = torch.cat([t.to(self.device) for t in tensors]) if count > 1 else tensors[0].to(self.device).contiguous()
        ws_bytes = int(L.acimg_inflate_workspace(total_src, total_out, count, self.chunk_bytes))
        if ws_bytes == 0:
            raise ValueError("inflate: %d streams of %d bytes together are outside the decoder's range" % (count, total_src))
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=self.device)
        out = torch.empty(total_out, dtype=torch.uint8, device=self.device)
        status = torch.empty(count, dtype=torch.int32, device=self.device)
        end_bits = torch.empty(count, dtype=torch.int64, device=self.device)
        _lib.check(L.acimg_inflate(src.data_ptr(), (C.c_long * count)(*lengths), (C.c_long * count)(*sizes), count,
                                   self.chunk_bytes, out.data_ptr(), status.data_ptr(), end_bits.data_ptr(), ws.data_ptr(),
                                   ws_bytes, ops.current_stream_handle(self.device)), "inflate")
        self.last_workspace = ws
        return out, status, end_bits

    def inflate_many(self, streams, sizes):
        """raw streams (bytes-like, arrays or uint8 tensors, on the host or the device) with their expected inflated
        sizes -> (uint8 device tensors, statuses, end bits), the last two as lists on the host.  The tensor of a stream
        whose status is not 0 holds unspecified bytes."""
        out, status, end_bits = self.inflate_launch(streams, sizes)
        return list(torch.split(out, [int(n) for n in sizes])), status.cpu().tolist(), end_bits.cpu().tolist()

    def inflate(self, stream, size):
        """-> the `size` inflated bytes of one raw stream; ValueError when the stream is not exactly that"""
        (out,), (st,), _ = self.inflate_many([stream], [size])
        if st != OK:
            raise ValueError("inflate: the stream is %s (status %d)" % (STATUS_NAMES.get(st, "?"), st))
        return out.cpu().numpy().tobytes()

    def chunk_table(self, nchunks):
        """the debug view of the last call's workspace: its first `nchunks` AcimgInflateChunk records as a numpy array"""
        raw = self.last_workspace[:nchunks * CHUNK_DTYPE.itemsize].cpu().numpy()
        return raw.view(CHUNK_DTYPE)

    # ---- gzip files ------------------------------------------------------------------------------------------------------
    def gunzip_device(self, raws, plans):
        """the device's part for the files with a plan: one call, one copy to PINNED host memory -> per file (data, status,
        end_bits), data a uint8 array; (None, None, None) for a file without a plan"""
        work = [i for i, p in enumerate(plans) if p is not None]
        res = [(None, None, None)] * len(raws)
        if not work:
            return res
        bodies, sizes = [], []
        for i in work:
            off, length, _, isize = plans[i]
            raw = raws[i]
            raw = np.frombuffer(raw, np.uint8) if not isinstance(raw, np.ndarray) else raw
            bodies.append(raw[off:off + length])
            sizes.append(isize)
        out, status, end_bits = self.inflate_launch(bodies, sizes)
        host = torch.empty(sum(sizes), dtype=torch.uint8, pin_memory=True)
        host.copy_(out, non_blocking=True)
        status, end_bits = status.cpu().tolist(), end_bits.cpu().tolist()
        torch.cuda.current_stream(self.device).synchronize()                   # the copy into `host` has landed
        arr, at = host.numpy(), 0
        for k, i in enumerate(work):
            res[i] = (arr[at:at + sizes[k]], status[k], end_bits[k])
            at += sizes[k]
        return res

    def gunzip_many(self, raws):
        """gzip file images -> their inflated bytes as uint8 arrays, in order; all of them in ONE device call"""
        plans = [gzip_plan(r) for r in raws]
        return [gzip_verify(r, p, *d) for r, p, d in zip(raws, plans, self.gunzip_device(raws, plans))]

    def gunzip(self, raw):
        return self.gunzip_many([raw])[0].tobytes()

    def zlib(self, data, size):
        """an RFC 1950 stream that inflates to `size` bytes -> those bytes, the Adler-32 checked on the host"""
        data = bytes(data)
        if len(data) < 7 or (data[0] & 15) != 8 or ((data[0] << 8) | data[1]) % 31 or data[1] & 0x20:
            raise ValueError("no zlib stream without a preset dictionary")
        (dev,), (st,), (end,) = self.inflate_many([data[2:-4]], [size])
        if st != OK or (end + 7) // 8 != len(data) - 6:
            raise ValueError("zlib stream: %s, ends at bit %d of %d bytes" % (STATUS_NAMES.get(st, "?"), end, len(data) - 6))
        out = dev.cpu().numpy().tobytes()
        if struct.unpack(">I", data[-4:])[0] != (_zlib.adler32(out) & 0xFFFFFFFF):
            raise ValueError("zlib stream: Adler-32 mismatch")
        return out
