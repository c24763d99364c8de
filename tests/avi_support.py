"""A RIFF AVI 1.0 reader for the tests, written against the format (not against acimg/avi.py): walks the chunk tree with
its word alignment and returns the header fields, the `movi` chunks with their positions and pad bytes, and `idx1`."""
import struct

STRH = ("fccType", "fccHandler", "dwFlags", "wPriority", "wLanguage", "dwInitialFrames", "dwScale", "dwRate", "dwStart",
        "dwLength", "dwSuggestedBufferSize", "dwQuality", "dwSampleSize", "left", "top", "right", "bottom")
AVIH = ("dwMicroSecPerFrame", "dwMaxBytesPerSec", "dwPaddingGranularity", "dwFlags", "dwTotalFrames", "dwInitialFrames",
        "dwStreams", "dwSuggestedBufferSize", "dwWidth", "dwHeight")


def _chunks(buf, lo, hi):
    """(fourcc, payload start, size) of the chunks in buf[lo:hi]; every chunk starts on an even offset"""
    at = lo
    while at < hi:
        assert at + 8 <= hi, "truncated chunk header at %d" % at
        cc, size = buf[at:at + 4], struct.unpack_from("<I", buf, at + 4)[0]
        assert at + 8 + size <= hi, "chunk %r at %d runs past its parent" % (cc, at)
        yield cc, at + 8, size
        at += 8 + size + (size & 1)
    assert at == hi or at == hi + 1, "chunks end at %d, parent at %d" % (at, hi)


def parse(buf):
    buf = bytes(buf)
    assert buf[:4] == b"RIFF" and buf[8:12] == b"AVI "
    riff = struct.unpack_from("<I", buf, 4)[0]
    assert riff + 8 == len(buf), "RIFF size %d, file %d" % (riff, len(buf))
    out = dict(streams=[], chunks=[], index=[], order=[])
    for cc, at, size in _chunks(buf, 12, len(buf)):
        kind = buf[at:at + 4] if cc == b"LIST" else None
        out["order"].append(kind or cc)
        if kind == b"hdrl":
            for c2, a2, s2 in _chunks(buf, at + 4, at + size):
                if c2 == b"avih":
                    assert s2 == 56
                    out["avih"] = dict(zip(AVIH, struct.unpack_from("<10I", buf, a2)))
                elif c2 == b"LIST" and buf[a2:a2 + 4] == b"strl":
                    st = {}
                    for c3, a3, s3 in _chunks(buf, a2 + 4, a2 + s2):
                        if c3 == b"strh":
                            assert s3 == 56
                            st["strh"] = dict(zip(STRH, struct.unpack_from("<4s4sIHHIIIIIIiI4h", buf, a3)))
                        elif c3 == b"strf":
                            st["strf"] = buf[a3:a3 + s3]
                    out["streams"].append(st)
        elif kind == b"movi":
            out["movi"] = at                                   # position of the 'movi' fourcc
            for c2, a2, s2 in _chunks(buf, at + 4, at + size):
                pad = buf[a2 + s2:a2 + s2 + 1] if s2 & 1 else None
                out["chunks"].append(dict(fourcc=c2, offset=a2 - 8 - at, size=s2, data=buf[a2:a2 + s2], pad=pad))
        elif cc == b"idx1":
            assert size % 16 == 0
            for i in range(size // 16):
                c2, flags, off, s2 = struct.unpack_from("<4sIII", buf, at + 16 * i)
                out["index"].append(dict(fourcc=c2, flags=flags, offset=off, size=s2))
    return out


def bitmap_info(strf):
    keys = ("biSize", "biWidth", "biHeight", "biPlanes", "biBitCount", "biCompression", "biSizeImage")
    return dict(zip(keys, struct.unpack_from("<IiiHH4sI", strf)))


def wave_format(strf):
    keys = ("wFormatTag", "nChannels", "nSamplesPerSec", "nAvgBytesPerSec", "nBlockAlign", "wBitsPerSample", "cbSize")
    return dict(zip(keys, struct.unpack_from("<HHIIHHH", strf)))
