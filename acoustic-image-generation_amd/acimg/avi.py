"""A RIFF AVI 1.0 writer on the standard library (struct): one Motion-JPEG video stream and one 16-bit mono PCM stream,
interleaved frame by frame - the clip `python -m acimg.show video --avi 1` writes where showvideo.py:239-263 runs ffmpeg
twice.  `hdrl` holds `avih`, a `vids` / `MJPG` stream list (BITMAPINFOHEADER, 24 bit) and an `auds` stream list (PCM
WAVEFORMATEX); `movi` holds per frame one `00dc` chunk (a complete JPEG file) followed by one `01wb` chunk (that frame's
samples); `idx1` lists every chunk, each flagged a key frame.  Chunks are word-aligned (one zero pad byte after an odd
payload, not counted in the chunk's size).  The counts in the headers are patched on `close()`.  No OpenDML: the file
stays below 2 GB (a ten-second clip is a few MB)."""
import struct

import numpy as np

AVIF_HASINDEX, AVIF_ISINTERLEAVED = 0x10, 0x100
AVIIF_KEYFRAME = 0x10
WAVE_FORMAT_PCM = 1
RIFF_LIMIT = (1 << 31) - 1


def normalize_pcm(samples):
    """integer samples of a whole clip -> int16: x / max|x| * 32767, rounded (the peak normalisation of video.py:48 on a
    16-bit track); a silent clip stays zeros"""
    x = np.asarray(samples).astype(np.float64).reshape(-1)
    peak = float(np.abs(x).max()) if x.size else 0.0
    if peak == 0.0:
        return np.zeros(x.shape, np.int16)
    return np.rint(x / peak * 32767.0).astype(np.int16)


def _chunk(fourcc, payload):
    return fourcc + struct.pack("<I", len(payload)) + payload + (b"\x00" if len(payload) & 1 else b"")


class AviWriter(object):
    """`add_frame(jpeg, pcm)` per frame, then `close()`.  fps: frames per second (an integer: dwRate over dwScale 1);
    sample_rate: PCM samples per second."""

    def __init__(self, path, width, height, fps, sample_rate):
        self.path = path
        self.width, self.height, self.fps, self.sample_rate = int(width), int(height), int(fps), int(sample_rate)
        if min(self.width, self.height, self.fps, self.sample_rate) < 1:
            raise ValueError("width, height, fps and sample_rate are positive")
        self.frames = self.samples = 0
        self.max_video = self.max_audio = 0
        self.index = []                         # (fourcc, offset from the 'movi' fourcc, payload size)
        self.f = open(path, "wb")
        self.f.write(self._headers(0))
        self.movi = self.f.tell() - 4           # position of the 'movi' fourcc
        self.bytes_written = None

    def _headers(self, movi_bytes):
        """everything up to and including the 'movi' fourcc, with the counts as they stand"""
        w, h = self.width, self.height
        rate = self.sample_rate * 2
        avih = struct.pack("<14I", 1000000 // self.fps, self.max_video * self.fps + rate, 0,
                           AVIF_HASINDEX | AVIF_ISINTERLEAVED, self.frames, 0, 2, max(self.max_video, self.max_audio), w, h,
                           0, 0, 0, 0)
        vstrh = b"vids" + b"MJPG" + struct.pack("<IHHIIIIIIiI4h", 0, 0, 0, 0, 1, self.fps, 0, self.frames, self.max_video,
                                                -1, 0, 0, 0, w, h)
        vstrf = struct.pack("<IiiHH4sIiiII", 40, w, h, 1, 24, b"MJPG", w * h * 3, 0, 0, 0, 0)
        astrh = b"auds" + b"\x00\x00\x00\x00" + struct.pack("<IHHIIIIIIiI4h", 0, 0, 0, 0, 1, self.sample_rate, 0, self.samples,
                                                            self.max_audio, -1, 2, 0, 0, 0, 0)
        astrf = struct.pack("<HHIIHHH", WAVE_FORMAT_PCM, 1, self.sample_rate, rate, 2, 16, 0)
        hdrl = b"hdrl" + _chunk(b"avih", avih)
        hdrl += _chunk(b"LIST", b"strl" + _chunk(b"strh", vstrh) + _chunk(b"strf", vstrf))
        hdrl += _chunk(b"LIST", b"strl" + _chunk(b"strh", astrh) + _chunk(b"strf", astrf))
        head = _chunk(b"LIST", hdrl) + b"LIST" + struct.pack("<I", 4 + movi_bytes) + b"movi"
        riff = 4 + len(head) + movi_bytes + 8 + 16 * len(self.index)
        if riff > RIFF_LIMIT:
            raise ValueError("an AVI 1.0 file holds less than 2 GB")
        return b"RIFF" + struct.pack("<I", riff) + b"AVI " + head

    def _add(self, fourcc, payload):
        self.index.append((fourcc, self.f.tell() - self.movi, len(payload)))
        self.f.write(_chunk(fourcc, payload))

    def add_frame(self, jpeg, pcm):
        """jpeg: the bytes of one complete JPEG file; pcm: this frame's int16 samples (array or little-endian bytes)"""
        if self.f is None:
            raise ValueError("the file is closed")
        audio = pcm if isinstance(pcm, (bytes, bytearray)) else np.ascontiguousarray(pcm, dtype="<i2").tobytes()
        if len(audio) & 1:
            raise ValueError("16-bit samples take an even number of bytes")
        self._add(b"00dc", bytes(jpeg))
        self._add(b"01wb", bytes(audio))
        self.frames += 1
        self.samples += len(audio) // 2
        self.max_video, self.max_audio = max(self.max_video, len(jpeg)), max(self.max_audio, len(audio))

    def close(self):
        """write `idx1`, patch the sizes and counts of the headers; returns the file's size in bytes"""
        if self.f is None:
            return self.bytes_written
        movi_bytes = self.f.tell() - (self.movi + 4)
        idx = b"".join(cc + struct.pack("<III", AVIIF_KEYFRAME, off, size) for cc, off, size in self.index)
        self.f.write(_chunk(b"idx1", idx))
        self.bytes_written = self.f.tell()
        self.f.seek(0)
        self.f.write(self._headers(movi_bytes))
        self.f.close()
        self.f = None
        return self.bytes_written

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False
