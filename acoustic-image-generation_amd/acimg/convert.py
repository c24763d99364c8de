"""`python -m acimg.convert ROOT_RAW_DIR OUT_DIR [--modalities 1 2] [--list FILE] [--device cuda:0] [--workers N]
[--deflate zlib|device] [--assemble host|device]`:
convert_data.py of the reference - raw recordings (`I_%06d.bmp` frames, one mono WAV) to the GZIP TFRecords of
one-second `SequenceExample`s that every loader of this package reads.

* walk (:182-204): `sorted(glob(ROOT/*/*/video/))`; the class is the `class_<c>` path component, the location `data_<nnn>`,
  `video_time` the integer after the colon on the first line of `<recording>/video_time.txt`; `video_time <= 0` is skipped.
* output (:239-279): `OUT/class_<c>/data_<nnn:03d>/Data_<k:03d>.tfrecord`, k = 1 .. video_time, one record each: context
  `classes`, `location`, `audio_data/mics` = 1, `audio_data/samples` = 1024, `video/height|width|depth` = 224, 298, 3 in
  that order; feature lists `audio/data` and `video/image` of 12 steps.
* audio (:30-36, :226-228): the first fs * video_time samples of `audio/output_audio2.wav` as int32; step j of record k
  is samples [(12 (k - 1) + j) * 1024, + 1024).  Only mono PCM of 16 or 32 bits at 12288 Hz is taken - the rate at which
  those chunks line up with the frames; anything else is refused by name (the reference writes unusable records there).
* video (:141-158): frame `cv2.imread` -> `cv2.resize(..., INTER_CUBIC)` to smallest side 224 (`_smallest_size_at_least`
  with its `int()` truncation) -> central 224 x 298 crop, bytes in BGR order.  OpenCV is not involved: a record's twelve
  BMP FILES go as they are into one pinned buffer and up to the device, where `acimg_resize_cubic_u8` reads the pixels
  in place (header offset, padded and bottom-up rows through its offset / signed row stride) with tables that cover the
  crop window only.  24-bit `BI_RGB` files only; a frame whose resized size is below 224 x 298 is refused (the
  reference slices with a negative offset there), as is a change of geometry inside a recording.
* workers: reading files and building + deflating records run on `--workers` threads; the device does the resize.
  `--deflate device` (default `zlib`): the workers build and frame the records, and the calling thread hands what has
  gathered to ONE `acimg.deflate.DeviceDeflater.compress_many` - RFC 1951 on the device, read by the same loaders.
  `--assemble device` (default `host`; needs `--deflate device`): the resized frames stay in a device pool, the workers
  build only the records' skeletons (`tfio.build_record_layout`), and the calling thread assembles, checksums and
  deflates a batch on the device (`acimg_record_gather`, `acimg_checksum`, `acimg_deflate`): the files are the same bytes.
* a recording with fewer than 12 * video_time frames is refused before anything of it is written.
* `--list FILE`: the produced paths, sorted, one per line - what `--train_file` takes (the list step of framecount.py)."""
import argparse
import collections
import concurrent.futures
import ctypes as C
import glob
import os
import re
import struct
import sys
import time

import numpy as np

NUMBER_OF_SAMPLES = 1024
FRAMES_PER_SECOND = 12
SAMPLE_RATE = NUMBER_OF_SAMPLES * FRAMES_PER_SECOND      # 12288: a frame's chunk of sound lasts exactly a frame
SMALLEST_SIDE = 224
CROP_H, CROP_W = 224, 298
MAX_WORKERS = 16
WAV_NAME = "output_audio2.wav"


class ConvertError(ValueError):
    """an input the converter refuses; the text names the file"""


# ---- BMP ------------------------------------------------------------------------------------------------------------------
BmpLayout = collections.namedtuple("BmpLayout", "height width pixel_offset row_stride file_bytes")


def parse_bmp_header(data, name="<bmp>"):
    """the first 54 bytes of a BMP file -> BmpLayout: the top row starts at `pixel_offset`, row y lies y * `row_stride`
    bytes from it (negative for the usual bottom-up file), `file_bytes` is the least length that holds every row.
    Only what `cv2.imread` reads as plain 8-bit BGR is taken: BITMAPINFOHEADER or later, one plane, 24 bits, BI_RGB."""
    data = bytes(data[:54])
    if len(data) < 54 or data[:2] != b"BM":
        raise ConvertError("%s: not a BMP file" % name)
    offset, hsize = struct.unpack_from("<II", data, 10)
    if hsize < 40:
        raise ConvertError("%s: BMP header of %d bytes (a BITMAPINFOHEADER has 40)" % (name, hsize))
    width, height, planes, bpp, compression = struct.unpack_from("<iiHHI", data, 18)
    if bpp != 24 or compression != 0 or planes != 1:
        raise ConvertError("%s: %d-bit BMP with compression %d: only 24-bit BI_RGB files are converted"
                           % (name, bpp, compression))
    if width < 1 or height == 0 or height == -2 ** 31 or offset < 14 + hsize:
        raise ConvertError("%s: BMP of %d x %d pixels at offset %d" % (name, width, height, offset))
    rows = abs(height)
    pitch = (3 * width + 3) // 4 * 4
    if height > 0:
        return BmpLayout(rows, width, offset + (rows - 1) * pitch, -pitch, offset + (rows - 1) * pitch + 3 * width)
    return BmpLayout(rows, width, offset, pitch, offset + (rows - 1) * pitch + 3 * width)


def bmp_pixels(data, name="<bmp>"):
    """a whole BMP file -> uint8 [H,W,3] in stored (BGR) order, top row first: `cv2.imread` of the file (host; tools and
    tests - the converter itself never unpacks a frame)"""
    lay = parse_bmp_header(data, name)
    buf = np.frombuffer(data, dtype=np.uint8)
    if buf.size < lay.file_bytes:
        raise ConvertError("%s: %d bytes, the pixels need %d" % (name, buf.size, lay.file_bytes))
    rows = [buf[lay.pixel_offset + y * lay.row_stride:][:3 * lay.width] for y in range(lay.height)]
    return np.stack(rows).reshape(lay.height, lay.width, 3)


# ---- WAV ------------------------------------------------------------------------------------------------------------------
def read_wav(path):
    """(sample rate, int32 [samples]) of a mono PCM file of 16 or 32 bits: `np.int32(scipy.io.wavfile.read(path)[1])`"""
    with open(path, "rb") as f:
        data = f.read()
    if len(data) < 12 or data[:4] != b"RIFF" or data[8:12] != b"WAVE":
        raise ConvertError("%s: not a RIFF/WAVE file" % path)
    pos, fmt, samples = 12, None, None
    while pos + 8 <= len(data):
        tag, size = data[pos:pos + 4], struct.unpack_from("<I", data, pos + 4)[0]
        body = data[pos + 8:pos + 8 + size]
        if tag == b"fmt ":
            if len(body) < 16:
                raise ConvertError("%s: fmt chunk of %d bytes" % (path, len(body)))
            fmt = struct.unpack_from("<HHIIHH", body)
            if fmt[0] == 0xFFFE and len(body) >= 26:         # WAVE_FORMAT_EXTENSIBLE: the sub-format's first word
                fmt = (struct.unpack_from("<H", body, 24)[0],) + fmt[1:]
        elif tag == b"data":
            samples = body
            break
        pos += 8 + size + (size & 1)
    if fmt is None or samples is None:
        raise ConvertError("%s: no fmt / data chunk" % path)
    code, channels, rate, _, _, bits = fmt
    if code != 1 or channels != 1 or bits not in (16, 32):
        raise ConvertError("%s: format %d, %d channel(s), %d bits: only mono PCM of 16 or 32 bits is converted"
                           % (path, code, channels, bits))
    width = bits // 8
    a = np.frombuffer(samples[:len(samples) // width * width], dtype="<i%d" % width)
    return int(rate), a.astype(np.int32)


def read_wav_audio_data(path, video_time):
    """`_read_wav_audio_data` (:30-36): the first fs * video_time samples as int32; fs must be 12288"""
    rate, a = read_wav(path)
    if rate != SAMPLE_RATE:
        raise ConvertError("%s: %d Hz: only %d Hz is converted (%d samples for each of %d frames a second; resampling is "
                           "out of scope)" % (path, rate, SAMPLE_RATE, NUMBER_OF_SAMPLES, FRAMES_PER_SECOND))
    need = rate * int(video_time)
    if a.size < need:
        raise ConvertError("%s: %d samples, %d s need %d" % (path, a.size, video_time, need))
    return a[:need]


# ---- geometry -------------------------------------------------------------------------------------------------------------
def smallest_size_at_least(height, width, smallest_side=SMALLEST_SIDE):
    """`_smallest_size_at_least` (:70-93), the `int()` truncation included"""
    height, width, smallest_side = float(height), float(width), float(smallest_side)
    scale = smallest_side / width if height > width else smallest_side / height
    return int(height * scale), int(width * scale)


def crop_geometry(height, width, name="frame"):
    """(new_h, new_w, offset_y, offset_x): the resize target and the central 224 x 298 window of :120-138"""
    new_h, new_w = smallest_size_at_least(height, width)
    if new_h < CROP_H or new_w < CROP_W:
        raise ConvertError("%s: %d x %d (height x width) resizes to %d x %d, below the %d x %d crop"
                           % (name, height, width, new_h, new_w, CROP_H, CROP_W))
    return new_h, new_w, (new_h - CROP_H) // 2, (new_w - CROP_W) // 2


def cubic_tables(n_in, n_out, first=0, count=None):
    """(idx int32 [count,4], coef int16 [count,4]) of `acimg_resize_cubic_tables`"""
    from . import _lib
    count = n_out - first if count is None else count
    idx = np.zeros((max(count, 1), 4), np.int32)
    coef = np.zeros((max(count, 1), 4), np.int16)
    _lib.check(_lib.load().acimg_resize_cubic_tables(int(n_in), int(n_out), int(first), int(count),
                                                     idx.ctypes.data_as(C.c_void_p), coef.ctypes.data_as(C.c_void_p)),
               "resize_cubic_tables")
    return idx, coef


class FrameResizer(object):
    """INTER_CUBIC resize of H x W frames to (new_h, new_w) and the window [off_y, off_y + out_h) x [off_x, off_x + out_w)
    of the result, on `device`.  Default: the converter's geometry (`crop_geometry`).  The tables are built once."""

    def __init__(self, device, height, width, new_size=None, window=None):
        import torch
        self.device = torch.device(device)
        self.height, self.width = int(height), int(width)
        if new_size is None:
            new_h, new_w, off_y, off_x = crop_geometry(height, width)
            out_h, out_w = CROP_H, CROP_W
        else:
            new_h, new_w = new_size
            off_y, off_x, out_h, out_w = window if window is not None else (0, 0, new_h, new_w)
        self.new_size, self.window = (int(new_h), int(new_w)), (int(off_y), int(off_x), int(out_h), int(out_w))
        self.out_h, self.out_w = int(out_h), int(out_w)
        tabs = cubic_tables(height, new_h, off_y, out_h) + cubic_tables(width, new_w, off_x, out_w)
        self.tables = tuple(torch.from_numpy(t).to(self.device) for t in tabs)

    def resize(self, src, frame_stride, pixel_offset, row_stride, n, out=None):
        """src: uint8 device tensor holding n frames `frame_stride` bytes apart, each frame's top row at `pixel_offset`,
        rows `row_stride` (signed) bytes apart -> uint8 [n, out_h, out_w, 3] on the device (stream-ordered)"""
        import torch

        from . import _lib, ops
        if src.dtype != torch.uint8 or src.device != self.device or not src.is_contiguous():
            raise ValueError("src is a contiguous uint8 tensor on %s" % self.device)
        if n < 1 or src.numel() < n * int(frame_stride):
            raise ValueError("%d frames of stride %d in a buffer of %d bytes" % (n, frame_stride, src.numel()))
        if out is None:
            out = torch.empty(n, self.out_h, self.out_w, 3, dtype=torch.uint8, device=self.device)
        elif (out.dtype != torch.uint8 or tuple(out.shape) != (n, self.out_h, self.out_w, 3) or not out.is_contiguous()
              or out.device != self.device):
            raise ValueError("out is a contiguous uint8 [%d,%d,%d,3] tensor on %s" % (n, self.out_h, self.out_w, self.device))
        iy, cy, ix, cx = self.tables
        _lib.check(_lib.load().acimg_resize_cubic_u8(
            src.data_ptr(), int(frame_stride), int(pixel_offset), int(row_stride), int(n), self.height, self.width,
            iy.data_ptr(), cy.data_ptr(), ix.data_ptr(), cx.data_ptr(), self.out_h, self.out_w, out.data_ptr(),
            ops.current_stream_handle(self.device)), "resize_cubic_u8")
        return out

    def resize_frames(self, frames):
        """uint8 [n,H,W,3] dense (host array or tensor) -> uint8 [n, out_h, out_w, 3] on the device"""
        import torch
        f = torch.as_tensor(frames).to(self.device).contiguous()
        if f.dtype != torch.uint8 or f.dim() != 4 or tuple(f.shape[1:]) != (self.height, self.width, 3):
            raise ValueError("frames are uint8 [n,%d,%d,3], got %s %s" % (self.height, self.width, f.dtype, tuple(f.shape)))
        return self.resize(f.reshape(-1), self.height * self.width * 3, 0, self.width * 3, int(f.shape[0]))


# ---- the walk (:182-204) --------------------------------------------------------------------------------------------------
Recording = collections.namedtuple("Recording", "directory classes location video_time video_dir wav")


def read_video_time(path):
    try:
        with open(path) as f:
            return int(f.readline().split(":")[1].strip())
    except (OSError, IndexError, ValueError) as e:
        raise ConvertError("%s: no `<name>: <seconds>` first line (%s)" % (path, e))


def _component_number(parts, prefix, video_dir):
    hits = [p for p in parts if re.match(prefix + "_.*", p)]
    try:
        return int(hits[0].split("_")[1])
    except (IndexError, ValueError):
        raise ConvertError("%s: no %s_<number> path component" % (video_dir, prefix))


def find_recordings(root_raw_dir):
    """every `ROOT/*/*/video/` in sorted order -> [Recording]; recordings with video_time <= 0 are left out (:200)"""
    out = []
    for video_dir in sorted(glob.glob("{}/*/*/video/".format(root_raw_dir))):
        parts = video_dir.split("/")
        directory = "/".join(parts[:-2])
        video_time = read_video_time(directory + "/video_time.txt")
        if video_time <= 0:
            continue
        out.append(Recording(directory, _component_number(parts, "class", video_dir),
                             _component_number(parts, "data", video_dir), video_time, video_dir.rstrip("/"),
                             "{}/audio/{}".format(directory, WAV_NAME)))
    return out


def frame_path(video_dir, index):
    """frame `index` (from 1) of a recording"""
    return "{}/I_{:06d}.bmp".format(video_dir, index)


def record_path(out_dir, rec, k):
    return "{}/class_{}/data_{:0>3d}/Data_{:0>3d}.tfrecord".format(out_dir, rec.classes, rec.location, k)


def build_record(rec, audio_steps, video_steps):
    """the serialized SequenceExample of :250-278; a modality that is None is left out as there"""
    from . import tfio
    ctx = collections.OrderedDict((("classes", np.array([rec.classes])), ("location", np.array([rec.location]))))
    lists = collections.OrderedDict()
    if audio_steps is not None:
        ctx["audio_data/mics"] = np.array([1])
        ctx["audio_data/samples"] = np.array([NUMBER_OF_SAMPLES])
        lists["audio/data"] = [np.ascontiguousarray(a, dtype="<i4").tobytes() for a in audio_steps]
    if video_steps is not None:
        ctx["video/height"] = np.array([video_steps.shape[1]])
        ctx["video/width"] = np.array([video_steps.shape[2]])
        ctx["video/depth"] = np.array([video_steps.shape[3]])
        lists["video/image"] = [f.tobytes() for f in video_steps]
    return tfio.build_sequence_example(ctx, lists)


def _write_record(path, rec, audio_steps, video_steps):
    """worker: build, deflate and write one record; returns seconds spent"""
    from . import tfio
    t0 = time.perf_counter()
    os.makedirs(os.path.dirname(path), exist_ok=True)
    tfio.write_tfrecord(path, [build_record(rec, audio_steps, video_steps)], compression="GZIP")
    return time.perf_counter() - t0


def _frame_record(path, rec, audio_steps, video_steps):
    """worker of `--deflate device`: build and frame one record -> (path, the file's uncompressed bytes, seconds spent)"""
    from . import tfio
    t0 = time.perf_counter()
    os.makedirs(os.path.dirname(path), exist_ok=True)
    buf = tfio.frame_record(build_record(rec, audio_steps, video_steps))
    return path, buf, time.perf_counter() - t0


def build_record_layout(rec, audio_steps, frame_bytes, shape):
    """`tfio.frame_record(build_record(...))` as a layout: the video frames (shape = (steps, H, W, depth), None: no video)
    are external values of `frame_bytes` bytes each"""
    from . import tfio
    ctx = collections.OrderedDict((("classes", np.array([rec.classes])), ("location", np.array([rec.location]))))
    lists = collections.OrderedDict()
    if audio_steps is not None:
        ctx["audio_data/mics"] = np.array([1])
        ctx["audio_data/samples"] = np.array([NUMBER_OF_SAMPLES])
        lists["audio/data"] = [np.ascontiguousarray(a, dtype="<i4").tobytes() for a in audio_steps]
    if shape is not None:
        ctx["video/height"] = np.array([shape[1]])
        ctx["video/width"] = np.array([shape[2]])
        ctx["video/depth"] = np.array([shape[3]])
        lists["video/image"] = [tfio.External(frame_bytes) for _ in range(shape[0])]
    return tfio.build_record_layout(ctx, lists)


def _layout_record(path, rec, audio_steps, slot):
    """worker of `--assemble device`: the record's skeleton -> (path, layout, pool slot or None, seconds spent)"""
    t0 = time.perf_counter()
    os.makedirs(os.path.dirname(path), exist_ok=True)
    shape = None if slot is None else (FRAMES_PER_SECOND, CROP_H, CROP_W, 3)
    layout = build_record_layout(rec, audio_steps, CROP_H * CROP_W * 3, shape)
    return path, layout, slot, time.perf_counter() - t0


def _read_frame(path, row, layout):
    """worker: one BMP file as it is into `row` (a uint8 view of the pinned staging buffer); returns seconds spent"""
    t0 = time.perf_counter()
    with open(path, "rb") as f:
        got = f.readinto(memoryview(row))        # the row holds layout.file_bytes: all but the last row's padding
    if got < 54:
        raise ConvertError("%s: %d bytes are no BMP file" % (path, got))
    lay = parse_bmp_header(row[:54].tobytes(), path)
    if lay != layout or got < lay.file_bytes:
        raise ConvertError("%s: %d x %d pixels in %d bytes, the recording's first frame has %d x %d in %d: all frames of a "
                           "recording share one geometry" % (path, lay.height, lay.width, got, layout.height, layout.width,
                                                             layout.file_bytes))
    return time.perf_counter() - t0


DEFLATE_CHOICES = ("zlib", "device")
ASSEMBLE_CHOICES = ("host", "device")


def make_deflater(deflate, device):
    """'zlib' -> None (the workers write through gzip.open); 'device' -> a DeviceDeflater"""
    if deflate not in DEFLATE_CHOICES:
        raise ConvertError("--deflate is one of %s, got %r" % (", ".join(DEFLATE_CHOICES), deflate))
    if deflate == "zlib":
        return None
    from .deflate import DeviceDeflater
    return DeviceDeflater(device)


def drain_writes(writes, keep, deflater):
    """wait for the oldest futures of `writes` until `keep` are left -> seconds of deflate.  With a deflater the futures
    hold framed records, not written files: they are taken once twice `keep` have gathered (all of them for keep = 0),
    compressed in one `compress_many` and written here."""
    if deflater is None:
        seconds = 0.0
        while len(writes) > keep:
            seconds += writes.popleft().result()
        return seconds
    if keep and len(writes) <= 2 * keep:
        return 0.0
    ready = []
    while len(writes) > keep:
        ready.append(writes.popleft().result())
    if not ready:
        return 0.0
    from .deflate import write_gzip_files
    t0 = time.perf_counter()
    write_gzip_files(deflater, [(path, buf) for path, buf, _ in ready])
    return sum(r[2] for r in ready) + time.perf_counter() - t0


class DeviceAssembler(object):
    """`--assemble device`: a pool of frame slots on the device and the batch step that turns skeletons + slots into gzip
    files.  One stream carries, for the whole batch: one skeleton upload, one `acimg_record_gather`, one `acimg_checksum`
    (masked CRC-32C of the data spans, stored into the trailers), one `acimg_checksum` (CRC-32 of the framed records), one
    `acimg_deflate`; then byte counts and CRCs come back in one small transfer and the packed streams in another."""

    SLOT_BYTES = FRAMES_PER_SECOND * CROP_H * CROP_W * 3

    def __init__(self, deflater, slots):
        import torch

        from .checksum import DeviceChecksum
        self.deflater, self.device = deflater, deflater.device
        self.sums = DeviceChecksum(self.device)
        self.pool = torch.empty(int(slots), self.SLOT_BYTES, dtype=torch.uint8, device=self.device)
        self.free = collections.deque(range(int(slots)))

    def slot_frames(self, slot):
        return self.pool[slot].view(FRAMES_PER_SECOND, CROP_H, CROP_W, 3)

    def write(self, ready):
        """ready: [(path, RecordLayout, slot or None)] -> the files; the slots are free again on return"""
        import torch

        from .checksum import CRC32, CRC32C_MASKED
        from .deflate import GZIP_HEADER
        frame = CROP_H * CROP_W * 3
        skeleton = b"".join(lay.skeleton for _, lay, _ in ready)
        sizes = [len(lay.skeleton) for _, lay, _ in ready]
        segments, spans, stores, base = [], [], [], 0
        for _, lay, slot in ready:
            for off, n in lay.pieces():
                segments.append((base + off, base + off, n, 0))
            for j, (off, n) in enumerate(lay.holes):
                segments.append((base + off, slot * self.SLOT_BYTES + j * frame, n, 1))
            if spans:                               # the trailer before this record and its 12-byte header: a payload of
                spans.append(16)                    # no interest that keeps the data spans one behind the other
                stores.append(-1)
            spans.append(lay.data[1])
            stores.append(base + lay.trailer)
            base += len(lay.skeleton)
        src0 = torch.from_numpy(np.frombuffer(skeleton, np.uint8).copy()).to(self.device, non_blocking=False)
        framed = torch.empty(base, dtype=torch.uint8, device=self.device)
        self.sums.gather(src0, self.pool.view(-1), segments, framed)
        self.sums.packed(framed[12:], spans, CRC32C_MASKED, framed, stores)
        crcs = self.sums.packed(framed, sizes, CRC32)
        streams, values = self.deflater._download(*self.deflater._launch(framed, sizes), sums=crcs)
        for _, _, slot in ready:
            if slot is not None:
                self.free.append(slot)
        for (path, _, _), stream, crc, n in zip(ready, streams, values, sizes):
            with open(path, "wb") as f:
                f.write(GZIP_HEADER + stream + struct.pack("<II", crc, n & 0xFFFFFFFF))


class Converter(object):
    """The pipeline of one `convert` call: `workers` threads read frames into pinned buffers and deflate finished
    records; the calling thread uploads a record's files, launches the resize and brings the 12 frames back.
    `times`: seconds in read and deflate (summed over the workers), and in upload + resize + download (wall).
    `deflate="device"`: the workers only build and frame the records; the calling thread compresses what is ready in one
    `DeviceDeflater.compress_many` and writes the files (its seconds count as deflate too).
    `assemble="device"` (with `deflate="device"`): the frames stay in a `DeviceAssembler`'s pool, the workers build
    skeletons, and the calling thread assembles, checksums and deflates what is ready on the device."""

    def __init__(self, out_dir, modalities=None, device="cuda:0", workers=4, log=None, deflate="zlib", assemble="host"):
        if assemble not in ASSEMBLE_CHOICES:
            raise ConvertError("--assemble is one of %s, got %r" % (", ".join(ASSEMBLE_CHOICES), assemble))
        if assemble == "device" and deflate != "device":
            raise ConvertError("--assemble device needs --deflate device (the host's zlib wants the record in host memory)")
        self.out_dir = out_dir
        self.audio = modalities is None or 1 in modalities
        self.video = modalities is None or 2 in modalities
        self.device = device
        self.workers = max(1, min(int(workers), MAX_WORKERS))
        self.log = log or (lambda *a: None)
        self.times = dict(read=0.0, device=0.0, deflate=0.0)
        self.records = 0
        self._exec = concurrent.futures.ThreadPoolExecutor(max_workers=self.workers, thread_name_prefix="acimg-convert")
        self._writes = collections.deque()
        self._deflater = make_deflater(deflate, device)
        # a batch is taken once more than 4 * workers records have gathered (drain_writes' rule) and its slots are free
        # again when it has been downloaded: 4 * workers + 2 slots always leave one for the record being resized
        self._assembler = DeviceAssembler(self._deflater, 4 * self.workers + 2) if assemble == "device" else None

    def close(self):
        self._drain(0)
        self._exec.shutdown(wait=True)

    def _drain(self, keep):
        if self._assembler is None:
            self.times["deflate"] += drain_writes(self._writes, keep, self._deflater)
            return
        if keep and len(self._writes) <= 2 * keep:
            return
        ready = []
        while len(self._writes) > keep:
            ready.append(self._writes.popleft().result())
        if ready:
            t0 = time.perf_counter()
            self._assembler.write([r[:3] for r in ready])
            self.times["deflate"] += sum(r[3] for r in ready) + time.perf_counter() - t0

    def _check(self, rec):
        """everything that can be refused before a byte of the recording is written -> (audio, layout)"""
        audio = read_wav_audio_data(rec.wav, rec.video_time) if self.audio else None
        layout = None
        if self.video:
            need = FRAMES_PER_SECOND * rec.video_time
            for i in range(1, need + 1):
                if not os.path.isfile(frame_path(rec.video_dir, i)):
                    raise ConvertError("%s: frame %d of the %d that %d s need is missing"
                                       % (frame_path(rec.video_dir, i), i, need, rec.video_time))
            first = frame_path(rec.video_dir, 1)
            with open(first, "rb") as f:
                layout = parse_bmp_header(f.read(54), first)
            if os.path.getsize(first) < layout.file_bytes:
                raise ConvertError("%s: %d bytes, the pixels need %d" % (first, os.path.getsize(first), layout.file_bytes))
            crop_geometry(layout.height, layout.width, first)
        return audio, layout

    def recording(self, rec):
        """convert one recording -> the paths written"""
        import torch
        audio, layout = self._check(rec)
        paths = [record_path(self.out_dir, rec, k) for k in range(1, rec.video_time + 1)]
        if self.video:
            resizer = FrameResizer(self.device, layout.height, layout.width)
            stride = layout.file_bytes
            staging = [torch.empty(FRAMES_PER_SECOND, stride, dtype=torch.uint8).pin_memory() for _ in range(2)]
            if self._assembler is None:
                host = [torch.empty(FRAMES_PER_SECOND, CROP_H, CROP_W, 3, dtype=torch.uint8).pin_memory() for _ in range(2)]
            dev = torch.empty(FRAMES_PER_SECOND, stride, dtype=torch.uint8, device=resizer.device)

            def read(k):      # record k (from 0) into staging set k % 2
                rows = staging[k % 2].numpy()
                return [self._exec.submit(_read_frame, frame_path(rec.video_dir, FRAMES_PER_SECOND * k + j + 1), rows[j], layout)
                        for j in range(FRAMES_PER_SECOND)]
            reads = read(0)
        for k in range(rec.video_time):
            audio_steps = video_steps = slot = None
            if self.audio:
                lo = FRAMES_PER_SECOND * k * NUMBER_OF_SAMPLES
                audio_steps = audio[lo:lo + FRAMES_PER_SECOND * NUMBER_OF_SAMPLES].reshape(FRAMES_PER_SECOND, NUMBER_OF_SAMPLES)
            if self.video:
                self.times["read"] += sum(f.result() for f in reads)
                if k + 1 < rec.video_time:
                    reads = read(k + 1)
                t0 = time.perf_counter()
                dev.copy_(staging[k % 2], non_blocking=True)
                if self._assembler is not None:     # the frames stay on the device, in a slot of the pool
                    slot = self._assembler.free.popleft()
                    resizer.resize(dev.reshape(-1), stride, layout.pixel_offset, layout.row_stride, FRAMES_PER_SECOND,
                                   out=self._assembler.slot_frames(slot))
                else:
                    out = resizer.resize(dev.reshape(-1), stride, layout.pixel_offset, layout.row_stride, FRAMES_PER_SECOND)
                    host[k % 2].copy_(out, non_blocking=True)
                torch.cuda.current_stream(resizer.device).synchronize()
                self.times["device"] += time.perf_counter() - t0
                if self._assembler is None:
                    video_steps = host[k % 2].numpy().copy()
            if self._assembler is not None:
                self._writes.append(self._exec.submit(_layout_record, paths[k], rec, audio_steps, slot))
            else:
                self._writes.append(self._exec.submit(_write_record if self._deflater is None else _frame_record, paths[k], rec,
                                                      audio_steps, video_steps))
            self._drain(2 * self.workers)
            self.records += 1
            self.log("{} - Writing {}".format(time.strftime("%Y-%m-%d %H:%M:%S"), paths[k]))
        return paths


def convert(root_raw_dir, out_dir, modalities=None, list_file=None, device="cuda:0", workers=4, log=None, deflate="zlib",
            assemble="host"):
    """the whole data set -> (sorted list of the files written, the Converter with its `times`)"""
    root_raw_dir = os.path.abspath(os.path.expanduser(root_raw_dir))
    out_dir = os.path.abspath(os.path.expanduser(out_dir))
    conv = Converter(out_dir, modalities, device, workers, log, deflate, assemble)
    paths = []
    try:
        for rec in find_recordings(root_raw_dir):
            paths += conv.recording(rec)
    finally:
        conv.close()
    paths.sort()
    if list_file:
        with open(list_file, "w") as f:
            f.write("".join(p + "\n" for p in paths))
    return paths, conv


def _str2dir(name):
    if not os.path.isdir(name):
        raise argparse.ArgumentTypeError("{} is not a directory!".format(name))
    return os.path.abspath(os.path.expanduser(name))


def build_parser():
    p = argparse.ArgumentParser(prog="python -m acimg.convert", description=__doc__.split("\n\n")[0])
    p.add_argument("root_raw_dir", help="Synchronized raw files data set root directory", type=_str2dir)
    p.add_argument("out_dir", help="Directory where to store the converted data", type=_str2dir)
    p.add_argument("--modalities", help="Modalities to consider. 0: Audio images. 1: Audio data. 2: Video data.",
                   nargs="*", type=int)
    p.add_argument("--list", dest="list_file", help="write the produced paths, sorted, one per line (a --train_file)")
    p.add_argument("--device", default="cuda:0")
    p.add_argument("--workers", type=int, default=4, help="threads that read frames and deflate records (at most 16)")
    p.add_argument("--deflate", default="zlib", choices=DEFLATE_CHOICES,
                   help="zlib: the workers gzip the records (level 9); device: the GPU deflates them, batched")
    p.add_argument("--assemble", default="host", choices=ASSEMBLE_CHOICES,
                   help="device (needs --deflate device): records are assembled and checksummed on the GPU, the same bytes")
    return p


def main(argv=None):
    args = build_parser().parse_args(argv)
    paths, conv = convert(args.root_raw_dir, args.out_dir, args.modalities, args.list_file, args.device, args.workers,
                          log=print, deflate=args.deflate, assemble=args.assemble)
    print("{} records; seconds in read {:.2f}, upload + resize {:.2f}, deflate {:.2f}".format(
        len(paths), conv.times["read"], conv.times["device"], conv.times["deflate"]))
    return 0


if __name__ == "__main__":
    sys.exit(main())
