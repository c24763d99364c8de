"""TensorBoard event files without TensorFlow or the tensorboard package: what `tf.summary.FileWriter` leaves for the
reference's logger (logger/logger.py, trainer/mfcctrainer.py:255-297,343-357,373-378).

An event file is a sequence of uncompressed TFRecords (`tfio`'s framing: masked CRC-32C of the length and of the
payload), each one serialized `Event`.  The first holds `file_version = "brain.Event:2"`; every other one a `Summary`
of `Summary.Value`s at a step.  Field numbers (the public event.proto / summary.proto):

    Event          wall_time = 1 (double), step = 2 (int64), file_version = 3 (string), summary = 5
    Summary        value = 1 (repeated)
    Summary.Value  tag = 1, simple_value = 2 (float), image = 4, histo = 5
    Summary.Image  height = 1, width = 2, colorspace = 3, encoded_image_string = 4
    HistogramProto min = 1, max = 2, num = 3, sum = 4, sum_squares = 5 (doubles), bucket_limit = 6, bucket = 7 (packed)

Images are PNGs from `png.encode_png`: the pixels TensorFlow would write, not its zlib stream.  `read_events` decodes a
file into plain dicts (tests, and users without TensorBoard).
"""
import os
import re
import socket
import struct
import sys
import time

import numpy as np

from . import png, tfio
from .tfio import _fields, _key, _ld, _put_varint, _signed64

FILE_VERSION = "brain.Event:2"
DBL_MAX = sys.float_info.max

_BAD_TAG_CHAR = re.compile(r"[^-/\w\.]", re.ASCII)


def sanitize_tag(name):
    """TF-1's rule for summary names: every character outside [A-Za-z0-9_.-/] becomes '_', a leading '/' is stripped
    ('l2 loss' -> 'l2_loss', 'kernel:0' -> 'kernel_0')"""
    return _BAD_TAG_CHAR.sub("_", name).lstrip("/")


def image_tags(name, max_outputs):
    """the tags tf.summary.image(name, ..., max_outputs) writes: name/image, or name/image/<i> for more than one"""
    base = sanitize_tag(name)
    if int(max_outputs) == 1:
        return [base + "/image"]
    return ["%s/image/%d" % (base, i) for i in range(int(max_outputs))]


# ---- histogram buckets --------------------------------------------------------------------------------------------------
_LIMITS = None


def default_bucket_limits():
    """TF's default histogram limits: v = 1e-12, v *= 1.1 while v < 1e20 (774 values), then DBL_MAX; the mirrored
    negatives in front with 0.0 between: 1551 ascending doubles"""
    global _LIMITS
    if _LIMITS is None:
        pos = []
        v = 1e-12
        while v < 1e20:
            pos.append(v)
            v *= 1.1
        pos.append(DBL_MAX)
        _LIMITS = tuple([-x for x in reversed(pos)] + [0.0] + pos)
    return list(_LIMITS)


def compress_buckets(counts, limits):
    """TF's EncodeToProto: walk the buckets; a run of empty buckets collapses into one entry that carries the run's last
    limit and a count of 0; nothing emitted -> one entry (DBL_MAX, 0).  Returns (bucket_limit, bucket) lists."""
    out_l, out_c = [], []
    n, i = len(counts), 0
    while i < n:
        end, count = float(limits[i]), float(counts[i])
        i += 1
        if count <= 0.0:
            while i < n and counts[i] <= 0:
                end, count = float(limits[i]), float(counts[i])
                i += 1
        out_l.append(end)
        out_c.append(count)
    if not out_l:
        out_l, out_c = [DBL_MAX], [0.0]
    return out_l, out_c


# ---- encoders -------------------------------------------------------------------------------------------------------------
def _double(fn, x):
    return _key(fn, 1) + struct.pack("<d", float(x))


def _packed_doubles(fn, xs):
    return _ld(fn, struct.pack("<%dd" % len(xs), *[float(x) for x in xs]))


def scalar_value(tag, x):
    """Summary.Value{tag, simple_value}: the value as a float32"""
    return _ld(1, tag.encode("utf-8")) + _key(2, 5) + struct.pack("<f", float(np.float32(x)))


def image_value(tag, rgb_uint8):
    """Summary.Value{tag, image}: [H,W,3] uint8 -> Summary.Image{height, width, colorspace = 3, PNG}"""
    a = np.asarray(rgb_uint8)
    img = (_key(1, 0) + _put_varint(int(a.shape[0])) + _key(2, 0) + _put_varint(int(a.shape[1])) + _key(3, 0)
           + _put_varint(3) + _ld(4, png.encode_png(a)))
    return _ld(1, tag.encode("utf-8")) + _ld(4, img)


def histogram_value(tag, min, max, num, sum, sum_squares, counts, limits):
    """Summary.Value{tag, histo}: counts [L] over limits [L], compressed as `compress_buckets`"""
    bl, bc = compress_buckets(counts, limits)
    h = (_double(1, min) + _double(2, max) + _double(3, num) + _double(4, sum) + _double(5, sum_squares)
         + _packed_doubles(6, bl) + _packed_doubles(7, bc))
    return _ld(1, tag.encode("utf-8")) + _ld(5, h)


def _event(wall_time, step=0, file_version=None, values=None):
    e = _double(1, wall_time)
    if step:
        e += _key(2, 0) + _put_varint(int(step))
    if file_version is not None:
        e += _ld(3, file_version.encode("utf-8"))
    if values is not None:
        e += _ld(5, b"".join(_ld(1, v) for v in values))
    return e


def _frame(record):
    head = struct.pack("<Q", len(record))
    return (head + struct.pack("<I", tfio.mask_crc(tfio.crc32c(head))) + record
            + struct.pack("<I", tfio.mask_crc(tfio.crc32c(record))))


class EventFileWriter(object):
    """`<logdir>/events.out.tfevents.<int(clock()):010d>.<hostname>`; the first record is the version event.  `clock`
    and `hostname` are injectable: with both fixed, the file name and every byte are reproducible."""

    def __init__(self, logdir, clock=time.time, hostname=None):
        os.makedirs(logdir, exist_ok=True)
        self.clock = clock
        host = socket.gethostname() if hostname is None else hostname
        now = clock()
        self.path = os.path.join(logdir, "events.out.tfevents.%010d.%s" % (int(now), host))
        self._f = open(self.path, "wb")
        self._f.write(_frame(_event(now, file_version=FILE_VERSION)))

    def add_summary(self, values, step):
        """values: a list of encoded Summary.Value"""
        self._f.write(_frame(_event(self.clock(), step=step, values=list(values))))

    def flush(self):
        if self._f is not None:
            self._f.flush()

    def close(self):
        if self._f is not None:
            self._f.close()
            self._f = None


# ---- reader ---------------------------------------------------------------------------------------------------------------
def _f64(v):
    return struct.unpack("<d", struct.pack("<Q", v))[0]


def _doubles(wt, v):
    if wt == 2:
        b = bytes(v)
        return list(struct.unpack("<%dd" % (len(b) // 8), b))
    return [_f64(v)]


def _read_histo(buf):
    h = dict(min=0.0, max=0.0, num=0.0, sum=0.0, sum_squares=0.0, bucket_limit=[], bucket=[])
    names = {1: "min", 2: "max", 3: "num", 4: "sum", 5: "sum_squares"}
    for fn, wt, v in _fields(buf):
        if fn in names:
            h[names[fn]] = _f64(v)
        elif fn == 6:
            h["bucket_limit"] += _doubles(wt, v)
        elif fn == 7:
            h["bucket"] += _doubles(wt, v)
    return h


def _read_image(buf):
    im = dict(height=0, width=0, colorspace=0, encoded_image_string=b"")
    names = {1: "height", 2: "width", 3: "colorspace"}
    for fn, wt, v in _fields(buf):
        if fn in names:
            im[names[fn]] = int(v)
        elif fn == 4:
            im["encoded_image_string"] = bytes(v)
    return im


def _read_value(buf):
    out = dict(tag="")
    for fn, wt, v in _fields(buf):
        if fn == 1:
            out["tag"] = bytes(v).decode("utf-8")
        elif fn == 2:
            out["simple_value"] = struct.unpack("<f", struct.pack("<I", v))[0]
        elif fn == 4:
            out["image"] = _read_image(v)
        elif fn == 5:
            out["histo"] = _read_histo(v)
    return out


def read_events(path, verify=True):
    """[{wall_time, step, file_version | summary: [{tag, simple_value | image | histo}]}] of an event file"""
    out = []
    for rec in tfio.read_tfrecord(path, compression="", verify=verify):
        e = dict(wall_time=0.0, step=0)
        for fn, wt, v in _fields(rec):
            if fn == 1:
                e["wall_time"] = _f64(v)
            elif fn == 2:
                e["step"] = _signed64(v)
            elif fn == 3:
                e["file_version"] = bytes(v).decode("utf-8")
            elif fn == 5:
                e["summary"] = [_read_value(x) for f2, _, x in _fields(v) if f2 == 1]
        out.append(e)
    return out
