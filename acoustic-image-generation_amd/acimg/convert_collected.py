"""`python -m acimg.convert_collected ROOT_RAW_DIR OUT_DIR [--modalities 1 2] [--device cuda:0] [--workers N] [--list FILE]
[--deflate zlib|device] [--inflate zlib|device]`:
convert_data4.py of the reference - the two-object test set (`<id>.png`, `<id>.wav` in one folder) to the GZIP TFRecords
of one `SequenceExample` each, labelled `classnumber`, that `acimg.data.ClassRecordLoader` reads.

* walk (:174-192): `ROOT/test_list.txt` names the `.png` files to take; they lie in `ROOT` itself with `<id>.wav` beside
  each.  The reference takes them in `os.listdir` order; here they are taken sorted by integer id, so a run is
  reproducible.  A listed file that is absent, and a name whose stem is not the canonical decimal form of an integer
  (the reference writes `7.tfrecord` for `007.png` and then lists `007.tfrecord`), are refused before a byte is written.
* label (:180-181, :216): `classnumber = classesnames[id - 1]`, the reference's 23-entry table (data, restated below).
  An id outside 1 .. 23 is refused by name: there, 0 silently wraps to the last entry and 24 raises IndexError.
* output (:205-240): `OUT/<id>.tfrecord`, one record: context `audio_data/mics` = 1, `audio_data/samples` = the clip's
  length and `classnumber` (these three only when audio is included, as there), `video/height|width|depth` = the file's
  own size and 3; feature lists `audio/data` (the whole clip, int32, ONE step) and `video/image` (one frame, B G R
  bytes).  No resize: the reference stores the PNG at its own size and only prints the size when it is not 224 x 298;
  the same is logged here and the record is written.  `ROOT/test.txt` (:242-245), or `--list`, receives
  `OUT/<name>.tfrecord` for every line of `test_list.txt`, in that file's order.
* video (:138-149): `cv2.imread` - here `png.parse_png` on the host and the kernels of csrc/png_decode.hip on the device:
  every legal PNG (15 colour-type / depth forms, Adam7, any filters), everything else refused by name before a launch, a
  device status other than 0 after the decode - in both cases before a byte of the batch is written.  `--inflate zlib`
  (default): the workers inflate the scanlines; `--inflate device`: `acimg.inflate` does, and they never reach the host.
* audio (:27-32): `np.int32(librosa.core.resample(data * 1.0, fs, 12288))` of the whole file with
  `convert_boxes.Resampler`; mono PCM as there, stereo refused by name.
* workers and `--deflate`: as in `acimg.convert_boxes`."""
import argparse
import collections
import concurrent.futures
import gzip
import os
import sys
import time

import numpy as np

from .convert_boxes import (DEFLATE_CHOICES, MAX_WORKERS, ConvertError, Resampler, _str2dir, drain_writes, make_deflater,
                            read_wav)
from .png import INFLATE_CHOICES

BATCH = 256
FRAME_H, FRAME_W = 224, 298
# :180: the class of recording <id> is CLASS_OF_ID[id - 1]; the classes are :182-183
CLASS_OF_ID = (9, 9, 9, 9, 9, 9, 2, 9, 9, 4, 6, 7, 6, 1, 1, 8, 8, 2, 2, 0, 2, 3, 5)
CLASS_NAMES = ("Train", "Boat", "Drone", "Fountain", "Drill", "Razor", "Hair dryer", "Vacuumcleaner", "Cart", "Traffic")


def class_of(ident, name="<png>"):
    if not 1 <= ident <= len(CLASS_OF_ID):
        raise ConvertError("%s: id %d has no class: the table holds ids 1 .. %d" % (name, ident, len(CLASS_OF_ID)))
    return CLASS_OF_ID[ident - 1]


def build_class_record(classnumber, audio, video):
    """the serialized SequenceExample of :211-240; a modality that is None is left out as there"""
    from . import tfio
    ctx, lists = collections.OrderedDict(), collections.OrderedDict()
    if audio is not None:
        ctx["audio_data/mics"] = np.array([1])
        ctx["audio_data/samples"] = np.array([len(audio)])
        ctx["classnumber"] = np.array([int(classnumber)])
    if video is not None:
        ctx["video/height"] = np.array([video.shape[0]])
        ctx["video/width"] = np.array([video.shape[1]])
        ctx["video/depth"] = np.array([video.shape[2]])
    if audio is not None:
        lists["audio/data"] = [np.ascontiguousarray(audio, dtype="<i4").tobytes()]
    if video is not None:
        lists["video/image"] = [np.ascontiguousarray(video, dtype=np.uint8).tobytes()]
    return tfio.build_sequence_example(ctx, lists)


# ---- the walk (:174-192) ----------------------------------------------------------------------------------------------------
Item = collections.namedtuple("Item", "ident png wav out classnumber")


def find_files(root_raw_dir, out_dir):
    """-> ([Item] sorted by id, the lines of test_list.txt in its order)"""
    list_path = os.path.join(root_raw_dir, "test_list.txt")
    try:
        with open(list_path) as f:
            listed = [ln.replace("\n", "") for ln in f.readlines()]
    except OSError as e:
        raise ConvertError("%s: the list of files to convert cannot be read (%s)" % (list_path, e))
    names = sorted(set(n for n in listed if n))
    items = []
    for name in names:
        stem = name[:-4]
        if not name.endswith(".png") or not stem.isdigit() or not stem.isascii() or str(int(stem)) != stem:
            raise ConvertError("%s: %r is not <id>.png with the id in canonical decimal form" % (list_path, name))
        ident = int(stem)
        path = os.path.join(root_raw_dir, name)
        items.append(Item(ident, path, os.path.join(root_raw_dir, "%d.wav" % ident), "{}/{}.tfrecord".format(out_dir, ident),
                          class_of(ident, path)))
    # the reference reads <id>.wav whether or not audio is included (:191-193)
    missing = [p for i in items for p in (i.png, i.wav) if not os.path.isfile(p)]
    if missing:
        raise ConvertError("%s: %d file(s) of the listed recordings are not in %s, the first is %s"
                           % (list_path, len(missing), root_raw_dir, os.path.basename(missing[0])))
    return sorted(items, key=lambda i: i.ident), listed


Loaded = collections.namedtuple("Loaded", "png info inflated rate samples read parse")


def _load(item, audio, video, inflate):
    """worker: read and parse one file's inputs, inflate the scanlines for `--inflate zlib`; every refusal of the host
    side happens here"""
    from . import png
    t0 = time.perf_counter()
    data = rate = samples = info = inflated = None
    if video:
        try:
            with open(item.png, "rb") as f:
                data = f.read()
        except OSError as e:
            raise ConvertError("%s: %s" % (e.filename, e.strerror))
    if audio:
        rate, samples = read_wav(item.wav)                # reads and parses; counted as read
    t1 = time.perf_counter()
    if video:
        info = png.parse_png(data, item.png)
        if inflate == "zlib":
            inflated = png.inflate_host(info, item.png)
    return Loaded(data, info, inflated, rate, samples, t1 - t0, time.perf_counter() - t1)


def _write(path, classnumber, audio, video):
    """worker: build, deflate and write one record; returns seconds spent.  One gzip member of level 9 without a name
    and with MTIME 0, as TensorFlow's writer leaves them: a second run writes the same bytes."""
    from . import tfio
    t0 = time.perf_counter()
    data = gzip.compress(tfio.frame_record(build_class_record(classnumber, audio, video)), 9, mtime=0)
    with open(path, "wb") as f:
        f.write(data)
    return time.perf_counter() - t0


def _frame(path, classnumber, audio, video):
    """worker of `--deflate device`: build and frame one record -> (path, the file's uncompressed bytes, seconds spent)"""
    from . import tfio
    t0 = time.perf_counter()
    buf = tfio.frame_record(build_class_record(classnumber, audio, video))
    return path, buf, time.perf_counter() - t0


class CollectedConverter(object):
    """The pipeline of one `convert` call, after `convert_boxes.BoxConverter`.  `times`: seconds in read and in parse
    (+ inflate for inflate="zlib"), summed over the workers; on the device (upload + inflate + decode + resample +
    download, wall); in deflate (summed over the workers, or the device's batches)."""

    def __init__(self, modalities=None, device="cuda:0", workers=4, log=None, batch=BATCH, deflate="zlib", inflate="zlib"):
        if inflate not in INFLATE_CHOICES:
            raise ConvertError("--inflate is one of %s, got %r" % (", ".join(INFLATE_CHOICES), inflate))
        self.audio = modalities is None or 1 in modalities
        self.video = modalities is None or 2 in modalities
        self.device, self.inflate = device, inflate
        self.workers = max(1, min(int(workers), MAX_WORKERS))
        self.batch = max(1, int(batch))
        self.log = log or (lambda *a: None)
        self.times = dict(read=0.0, parse=0.0, device=0.0, deflate=0.0)
        self.records = 0
        self._exec = concurrent.futures.ThreadPoolExecutor(max_workers=self.workers, thread_name_prefix="acimg-collected")
        self._writes = collections.deque()
        self._deflater = make_deflater(deflate, device)
        self._decoder = self._resampler = None

    def close(self):
        self._drain(0)
        self._exec.shutdown(wait=True)

    def _drain(self, keep):
        self.times["deflate"] += drain_writes(self._writes, keep, self._deflater)

    def _device_side(self, items, loaded):
        """-> ([uint8 [H,W,3] frame per file] on the host or None, [int32 clip per file] or None)"""
        from . import png
        frames = clips = None
        if self.video:
            if self._decoder is None:
                self._decoder = png.PngDecoder(self.device, self.inflate)
            pixels, status = self._decoder.decode_many([l.png for l in loaded], [l.info for l in loaded],
                                                       None if self.inflate == "device" else [l.inflated for l in loaded],
                                                       [it.png for it in items])
            frames = [p.cpu().numpy() for p in pixels]
            for it, s in zip(items, status.tolist()):
                if s:
                    raise ConvertError("%s: corrupt PNG: %s" % (it.png, png.STATUS_TEXT.get(s, s)))
        if self.audio:
            if self._resampler is None:
                self._resampler = Resampler(self.device)
            clips = [self._resampler.resample(l.samples, l.rate, it.wav) for it, l in zip(items, loaded)]
        return frames, clips

    def convert_batch(self, items):
        """one batch: everything that can be refused is refused before a byte of the batch is written -> the paths"""
        loaded = list(self._exec.map(lambda it: _load(it, self.audio, self.video, self.inflate), items))
        self.times["read"] += sum(l.read for l in loaded)
        self.times["parse"] += sum(l.parse for l in loaded)
        t0 = time.perf_counter()
        frames, clips = self._device_side(items, loaded)
        self.times["device"] += time.perf_counter() - t0
        for k, (it, l) in enumerate(zip(items, loaded)):
            if frames is not None and frames[k].shape[:2] != (FRAME_H, FRAME_W):
                self.log("{} {} {}".format(frames[k].shape[1], frames[k].shape[0], frames[k].shape[2]))      # :146-147
            self._writes.append(self._exec.submit(_write if self._deflater is None else _frame, it.out, it.classnumber,
                                                  None if clips is None else clips[k],
                                                  None if frames is None else frames[k]))
            self.records += 1
            self.log("{} - Writing {}".format(time.strftime("%Y-%m-%d %H:%M:%S"), it.out))
        self._drain(2 * self.workers)
        return [it.out for it in items]


def convert(root_raw_dir, out_dir, modalities=None, list_file=None, device="cuda:0", workers=4, log=None, batch=BATCH,
            deflate="zlib", inflate="zlib"):
    """the whole data set -> (the files written, by id; the CollectedConverter with its `times`)"""
    root_raw_dir = os.path.abspath(os.path.expanduser(root_raw_dir))
    out_dir = os.path.abspath(os.path.expanduser(out_dir))
    items, listed = find_files(root_raw_dir, out_dir)
    conv = CollectedConverter(modalities, device, workers, log, batch, deflate, inflate)
    paths = []
    try:
        for at in range(0, len(items), conv.batch):
            paths += conv.convert_batch(items[at:at + conv.batch])
    finally:
        conv.close()
    with open(list_file or os.path.join(root_raw_dir, "test.txt"), "w") as f:                  # :242-245
        f.write("".join(out_dir + "/" + name.replace(".png", ".tfrecord") + "\n" for name in listed if name))
    return paths, conv


def build_parser():
    p = argparse.ArgumentParser(prog="python -m acimg.convert_collected", description=__doc__.split("\n\n")[0])
    p.add_argument("root_raw_dir", help="folder of the two-object test set: test_list.txt, <id>.png, <id>.wav", type=_str2dir)
    p.add_argument("out_dir", help="Directory where to store the converted data", type=_str2dir)
    p.add_argument("--modalities", help="Modalities to consider. 1: Audio data. 2: Video data.", nargs="*", type=int)
    p.add_argument("--list", dest="list_file", help="write the produced paths here instead of ROOT_RAW_DIR/test.txt")
    p.add_argument("--device", default="cuda:0")
    p.add_argument("--workers", type=int, default=4, help="threads that read, parse, inflate and deflate (at most 16)")
    p.add_argument("--deflate", default="zlib", choices=DEFLATE_CHOICES,
                   help="zlib: the workers gzip the records (level 9); device: the GPU deflates them, batched")
    p.add_argument("--inflate", default="zlib", choices=INFLATE_CHOICES,
                   help="zlib: the workers inflate the PNG scanlines; device: the GPU does, batched")
    return p


def main(argv=None):
    args = build_parser().parse_args(argv)
    paths, conv = convert(args.root_raw_dir, args.out_dir, args.modalities, args.list_file, args.device, args.workers,
                          log=print, deflate=args.deflate, inflate=args.inflate)
    print("{} records; seconds in read {:.2f}, parse {:.2f}, device {:.2f}, deflate {:.2f}".format(
        len(paths), conv.times["read"], conv.times["parse"], conv.times["device"], conv.times["deflate"]))
    return 0


if __name__ == "__main__":
    sys.exit(main())
