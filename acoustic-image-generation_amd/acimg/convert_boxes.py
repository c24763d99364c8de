"""`python -m acimg.convert_boxes ROOT_RAW_DIR OUT_DIR [--modalities 1 2] [--device cuda:0] [--workers N] [--list FILE]
[--deflate zlib|device]`:
convert_data2.py of the reference - the annotated Flickr-SoundNet files (`<id>.jpg`, `<id>.wav`, `<id>.xml`) to the GZIP
TFRecords of one box-annotated `SequenceExample` each that `acimg.data.BoxRecordLoader` reads and
`python -m acimg.localize --datatype flickr` scores.

* walk (:195-211): `ROOT/test_list.txt` names the `.jpg` files to take; they lie under `ROOT/Dataset/Data/*/` (folders in
  sorted order, names sorted inside a folder) with `<id>.wav` beside each; the annotation is
  `ROOT/Dataset/Annotations/<id>.xml`.  A listed file that no folder holds is refused before anything is written (the
  reference asserts that at its end).
* output (:264-307): `OUT/<id>.tfrecord`, one record: context `audio_data/mics` = 1, `audio_data/samples` = the clip's
  length, `video/height|width|depth` = 224, 298, 3; feature lists `xmin`, `xmax`, `ymin`, `ymax`, `typescene` (int32 [3]
  each), `audio/data` (the whole clip, int32, ONE step) and `video/image` (one frame).  The produced paths, in walk
  order, go to `ROOT/test.txt` (:309-311) or to `--list`.
* boxes (:224-260): up to three `person` entries; a coordinate v becomes int(np.round(v * 298 / 256)) or
  int(np.round(v * 224 / 256)) - half to even, and the 256 whatever the file's size, as there; `typescene` is 1 for
  `object`, 0 otherwise.  A fourth person (an IndexError there) and a `file_name` other than `<id>.jpg` (an assert there)
  are refused by name.
* video (:157-170): `cv2.imread` -> `cv2.resize(..., (298, 224), INTER_CUBIC)`, no crop, bytes in BGR order.  Neither
  OpenCV nor any imaging library is involved: the files of a batch are parsed on the host (`jpeg.parse_jpeg`), decoded
  on the device by the kernels of csrc/jpeg_decode.hip, and the pixels stay there for `acimg_resize_cubic_u8`.
  Sequential (baseline, extended) and complete progressive Huffman files of 8 bits; everything else is refused by name
  before a launch, a corrupt scan after the decode - in both cases before a byte of the batch is written.
* audio (:32-49): `np.int32(librosa.core.resample(data * 1.0, fs, 12288))` of the whole file - `Resampler`, the
  windowed-sinc kernel of csrc/resample.hip with resampy's `kaiser_best` filter built here; 12288 Hz passes through.
  Mono PCM of 16 or 32 bits (`convert.read_wav`); stereo is refused by name (`data * 1.0` of a two-column array resamples
  the wrong axis there).
* workers: reading + parsing files and building + deflating records run on `--workers` threads (at most 16); the calling
  thread runs the device, `BATCH` files per launch (a file without restart markers is decoded by one lane).
  `--deflate device` (default `zlib`): as in `acimg.convert`, the workers frame the records and the calling thread
  compresses a batch of them in one `DeviceDeflater.compress_many`."""
import argparse
import collections
import concurrent.futures
import glob
import math
import os
import sys
import time
import xml.etree.ElementTree as ET

import numpy as np

from .convert import (CROP_H, CROP_W, DEFLATE_CHOICES, MAX_WORKERS, SAMPLE_RATE, ConvertError, FrameResizer, _str2dir,
                      drain_writes, make_deflater, read_wav)

BATCH = 256
ANNOTATION_SIDE = 256                 # :225-228: the scale is 298 / 256 and 224 / 256 whatever the file's size
MAX_PERSONS = 3
NUM_ZEROS, PRECISION, BETA, ROLLOFF = 64, 9, 14.769656459379492, 0.9475937167399596      # resampy's kaiser_best


# ---- audio ------------------------------------------------------------------------------------------------------------------
def sinc_window(ratio):
    """resampy's `sinc_window` with the `kaiser_best` parameters -> (win, delta, entries per zero crossing): the right
    half of the symmetric filter, times `ratio` when downsampling; delta = first differences with a 0 appended"""
    num_table = 2 ** PRECISION
    n = num_table * NUM_ZEROS
    sinc = ROLLOFF * np.sinc(ROLLOFF * np.linspace(0, NUM_ZEROS, num=n + 1, endpoint=True))
    win = np.kaiser(2 * n + 1, BETA)[n:] * sinc
    if ratio < 1:
        win = win * ratio
    delta = np.zeros_like(win)
    delta[:-1] = np.diff(win)
    return win, delta, num_table


def resampled_length(n_in, rate, target=SAMPLE_RATE):
    """(samples formed, samples returned) = int(len * ratio), ceil(len * ratio)"""
    ratio = float(target) / rate
    return int(n_in * ratio), int(math.ceil(n_in * ratio))


class Resampler(object):
    """`np.int32(librosa.core.resample(data * 1.0, rate, target))` on `device`; the filter of a rate is built once"""

    def __init__(self, device, target=SAMPLE_RATE):
        import torch
        self.device, self.target = torch.device(device), int(target)
        self._tables = {}

    def table(self, rate):
        """(win, delta) fp64 tensors on the device, entries per zero crossing"""
        import torch
        if rate not in self._tables:
            win, delta, num_table = sinc_window(float(self.target) / rate)
            self._tables[rate] = (torch.from_numpy(win).to(self.device), torch.from_numpy(delta).to(self.device), num_table)
        return self._tables[rate]

    def resample_device(self, samples, rate, name="<wav>"):
        """int32 [len] (array or tensor) at `rate` -> (fp64 [n_out], int32 [n_out]) device tensors, stream-ordered"""
        import torch

        from . import _lib, ops
        x = torch.as_tensor(samples)
        if x.dtype != torch.int32 or x.dim() != 1 or x.numel() < 1:
            raise ConvertError("%s: %s samples of shape %s: one channel of int32 is resampled" % (name, x.dtype, tuple(x.shape)))
        if rate < 1:
            raise ConvertError("%s: a sample rate of %d Hz" % (name, rate))
        x = x.to(self.device).contiguous()
        win, delta, num_table = self.table(int(rate))
        L = _lib.load()
        n_out = int(L.acimg_resample_length(x.numel(), int(rate), self.target, None))
        if n_out != resampled_length(x.numel(), rate, self.target)[1] or n_out < 1:
            raise ConvertError("%s: %d samples at %d Hz give no clip at %d Hz" % (name, x.numel(), rate, self.target))
        y = torch.empty(n_out, dtype=torch.float64, device=self.device)
        yi = torch.empty(n_out, dtype=torch.int32, device=self.device)
        _lib.check(L.acimg_resample_sinc(x.data_ptr(), x.numel(), int(rate), self.target, win.data_ptr(), delta.data_ptr(),
                                         win.numel(), num_table, y.data_ptr(), yi.data_ptr(), n_out,
                                         ops.current_stream_handle(self.device)), "resample_sinc")
        return y, yi

    def resample(self, samples, rate, name="<wav>"):
        """-> int32 [n_out] on the host; `rate == target` passes through unresampled, as librosa does"""
        if int(rate) == self.target:
            return np.ascontiguousarray(samples, dtype=np.int32)
        return self.resample_device(samples, rate, name)[1].cpu().numpy()


# ---- annotation (:224-260) ------------------------------------------------------------------------------------------------
def scale_box(v, size):
    """int(np.round(v * size / 256)), half to even"""
    return int(np.round(np.int32(v) * (size / float(ANNOTATION_SIDE))))


def parse_annotation(text, ident, name="<xml>"):
    """the XML of one file -> (boxes int32 [4,3]: xmin, xmax, ymin, ymax rows, typescene int32 [3])"""
    try:
        root = ET.fromstring(text)
    except ET.ParseError as e:
        raise ConvertError("%s: no XML (%s)" % (name, e))
    found = root.find("file_name")
    if found is None or found.text != "%s.jpg" % ident:
        raise ConvertError("%s: file_name %r, the annotation of %s.jpg is expected"
                           % (name, None if found is None else found.text, ident))
    persons = root.findall("person")
    if len(persons) > MAX_PERSONS:
        raise ConvertError("%s: %d person entries, a record holds %d" % (name, len(persons), MAX_PERSONS))
    boxes, scene = np.zeros((4, 3), np.int32), np.zeros(3, np.int32)
    for p, member in enumerate(persons):
        box = member.find("bbox")
        try:
            scene[p] = 1 if box.find("type").text == "object" else 0
            for row, (key, size) in enumerate((("xmin", CROP_W), ("xmax", CROP_W), ("ymin", CROP_H), ("ymax", CROP_H))):
                boxes[row, p] = scale_box(int(box.find(key).text), size)
        except (AttributeError, TypeError, ValueError) as e:
            raise ConvertError("%s: person %d has no integer bbox with a type (%s)" % (name, p + 1, e))
    return boxes, scene


def build_box_record(boxes, scene, audio, video):
    """the serialized SequenceExample of :270-306; a modality that is None is left out as there"""
    from . import tfio
    ctx, lists = collections.OrderedDict(), collections.OrderedDict()
    if audio is not None:
        ctx["audio_data/mics"] = np.array([1])
        ctx["audio_data/samples"] = np.array([len(audio)])
    if video is not None:
        ctx["video/height"] = np.array([video.shape[0]])
        ctx["video/width"] = np.array([video.shape[1]])
        ctx["video/depth"] = np.array([video.shape[2]])
    b = np.ascontiguousarray(boxes, dtype="<i4").reshape(4, 3)
    for key, row in zip(("xmin", "xmax", "ymin", "ymax"), b):
        lists[key] = [row.tobytes()]
    lists["typescene"] = [np.ascontiguousarray(scene, dtype="<i4").tobytes()]
    if audio is not None:
        lists["audio/data"] = [np.ascontiguousarray(audio, dtype="<i4").tobytes()]
    if video is not None:
        lists["video/image"] = [np.ascontiguousarray(video, dtype=np.uint8).tobytes()]
    return tfio.build_sequence_example(ctx, lists)


# ---- the walk (:195-211) ----------------------------------------------------------------------------------------------------
Item = collections.namedtuple("Item", "ident jpg wav xml out")


def find_files(root_raw_dir, out_dir):
    """the listed files in walk order -> [Item]"""
    list_path = os.path.join(root_raw_dir, "test_list.txt")
    try:
        with open(list_path) as f:
            listed = [ln.replace("\n", "") for ln in f.readlines()]
    except OSError as e:
        raise ConvertError("%s: the list of files to convert cannot be read (%s)" % (list_path, e))
    wanted = set(n for n in listed if n)
    dataset = os.path.join(root_raw_dir, "Dataset")
    items = []
    for folder in sorted(glob.glob("{}/Data/*/".format(dataset))):
        for name in sorted(os.listdir(folder)):
            if name.endswith(".jpg") and name in wanted:
                ident = name.split(".jpg")[0]
                items.append(Item(ident, os.path.join(folder, name), os.path.join(folder, ident + ".wav"),
                                  os.path.join(dataset, "Annotations", ident + ".xml"),
                                  "{}/{}.tfrecord".format(out_dir, ident)))
    missing = sorted(wanted - set(os.path.basename(i.jpg) for i in items))
    if missing:
        raise ConvertError("%s: %d listed file(s) are in no folder of %s/Data, the first is %s"
                           % (list_path, len(missing), dataset, missing[0]))
    return items


Loaded = collections.namedtuple("Loaded", "jpeg info rate samples boxes scene read parse")


def _load(item, audio, video):
    """worker: read and parse one file's inputs; every refusal of the host side happens here"""
    from . import jpeg
    t0 = time.perf_counter()
    data = rate = samples = info = None
    try:
        if video:
            with open(item.jpg, "rb") as f:
                data = f.read()
        with open(item.xml, "rb") as f:
            xml = f.read()
    except OSError as e:
        raise ConvertError("%s: %s" % (e.filename, e.strerror))
    t1 = time.perf_counter()
    if audio:
        rate, samples = read_wav(item.wav)                # reads and parses; counted as read
    t2 = time.perf_counter()
    if video:
        info = jpeg.parse_jpeg(data, item.jpg)
    boxes, scene = parse_annotation(xml, item.ident, item.xml)
    t3 = time.perf_counter()
    return Loaded(data, info, rate, samples, boxes, scene, t2 - t0, t3 - t2)


def _write(path, boxes, scene, audio, video):
    """worker: build, deflate and write one record; returns seconds spent"""
    from . import tfio
    t0 = time.perf_counter()
    tfio.write_tfrecord(path, [build_box_record(boxes, scene, audio, video)], compression="GZIP")
    return time.perf_counter() - t0


def _frame(path, boxes, scene, audio, video):
    """worker of `--deflate device`: build and frame one record -> (path, the file's uncompressed bytes, seconds spent)"""
    from . import tfio
    t0 = time.perf_counter()
    buf = tfio.frame_record(build_box_record(boxes, scene, audio, video))
    return path, buf, time.perf_counter() - t0


class BoxConverter(object):
    """The pipeline of one `convert` call.  `times`: seconds in read and parse (summed over the workers), on the device
    (upload + decode + resize + resample + download, wall) and in deflate (summed over the workers).  `deflate="device"`:
    as in acimg.convert, the workers frame the records and the calling thread compresses a batch in one call."""

    def __init__(self, modalities=None, device="cuda:0", workers=4, log=None, batch=BATCH, deflate="zlib"):
        self.audio = modalities is None or 1 in modalities
        self.video = modalities is None or 2 in modalities
        self.device = device
        self.workers = max(1, min(int(workers), MAX_WORKERS))
        self.batch = max(1, int(batch))
        self.log = log or (lambda *a: None)
        self.times = dict(read=0.0, parse=0.0, device=0.0, deflate=0.0)
        self.records = 0
        self._exec = concurrent.futures.ThreadPoolExecutor(max_workers=self.workers, thread_name_prefix="acimg-boxes")
        self._writes = collections.deque()
        self._deflater = make_deflater(deflate, device)
        self._decoder = self._resampler = None
        self._resizers = {}

    def close(self):
        self._drain(0)
        self._exec.shutdown(wait=True)

    def _drain(self, keep):
        self.times["deflate"] += drain_writes(self._writes, keep, self._deflater)

    def _device_side(self, items, loaded):
        """-> (frames uint8 [n,224,298,3] on the host or None, [int32 clip per file] or None)"""
        import torch

        from . import jpeg
        frames = clips = None
        if self.video:
            if self._decoder is None:
                self._decoder = jpeg.JpegDecoder(self.device)
            files, infos = [l.jpeg for l in loaded], [l.info for l in loaded]
            groups = collections.OrderedDict()
            for i, g in enumerate(infos):
                groups.setdefault(jpeg.group_key(g), []).append(i)
            out = torch.empty(len(items), CROP_H, CROP_W, 3, dtype=torch.uint8, device=self._decoder.device)
            status = []
            for key, members in groups.items():
                H, W = key[:2]
                if (H, W) not in self._resizers:
                    self._resizers[(H, W)] = FrameResizer(self.device, H, W, new_size=(CROP_H, CROP_W))
                _, _, bgr, st = self._decoder.stages([files[i] for i in members], [infos[i] for i in members])
                small = self._resizers[(H, W)].resize(bgr.reshape(-1), H * W * 3, 0, W * 3, len(members))
                out[torch.as_tensor(members, device=out.device)] = small
                status.append((members, st))
            frames = out.cpu().numpy()
            for members, st in status:
                for i, s in zip(members, st.cpu().tolist()):
                    if s:
                        raise ConvertError("%s: corrupt JPEG scan: %s" % (items[i].jpg, jpeg.STATUS_TEXT.get(s, s)))
        if self.audio:
            if self._resampler is None:
                self._resampler = Resampler(self.device)
            clips = [self._resampler.resample(l.samples, l.rate, it.wav) for it, l in zip(items, loaded)]
        return frames, clips

    def convert_batch(self, items):
        """one batch: everything that can be refused is refused before a byte of the batch is written -> the paths"""
        loaded = list(self._exec.map(lambda it: _load(it, self.audio, self.video), items))
        self.times["read"] += sum(l.read for l in loaded)
        self.times["parse"] += sum(l.parse for l in loaded)
        t0 = time.perf_counter()
        frames, clips = self._device_side(items, loaded)
        self.times["device"] += time.perf_counter() - t0
        for k, (it, l) in enumerate(zip(items, loaded)):
            self._writes.append(self._exec.submit(_write if self._deflater is None else _frame, it.out, l.boxes, l.scene,
                                                  None if clips is None else clips[k],
                                                  None if frames is None else frames[k]))
            self.records += 1
            self.log("{} - Writing {}".format(time.strftime("%Y-%m-%d %H:%M:%S"), it.out))
        self._drain(2 * self.workers)
        return [it.out for it in items]


def convert(root_raw_dir, out_dir, modalities=None, list_file=None, device="cuda:0", workers=4, log=None, batch=BATCH,
            deflate="zlib"):
    """the whole data set -> (the files written, in walk order; the BoxConverter with its `times`)"""
    root_raw_dir = os.path.abspath(os.path.expanduser(root_raw_dir))
    out_dir = os.path.abspath(os.path.expanduser(out_dir))
    items = find_files(root_raw_dir, out_dir)
    conv = BoxConverter(modalities, device, workers, log, batch, deflate)
    paths = []
    try:
        for at in range(0, len(items), conv.batch):
            paths += conv.convert_batch(items[at:at + conv.batch])
    finally:
        conv.close()
    with open(list_file or os.path.join(root_raw_dir, "test.txt"), "w") as f:
        f.write("".join(p + "\n" for p in paths))
    return paths, conv


def build_parser():
    p = argparse.ArgumentParser(prog="python -m acimg.convert_boxes", description=__doc__.split("\n\n")[0])
    p.add_argument("root_raw_dir", help="Flickr-SoundNet root: test_list.txt, Dataset/Data/*/, Dataset/Annotations/", type=_str2dir)
    p.add_argument("out_dir", help="Directory where to store the converted data", type=_str2dir)
    p.add_argument("--modalities", help="Modalities to consider. 1: Audio data. 2: Video data.", nargs="*", type=int)
    p.add_argument("--list", dest="list_file", help="write the produced paths here instead of ROOT_RAW_DIR/test.txt")
    p.add_argument("--device", default="cuda:0")
    p.add_argument("--workers", type=int, default=4, help="threads that read, parse and deflate (at most 16)")
    p.add_argument("--deflate", default="zlib", choices=DEFLATE_CHOICES,
                   help="zlib: the workers gzip the records (level 9); device: the GPU deflates them, batched")
    return p


def main(argv=None):
    args = build_parser().parse_args(argv)
    paths, conv = convert(args.root_raw_dir, args.out_dir, args.modalities, args.list_file, args.device, args.workers,
                          log=print, deflate=args.deflate)
    print("{} records; seconds in read {:.2f}, parse {:.2f}, device {:.2f}, deflate {:.2f}".format(
        len(paths), conv.times["read"], conv.times["parse"], conv.times["device"], conv.times["deflate"]))
    return 0


if __name__ == "__main__":
    sys.exit(main())
