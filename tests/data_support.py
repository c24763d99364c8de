"""Record files for the loader, trainer and command-line tests: the reference's two SequenceExample layouts (the 12-frame
outdoor record of convert_data.py:247-279 and the box-annotated record of convert_data2.py:264-305), the GZIP file writer,
and a stand-in for the loader's device side.  Every builder draws from the caller's generator in a fixed order (acoustic
images, audio, video), so a test's files depend on its seed and arguments alone."""
from collections import OrderedDict

import numpy as np

from localize_ref import random_boxes


def outdoor_arrays(rng, wide):
    """acoustic images [12,36,48,12] fp32 in [0, 1) (wide: in [-1, 4)), audio [12,1024] int32, video [12,224,298,3] uint8"""
    ai = rng.rand(12, 36, 48, 12).astype(np.float32)
    if wide:
        ai = ai * 5 - 1
    sa = (rng.randn(12, 1024) * 800).astype(np.int32)
    vi = rng.randint(0, 256, size=(12, 224, 298, 3)).astype(np.uint8)
    return ai, sa, vi


def outdoor_example(ai, sa, vi, cls, loc):
    from acimg import tfio
    ctx = OrderedDict([("classes", np.array([cls])), ("location", np.array([loc])),
                       ("audio_image/height", np.array([36])), ("audio_image/width", np.array([48])),
                       ("audio_image/depth", np.array([12])), ("audio_data/mics", np.array([1])),
                       ("audio_data/samples", np.array([1024])), ("video/height", np.array([224])),
                       ("video/width", np.array([298])), ("video/depth", np.array([3]))])
    lists = OrderedDict([("audio/image", [a.tobytes() for a in ai]), ("audio/data", [s.tobytes() for s in sa]),
                         ("video/image", [v.tobytes() for v in vi])])
    return tfio.build_sequence_example(ctx, lists)


def outdoor_record(rng, cls, loc, wide):
    return outdoor_example(*outdoor_arrays(rng, wide), cls, loc)


def write_outdoor_records(tmp, seed, labels, wide):
    """one GZIP file part<r>.tfrecord per (class, location) of `labels`, drawn from RandomState(seed) -> the paths"""
    from acimg import tfio
    rng = np.random.RandomState(seed)
    paths = []
    for r, (cls, loc) in enumerate(labels):
        p = str(tmp / ("part%d.tfrecord" % r))
        tfio.write_tfrecord(p, [outdoor_record(rng, cls, loc, wide)], compression="GZIP")
        paths.append(p)
    return paths


def box_record(boxes, scene, audio, video, drop=None, override=None):
    """one SequenceExample in the layout convert_data2.py:264-305 writes"""
    from acimg import tfio
    ctx = {"audio_data/mics": np.array([1]), "audio_data/samples": np.array([audio.shape[-1]]),
           "video/height": np.array([video.shape[-3]]), "video/width": np.array([video.shape[-2]]),
           "video/depth": np.array([video.shape[-1]])}
    b = np.asarray(boxes, np.int32).reshape(-1, 4, 3)
    fl = {"xmin": [r[0].tobytes() for r in b], "xmax": [r[1].tobytes() for r in b],
          "ymin": [r[2].tobytes() for r in b], "ymax": [r[3].tobytes() for r in b],
          "typescene": [np.asarray(s, np.int32).tobytes() for s in np.asarray(scene).reshape(-1, 3)],
          "audio/data": [np.asarray(audio, np.int32).reshape(-1).tobytes()],
          "video/image": [f.tobytes() for f in np.asarray(video, np.uint8).reshape(-1, *video.shape[-3:])]}
    for k, v in (override or {}).items():
        (ctx if k in ctx else fl)[k] = v
    for k in drop or ():
        ctx.pop(k, None)
        fl.pop(k, None)
    return tfio.build_sequence_example(ctx, fl)


def random_box_record(rng, length):
    """a box record of one frame and `length` audio samples (noise + one tone) with at least one annotator"""
    b = random_boxes(rng, 1)[0]
    b[1, 0] = 150                                        # at least one annotator
    t = np.arange(length) / 12288.0
    audio = (rng.randn(length) * 500 + 2000 * np.sin(2 * np.pi * rng.uniform(100, 3000) * t)).astype(np.int32)
    video = rng.randint(0, 256, size=(224, 298, 3)).astype(np.uint8)
    return box_record(b, [1, 0, 0], audio, video)


class FakePool(object):
    """what the loader's device side does, as sets: a page's frames are `resident` from upload until gathered"""

    def __init__(self, frames):
        self.frames = frames
        self.resident = {}          # page -> set of global frame numbers uploaded and not yet gathered
        self.where = {}             # slot -> global frame number
        self.emitted = []           # global frame numbers in gather order
        self.rows = []              # (offset, count) of every gather call
        self.pages_seen = set()
        self.next_frame = 0

    def upload(self, page, nframes):
        assert not self.resident.get(page), "page %d handed out with un-emitted frames %r" % (page, self.resident[page])
        self.pages_seen.add(page)
        self.resident[page] = set(range(self.next_frame, self.next_frame + nframes))
        for i in range(nframes):
            self.where[page * self.frames + i] = self.next_frame + i
        self.next_frame += nframes
        return nframes

    def gather(self, slots, offset):
        self.rows.append((offset, len(slots)))
        for s in slots:
            f = self.where[s]
            self.resident[s // self.frames].remove(f)
            self.emitted.append(f)
