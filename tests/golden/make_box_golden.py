"""Generates tests/golden/box_golden.npz by running the REFERENCE's own NumPy MFCC code of the box-annotated loader
(dataloader/frames.py `_build_spectrograms_function`, with its `createfilters` / `get_feats`) in the build container.

TensorFlow / cv2 are not installed, so they are stubbed with MagicMock module objects, as make_frontend_golden.py
does; only the pure NumPy methods of the loader run.  The clips are [1, L] int32 arrays (L = 12288, 36864 and an odd
length): the reading the loader here implements.  The same call on the [1, 1, L] array the TF pipeline
passes is recorded too (`degenerate_*`): its output does not depend on the audio.  Nothing from the reference is
copied: the fixture holds inputs and the outputs the reference computed from them.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_box_golden.py
"""
import importlib.abc
import importlib.machinery
import os
import sys
from unittest import mock

import numpy as np

REF = "/root/reference"
STUBS = ("tensorflow", "cv2", "torchfile", "librosa", "matplotlib", "sklearn")


class _StubFinder(importlib.abc.MetaPathFinder, importlib.abc.Loader):
    def find_spec(self, name, path, target=None):
        if name.split(".")[0] in STUBS:
            return importlib.machinery.ModuleSpec(name, self, is_package=True)
        return None

    def create_module(self, spec):
        m = mock.MagicMock(name=spec.name)
        m.__path__ = []
        m.__name__ = spec.name
        m.__spec__ = spec
        return m

    def exec_module(self, module):
        pass


def main():
    sys.dont_write_bytecode = True
    sys.meta_path.insert(0, _StubFinder())
    sys.path.insert(0, REF)
    from dataloader.frames import ActionsDataLoader  # noqa: E402

    loader = object.__new__(ActionsDataLoader)
    loader.sample_rate = 12288
    rng = np.random.RandomState(5)
    out = {}
    for i, length in enumerate((12288, 36864, 12289 + 2 * 1234)):
        t = np.arange(length) / 12288.0
        clip = (rng.randn(1, length) * 800 + 3000 * np.sin(2 * np.pi * (150 + 200 * i) * t)).astype(np.int32)
        out["clip%d" % i] = clip
        out["mfcc%d" % i] = loader._build_spectrograms_function(clip)
        with np.errstate(all="ignore"):
            out["degenerate%d" % i] = np.asarray(loader._build_spectrograms_function(clip.reshape(1, 1, length)))
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "box_golden.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, {k: v.shape for k, v in out.items()})


if __name__ == "__main__":
    main()
