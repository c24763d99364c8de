"""Writes tests/golden/render_golden.npz with matplotlib (a test-only dependency of the development machine; nothing
under acimg/ imports it): the uint8 tables of `jet` and `gray`, and a few small images with matplotlib's own
`cmap(Normalize()(x), bytes=True)[..., :3]` - the colour stage `plt.imshow(x, cmap=...)` applies when no vmin / vmax is
given (showvideo.py:225-228).

    python tests/golden/make_render_golden.py
"""
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))


def main():
    import matplotlib
    from matplotlib.colors import Normalize

    cmaps = {"jet": matplotlib.colormaps["jet"], "gray": matplotlib.colormaps["gray"]}
    out = {"matplotlib_version": np.array(matplotlib.__version__)}
    ramp = np.arange(256)
    for name, cm in cmaps.items():
        out["table_" + name] = cm(ramp, bytes=True)[:, :3].astype(np.uint8)

    rng = np.random.RandomState(5)
    images = {
        "f32": rng.rand(48, 48).astype(np.float32) * np.float32(3.7) - np.float32(1.2),
        "f64": rng.rand(40, 40) * 1e-3 + 0.0414,                     # the scale of find_logen's output
        "const": np.full((16, 16), 0.3, np.float32),
        "extremes": np.where(rng.rand(32, 40) < 0.3, 0.25, np.where(rng.rand(32, 40) < 0.5, 2.0, rng.rand(32, 40) + 0.5)),
        "ramp32": np.linspace(0, 1, 2048, dtype=np.float32).reshape(32, 64),   # every table boundary, float32
        "ramp64": np.linspace(-1, 1, 1024).reshape(16, 64),
    }
    for key, x in images.items():
        out["in_" + key] = x
        for name, cm in cmaps.items():
            out["out_%s_%s" % (key, name)] = cm(Normalize()(x), bytes=True)[..., :3].astype(np.uint8)
    np.savez_compressed(os.path.join(HERE, "render_golden.npz"), **out)
    print("wrote render_golden.npz: %d arrays" % len(out))


if __name__ == "__main__":
    main()
