"""Byte tables of the two colormaps the reference's figures use (`plt.cm.gray` under `plt.cm.jet`, showvideo.py:225-228):
256 RGB entries each, built in NumPy from the colormaps' published breakpoints the way a segmented colormap is sampled
- 256 points on [0, 1], piecewise-linear between breakpoints, clipped to [0, 1] - and turned into bytes as
`(lut * 255).astype(uint8)` (truncation, which is why 24 grey entries are i - 1 and not i).  No plotting library is
imported; tests/test_show_cpu.py holds both tables to matplotlib's own, entry for entry."""
import numpy as np

N_ENTRIES = 256

# (x, y_below, y_above) per breakpoint: the "jet" and "gray" segment data as published with matplotlib's colormaps
SEGMENTS = {
    "jet": {
        "red": ((0.00, 0, 0), (0.35, 0, 0), (0.66, 1, 1), (0.89, 1, 1), (1.00, 0.5, 0.5)),
        "green": ((0.000, 0, 0), (0.125, 0, 0), (0.375, 1, 1), (0.640, 1, 1), (0.910, 0, 0), (1.000, 0, 0)),
        "blue": ((0.00, 0.5, 0.5), (0.11, 1, 1), (0.34, 1, 1), (0.65, 0, 0), (1.00, 0, 0)),
    },
    "gray": {
        "red": ((0.0, 0, 0), (1.0, 1, 1)),
        "green": ((0.0, 0, 0), (1.0, 1, 1)),
        "blue": ((0.0, 0, 0), (1.0, 1, 1)),
    },
}


def _channel(points, n=N_ENTRIES):
    """one channel of a segmented colormap sampled at n points, float64 in [0, 1]"""
    p = np.asarray(points, dtype=np.float64)
    x, below, above = p[:, 0] * (n - 1), p[:, 1], p[:, 2]
    at = (n - 1) * np.linspace(0.0, 1.0, n)
    seg = np.searchsorted(x, at)[1:-1]                   # the breakpoint at or after each interior sample
    frac = (at[1:-1] - x[seg - 1]) / (x[seg] - x[seg - 1])
    inner = frac * (below[seg] - above[seg - 1]) + above[seg - 1]
    return np.clip(np.concatenate([[above[0]], inner, [below[-1]]]), 0.0, 1.0)


def float_table(name):
    """[256,3] float64 RGB of colormap `name`"""
    seg = SEGMENTS[name]
    return np.stack([_channel(seg[c]) for c in ("red", "green", "blue")], axis=1)


def byte_table(name):
    """[256,3] uint8 RGB of colormap `name`: what `cmap(x, bytes=True)` looks up"""
    if name not in SEGMENTS:
        raise ValueError("unknown colormap %r (have: %s)" % (name, ", ".join(sorted(SEGMENTS))))
    return (float_table(name) * 255).astype(np.uint8)
