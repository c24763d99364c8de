"""The NumPy restatement of the sample-rate converter (csrc/resample.hip, acimg.convert_boxes.Resampler), written from the
definition in DESIGN section 8: `np.int32(librosa.core.resample(data * 1.0, fs, 12288))` with resampy's `kaiser_best`
windowed sinc.  All output samples at once, one tap of every sample per step, in the device's order of operations (left
wing first, then the right wing, each in tap order; every product and sum is its own fp64 rounding, which is what NumPy
does anyway), so the device is held to it bit for bit."""
import math

import numpy as np

TARGET_RATE = 12288
NUM_ZEROS, PRECISION, BETA, ROLLOFF = 64, 9, 14.769656459379492, 0.9475937167399596      # resampy's kaiser_best


def sinc_window(ratio):
    """(win, delta, num_table): the right half of the Kaiser-windowed sinc, 2^PRECISION entries per zero crossing, times
    `ratio` when downsampling; delta = its first differences, a 0 appended"""
    num_table = 2 ** PRECISION
    n = num_table * NUM_ZEROS
    sinc = ROLLOFF * np.sinc(ROLLOFF * np.linspace(0, NUM_ZEROS, num=n + 1, endpoint=True))
    win = np.kaiser(2 * n + 1, BETA)[n:] * sinc
    if ratio < 1:
        win = win * ratio
    delta = np.zeros_like(win)
    delta[:-1] = np.diff(win)
    return win, delta, num_table


def lengths(n_in, rate, target=TARGET_RATE):
    """(samples formed, samples returned): int(len * ratio), padded with zeros to ceil(len * ratio)"""
    ratio = float(target) / rate
    return int(n_in * ratio), int(math.ceil(n_in * ratio))


def _wing(acc, x, win, delta, step, offset, eta, taps, index, direction):
    """acc += (win[o + i step] + eta delta[o + i step]) * x[index + direction * i] for i < taps, tap by tap"""
    for i in range(int(taps.max()) if taps.size else 0):
        live = i < taps
        w = np.where(live, offset + i * step, 0)
        xi = np.where(live, index + direction * i, 0)
        weight = win[w] + eta * delta[w]
        acc = acc + np.where(live, weight * x[xi], 0.0)
    return acc


def resample_f64(x, rate, target=TARGET_RATE, table=None):
    """int samples at `rate` -> fp64 [ceil(len * ratio)] at `target`; `rate == target` passes through"""
    x = np.asarray(x).astype(np.float64)
    if rate == target:
        return x
    ratio = float(target) / rate
    win, delta, num_table = table if table is not None else sinc_window(ratio)
    n_calc, n_out = lengths(x.size, rate, target)
    scale = min(1.0, ratio)
    step = int(scale * num_table)
    t = np.arange(n_calc)
    time = t * (1.0 / ratio)
    n = time.astype(np.int64)
    frac = scale * (time - n)
    pos = frac * num_table
    offset = pos.astype(np.int64)
    eta = pos - offset
    acc = _wing(np.zeros(n_calc), x, win, delta, step, offset, eta, np.minimum(n + 1, (win.size - offset) // step), n, -1)
    frac = scale - frac
    pos = frac * num_table
    offset = pos.astype(np.int64)
    eta = pos - offset
    acc = _wing(acc, x, win, delta, step, offset, eta, np.minimum(x.size - n - 1, (win.size - offset) // step), n + 1, 1)
    return np.concatenate([acc, np.zeros(n_out - n_calc)])


def to_int32(y):
    """truncate toward zero, clamp to the int32 range (where `np.int32(...)` of the reference is undefined)"""
    return np.clip(np.trunc(y), -2.0 ** 31, 2.0 ** 31 - 1).astype(np.int32)


def resample(x, rate, target=TARGET_RATE, table=None):
    return to_int32(resample_f64(x, rate, target, table))
