"""The payloads and histograms that tests/test_deflate_cpu.py runs through the restatement and tests/test_deflate_gpu.py
through the device: built once per process, never modified."""
import os

import numpy as np

import deflate_ref as ref

B = ref.BLOCK
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "jpeg_decode_golden.npz")


def fibonacci(n):
    out, a, b = [], 1, 1
    for _ in range(n):
        out.append(a)
        a, b = b, a + b
    return out


def smooth_fixture():
    """the 196608 bytes of pixels_smooth_420_256x256 of the committed JPEG fixture"""
    with np.load(GOLDEN) as g:
        return g["pixels_smooth_420_256x256"].tobytes()


def _payloads():
    rng = np.random.RandomState(5)
    noise = rng.randint(0, 256, 3 * B + 17).astype(np.uint8).tobytes()
    out = []
    for n in (1, 2, 3, B - 1, B, B + 1, 3 * B + 17):                      # B + 1: a one-byte last block
        out.append(("zeros_%d" % n, bytes(n)))                           # runs of 258 at distance 1
        out.append(("noise_%d" % n, noise[:n]))                          # the stored fallback
    out.append(("period3", (b"\x01\x7f\xfe" * (B + 6))[:3 * B + 17]))
    out.append(("period4", (b"abcd" * B)[:B + 1]))
    out.append(("second_block_repeats_first", noise[:B] * 2))           # the match across the boundary is not taken
    out.append(("one_literal_twice", b"\x41\x41"))                       # no match possible in 2 bytes
    counts = fibonacci(20)                                               # 17710 bytes; unlimited depth 19: the 15-bit limiter
    fib = np.concatenate([np.full(c, 11 * i + 3, np.uint8) for i, c in enumerate(counts)])
    rng.shuffle(fib)
    out.append(("fibonacci_counts", fib.tobytes()))
    out.append(("smooth_fixture", smooth_fixture()))
    t = np.arange(491520 // 4)
    clip = (2 ** 22 * np.sin(2 * np.pi * 700.0 * t / 12288.0) + rng.randn(t.size) * 2 ** 12).astype("<i4")
    out.append(("tone_plus_noise_int32", clip.tobytes()[:3 * B]))
    return out


PAYLOADS = _payloads()
assert max(len(p) for name, p in PAYLOADS if name != "smooth_fixture") <= 3 * B + 17

# (name, counts): the test puts them at scattered symbols of each alphabet
HISTOGRAMS = (("one_symbol", [7]), ("two_symbols", [3, 900]), ("all_equal", [5] * 19), ("fibonacci_9", fibonacci(9)),
              ("fibonacci_17", fibonacci(17)), ("fibonacci_19", fibonacci(19)), ("ties", [1, 1, 1, 2, 2, 3, 4, 4, 100, 100]))
ALPHABETS = ((286, 15), (30, 15), (19, 7))


def histogram_rows(nsym):
    """int32 [len(HISTOGRAMS) + 2][nsym]: every histogram's counts spread over the alphabet (stride 7 from symbol 1,
    wrapped: 7 is coprime to 286, 30 and 19), then one row with every symbol used once and one with none used"""
    rows = np.zeros((len(HISTOGRAMS) + 2, nsym), np.int32)
    for r, (_, counts) in enumerate(HISTOGRAMS):
        for k, c in enumerate(counts):
            s = (1 + 7 * k) % nsym
            assert rows[r, s] == 0
            rows[r, s] = c
    rows[len(HISTOGRAMS)] = 1
    return rows


def check_lengths(freq, lengths, limit, what):
    """the properties every code must have: 0 exactly for unused symbols, lengths 1..limit, Kraft sum exactly 1 with two or
    more used symbols, and the cost of a heapq Huffman build whenever that build's depth fits the limit"""
    freq, lengths = [int(f) for f in freq], [int(l) for l in lengths]
    used = [i for i, f in enumerate(freq) if f > 0]
    for i, (f, l) in enumerate(zip(freq, lengths)):
        assert (1 <= l <= limit) if f > 0 else l == 0, (what, i, f, l)
    if len(used) == 1:
        assert lengths[used[0]] == 1, what
    if len(used) >= 2:
        assert sum(1 << (limit - lengths[i]) for i in used) == 1 << limit, (what, "Kraft sum")
        cost, depth = ref.heap_huffman_cost(freq)
        if depth <= limit:
            assert sum(freq[i] * lengths[i] for i in used) == cost, (what, "cost")
        return depth
    return len(used)
