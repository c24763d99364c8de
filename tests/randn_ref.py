"""Plain numpy restatement of randn_kernel (csrc/optim.hip): Philox4x32-10 + Box-Muller, four samples per counter.

counter = (ctr_lo, ctr_hi, 0x9E3779B9, 0xBB67AE85) with ctr = quad + offset as a 64-bit sum, key = (seed_lo, seed_hi);
words (0, 1) and (2, 3) of the output feed one Box-Muller draw each: sample 4q + {0, 1} = r0 * {cos, sin}(2 pi u1),
sample 4q + {2, 3} = r1 * {cos, sin}(2 pi u3), r = sqrt(-2 log u).

The uniforms are restated, not idealised: u = ((float)(c >> 8) + 0.5f) * 2^-24 is fp32 arithmetic, so for
c >> 8 >= 2^23 the half is rounded away (to even) and u can be exactly 1.0 (then r = 0).  u is computed here in
np.float32 with the kernel's operation order; log, sqrt, sin and cos are fp64.
"""
import numpy as np

PHILOX_M0 = np.uint64(0xD2511F53)
PHILOX_M1 = np.uint64(0xCD9E8D57)
PHILOX_W0 = 0x9E3779B9
PHILOX_W1 = 0xBB67AE85
MASK32 = np.uint64(0xFFFFFFFF)
SHIFT32 = np.uint64(32)
DIST_SEED, DIST_N = 20240607, 1 << 22      # the fixed draw of the distribution tests


def philox4x32_10(ctr, key, rounds=10):
    """ctr: four uint32 arrays (or ints), key: two; returns the four output words as uint32 arrays"""
    c0, c1, c2, c3 = [np.atleast_1d(np.asarray(c, dtype=np.uint64)) & MASK32 for c in ctr]
    k0, k1 = [int(k) & 0xFFFFFFFF for k in key]
    for _ in range(rounds):
        p0 = PHILOX_M0 * c0                      # 32 x 32 -> 64 bits: no overflow in uint64
        p1 = PHILOX_M1 * c2
        n0 = (p1 >> SHIFT32) ^ c1 ^ np.uint64(k0)
        n1 = p1 & MASK32
        n2 = (p0 >> SHIFT32) ^ c3 ^ np.uint64(k1)
        n3 = p0 & MASK32
        c0, c1, c2, c3 = n0, n1, n2, n3
        k0 = (k0 + PHILOX_W0) & 0xFFFFFFFF
        k1 = (k1 + PHILOX_W1) & 0xFFFFFFFF
    return [c.astype(np.uint32) for c in (c0, c1, c2, c3)]


def uniform24(c):
    """the kernel's ((float)(c >> 8) + 0.5f) * (1.0f / 16777216.0f), in fp32"""
    f = (np.asarray(c, dtype=np.uint32) >> np.uint32(8)).astype(np.float32)      # < 2^24: exact
    return (f + np.float32(0.5)) * np.float32(1.0 / 16777216.0)


def randn_quads(quads, seed, offset=0):
    """[len(quads), 4] float64: the four samples of each quad index (sample 4q + k sits in column k)"""
    q = np.atleast_1d(np.asarray(quads, dtype=np.uint64))
    with np.errstate(over="ignore"):
        ctr = q + np.uint64(int(offset) & 0xFFFFFFFFFFFFFFFF)                   # 64-bit wrap-around sum
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    c = philox4x32_10((ctr & MASK32, ctr >> SHIFT32, PHILOX_W0, PHILOX_W1), (seed & 0xFFFFFFFF, seed >> 32))
    u0, u1, u2, u3 = [uniform24(w).astype(np.float64) for w in c]
    r0, r1 = np.sqrt(-2.0 * np.log(u0)), np.sqrt(-2.0 * np.log(u2))
    a0, a1 = 2.0 * np.pi * u1, 2.0 * np.pi * u3
    return np.stack([r0 * np.cos(a0), r0 * np.sin(a0), r1 * np.cos(a1), r1 * np.sin(a1)], axis=1)


def randn_ref(n, seed, offset=0):
    """float64 [n]: what acimg_randn(out, n, seed, offset) writes"""
    quads = (int(n) + 3) // 4
    return randn_quads(np.arange(quads, dtype=np.uint64), seed, offset).reshape(-1)[: int(n)]


def normal_checks(x):
    """the distribution statistics of the randn tests on a 1-D float64 torch tensor: dict of (value, bound).
    5 sigma (KS: alpha ~ 1e-3) conditions for n iid N(0, 1) samples"""
    import math

    import torch

    n = x.numel()
    m = x.mean().item()
    var = ((x - m) ** 2).mean().item()
    xs = torch.sort(x).values
    cdf = 0.5 * (1.0 + torch.erf(xs / math.sqrt(2.0)))
    i = torch.arange(n, dtype=torch.float64)
    ks = max(((i + 1) / n - cdf).max().item(), (cdf - i / n).max().item())
    out = {"mean": (abs(m), 5.0 / math.sqrt(n)), "var": (abs(var - 1.0), 5.0 * math.sqrt(2.0 / n)),
           "ks": (ks, 1.95 / math.sqrt(n))}
    for lag in (1, 2, 4):
        r = ((x[:-lag] - m) * (x[lag:] - m)).mean().item() / var
        out["autocorr%d" % lag] = (abs(r), 5.0 / math.sqrt(n))
    return out
