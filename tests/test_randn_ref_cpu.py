"""The numpy restatement of acimg_randn (tests/randn_ref.py) is anchored to published vectors before the GPU tests of
tests/test_glue_ops_gpu.py rely on it."""
import numpy as np
import torch

import randn_ref as rr

# Random123 kat_vectors, philox4x32 with 10 rounds: counter, key, expected
KAT = [
    ((0, 0, 0, 0), (0, 0), (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)),
    ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)),
    ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0),
     (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1)),
]

def test_philox4x32_10_known_answers():
    for ctr, key, want in KAT:
        got = tuple(int(w[0]) for w in rr.philox4x32_10(ctr, key))
        assert got == want, (["%08x" % v for v in got], ["%08x" % v for v in want])
    # vectorised over counters: the same words as one counter at a time
    ctrs = np.array([k[0] for k in KAT], dtype=np.uint64)
    out = rr.philox4x32_10([ctrs[:, i] for i in range(4)], KAT[2][1])
    for j in range(3):
        one = rr.philox4x32_10(KAT[j][0], KAT[2][1])
        assert [int(w[j]) for w in out] == [int(w[0]) for w in one]


def test_uniform_is_the_kernels_fp32_expression():
    """(float)(c >> 8) + 0.5f rounds the half away from 2^23 on: u can be exactly 1.0, never 0"""
    assert np.float32(2 ** 23 + 1) + np.float32(0.5) == np.float32(8388610)
    u = rr.uniform24(np.array([0, 0xFF, 0x100, (2 ** 23 + 1) << 8, 0xFFFFFFFF], dtype=np.uint32))
    assert u.dtype == np.float32
    assert u[0] == np.float32(2.0 ** -25) and u[1] == u[0] and u[2] == np.float32(1.5 * 2.0 ** -24)
    assert u[3] == np.float32(8388610 * 2.0 ** -24)
    assert u[4] == np.float32(1.0)
    # u == 1 gives radius 0, 2 u == 2 gives angle 2 pi: finite samples
    assert np.isfinite(rr.randn_ref(4099, 5)).all()


def test_counter_is_a_64_bit_sum_and_offsets_compose():
    big = rr.randn_ref(64, 77)
    assert np.array_equal(rr.randn_ref(16, 77, offset=5), big[20:36])
    assert np.array_equal(rr.randn_ref(7, 77), big[:7])
    # quad 2 at offset 2^32 - 2 has counter words (0, 1)
    carry = rr.randn_quads([2, 3], 9, offset=2 ** 32 - 2)
    w = rr.philox4x32_10(([0, 1], [1, 1], rr.PHILOX_W0, rr.PHILOX_W1), (9, 0))
    u = [rr.uniform24(x).astype(np.float64) for x in w]
    assert np.array_equal(carry[:, 0], np.sqrt(-2 * np.log(u[0])) * np.cos(2 * np.pi * u[1]))
    no_carry = rr.philox4x32_10(([0, 1], [0, 0], rr.PHILOX_W0, rr.PHILOX_W1), (9, 0))
    assert not np.array_equal(no_carry[0], w[0])
    # the high half of the seed is the second key word
    assert not np.array_equal(rr.randn_ref(8, 3), rr.randn_ref(8, 3 + (1 << 32)))


def test_reference_draw_passes_the_distribution_checks():
    """the 5 sigma / KS bounds of the GPU distribution test are conditions on one fixed draw: the reference itself
    meets every one of them for the chosen seed (were it not so, the seed would change, not the bound)"""
    x = torch.from_numpy(rr.randn_ref(rr.DIST_N, rr.DIST_SEED))
    assert torch.isfinite(x).all()
    for name, (val, bound) in rr.normal_checks(x).items():
        print("%s: %.3e (bound %.3e)" % (name, val, bound))
        assert val <= bound, (name, val, bound)
