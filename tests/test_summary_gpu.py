"""The two summary kernels against their NumPy restatements (tests/summary_ref.py), between guard bands:
`acimg_summary_images` bit for bit, `acimg_histogram_segments` exact in counts / min / max / num and within the worst-case
bound of any summation order in sum / sum_squares."""
from collections import OrderedDict

import numpy as np
import pytest
import torch

import summary_ref as sref
from guard_arena import GuardArena
from op_support import raw_lib

pytestmark = pytest.mark.gpu

CHUNK, GRID = 8192, 512          # csrc/summary.hip: elements per chunk, workgroups of the partial launch at most


def _below(k):
    """the largest fp32 below k"""
    return np.nextafter(np.float32(k), np.float32(-np.inf))


def _frame_case():
    """[3,36,48,12], image 0 rendered: group 0 non-negative with its maximum, 1 some negative, 2 a maximum below 1e-6,
    3 constant; images 1 and 2 hold larger values, negatives and NaNs that must not leak in"""
    rng = np.random.RandomState(5)
    x = (rng.rand(3, 36, 48, 12) * 5).astype(np.float32)
    x[0, 0, 0, 0] = 8.0                       # the maximum: scale 255 / 8 is exact, so the maximum itself gives 255
    x[0, :, :, 3:6] -= 2.0
    x[0, :, :, 6:9] = (rng.rand(36, 48, 3) * 9e-7).astype(np.float32)
    x[0, :, :, 9:12] = 2.5
    x[1] = x[1] * 100 - 250
    x[2, ::2] = np.nan
    return x, 0, 4, 1


def _strided_case():
    """[2,5,7,16], channels 3..8 of 16, both images: the tail (35 pixels), the stride and the channel offset.  image 0:
    group 0 one NaN and one Inf channel (red pixels; the extremes come from the finite values), group 1 all non-finite;
    image 1: group 0 scale exactly 1 with values just below an integer (truncation, not rounding) and the maximum itself,
    group 1 the negative rule with scale exactly 1.  Every channel outside 3..8 holds NaN."""
    rng = np.random.RandomState(6)
    x = np.full((2, 5, 7, 16), np.nan, np.float32)
    a = (rng.rand(5, 7, 3) * 4 + 1).astype(np.float32)
    a[1, 2, 0] = np.nan
    a[3, 4, 2] = np.inf
    a[0, 0, 1] = -np.inf
    x[0, :, :, 3:6] = a
    x[0, :, :, 6:9] = np.array([np.nan, np.inf, -np.inf], np.float32)
    b = np.array([_below(k) for k in rng.randint(1, 255, size=105)], np.float32).reshape(5, 7, 3)
    b[4, 6, 2] = 255.0
    b[0, 0, 0] = 0.0
    x[1, :, :, 3:6] = b
    c = np.array([_below(k) for k in rng.randint(-126, 127, size=105)], np.float32).reshape(5, 7, 3)
    c[2, 2, 2] = -127.0
    c[2, 3, 0] = 126.5
    x[1, :, :, 6:9] = c
    return x, 3, 2, 2


@pytest.mark.parametrize("case", [_frame_case, _strided_case])
def test_summary_images_bit_equal(device, case):
    from acimg import ops
    m, L = raw_lib()
    x, c0, G, n_images = case()
    N, H, W, ldc = x.shape
    want = sref.summary_images(x, c0, G, n_images)
    if case is _strided_case:
        assert want[0, 0, 1, 2].tolist() == [255, 0, 0] and want[0, 0, 3, 4].tolist() == [255, 0, 0]
        assert (want[0, 1].reshape(-1, 3) == (255, 0, 0)).all()
        assert want[1, 0, 4, 6, 2] == 255 and want[1, 0].max() == 255          # the maximum itself
        k = np.round(x[1, :, :, 3:6]).astype(int)
        sel = x[1, :, :, 3:6] != np.round(x[1, :, :, 3:6])
        assert (want[1, 0][sel] == k[sel] - 1).all()                            # trunc(k - ulp) = k - 1
        assert want[1, 1, 2, 2, 2] == 1                                         # -127 * 1 + 128
    else:
        assert want[0, 0].max() == 255 and (want[0, 2] == 0).all() and (want[0, 3] == 255).all()
        assert want[0, 1].min() < 128 < want[0, 1].max()
    xd = torch.from_numpy(x).to(device)
    nbytes = n_images * G * H * W * 3
    arena = GuardArena.for_sizes(device, [nbytes])
    out = arena.region(nbytes, fill=0x5A, name="out")
    st = ops.current_stream_handle(device)
    runs = []
    for _ in range(2):
        out.fill(0x5A)
        m.check(L.acimg_summary_images(xd.data_ptr(), ldc, H * W, c0, G, n_images, out.ptr, st), "summary_images")
        torch.cuda.synchronize(device)
        arena.check("summary_images")
        runs.append(out.u8.cpu().numpy().reshape(n_images, G, H, W, 3))
    assert np.array_equal(runs[0], want)
    assert np.array_equal(runs[0], runs[1])


def test_summary_images_wrapper(device):
    from acimg import ops
    x, c0, G, n_images = _frame_case()
    xd = torch.from_numpy(x).to(device)
    out = torch.zeros((n_images, G, 36, 48, 3), dtype=torch.uint8, device=device)
    ops.summary_images(ops.Plan(device, eager=True), xd, 12, 36 * 48, c0, G, n_images, out)
    assert np.array_equal(out.cpu().numpy(), sref.summary_images(x, c0, G, n_images))


# ---- histograms -----------------------------------------------------------------------------------------------------------
PAD = np.float32(5e-13)          # the garbage in every pad position: it would land in the bucket that ends at 1e-12


def _specials(limits):
    fin = [x for x in limits if 1e-30 < abs(x) < 1e30]
    pick = [fin[i] for i in np.linspace(0, len(fin) - 1, 20).astype(int)]
    out = [0.0, -0.0, 1e-40, -1e-40, 1.4e-45, -1.4e-45, 1.1754942e-38, 3e38, -3e38]
    for lim in pick:
        f = np.float32(lim)
        out += [f, np.nextafter(f, np.float32(-np.inf)), np.nextafter(f, np.float32(np.inf))]
    return np.array(out, np.float32)


@pytest.fixture(scope="module")
def hist_case():
    """the flat buffer, the segment table and the restatement's answer per segment, computed once"""
    from acimg import events
    limits = events.default_bucket_limits()
    rng = np.random.RandomState(9)
    big = (1, 1, 2056, 2048)
    assert big[2] * big[3] > GRID * CHUNK          # more than one sweep of the partial launch's grid
    # (dims, lo, hi); the fused-head case: two column boxes of ONE [40,12] matrix (its last column a pad)
    specs = [((4, 1, 1, 1), (0, 0, 0, 0), (3, 1, 1, 1)),
             ((3, 3, 8, 8), (0, 0, 0, 0), (3, 3, 5, 6)),
             ((40, 12, 1, 1), (0, 0, 0, 0), (40, 5, 1, 1)),
             ((40, 12, 1, 1), (0, 5, 0, 0), (40, 11, 1, 1)),
             (big, (0, 0, 0, 0), (1, 1, 2050, 2045)),
             ((6, 7, 1, 1), (1, 0, 0, 0), (6, 5, 1, 1))]          # rows of 7: no 16-byte loads
    offsets, off = [], 0
    for i, (dims, _, _) in enumerate(specs):
        if i == 3:
            offsets.append(offsets[2])
            continue
        offsets.append(off)
        off += -(-int(np.prod(dims)) // 64) * 64
    base = np.full(off + 64, PAD, np.float32)
    spec = _specials(limits)
    want = []
    for (dims, lo, hi), o in zip(specs, offsets):          # the boxes are disjoint: each is filled once
        n = int(np.prod(dims))
        view = base[o:o + n].reshape(dims)
        box = tuple(slice(a, b) for a, b in zip(lo, hi))
        vals = (rng.randn(*[b - a for a, b in zip(lo, hi)]) * 0.1).astype(np.float32)
        flat = vals.reshape(-1)
        if flat.size >= 2 * spec.size:
            flat[rng.choice(flat.size, spec.size, replace=False)] = spec
        elif flat.size >= 4:
            flat[:4] = [0.0, -0.0, 1e-40, -3e38]
        view[box] = vals
        want.append(sref.histogram(view[box], limits))
    table = np.array([[o] + list(d) + list(lo) + list(hi) for (d, lo, hi), o in zip(specs, offsets)], np.int64)
    total = int(sum(np.prod(d) for d, _, _ in specs))
    return base, table, limits, total, want, specs


def _run_hist(device, base, table, limits, total, arena=None, regions=None, ws_bytes=None):
    from acimg import ops
    m, L = raw_lib()
    V, nl = table.shape[0], len(limits)
    bd = torch.from_numpy(base).to(device)
    td = torch.from_numpy(table).to(device)
    ld = torch.tensor(limits, dtype=torch.float64, device=device)
    st = ops.current_stream_handle(device)
    r = regions
    rc = L.acimg_histogram_segments(bd.data_ptr(), td.data_ptr(), V, ld.data_ptr(), nl, total, r["counts"].ptr,
                                    r["stats"].ptr, r["nonfinite"].ptr, r["ws"].ptr, ws_bytes, st)
    torch.cuda.synchronize(device)
    return rc


def test_histogram_segments(device, hist_case):
    m, L = raw_lib()
    base, table, limits, total, want, specs = hist_case
    V, nl = table.shape[0], len(limits)
    q = int(L.acimg_histogram_segments_workspace(V, nl, total))
    assert q == -(-(V + 1) * 8 // 32) * 32 + 32 * (total // CHUNK + V)
    sizes = OrderedDict(counts=V * nl * 8, stats=V * 32, nonfinite=V * 8, ws=q)
    arena = GuardArena.for_sizes(device, sizes.values())
    r = OrderedDict((k, arena.region(n, fill=0x5A, name=k)) for k, n in sizes.items())
    # a workspace 16 bytes short is refused before anything is written
    assert _run_hist(device, base, table, limits, total, arena, r, q - 16) == -2
    assert bool((arena.buf[r["counts"].off:r["counts"].off + sizes["counts"]] == 0x5A).all())
    arena.check("histogram_segments, short workspace")
    runs = []
    for _ in range(2):
        for reg in r.values():
            reg.fill(0x5A)
        rc = _run_hist(device, base, table, limits, total, arena, r, q)
        assert rc == 0, m.last_error()
        arena.check("histogram_segments")
        runs.append((r["counts"].view(torch.int64, V, nl).cpu().numpy().copy(),
                     r["stats"].view(torch.float64, V, 4).cpu().numpy().copy(),
                     r["nonfinite"].view(torch.int64, V).cpu().numpy().copy()))
    counts, stats, bad = runs[0]
    edge = limits.index(1e-12)
    for v, (wc, ws, wbad) in enumerate(want):
        dims, lo, hi = specs[v]
        n = int(np.prod([b - a for a, b in zip(lo, hi)]))
        assert wbad == 0 and bad[v] == 0
        assert np.array_equal(counts[v], wc), (v, np.nonzero(counts[v] != wc)[0][:8])
        assert int(counts[v].sum()) == n == int(ws["num"])               # num: the box, not the padded extent
        assert counts[v][edge] == wc[edge]                               # no pad in the bucket that ends at 1e-12
        assert stats[v, 0] == ws["min"] and stats[v, 1] == ws["max"], (v, stats[v], ws)
        box = tuple(slice(a, b) for a, b in zip(lo, hi))
        o = int(table[v, 0])
        d = base[o:o + int(np.prod(dims))].reshape(dims)[box].astype(np.float64).reshape(-1)
        u = 2.0 ** -53
        print("segment %d: n = %d, |sum - ref| = %.3e (bound %.3e), |sq - ref| = %.3e (bound %.3e)" % (
            v, n, abs(stats[v, 2] - ws["sum"]), n * u * np.abs(d).sum(), abs(stats[v, 3] - ws["sum_squares"]),
            n * u * (d * d).sum()))
        assert abs(stats[v, 2] - ws["sum"]) <= n * u * np.abs(d).sum()
        assert abs(stats[v, 3] - ws["sum_squares"]) <= n * u * (d * d).sum()
    for a, b in zip(runs[0], runs[1]):
        assert a.tobytes() == b.tobytes()                                 # two runs: bit-equal


def test_histogram_segments_reports_nonfinite(device):
    from acimg import events, ops
    from acimg.logger import histogram_fields
    limits = events.default_bucket_limits()
    base = np.full(128, 0.25, np.float32)
    base[[1, 5]] = [np.nan, -np.inf]          # inside the box of segment 0
    base[7] = np.nan                          # a pad of segment 0
    table = np.array([[0, 8, 1, 1, 1, 0, 0, 0, 0, 6, 1, 1, 1], [64, 4, 4, 1, 1, 0, 0, 0, 0, 4, 4, 1, 1]], np.int64)
    V, nl = 2, len(limits)
    counts = torch.zeros((V, nl), dtype=torch.int64, device=device)
    stats = torch.zeros((V, 4), dtype=torch.float64, device=device)
    bad = torch.zeros((V,), dtype=torch.int64, device=device)
    ops.histogram_segments(ops.Plan(device, eager=True), torch.from_numpy(base).to(device),
                           torch.from_numpy(table).to(device), V, torch.tensor(limits, dtype=torch.float64, device=device),
                           nl, 24, counts, stats, bad)
    counts, stats, bad = counts.cpu().numpy(), stats.cpu().numpy(), bad.cpu().numpy()
    assert bad.tolist() == [2, 0]
    assert int(counts[0].sum()) == 4 and stats[0].tolist() == [0.25, 0.25, 1.0, 0.25]
    assert int(counts[1].sum()) == 16 and stats[1].tolist() == [0.25, 0.25, 4.0, 1.0]
    with pytest.raises(ValueError, match="Nan in summary histogram for: scope/kernel:0"):
        histogram_fields("scope/kernel:0", counts[0], stats[0], bad[0], limits)
    got = histogram_fields("scope/bias:0", counts[1], stats[1], bad[1], limits)
    assert got["num"] == 16.0 and got["sum"] == 4.0
