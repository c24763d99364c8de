"""Exact t-SNE on the device (acimg_tsne_*, acimg.retrieval.TSNE, `python -m acimg.retrieval tsne`) against the NumPy
restatement tests/tsne_ref.py.  Every bound below is worked out from the arithmetic (u = 2^-53, the unit roundoff of
fp64 under round-to-nearest), none from what the device returned; tests/test_tsne_cpu.py holds the seeded inputs to the
condition the exact comparisons (search steps, gain decisions) rest on: no decision quantity within 1e-10 of its
threshold.  The descent is chaotic (a 1e-15 relative change of P is of order 1 after 300 iterations), so trajectories are
never compared: every step is checked from the device's own state."""
import json
import os
import struct
import sys
import zlib

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import tsne_ref as ref  # noqa: E402
from guard_arena import CANARY, GuardArena  # noqa: E402

pytestmark = pytest.mark.gpu
U = 2.0 ** -53
POISON = float("nan")
LD = np.longdouble
_CACHE = {}


def tsne_reference(N, D, perplexity, seed):
    """the restatement's search of one seeded input, computed once and shared (never modified)"""
    key = (N, D, perplexity, seed)
    if key not in _CACHE:
        x = ref.affinity_input(N, D, seed)
        d = ref.distances(x)
        s = ref.search(d, perplexity)
        _CACHE[key] = dict(x=x, d=d, search=s, P=ref.symmetrize(s["cond"]))
    return _CACHE[key]


def padded(a, ld, device):
    t = torch.full((a.shape[0], ld), POISON, dtype=torch.float64)
    t[:, :a.shape[1]] = torch.from_numpy(a)
    return t.to(device)


@pytest.mark.parametrize("N,D,perplexity,seed", ref.AFFINITY_CASES)
def test_affinities_against_the_restatement(device, N, D, perplexity, seed):
    """steps exact, beta to 1e-12, pads untouched, symmetrisation bit-equal, and every p_{j|i} within
        (N + 8 + (D + 2) d_ij beta_i) u p_ref + 2^-1074
    of p_ref = exp(-d_ij beta_i) / S_i evaluated in extended precision (np.longdouble, 64 mantissa bits: its own error
    is below u / 1000 of every quantity) at the device's beta, which the line before held to the restatement's.
    The constants, to first order in u, every rounding at most u relative:
      D + 2: the device's d_ij: the difference x_i[d] - x_j[d] is rounded once and squared (2 u), the D terms, all
             positive, are accumulated by D fused multiply-adds (one rounding each: at most D u on the sum); an error
             eps of d moves exp(-d beta) by eps d beta relative;
      N:     S_i is a sum of N - 1 positive terms: at most (N - 2) u in any order; the device's tree is shallower;
      8:     the product d beta (1 u, times d beta: counted here since d beta < 745 where p > 0 matters and the bound
             is dominated by the D term), exp to 1 ulp = 2 u in the numerator and 2 u in the terms of S, the division
             (1 u), and 2 u left for the p-weighted mean of the distance errors inside S, which as rounding errors of
             independent sums do not line up;
      2^-1074: a quotient below 2^-1022 is rounded to a subnormal, half a spacing at most; one whole spacing allowed."""
    from acimg import ops
    r = tsne_reference(N, D, perplexity, seed)
    s = r["search"]
    ldx, ldp = D + 3, N + 5
    xd = padded(r["x"], ldx, device)
    P = torch.full((N, ldp), POISON, dtype=torch.float64, device=device)
    beta = torch.zeros(N, dtype=torch.float64, device=device)
    steps = torch.zeros(N, dtype=torch.int32, device=device)
    plan = ops.Plan(device, eager=True)
    ops.tsne_affinities(plan, xd, ldx, N, D, perplexity, P, ldp, beta, steps)
    torch.cuda.synchronize(device)
    got, gb, gs = P.cpu().numpy(), beta.cpu().numpy(), steps.cpu().numpy()
    assert np.array_equal(gs, s["steps"])
    np.testing.assert_allclose(gb, s["beta"], rtol=1e-12, atol=0)
    assert np.isnan(got[:, N:]).all()                         # the pad columns still hold the poison
    cond = got[:, :N]
    assert (np.diag(cond) == 0).all()
    x = r["x"].astype(LD)
    worst = 0.0
    for i in range(N):
        d = np.sum((x[i] - x) ** 2, axis=1)
        p = np.exp(-d * LD(gb[i]))
        p[i] = 0
        p_ref = p / p.sum()
        bound = (N + 8 + (D + 2) * d * LD(gb[i])) * U * p_ref + LD(2.0) ** -1074
        err = np.abs(cond[i].astype(LD) - p_ref)
        worst = max(worst, float(np.max(err / bound)))
        assert (err <= bound).all(), (i, int(np.argmax(err / bound)), float(np.max(err / bound)))
    print("affinities N=%d D=%d: largest error / bound = %.3f" % (N, D, worst))
    # symmetrisation: bit-equal to (A + A.T) / (2N), pads untouched
    ops.tsne_symmetrize(plan, P, ldp, N)
    torch.cuda.synchronize(device)
    sym = P.cpu().numpy()
    want = (cond + cond.T) / (2.0 * N)
    np.fill_diagonal(want, 0.0)
    assert np.array_equal(sym[:, :N], want)
    assert np.isnan(sym[:, N:]).all()


def _kl_bound(rows, mag, N):
    return (N * N + 16) * U * (mag[:, 5].sum() + abs(np.log(rows[:, 4].sum())))


def _check_step(t, Pld, N, lr):
    """one device iteration from the device's own state against the restatement from that state"""
    Y0, V0, G0 = (a.cpu().numpy().copy() for a in (t.Y, t.V, t.G))
    it = t.iteration
    e, m = ref.schedule(it, 12.0, ref.DESCENT_EXAGGERATION_ITERS)
    t.step(1, want_kl=True)
    torch.cuda.synchronize(t.device)
    rows_dev, kl_dev = t.rows.cpu().numpy(), float(t.kl.cpu()[0])
    Y1, V1, G1 = (a.cpu().numpy() for a in (t.Y, t.V, t.G))
    # rows: (N + 16) u sum|terms|.  A term's factors carry at most 14 u (w: 6 u - the rounded differences squared and
    # added, 1 +, the reciprocal; w^2 twice that; the product with P or the difference 1 u each; the KL term's two
    # logarithms 2 u each of THEIR magnitude, which the restatement's sum|terms| counts), and a term passes through at
    # most ceil(N / 256) + 8 additions of the fixed tree: below N + 2 for every N >= 7.
    rows, mag = ref.row_sums(Pld, Y0.astype(LD), True)
    er = (N + 16) * U
    assert (np.abs(rows_dev - rows) <= er * mag).all(), (it, np.max(np.abs(rows_dev - rows) / (er * mag + 1e-300)))
    # kl = sum of the N row parts + log Z: (N^2 + 16) u sum|terms| covers the rows' bound (N + 16) u, the N - 1
    # additions, Z's relative error (at most 2 (N + 16) u, so as much absolute in log Z) and the logarithm (2 u)
    Z = rows[:, 4].sum()
    kl_ref = rows[:, 5].sum() + np.log(Z)
    assert abs(kl_dev - kl_ref) <= _kl_bound(rows, mag, N), (it, kl_dev, kl_ref)
    # the update, from the restatement's rows: g = 4 (e A - R / Z).  A and R carry er * mag each; Z, a sum of
    # positive row sums each within er, is within 2 er relative (its own N - 1 additions included), which moves R / Z by
    # 2 er |R| / Z <= 2 er magR / Z; the products, the quotient and the difference add 4 u of the two parts' magnitudes
    Yr, Vr, Gr, g, inc, fragile = ref.update(rows, e, m, lr, Y0, V0, G0)
    assert not fragile.any(), it                              # a condition on the inputs (tests/test_tsne_cpu.py)
    gb = 4.0 * (er + 4 * U) * (e * mag[:, 0:2] + 3.0 * mag[:, 2:4] / Z)
    # G: exactly one of the three rule outcomes, and the one the restatement's decision picks
    assert np.array_equal(G1, Gr), it
    assert ((G1 == G0 + 0.2) | (G1 == G0 * 0.8) | (G1 == 0.01)).all(), it
    # V = m V - lr G g: lr G times g's bound, 3 u for the three products and the difference; Y += V: one more rounding
    vb = lr * Gr * gb + 3 * U * (np.abs(m * V0) + np.abs(lr * Gr * g))
    assert (np.abs(V1 - Vr) <= vb).all(), (it, np.max(np.abs(V1 - Vr) / vb))
    assert (np.abs(Y1 - Yr) <= vb + U * np.abs(Yr)).all(), it
    return inc


@pytest.mark.parametrize("N,D,perplexity,seed,lr", ref.DESCENT_CASES)
def test_gradient_and_update_step_by_step(device, N, D, perplexity, seed, lr):
    """steps 0..5 with exaggeration_iters = 3: both values of the exaggeration and of the momentum; the rows, the
    divergence, G (exact), V and Y after every step, each from the device's own state before it"""
    from acimg import retrieval
    P = tsne_reference(N, D, perplexity, seed)["P"]
    t = retrieval.TSNE(device)
    t.init(P, ref.initial(N), learning_rate=lr, exaggeration_iters=ref.DESCENT_EXAGGERATION_ITERS)
    assert torch.equal(t.V.cpu(), torch.zeros(N, 2, dtype=torch.float64)) and float(t.G.min()) == 1.0
    Pld = P.astype(LD)
    seen = set()
    for _ in range(ref.DESCENT_STEPS):
        seen |= set(np.unique(_check_step(t, Pld, N, lr)).tolist())
    assert t.iteration == ref.DESCENT_STEPS and seen == {False, True}     # both gain rules were exercised
    # without want_kl the row's KL slot is 0 and kl is left alone
    before = t.kl.clone()
    t.step(1)
    torch.cuda.synchronize(device)
    assert float(t.rows[:, 5].abs().max()) == 0.0 and torch.equal(t.kl, before)
    # divergence(): the KL at the current Y, no state change
    Y = t.Y.clone()
    kl = float(t.divergence().cpu()[0])
    assert torch.equal(t.Y, Y) and t.iteration == ref.DESCENT_STEPS + 1
    rows, mag = ref.row_sums(Pld, Y.cpu().numpy().astype(LD), True)
    assert abs(kl - ref.kl_of(rows)) <= _kl_bound(rows, mag, N)


def test_two_runs_of_fifty_iterations_are_bit_identical(device):
    from acimg import retrieval
    N, D, perplexity, seed, lr = ref.DESCENT_CASES[1]
    x = tsne_reference(N, D, perplexity, seed)["x"]
    out = []
    for _ in range(2):
        t = retrieval.TSNE(device)
        P, beta, steps = t.affinities(x, perplexity)
        t.init(P, ref.initial(N), learning_rate=lr).step(50, want_kl=True)
        torch.cuda.synchronize(device)
        out.append([a.cpu().numpy().copy() for a in (P, beta, steps, t.Y, t.V, t.G, t.kl, t.rows)])
    for a, b in zip(*out):
        assert np.array_equal(a, b)
    assert np.isfinite(out[0][3]).all() and np.isfinite(out[0][6]).all()


def test_caller_memory_of_the_four_entries(device):
    """every output between guard bands (tests/guard_arena.py), leading dimensions padded: nothing outside the stated
    extents is written - the pad columns of P keep their fill, the bands their canary"""
    from acimg import _lib, ops
    L = _lib.load()
    N, D, perplexity, seed = ref.AFFINITY_CASES[1]
    r = tsne_reference(N, D, perplexity, seed)
    ldx, ldp, FILL = D + 3, N + 5, 0x7B
    sizes = dict(P=N * ldp * 8, beta=N * 8, steps=N * 4, rows=N * 6 * 8, Y=N * 2 * 8, V=N * 2 * 8, G=N * 2 * 8, kl=8)
    arena = GuardArena.for_sizes(device, list(sizes.values()))
    reg = {k: arena.region(n, fill=FILL, name=k) for k, n in sizes.items()}
    xd = padded(r["x"], ldx, device)
    st = ops.current_stream_handle(device)
    assert L.acimg_tsne_affinities(xd.data_ptr(), ldx, N, D, perplexity, reg["P"].ptr, ldp, reg["beta"].ptr,
                                   reg["steps"].ptr, st) == 0
    torch.cuda.synchronize(device)
    arena.check("tsne_affinities")
    Pv = reg["P"].view(torch.float64, N, ldp)

    def pads_keep_their_fill():
        return bool((Pv[:, N:].contiguous().view(torch.uint8) == FILL).all())
    assert pads_keep_their_fill()
    assert np.array_equal(reg["steps"].view(torch.int32, N).cpu().numpy(), r["search"]["steps"])
    assert L.acimg_tsne_symmetrize(reg["P"].ptr, ldp, N, st) == 0
    torch.cuda.synchronize(device)
    arena.check("tsne_symmetrize")
    assert pads_keep_their_fill()
    sym = Pv[:, :N].cpu().numpy()
    assert np.array_equal(sym, sym.T) and abs(sym.sum() - 1.0) <= N * N * U
    reg["Y"].view(torch.float64, N, 2).copy_(torch.from_numpy(ref.initial(N)))
    reg["V"].view(torch.float64, N, 2).zero_()
    reg["G"].view(torch.float64, N, 2).fill_(1.0)
    for want_kl, kl in ((1, reg["kl"].ptr), (0, None)):
        assert L.acimg_tsne_gradient(reg["P"].ptr, ldp, N, reg["Y"].ptr, want_kl, reg["rows"].ptr, st) == 0
        torch.cuda.synchronize(device)
        arena.check("tsne_gradient")
        assert L.acimg_tsne_update(reg["rows"].ptr, N, 12.0, 0.5, 50.0, reg["Y"].ptr, reg["V"].ptr, reg["G"].ptr, kl,
                                   st) == 0
        torch.cuda.synchronize(device)
        arena.check("tsne_update")
    assert L.acimg_tsne_update(reg["rows"].ptr, N, 1.0, 0.0, 1.0, None, None, None, reg["kl"].ptr, st) == 0
    torch.cuda.synchronize(device)
    arena.check("tsne_update (divergence only)")
    assert np.isfinite(reg["Y"].view(torch.float64, N, 2).cpu().numpy()).all()
    assert CANARY != FILL


@pytest.fixture(scope="module")
def cluster_run(device):
    from acimg import retrieval
    x, labels = ref.clusters()
    t = retrieval.TSNE(device)
    Y, trace = t.fit_transform(x, perplexity=10.0, n_iter=500, seed=0, learning_rate=12.5)
    return x, labels, Y, trace, t


def test_clusters_end_to_end(device, cluster_run):
    """three Gaussian clusters in 16-D (centres 10 randn, unit noise, 50 rows each), perplexity 10, learning rate
    12.5 = N / 12, 500 iterations: purity 1.0, and the final KL inside the restatement's own range over its five
    initial seeds widened by its spread on each side.  The committed restatement gives, for seeds 0..4,
    0.651118, 0.641349, 0.660152, 0.646537, 0.639049: min 0.639049, max 0.660152, spread 0.021103, so the accepted
    range is [0.617946, 0.681255] (tests/test_tsne_cpu.py: all five reach purity 1.0)."""
    x, labels, Y, trace, t = cluster_run
    assert Y.shape == (150, 2) and Y.dtype == np.float64 and np.isfinite(Y).all()
    assert ref.purity(Y, labels) == 1.0
    lo, hi = 0.639049, 0.660152
    kl = trace[-1][1]
    print("clusters: final KL %.6f, trace %s" % (kl, trace))
    assert lo - (hi - lo) <= kl <= hi + (hi - lo)
    assert [it for it, _ in trace] == list(range(0, 500, 50)) + [500]
    # the trace's last entry is the divergence of the returned map, and the first that of the initial one (against the
    # restatement's P, which the affinity bounds put within 1e-12 relative of the device's: 1e-9 is ample)
    P = ref.joint(x, 10.0)
    assert abs(kl - ref.kl_divergence(P, Y)) <= 1e-9 * kl
    assert abs(trace[0][1] - ref.kl_divergence(P, ref.initial(150, 0))) <= 1e-9 * trace[0][1]
    assert t.learning_rate == 12.5 and t.iteration == 500


def _png_pixels(path):
    data = open(path, "rb").read()
    assert data[:8] == b"\x89PNG\r\n\x1a\n"
    w, h, depth, ctype = struct.unpack(">IIBB", data[16:26])
    assert (depth, ctype) == (8, 2)
    pos, idat = 8, b""
    while pos < len(data):
        n, kind = struct.unpack(">I", data[pos:pos + 4])[0], data[pos + 4:pos + 8]
        if kind == b"IDAT":
            idat += data[pos + 8:pos + 8 + n]
        pos += 12 + n
    raw = np.frombuffer(zlib.decompress(idat), np.uint8).reshape(h, 1 + 3 * w)
    assert (raw[:, 0] == 0).all()
    return raw[:, 1:].reshape(h, w, 3)


def test_tsne_tool_writes_the_four_files(device, tmp_path):
    from acimg import retrieval
    x, labels = ref.clusters(seed=5, k=3, per=20, D=8)
    ck = str(tmp_path / "ckpt" / "epoch_3.ckpt")
    d = retrieval.dump_dir(ck, "testing", "Video")
    os.makedirs(d)
    np.save("%s/testing_data.npy" % d, x)
    np.save("%s/testing_labels.npy" % d, np.eye(10, dtype=int)[labels])
    argv = ["tsne", ck, "Video", "testing", "--perplexity", "8", "--n_iter", "60", "--seed", "2", "--device", str(device)]
    assert retrieval.main(argv) == 0
    f_map, f_index, f_json, f_png = retrieval.tsne_files(ck, "Video", "testing")
    Y, trace = retrieval.TSNE(device).fit_transform(x, perplexity=8.0, n_iter=60, seed=2)
    assert np.array_equal(np.load(f_map), Y)
    assert np.array_equal(np.load(f_index), np.arange(60))
    with open(f_json) as f:
        js = json.load(f)
    assert (js["N"], js["num_rows"], js["perplexity"], js["n_iter"], js["seed"]) == (60, 60, 8.0, 60, 2)
    assert js["learning_rate"] == 50.0 and js["kl_trace"] == [[t, v] for t, v in trace] and js["kl"] == trace[-1][1]
    assert [t for t, _ in js["kl_trace"]] == [0, 50, 60]
    img = _png_pixels(f_png)
    assert img.shape == (800, 800, 3)
    assert np.array_equal(img, retrieval.rasterize_scatter(Y, labels, 10))
    pal = retrieval.hls_palette(10)
    present = [c for c in range(10) if (img == pal[c]).all(axis=2).any()]
    assert len(present) >= 2 and set(present) <= {0, 1, 2}
    # more rows than --max_points: a seeded ascending subsample, recorded in the index file
    assert retrieval.main(argv + ["--max_points", "40"]) == 0
    idx = np.load(f_index)
    assert np.array_equal(idx, retrieval.tsne_subsample(60, 40, 2)) and np.load(f_map).shape == (40, 2)
    Ys, _ = retrieval.TSNE(device).fit_transform(x[idx], perplexity=8.0, n_iter=60, seed=2)
    assert np.array_equal(np.load(f_map), Ys)
