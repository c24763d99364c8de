"""NumPy fp64 restatement of the exact t-SNE that include/acimg.h states (acimg_tsne_*): distances, the per-row precision
search, the symmetrisation, the row sums of the gradient, the update rule and the divergence.  Besides the values it
reports what the tests' bounds and input conditions need: for every search step its `diff` and the decision taken, for
every sum the sum of the absolute values of its terms, and which rows / elements are FRAGILE - a decision quantity
within FRAGILE of its threshold, where a rounding difference between two correct implementations may flip the decision.
Plain NumPy, vectorised over rows; no GPU."""
import numpy as np

MAX_STEPS = 100
SEARCH_TOL = 1e-5
FRAGILE = 1e-10
STOP, UP, DOWN = 0, 1, 2            # decisions of a search step: |diff| <= tol, diff > 0, otherwise


def distances(x):
    """d_ij = sum_d (x_i[d] - x_j[d])^2 in direct-difference form, [N,N]"""
    x = np.asarray(x, np.float64)
    out = np.empty((x.shape[0], x.shape[0]))
    for i in range(x.shape[0]):
        out[i] = np.sum((x[i] - x) ** 2, axis=1)
    return out


def search(d, perplexity):
    """the precision search of every row of the distance matrix d -> dict:
    cond [N,N] p_{j|i} (diagonal 0); beta [N]; steps [N] int (steps evaluated); S [N]; trace: list over steps of
    (active rows, diff, decision); fragile [N] bool"""
    N = d.shape[0]
    logp = np.log(perplexity)
    off = ~np.eye(N, dtype=bool)
    beta = np.ones(N)
    lo, hi = np.full(N, -np.inf), np.full(N, np.inf)
    steps = np.zeros(N, dtype=np.int32)
    S_out, p_out = np.zeros(N), np.zeros((N, N))
    fragile = np.zeros(N, dtype=bool)
    active = np.arange(N)
    trace = []
    for step in range(MAX_STEPS):
        if active.size == 0:
            break
        b = beta[active]
        p = np.exp(-d[active] * b[:, None]) * off[active]
        S = p.sum(axis=1)
        S[S == 0.0] = 1e-8
        H = np.log(S) + b * np.sum(d[active] * p, axis=1) / S
        diff = H - logp
        steps[active] = step + 1
        S_out[active], p_out[active] = S, p
        stop = np.abs(diff) <= SEARCH_TOL
        decision = np.where(stop, STOP, np.where(diff > 0.0, UP, DOWN))
        trace.append((active.copy(), diff.copy(), decision))
        fragile[active] |= np.abs(np.abs(diff) - SEARCH_TOL) <= FRAGILE
        fragile[active] |= np.abs(diff) <= FRAGILE
        if step == MAX_STEPS - 1:
            break
        for rows, up in ((active[decision == UP], True), (active[decision == DOWN], False)):
            if up:
                lo[rows] = beta[rows]
                beta[rows] = np.where(np.isinf(hi[rows]), beta[rows] * 2.0, (beta[rows] + hi[rows]) / 2.0)
            else:
                hi[rows] = beta[rows]
                beta[rows] = np.where(np.isinf(lo[rows]), beta[rows] / 2.0, (beta[rows] + lo[rows]) / 2.0)
        active = active[~stop]
    return dict(cond=p_out / S_out[:, None], beta=beta, steps=steps, S=S_out, trace=trace, fragile=fragile)


def symmetrize(cond):
    """P = (A + A.T) / (2N): one addition, one true division; zero diagonal"""
    N = cond.shape[0]
    P = (cond + cond.T) / (2.0 * N)
    np.fill_diagonal(P, 0.0)
    return P


def joint(x, perplexity):
    return symmetrize(search(distances(x), perplexity)["cond"])


def row_sums(P, Y, want_kl=True):
    """-> (rows [N,6], mag [N,6]): what acimg_tsne_gradient leaves, and the sums of the absolute values of the terms"""
    N = P.shape[0]
    dx = Y[:, None, 0] - Y[None, :, 0]
    dy = Y[:, None, 1] - Y[None, :, 1]
    w = 1.0 / (1.0 + (dx * dx + dy * dy))
    np.fill_diagonal(w, 0.0)
    rows, mag = np.zeros((N, 6)), np.zeros((N, 6))
    terms = [P * w * dx, P * w * dy, w * w * dx, w * w * dy, w]
    if want_kl:
        pos = P > 0.0
        wl = np.where(pos, w, 1.0)
        pl = np.where(pos, P, 1.0)
        terms.append(np.where(pos, P * (np.log(pl) - np.log(wl)), 0.0))
        # the magnitude of a KL term counts both logarithms: they are rounded before they are subtracted
        klmag = np.where(pos, P * (np.abs(np.log(pl)) + np.abs(np.log(wl))), 0.0)
    for c, t in enumerate(terms):
        rows[:, c] = t.sum(axis=1)
        mag[:, c] = np.abs(t).sum(axis=1)
    if want_kl:
        mag[:, 5] = klmag.sum(axis=1)
    return rows, mag


def gradient(rows, e):
    """g [N,2] and Z from the row sums"""
    Z = rows[:, 4].sum()
    return 4.0 * (e * rows[:, 0:2] - rows[:, 2:4] / Z), Z


def kl_of(rows):
    return rows[:, 5].sum() + np.log(rows[:, 4].sum())


def update(rows, e, momentum, learning_rate, Y, V, G):
    """one update from the row sums -> (Y, V, G, g, inc, fragile [N,2] bool)"""
    g, _ = gradient(rows, e)
    gv = g * V
    inc = gv < 0.0
    fragile = np.abs(gv) <= FRAGILE * np.abs(g) * np.abs(V)
    fragile &= V != 0.0                      # V == 0 (the first iteration): g * V is an exact zero in any arithmetic
    G = np.maximum(np.where(inc, G + 0.2, G * 0.8), 0.01)
    V = momentum * V - learning_rate * G * g
    return Y + V, V, G, g, inc, fragile


def schedule(t, early_exaggeration=12.0, exaggeration_iters=250):
    """(e, momentum) of iteration t"""
    return (early_exaggeration, 0.5) if t < exaggeration_iters else (1.0, 0.8)


def auto_learning_rate(N, early_exaggeration=12.0):
    return max(N / early_exaggeration / 4.0, 50.0)


def initial(N, seed=0):
    return 1e-4 * np.random.RandomState(seed).randn(N, 2)


def descend(P, Y0, n_iter, learning_rate, early_exaggeration=12.0, exaggeration_iters=250, kl_every=0):
    """-> (Y, V, G, [(t, KL_t)], fragile elements seen)"""
    Y, V, G = Y0.copy(), np.zeros_like(Y0), np.ones_like(Y0)
    trace, nfragile = [], 0
    for t in range(n_iter):
        want = bool(kl_every) and t % kl_every == 0
        rows, _ = row_sums(P, Y, want)
        if want:
            trace.append((t, kl_of(rows)))
        e, m = schedule(t, early_exaggeration, exaggeration_iters)
        Y, V, G, _, _, fr = update(rows, e, m, learning_rate, Y, V, G)
        nfragile += int(fr.sum())
    return Y, V, G, trace, nfragile


def kl_divergence(P, Y):
    return kl_of(row_sums(P, Y, True)[0])


def purity(Y, labels):
    """fraction of rows whose nearest neighbour in the map has their own label"""
    d = distances(Y)
    np.fill_diagonal(d, np.inf)
    return float(np.mean(labels[np.argmin(d, axis=1)] == labels))


def clusters(seed=0, k=3, per=50, D=16):
    """the end-to-end input: k Gaussian clusters, centres 10 * randn, unit noise -> (x [k*per, D], labels)"""
    rng = np.random.RandomState(seed)
    centres = 10.0 * rng.randn(k, D)
    labels = np.repeat(np.arange(k), per)
    return centres[labels] + rng.randn(k * per, D), labels


def affinity_input(N, D, seed):
    """the affinity tests' input: unit Gaussian rows scaled so that neighbour distances are of order 1"""
    return np.random.RandomState(seed).randn(N, D) / np.sqrt(D)


# (N, D, perplexity, seed) of the device affinity tests; the seeds are chosen so that no row is fragile
# (tests/test_tsne_cpu.py holds them to that)
AFFINITY_CASES = [(70, 5, 5.0, 0), (257, 33, 30.0, 0), (300, 150, 40.0, 0)]
# (N, D, perplexity, seed, learning rate) of the device descent tests: steps 0..5 with exaggeration_iters = 3
DESCENT_CASES = [(70, 5, 5.0, 0, 50.0), (257, 33, 30.0, 0, 50.0)]
DESCENT_EXAGGERATION_ITERS = 3
DESCENT_STEPS = 6
