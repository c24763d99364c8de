"""Time of the exact t-SNE on one GPU: the affinities (acimg_tsne_affinities + acimg_tsne_symmetrize) and one iteration
of the descent (acimg_tsne_gradient + acimg_tsne_update) with and without the divergence, for N rows of D random fp64
features.  An iteration reads the dense P once, so its time stands next to the HBM bound of 8 N^2 bytes at --hbm-tbs.
Timed with CUDA events over --steps repetitions after --warmup; one JSON line per N.

With --sklearn N (and scikit-learn importable) one `TSNE(method="exact")` fit of N rows on the host stands beside it
as the CPU baseline (300 iterations, affinities included; not a test).

    python tools/bench_tsne.py --sizes 2048 8192 16384 --dim 150
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "acoustic-image-generation_amd"))

import numpy as np  # noqa: E402
import torch  # noqa: E402


def timed(dev, fn, warmup, steps):
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    out = []
    for i in range(warmup + steps):
        ev[0].record()
        fn()
        ev[1].record()
        torch.cuda.synchronize(dev)
        if i >= warmup:
            out.append(ev[0].elapsed_time(ev[1]))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[2048, 8192, 16384])
    ap.add_argument("--dim", type=int, default=150)
    ap.add_argument("--perplexity", type=float, default=40.0)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--iters", type=int, default=20, help="iterations per timed repetition of the descent")
    ap.add_argument("--hbm-tbs", type=float, default=8.0, help="HBM bandwidth the bound is stated at, TB/s")
    ap.add_argument("--sklearn", type=int, default=0, help="rows of the host baseline (0: none)")
    a = ap.parse_args()

    from acimg import retrieval

    dev = torch.device("cuda:0")
    for n in a.sizes:
        x = torch.from_numpy(np.random.RandomState(0).randn(n, a.dim)).to(dev)
        t = retrieval.TSNE(dev)
        aff = timed(dev, lambda: t.affinities(x, a.perplexity), a.warmup, a.steps)
        P, beta, steps = t.affinities(x, a.perplexity)
        t.init(P, retrieval.initial_map(n))
        t.step(250)                                # past the start, where every w is 1 to eight digits
        plain = timed(dev, lambda: t.step(a.iters), a.warmup, a.steps)
        with_kl = timed(dev, lambda: t.step(a.iters, want_kl=True), a.warmup, a.steps)
        bound_ms = 8.0 * n * n / (a.hbm_tbs * 1e12) * 1e3
        it_ms, kl_ms = float(np.median(plain)) / a.iters, float(np.median(with_kl)) / a.iters
        print(json.dumps(dict(N=n, D=a.dim, perplexity=a.perplexity, affinities_ms=float(np.median(aff)),
                              affinities_ms_all=aff, search_steps_mean=float(steps.double().mean()),
                              search_steps_max=int(steps.max()), iteration_ms=it_ms, iteration_kl_ms=kl_ms,
                              iteration_ms_all=[v / a.iters for v in plain],
                              iteration_kl_ms_all=[v / a.iters for v in with_kl], p_bytes=8 * n * n,
                              hbm_bound_ms=bound_ms, hbm_tbs=a.hbm_tbs, fraction_of_hbm_bound=bound_ms / it_ms,
                              kl=float(t.divergence().cpu()[0]))), flush=True)
        del t, P, x
        torch.cuda.empty_cache()
    if a.sklearn:
        try:
            from sklearn.manifold import TSNE
        except ImportError:
            print(json.dumps(dict(sklearn=None, note="scikit-learn is not importable here")), flush=True)
            return
        x = np.random.RandomState(0).randn(a.sklearn, a.dim)
        kw = dict(n_components=2, random_state=0, perplexity=a.perplexity, method="exact")
        try:
            est = TSNE(max_iter=300, **kw)
        except TypeError:                          # before scikit-learn 1.5 the argument was n_iter
            est = TSNE(n_iter=300, **kw)
        t0 = time.perf_counter()
        est.fit_transform(x)
        s = time.perf_counter() - t0
        print(json.dumps(dict(sklearn_exact_s=s, sklearn_ms_per_iteration=s * 1e3 / 300, iterations=300, N=a.sklearn,
                              D=a.dim, threads=os.environ.get("OMP_NUM_THREADS"))), flush=True)


if __name__ == "__main__":
    main()
