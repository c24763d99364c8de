"""Time of the latent-space retrieval on one GPU against the host path of retrieve.py.

Device: `acimg_knn_topk` (K nearest gallery rows, fp64) + `acimg_knn_vote` (first-hit ranks), timed together with CUDA
events over --steps calls after --warmup, for Q = G rows of D random fp64 features.  Host: what retrieve.py does per
anchor, `scipy.spatial.distance.cdist` + `np.argsort` over the whole gallery, timed on --host-anchors anchors and
extrapolated linearly to Q (the per-anchor work does not depend on the anchor).  The host anchors' first K indices
are compared with the device's (random features: no ties).  Prints one JSON line per (Q, D).

    python tools/bench_retrieval.py --sizes 20000 100000 --dims 150 1024 --k 30
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[20000, 100000])
    ap.add_argument("--dims", type=int, nargs="+", default=[150, 1024])
    ap.add_argument("--k", type=int, default=30)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--host-anchors", type=int, default=20)
    a = ap.parse_args()
    from scipy.spatial import distance

    from acimg import ops

    dev = torch.device("cuda:0")
    plan = ops.Plan(dev, eager=True)
    g = torch.Generator(device=dev).manual_seed(0)
    for n in a.sizes:
        for D in a.dims:
            q = torch.randn(n, D, generator=g, device=dev, dtype=torch.float64)
            gal = torch.randn(n, D, generator=g, device=dev, dtype=torch.float64)
            ql = torch.randint(0, 10, (n,), generator=g, device=dev, dtype=torch.int32)
            dist2 = torch.empty(n, a.k, dtype=torch.float64, device=dev)
            idx = torch.empty(n, a.k, dtype=torch.int32, device=dev)
            hit = torch.empty(n, dtype=torch.int32, device=dev)
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
            times = []
            for i in range(a.warmup + a.steps):
                ev[0].record()
                ops.knn_topk(plan, q, D, n, gal, D, n, D, a.k, dist2, idx)
                ops.knn_vote(plan, idx, a.k, n, a.k, ql, ql, 10, None, hit)
                ev[1].record()
                torch.cuda.synchronize(dev)
                if i >= a.warmup:
                    times.append(ev[0].elapsed_time(ev[1]))
            gal_h = gal.cpu().numpy()
            q_h = q[:a.host_anchors].cpu().numpy()
            got = idx[:a.host_anchors].cpu().numpy()
            t0 = time.perf_counter()
            same = 0
            for i in range(a.host_anchors):
                dd = distance.cdist(q_h[i:i + 1], gal_h, "euclidean")
                order = np.squeeze(np.argsort(dd))
                same += int(np.array_equal(order[:a.k], got[i]))
            host_s = (time.perf_counter() - t0) / a.host_anchors * n
            dev_ms = float(np.median(times))
            print(json.dumps(dict(Q=n, G=n, D=D, K=a.k, device_ms=dev_ms, device_ms_all=times,
                                  host_s_extrapolated=host_s, host_anchors=a.host_anchors,
                                  host_anchors_matching=same, speedup=host_s * 1e3 / dev_ms,
                                  fp64_pair_rate_tflops=3.0 * n * n * D / (dev_ms * 1e-3) / 1e12)), flush=True)
            del q, gal, dist2, idx, gal_h


if __name__ == "__main__":
    main()
