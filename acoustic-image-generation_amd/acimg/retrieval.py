"""Nearest-neighbour evaluation of the learned latent space: `python -m acimg.retrieval knn | retrieve | tsne`.

Stands where the reference's two scripts on the extracted feature dumps (`python -m acimg.features`) stand, with their
positional arguments and directory layout (`<checkpoint dir>/<set>_<encoder>_<n>/<set>_{data,labels}.npy`):
* `knn <init_checkpoint> <encoder_type> <set> [--k 15]`: knn.py.  The `<set>` dump is classified by a uniform-weight
  k-NN vote over the `training` dump (KNeighborsClassifier(n_neighbors=15), :102-104; ties to the smallest class).
  Writes `<checkpoint dir>/<set>_<encoder>_<n>_<set>_knn_value.txt` = 'Accuracy={} k={}\\n' (:105-113) and `knn.json`
  (predictions, per-class counts) in the `<set>` dump directory.
* `retrieve <init_checkpoint> <anchor> <gallery> <set> <datatype>`: retrieve.py.  Every anchor row ranks the gallery
  rows by Euclidean distance (cdist + argsort, :53-57).  Writes `<anchor dir>_<anchor>_<gallery>_<set>_retrieval.txt`
  with the rank-1/2/5/10/30 hit rates in the script's format (:152-160) and `retrieval.json` (the rank counts and the
  confusion matrices at 1 / 5 / 10 in the script's normalisation, :86-96) in the gallery dump directory.  A class with
  no anchors has a `null` row where the reference's division gives NaN.  There is no confusion-matrix PNG.
  The classes are 10 for outdoor, 9 for music and 14 otherwise.

* `tsne <init_checkpoint> <encoder_type> <set> [--perplexity 40 --n_iter 300 --seed 0 --learning_rate auto
  --max_points 16384]`: the map knn.py draws of the `<set>` dump (TSNE(n_components=2, random_state=0, perplexity=40,
  n_iter=300), :67-90), as exact t-SNE in fp64 on the device (`acimg_tsne_*`; class TSNE below).  A dump of more than
  `--max_points` rows is subsampled (seeded, without replacement, indices ascending): the dense P is 8 N^2 bytes.
  Writes `<set>_tsne.npy` (the map), `<set>_tsne_index.npy` (the rows used), `tsne.json` (parameters, N, learning rate,
  KL trace, final KL) and `<set>_tsne.png` (one disc per row, coloured by class with seaborn's `hls` palette; no class
  digits: the project draws no text) in the `<set>` dump directory.

Both searches are exact, in fp64, on the device (`acimg_knn_topk`, `acimg_knn_vote`): squared direct-difference
distances ordered by (distance, gallery index), so ties go to the lower index.

Two quirks of retrieve.py are handled explicitly:
* it indexes the ANCHOR label array with gallery indices (:61-82) and divides the rank counts by the GALLERY size
  (:152-156).  Both are right only when the two dumps come from the same records in the same order (two encoders of
  one set);
* so `retrieve` refuses (ValueError) two dumps whose label arrays differ.  When they are equal it reproduces the
  reference's numbers exactly.
"""
import argparse
import colorsys
import json
import os
import sys

import numpy as np
import torch

from . import _lib, ops, png

KNN_K = 15
RETRIEVAL_K = 30
RANKS = (1, 2, 5, 10, 30)
MAX_K = 64
MAX_CLASSES = 64
TSNE_PERPLEXITY = 40.0
TSNE_ITERS = 300
TSNE_EARLY_EXAGGERATION = 12.0
TSNE_EXAGGERATION_ITERS = 250
TSNE_MAX_POINTS = 16384
TSNE_CANVAS = 800
TSNE_MARGIN = 0.05
TSNE_RADIUS = 3


class NearestNeighbours(object):
    """Exact fp64 k-nearest-neighbour search on one device.  Feature arrays are [N, D] (or [N, ...], flattened),
    numpy or torch, host or device."""

    def __init__(self, device):
        self.device = torch.device(device)
        self.plan = ops.Plan(self.device, eager=True)

    def _rows(self, x):
        t = x if isinstance(x, torch.Tensor) else torch.from_numpy(np.asarray(x))
        t = t.reshape(t.shape[0], -1)
        return t.to(device=self.device, dtype=torch.float64).contiguous()

    def _labels(self, y, n, what):
        t = y if isinstance(y, torch.Tensor) else torch.from_numpy(np.asarray(y))
        t = t.reshape(-1)
        if t.numel() != n:
            raise ValueError("%s: %d labels for %d rows" % (what, t.numel(), n))
        if t.is_floating_point() and not bool((t == t.round()).all()):
            raise ValueError("%s: labels must be integers" % what)
        t = t.to(torch.int64)
        if n and (int(t.min()) < 0 or int(t.max()) >= MAX_CLASSES):
            raise ValueError("%s: labels must lie in [0, %d)" % (what, MAX_CLASSES))
        return t.to(device=self.device, dtype=torch.int32).contiguous()

    def kneighbors(self, query, gallery, k):
        """-> (dist2 float64 [Q,k], idx int32 [Q,k]) device tensors: squared Euclidean distances and gallery indices,
        ascending by (dist2, index); -1 / +inf in the slots past the gallery size"""
        q, g = self._rows(query), self._rows(gallery)
        k = int(k)
        if not 1 <= k <= MAX_K:
            raise ValueError("k = %d outside [1, %d]" % (k, MAX_K))
        if q.shape[1] != g.shape[1]:
            raise ValueError("feature widths differ: %d vs %d" % (q.shape[1], g.shape[1]))
        Q, G, D = q.shape[0], g.shape[0], q.shape[1]
        dist2 = torch.empty(Q, k, dtype=torch.float64, device=self.device)
        idx = torch.empty(Q, k, dtype=torch.int32, device=self.device)
        ops.knn_topk(self.plan, q, D, Q, g, D, G, D, k, dist2, idx)
        return dist2, idx

    def _vote(self, idx, gallery_labels, query_labels, want_pred, want_hit):
        Q, k = idx.shape
        ncls = int(max(int(gallery_labels.max()), int(query_labels.max()) if query_labels is not None else 0)) + 1
        pred = torch.empty(Q, dtype=torch.int32, device=self.device) if want_pred else None
        hit = torch.empty(Q, dtype=torch.int32, device=self.device) if want_hit else None
        ops.knn_vote(self.plan, idx, k, Q, k, gallery_labels, query_labels, ncls, pred, hit)
        return pred, hit

    def knn_predict(self, train, train_labels, test, k=KNN_K):
        """KNeighborsClassifier(n_neighbors=k).fit(train, train_labels).predict(test) with uniform weights: the most
        frequent label among the k nearest training rows, the smallest label on a tie -> int32 numpy [len(test)]"""
        tr = self._rows(train)
        if tr.shape[0] < int(k):
            raise ValueError("k = %d exceeds the %d training rows" % (int(k), tr.shape[0]))
        lab = self._labels(train_labels, tr.shape[0], "train_labels")
        _, idx = self.kneighbors(test, tr, k)
        pred, _ = self._vote(idx, lab, None, True, False)
        return pred.cpu().numpy()

    def first_hits(self, anchor, anchor_labels, gallery, gallery_labels, k=RETRIEVAL_K, return_neighbours=False):
        """1-based rank of the first of the k nearest gallery rows that shares the anchor's label, 0 if none ->
        int32 numpy [len(anchor)] (a rank-r hit of retrieve.py is 1 <= first_hit <= r); with return_neighbours also
        the int32 [len(anchor), k] neighbour indices"""
        a, g = self._rows(anchor), self._rows(gallery)
        al = self._labels(anchor_labels, a.shape[0], "anchor_labels")
        gl = self._labels(gallery_labels, g.shape[0], "gallery_labels")
        _, idx = self.kneighbors(a, g, k)
        _, hit = self._vote(idx, gl, al, False, True)
        hit = hit.cpu().numpy()
        return (hit, idx.cpu().numpy()) if return_neighbours else hit

class TSNE(object):
    """Exact two-component t-SNE in fp64 on one device (include/acimg.h, acimg_tsne_*): the affinities of a feature
    array, and a descent that can be stepped (`init`, `step`) or run whole (`fit_transform`).  The state `Y`, `V`, `G`
    ([N,2] device tensors), `iteration`, and `kl` (a [1] device tensor: the divergence at the Y the last iteration run
    with want_kl started from) is public."""

    def __init__(self, device):
        self.device = torch.device(device)
        self.plan = ops.Plan(self.device, eager=True)
        self.P = self.Y = self.V = self.G = self.rows = None
        self.kl = torch.zeros(1, dtype=torch.float64, device=self.device)
        self.iteration = 0

    def _rows(self, x, perplexity):
        t = x if isinstance(x, torch.Tensor) else torch.from_numpy(np.asarray(x))
        t = t.reshape(t.shape[0], -1).to(dtype=torch.float64)
        N = t.shape[0]
        if N < 4:
            raise ValueError("t-SNE needs at least 4 rows, got %d" % N)
        if not 1.0 < float(perplexity) < N - 1:
            raise ValueError("perplexity %g outside (1, N - 1 = %d)" % (perplexity, N - 1))
        if not bool(torch.isfinite(t).all()):
            raise ValueError("t-SNE input holds non-finite values")
        return t.to(self.device).contiguous()

    def conditional(self, x, perplexity):
        """-> (p_{j|i} float64 [N,N] with a zero diagonal, beta float64 [N], steps int32 [N]) device tensors: the rows
        before symmetrisation, the precision every row's search ended at, and its number of steps"""
        t = self._rows(x, perplexity)
        N, D = t.shape
        P = torch.empty(N, N, dtype=torch.float64, device=self.device)
        beta = torch.empty(N, dtype=torch.float64, device=self.device)
        steps = torch.empty(N, dtype=torch.int32, device=self.device)
        ops.tsne_affinities(self.plan, t, D, N, D, perplexity, P, N, beta, steps)
        return P, beta, steps

    def affinities(self, x, perplexity):
        """-> (P float64 [N,N]: the joint, symmetrised matrix (sums to 1), beta, steps)"""
        P, beta, steps = self.conditional(x, perplexity)
        ops.tsne_symmetrize(self.plan, P, P.shape[1], P.shape[0])
        return P, beta, steps

    def init(self, P, y0, learning_rate="auto", early_exaggeration=TSNE_EARLY_EXAGGERATION,
             exaggeration_iters=TSNE_EXAGGERATION_ITERS):
        """start a descent on the joint matrix P [N,N] from y0 [N,2]: V = 0, G = 1, iteration 0"""
        P = P if isinstance(P, torch.Tensor) else torch.from_numpy(np.asarray(P))
        if P.dim() != 2 or P.shape[0] != P.shape[1]:
            raise ValueError("P must be square, got %s" % (tuple(P.shape),))
        self.P = P.to(device=self.device, dtype=torch.float64).contiguous()
        N = self.P.shape[0]
        y0 = torch.from_numpy(np.ascontiguousarray(y0, dtype=np.float64)) if not isinstance(y0, torch.Tensor) else y0
        if tuple(y0.shape) != (N, 2):
            raise ValueError("y0 must be [%d, 2], got %s" % (N, tuple(y0.shape)))
        self.Y = y0.to(device=self.device, dtype=torch.float64).clone().contiguous()
        self.V = torch.zeros_like(self.Y)
        self.G = torch.ones_like(self.Y)
        self.rows = torch.zeros(N, 6, dtype=torch.float64, device=self.device)
        self.early_exaggeration = float(early_exaggeration)
        self.exaggeration_iters = int(exaggeration_iters)
        auto = isinstance(learning_rate, str) and learning_rate == "auto"
        self.learning_rate = auto_learning_rate(N, self.early_exaggeration) if auto else float(learning_rate)
        self.iteration = 0
        return self

    def _iterate(self, want_kl, kl):
        N = self.P.shape[0]
        early = self.iteration < self.exaggeration_iters
        ops.tsne_gradient(self.plan, self.P, self.P.shape[1], N, self.Y, want_kl, self.rows)
        ops.tsne_update(self.plan, self.rows, N, self.early_exaggeration if early else 1.0, 0.5 if early else 0.8,
                        self.learning_rate, self.Y, self.V, self.G, kl if want_kl else None)
        self.iteration += 1

    def step(self, n=1, want_kl=False):
        """n iterations (two launches each, enqueued without a host wait); with want_kl every one of them also leaves
        the divergence at the Y it started from in `kl`"""
        for _ in range(int(n)):
            self._iterate(want_kl, self.kl)
        return self

    def divergence(self, kl=None):
        """enqueue KL(P || Q) at the current Y into `kl` (default: self.kl); changes no state"""
        kl = self.kl if kl is None else kl
        N = self.P.shape[0]
        ops.tsne_gradient(self.plan, self.P, self.P.shape[1], N, self.Y, True, self.rows)
        ops.tsne_update(self.plan, self.rows, N, 1.0, 0.0, 1.0, None, None, None, kl)
        return kl

    def fit_transform(self, x, perplexity=TSNE_PERPLEXITY, n_iter=TSNE_ITERS, seed=0, learning_rate="auto", y0=None,
                      display=50):
        """-> (Y numpy float64 [N,2], [(iteration, KL)]): KL at the start of every `display`-th iteration and, last,
        (n_iter, KL of the returned map).  The whole run is enqueued; the trace is read back once at the end."""
        P, _, _ = self.affinities(x, perplexity)
        N = P.shape[0]
        if y0 is None:
            y0 = initial_map(N, seed)
        self.init(P, y0, learning_rate)
        n_iter, display = int(n_iter), int(display)
        shown = [t for t in range(n_iter) if display > 0 and t % display == 0]
        trace = torch.zeros(len(shown) + 1, dtype=torch.float64, device=self.device)
        for t in range(n_iter):
            want = display > 0 and t % display == 0
            self._iterate(want, ops.Ptr(trace, 2 * (t // display)) if want else None)
        self.divergence(ops.Ptr(trace, 2 * len(shown)))
        kl = trace.cpu().numpy()
        return self.Y.cpu().numpy(), [(int(t), float(v)) for t, v in zip(shown + [n_iter], kl)]


def auto_learning_rate(N, early_exaggeration=TSNE_EARLY_EXAGGERATION):
    """sklearn's current learning_rate="auto": max(N / early_exaggeration / 4, 50)"""
    return max(N / float(early_exaggeration) / 4.0, 50.0)


def initial_map(N, seed=0):
    """1e-4 * RandomState(seed).randn(N, 2), drawn on the host"""
    return 1e-4 * np.random.RandomState(int(seed)).randn(int(N), 2)


# ---- the scripts' paths ----------------------------------------------------------------------------------------------
def checkpoint_parts(init_checkpoint):
    """(checkpoint directory, checkpoint number): knn.py:26-30, retrieve.py:25-27"""
    s = init_checkpoint.split("/")[-1]
    return "/".join(init_checkpoint.split("/")[:-1]), (s.split("_")[1]).split(".ckpt")[0]


def dump_dir(init_checkpoint, dataset, encoder_type):
    path, n = checkpoint_parts(init_checkpoint)
    return "{}/{}_{}_{}".format(path, dataset, encoder_type, n)


def knn_value_file(init_checkpoint, encoder_type, dataset):
    return "{}_{}_knn_value.txt".format(dump_dir(init_checkpoint, dataset, encoder_type), dataset)


def retrieval_file(init_checkpoint, anchor, gallery, dataset):
    return "{}_{}_{}_{}_retrieval.txt".format(dump_dir(init_checkpoint, dataset, anchor), anchor, gallery, dataset)


def tsne_files(init_checkpoint, encoder_type, dataset):
    """(map .npy, index .npy, tsne.json, .png) in the `<set>` dump directory"""
    d = dump_dir(init_checkpoint, dataset, encoder_type)
    return ("{}/{}_tsne.npy".format(d, dataset), "{}/{}_tsne_index.npy".format(d, dataset), "{}/tsne.json".format(d),
            "{}/{}_tsne.png".format(d, dataset))


def load_dump(data_dir, dataset):
    """(features [N,-1] float64, one-hot labels as stored) of `<data_dir>/<dataset>_{data,labels}.npy`"""
    fd, fl = "{}/{}_data.npy".format(data_dir, dataset), "{}/{}_labels.npy".format(data_dir, dataset)
    for f in (fd, fl):
        if not os.path.isfile(f):
            raise FileNotFoundError("missing feature dump %s" % f)
    feats = np.load(fd)
    feats = np.reshape(feats, (feats.shape[0], -1)).astype(np.float64)
    labels = np.load(fl)
    if labels.shape[0] != feats.shape[0]:
        raise ValueError("%s: %d labels for %d feature rows" % (data_dir, labels.shape[0], feats.shape[0]))
    return feats, labels


def num_classes(datatype):
    """retrieve.py:43-48"""
    return 10 if datatype == "outdoor" else 9 if datatype == "music" else 14


# ---- the two tools ---------------------------------------------------------------------------------------------------
def knn_accuracy_line(pred, labels, k):
    counter = int(np.sum(np.asarray(pred) == np.asarray(labels)))
    return "Accuracy={} k={}\n".format(counter / float(len(labels)), k)


def run_knn(init_checkpoint, encoder_type, dataset, k=KNN_K, device="cuda:0", nn=None, log=print):
    """knn.py: returns the knn.json dict (+ 'file': the accuracy file)"""
    train_dir = dump_dir(init_checkpoint, "training", encoder_type)
    test_dir = dump_dir(init_checkpoint, dataset, encoder_type)
    ftr, ltr = load_dump(train_dir, "training")
    fte, lte = load_dump(test_dir, dataset)
    ltr, lte = np.argmax(ltr, axis=1), np.argmax(lte, axis=1)
    log(ltr.shape[0])
    log(lte.shape[0])
    nn = nn or NearestNeighbours(device)
    pred = nn.knn_predict(ftr, ltr, fte, k)
    line = knn_accuracy_line(pred, lte, k)
    log(line)
    out = knn_value_file(init_checkpoint, encoder_type, dataset)
    with open(out, "w") as f:
        f.write(line)
    ncls = int(max(ltr.max(), lte.max())) + 1
    res = dict(k=int(k), num_train=int(ltr.shape[0]), num_test=int(lte.shape[0]),
               accuracy=float(np.sum(pred == lte) / float(len(lte))), predictions=[int(v) for v in pred],
               labels=[int(v) for v in lte], test_per_class=np.bincount(lte, minlength=ncls).tolist(),
               correct_per_class=np.bincount(lte[pred == lte], minlength=ncls).tolist(),
               predicted_per_class=np.bincount(pred, minlength=ncls).tolist())
    with open(os.path.join(test_dir, "knn.json"), "w") as f:
        json.dump(res, f, indent=1)
    res["file"] = out
    return res


def retrieval_summary(first_hit, neighbours, labels, numcl):
    """retrieve.py:49-96, 152-156 from the first-hit ranks and the first 10 neighbours of every anchor (labels: the
    anchors' = the gallery's class indices)"""
    labels = np.asarray(labels)
    G = labels.shape[0]
    counts = {r: int(np.sum((first_hit >= 1) & (first_hit <= r))) for r in RANKS}
    cm1 = np.zeros([numcl, numcl], dtype=float)
    cm5 = np.zeros([numcl, numcl], dtype=float)
    cm10 = np.zeros([numcl, numcl], dtype=float)
    nsc = np.zeros([numcl], dtype=int)
    for a in range(labels.shape[0]):
        la, nb = labels[a], labels[neighbours[a, :10]]
        nsc[la] += 1
        cm1[la, nb[0]] += 1
        for b in range(5):
            cm5[la, nb[b]] += 1
        for b in range(10):
            cm10[la, nb[b]] += 1
    with np.errstate(invalid="ignore", divide="ignore"):
        cm1 = cm1 / nsc.reshape(-1, 1)
        cm5 = cm5 / nsc.reshape(-1, 1) / 5.0
        cm10 = cm10 / nsc.reshape(-1, 1) / 10.0
    rates = [1.0 * counts[r] / G for r in RANKS]

    def rows(m):
        return [None if nsc[i] == 0 else [float(v) for v in m[i]] for i in range(numcl)]
    return dict(rank_counts={str(r): counts[r] for r in RANKS}, rank_rates={str(r): v for r, v in zip(RANKS, rates)},
                num_samples_class=nsc.tolist(), confusion_matrix1=rows(cm1), confusion_matrix5=rows(cm5),
                confusion_matrix10=rows(cm10),
                text="Accuracy {:6f} rank2 {:6f} rank5 {:6f} rank10 {:6f} rank30 {:6f}".format(*rates))


def run_retrieve(init_checkpoint, anchor, gallery, dataset, datatype, device="cuda:0", nn=None, log=print):
    """retrieve.py: returns the retrieval.json dict (+ 'file': the rank file)"""
    adir = dump_dir(init_checkpoint, dataset, anchor)
    gdir = dump_dir(init_checkpoint, dataset, gallery)
    fa, la_raw = load_dump(adir, dataset)
    fg, lg_raw = load_dump(gdir, dataset)
    if la_raw.shape != lg_raw.shape or not np.array_equal(la_raw, lg_raw):
        raise ValueError("retrieve: the anchor (%s) and gallery (%s) label arrays differ; retrieve.py indexes the "
                         "anchor labels with gallery indices and divides by the gallery size, which is only right for "
                         "two dumps of the same records in the same order" % (adir, gdir))
    labels = np.argmax(la_raw, axis=1)
    numcl = num_classes(datatype)
    if labels.size and int(labels.max()) >= numcl:
        raise ValueError("retrieve: label %d outside the %d classes of datatype %r" % (labels.max(), numcl, datatype))
    if fg.shape[0] < 10:
        raise ValueError("retrieve: %d gallery rows; the confusion matrices read 10 neighbours" % fg.shape[0])
    log(fa.shape[0])
    log(fg.shape[0])
    nn = nn or NearestNeighbours(device)
    hit, idx = nn.first_hits(fa, labels, fg, labels, RETRIEVAL_K, return_neighbours=True)
    res = retrieval_summary(hit, idx, labels, numcl)
    log(res["text"])
    out = retrieval_file(init_checkpoint, anchor, gallery, dataset)
    with open(out, "w") as f:
        f.write(res["text"])
    res.update(num_anchors=int(fa.shape[0]), num_gallery=int(fg.shape[0]), num_classes=numcl, datatype=datatype,
               first_hit=[int(v) for v in hit])
    with open(os.path.join(gdir, "retrieval.json"), "w") as f:
        json.dump(res, f, indent=1)
    res["file"] = out
    return res


def hls_palette(n):
    """seaborn's color_palette("hls", n) (the palette of knn.py's commented plot) as uint8 [n,3]: hue i / n + 0.01,
    lightness 0.6, saturation 0.65"""
    return np.array([[int(round(255.0 * c)) for c in colorsys.hls_to_rgb((i / float(n) + 0.01) % 1.0, 0.6, 0.65)]
                     for i in range(n)], dtype=np.uint8).reshape(n, 3)


def scatter_pixels(Y, size=TSNE_CANVAS, margin=TSNE_MARGIN):
    """integer pixel centres [N,2] (column, row) of the map scaled uniformly into a size x size canvas with `margin`
    of it free on every side; the map's y axis points up"""
    Y = np.asarray(Y, np.float64)
    lo, hi = Y.min(axis=0), Y.max(axis=0)
    span = float(max(hi[0] - lo[0], hi[1] - lo[1]))
    scale = size * (1.0 - 2.0 * margin) / span if span > 0 else 0.0
    mid = 0.5 * (lo + hi)
    cx = 0.5 * size + (Y[:, 0] - mid[0]) * scale
    cy = 0.5 * size - (Y[:, 1] - mid[1]) * scale
    pix = np.stack([np.floor(cx), np.floor(cy)], axis=1).astype(np.int64)
    return np.clip(pix, 0, size - 1)


def rasterize_scatter(Y, classes, num_classes, size=TSNE_CANVAS, radius=TSNE_RADIUS, margin=TSNE_MARGIN):
    """white [size,size,3] uint8 canvas with one filled disc (pixels within `radius` of the centre) per row of Y in
    its class's palette colour, drawn in row order: later rows paint over earlier ones"""
    img = np.full((size, size, 3), 255, dtype=np.uint8)
    pal = hls_palette(num_classes)
    o = np.arange(-radius, radius + 1)
    disc = (o[:, None] ** 2 + o[None, :] ** 2) <= radius * radius
    for (px, py), c in zip(scatter_pixels(Y, size, margin), np.asarray(classes).reshape(-1)):
        y0, y1, x0, x1 = max(py - radius, 0), min(py + radius + 1, size), max(px - radius, 0), min(px + radius + 1, size)
        m = disc[y0 - (py - radius):y1 - (py - radius), x0 - (px - radius):x1 - (px - radius)]
        img[y0:y1, x0:x1][m] = pal[int(c)]
    return img


def tsne_subsample(n, max_points, seed):
    """the rows embedded: all of them, or a seeded sample of max_points without replacement, ascending"""
    if n <= max_points:
        return np.arange(n)
    return np.sort(np.random.RandomState(int(seed)).choice(n, int(max_points), replace=False))


def run_tsne(init_checkpoint, encoder_type, dataset, perplexity=TSNE_PERPLEXITY, n_iter=TSNE_ITERS, seed=0,
             learning_rate="auto", max_points=TSNE_MAX_POINTS, device="cuda:0", tsne=None, log=print):
    """knn.py:67-90: returns the tsne.json dict (+ 'files')"""
    test_dir = dump_dir(init_checkpoint, dataset, encoder_type)
    feats, labels = load_dump(test_dir, dataset)
    if int(max_points) < 4:
        raise ValueError("tsne: max_points = %d below 4" % int(max_points))
    index = tsne_subsample(feats.shape[0], int(max_points), seed)
    classes = np.argmax(labels, axis=1)[index]
    numcl = int(labels.shape[1])
    log(feats.shape[0])
    tsne = tsne or TSNE(device)
    Y, trace = tsne.fit_transform(feats[index], perplexity=perplexity, n_iter=n_iter, seed=seed,
                                  learning_rate=learning_rate)
    for t, v in trace:
        log("iteration {} KL {:.6f}".format(t, v))
    f_map, f_index, f_json, f_png = tsne_files(init_checkpoint, encoder_type, dataset)
    np.save(f_map, Y)
    np.save(f_index, index)
    png.write_png(f_png, rasterize_scatter(Y, classes, numcl))
    res = dict(perplexity=float(perplexity), n_iter=int(n_iter), seed=int(seed), max_points=int(max_points),
               early_exaggeration=TSNE_EARLY_EXAGGERATION, exaggeration_iters=TSNE_EXAGGERATION_ITERS,
               num_rows=int(feats.shape[0]), N=int(len(index)), num_classes=numcl,
               learning_rate=float(tsne.learning_rate), kl_trace=[[t, v] for t, v in trace], kl=trace[-1][1])
    with open(f_json, "w") as f:
        json.dump(res, f, indent=1)
    res["files"] = (f_map, f_index, f_json, f_png)
    return res


def build_parser():
    ap = argparse.ArgumentParser(prog="python -m acimg.retrieval", description=__doc__.split("\n")[0])
    sub = ap.add_subparsers(dest="tool", required=True)
    k = sub.add_parser("knn", help="knn.py: k-NN classification of a dump against the training dump")
    k.add_argument("init_checkpoint", type=str)
    k.add_argument("encoder_type", type=str)
    k.add_argument("set", type=str)
    k.add_argument("--k", type=int, default=KNN_K)
    k.add_argument("--device", type=str, default="cuda:0")
    r = sub.add_parser("retrieve", help="retrieve.py: rank-r retrieval of a gallery dump for every anchor")
    r.add_argument("init_checkpoint", type=str)
    r.add_argument("anchor", type=str)
    r.add_argument("gallery", type=str)
    r.add_argument("set", type=str)
    r.add_argument("datatype", type=str)
    r.add_argument("--device", type=str, default="cuda:0")
    t = sub.add_parser("tsne", help="knn.py: exact t-SNE map of a dump, with a PNG scatter coloured by class")
    t.add_argument("init_checkpoint", type=str)
    t.add_argument("encoder_type", type=str)
    t.add_argument("set", type=str)
    t.add_argument("--perplexity", type=float, default=TSNE_PERPLEXITY)
    t.add_argument("--n_iter", type=int, default=TSNE_ITERS)
    t.add_argument("--seed", type=int, default=0)
    t.add_argument("--learning_rate", type=str, default="auto")
    t.add_argument("--max_points", type=int, default=TSNE_MAX_POINTS)
    t.add_argument("--device", type=str, default="cuda:0")
    return ap


def main(argv=None):
    a = build_parser().parse_args(argv)
    _lib.load()
    if a.tool == "knn":
        run_knn(a.init_checkpoint, a.encoder_type, a.set, k=a.k, device=a.device)
    elif a.tool == "tsne":
        run_tsne(a.init_checkpoint, a.encoder_type, a.set, perplexity=a.perplexity, n_iter=a.n_iter, seed=a.seed,
                 learning_rate=a.learning_rate if a.learning_rate == "auto" else float(a.learning_rate),
                 max_points=a.max_points, device=a.device)
    else:
        run_retrieve(a.init_checkpoint, a.anchor, a.gallery, a.set, a.datatype, device=a.device)
    return 0


if __name__ == "__main__":
    sys.exit(main())
