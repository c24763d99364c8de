"""Nearest-neighbour evaluation of the learned latent space: `python -m acimg.retrieval knn | retrieve`.

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
import json
import os
import sys

import numpy as np
import torch

from . import _lib, ops

KNN_K = 15
RETRIEVAL_K = 30
RANKS = (1, 2, 5, 10, 30)
MAX_K = 64
MAX_CLASSES = 64


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
    return ap


def main(argv=None):
    a = build_parser().parse_args(argv)
    _lib.load()
    if a.tool == "knn":
        run_knn(a.init_checkpoint, a.encoder_type, a.set, k=a.k, device=a.device)
    else:
        run_retrieve(a.init_checkpoint, a.anchor, a.gallery, a.set, a.datatype, device=a.device)
    return 0


if __name__ == "__main__":
    sys.exit(main())
