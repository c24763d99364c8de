"""NumPy restatement of the latent-space evaluation (knn.py, retrieve.py) that the device kernels are tested against:
fp64 direct-difference squared distances, the stable (distance, index) neighbour order, the uniform k-NN vote (smallest
class on a tie), the first-hit ranks and retrieve.py's rank rates and confusion matrices."""
import numpy as np


def dist2(query, gallery):
    """[Q,G] sum_d (q - g)^2 in fp64, direct-difference form (row by row: no [Q,G,D] temporary)"""
    q = np.asarray(query, np.float64).reshape(len(query), -1)
    g = np.asarray(gallery, np.float64).reshape(len(gallery), -1)
    out = np.empty((q.shape[0], g.shape[0]), np.float64)
    for i in range(q.shape[0]):
        d = q[i][None, :] - g
        out[i] = np.einsum("gd,gd->g", d, d)
    return out


def kneighbors(query, gallery, k):
    """(dist2 [Q,k], idx [Q,k]) ascending by (dist2, index); slots past the gallery: +inf / -1"""
    d = dist2(query, gallery)
    order = np.argsort(d, axis=1, kind="stable")[:, :k]
    dd = np.take_along_axis(d, order, 1)
    Q, G = d.shape
    if k > G:
        dd = np.concatenate([dd, np.full((Q, k - G), np.inf)], 1)
        order = np.concatenate([order, np.full((Q, k - G), -1)], 1)
    return dd, order.astype(np.int32)


def vote(idx, gallery_labels, num_classes):
    """most frequent label among the neighbours, the smallest class on a tie; -1 entries skipped"""
    gl = np.asarray(gallery_labels)
    pred = np.zeros(len(idx), np.int32)
    for q, row in enumerate(np.asarray(idx)):
        lab = gl[row[row >= 0]]
        pred[q] = int(np.argmax(np.bincount(lab, minlength=num_classes)))
    return pred


def first_hit(idx, gallery_labels, query_labels):
    """1-based rank of the first neighbour with the query's label, 0 if none"""
    gl, ql = np.asarray(gallery_labels), np.asarray(query_labels)
    out = np.zeros(len(idx), np.int32)
    for q, row in enumerate(np.asarray(idx)):
        hits = [j for j, g in enumerate(row) if g >= 0 and gl[g] == ql[q]]
        out[q] = hits[0] + 1 if hits else 0
    return out


def knn_line(pred, labels, k):
    """knn.py:105-113"""
    counter = sum(1 for p, y in zip(pred, labels) if p == y)
    return "Accuracy={} k={}\n".format(counter / float(len(labels)), k)


def retrieval(features, features1, labels, numcl):
    """retrieve.py:49-96, 152-158 with the stable order: (text, rank counts {r: n}, cm1, cm5, cm10 with NaN rows)"""
    d = dist2(features, features1)
    G = d.shape[1]
    index = np.argsort(d, axis=1, kind="stable")
    labels = np.asarray(labels)
    ranks = {1: 0, 2: 0, 5: 0, 10: 0, 30: 0}
    cm1, cm5, cm10 = (np.zeros([numcl, numcl]) for _ in range(3))
    nsc = np.zeros([numcl], int)
    for a in range(d.shape[0]):
        nb = labels[index[a]]
        for r in ranks:
            if labels[a] in nb[:r]:
                ranks[r] += 1
        nsc[labels[a]] += 1
        cm1[labels[a], nb[0]] += 1
        for b in range(5):
            cm5[labels[a], nb[b]] += 1
        for b in range(10):
            cm10[labels[a], nb[b]] += 1
    with np.errstate(invalid="ignore", divide="ignore"):
        cm1 = cm1 / nsc.reshape(-1, 1)
        cm5 = cm5 / nsc.reshape(-1, 1) / 5.0
        cm10 = cm10 / nsc.reshape(-1, 1) / 10.0
    rates = [1.0 * ranks[r] / G for r in (1, 2, 5, 10, 30)]
    text = "Accuracy {:6f} rank2 {:6f} rank5 {:6f} rank10 {:6f} rank30 {:6f}".format(*rates)
    return text, ranks, cm1, cm5, cm10


def int_features(rng, Q, G, D):
    """integer-valued queries and gallery (every distance exact in any order) with duplicated rows and zero distances"""
    q = rng.randint(-8, 9, size=(Q, D)).astype(np.float64)
    g = rng.randint(-8, 9, size=(G, D)).astype(np.float64)
    if G > 1:
        dup = rng.randint(0, G, size=(G // 3, 2))     # duplicated gallery rows: exact ties broken by index
        g[dup[:, 0]] = g[dup[:, 1]]
    if G > 2 and Q > 0:
        g[-1] = q[0]                                  # a zero distance
        g[G // 2] = q[0]
    return q, g
