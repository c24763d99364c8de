"""fp64 NumPy restatement of the clip evaluation (include/acimg.h: acimg_clip_eval): per clip the mean of the F frame
logits, softmax cross-entropy against the label, prediction = lowest index among exact ties at the maximum (tf.argmax);
over a data set the loss sum, the integer counters and the confusion matrix (row = label, column = prediction).  A label
outside [0, K) counts in `invalid` and in nothing else."""
import numpy as np


def clip_means(logits, clips, F):
    """logits [clips * F, K] -> [clips, K] float64"""
    x = np.asarray(logits, dtype=np.float64)
    return x.reshape(clips, F, x.shape[-1]).sum(axis=1) / F


def clip_eval(logits, labels, F, K):
    """-> dict(clip_loss [clips] (0 where the label is invalid), clip_pred [clips], loss_sum, clips, correct, invalid,
    confusion int64 [K, K])"""
    labels = np.asarray(labels, dtype=np.int64)
    clips = labels.shape[0]
    m = clip_means(np.asarray(logits)[:, :K], clips, F)
    mx = m.max(axis=1, keepdims=True)
    lse = np.log(np.exp(m - mx).sum(axis=1)) + mx[:, 0]
    pred = np.argmax(m == mx, axis=1).astype(np.int64)          # first True = lowest index among exact ties
    valid = (labels >= 0) & (labels < K)
    loss = np.zeros(clips, dtype=np.float64)
    confusion = np.zeros((K, K), dtype=np.int64)
    for n in range(clips):
        if valid[n]:
            loss[n] = lse[n] - m[n, labels[n]]
            confusion[labels[n], pred[n]] += 1
    return dict(clip_loss=loss, clip_pred=pred, loss_sum=float(loss.sum()), clips=int(valid.sum()),
                correct=int((valid & (pred == labels)).sum()), invalid=int((~valid).sum()), confusion=confusion)


def per_class_recall(confusion):
    """confusion[c][c] / row sum per class; None for a class with no clip"""
    c = np.asarray(confusion, dtype=np.int64)
    return [(float(c[k, k]) / float(c[k].sum()) if c[k].sum() else None) for k in range(c.shape[0])]


def fold(start, values):
    """the documented loss_sum: `values` (float32) added one by one, in order, onto the float64 `start`"""
    acc = np.float64(start)
    for v in np.asarray(values, dtype=np.float32):
        acc = acc + np.float64(v)
    return float(acc)
