"""Energy-map localisation metric, the step right after the generator in every evaluation script of the
reference: `find_logen` on the real and the generated acoustic image, mean-threshold masks,
IoU, hit if IoU > tau (iouenergythreshold.py:213-236); accuracy over tau in {0, .1, ..., 1} integrated with the
trapezoid rule (areaundercurve.py:26-40, sklearn.metrics.auc).  The per-sample work (2 x 1728 inverse-DCT +
exp pixels, two means, two mask counts) runs on the GPU; the 11-point curve is host arithmetic.

`BoxIoU` is the Flickr-SoundNet variant (showimages_bb.py:286-320): the generated image's mask, resized to the
224 x 298 frame, against the consensus map of up to three annotators' boxes (`acimg_box_iou`)."""
import numpy as np
import torch

from . import ops
from .frontend import FrontEnd

THRESHOLDS = [0.0, 0.1, 0.2, 0.3, 0.4, 0.5, 0.6, 0.7, 0.8, 0.9, 1.0]


class EnergyIoU(object):
    def __init__(self, device):
        self.device = torch.device(device)
        self.fe = FrontEnd(self.device)

    def iou(self, real, generated):
        """real, generated: float32 [N,36,48,12] device tensors -> IoU per sample [N] (device)"""
        N = real.shape[0]
        P = real.shape[1] * real.shape[2]
        a = self.fe.find_logen(real)
        b = self.fe.find_logen(generated)
        out = torch.empty(N, dtype=torch.float32, device=self.device)
        ops.mask_iou(self.fe.plan, a, b, N, P, out)
        return out


class BoxIoU(object):
    def __init__(self, device):
        self.device = torch.device(device)
        self.fe = FrontEnd(self.device)

    def iou(self, generated, boxes, counts=None, mask_out=None):
        """generated: float32 [N,36,48,12] device tensor; boxes: int32 [N,4,3] (xmin, xmax, ymin, ymax rows; host or
        device) -> IoU per sample [N] float32 (device; NaN where mask and boxes are both empty).  counts: optional
        int32 [N,2] device tensor receiving numerator / denominator in half-units; mask_out: optional uint8
        [N,224,298] device tensor receiving the resized mask."""
        N = generated.shape[0]
        logen = self.fe.find_logen(generated)
        b = boxes.to(device=self.device, dtype=torch.int32).reshape(N, 4, 3).contiguous()
        out = torch.empty(N, dtype=torch.float32, device=self.device)
        ops.box_iou(self.fe.plan, logen, b, N, out, counts, mask_out)
        return out

    def iou64(self, generated, boxes):
        """the same IoU as float64 host values num / den from the exact half-unit counts (the reference's own float64
        ratio, so `> tau` decides as it does even where float32 would round across tau)"""
        N = generated.shape[0]
        counts = torch.empty(N, 2, dtype=torch.int32, device=self.device)
        self.iou(generated, boxes, counts=counts)
        c = counts.cpu().numpy().astype(np.float64)
        with np.errstate(invalid="ignore", divide="ignore"):
            return c[:, 0] / c[:, 1]


def mean_iou(ious):
    """(mean over the finite IoUs, number of NaN IoUs): a NaN (empty mask and no box) is a miss at every tau in
    `accuracy_curve`; it is reported here, not averaged in or dropped silently"""
    v = np.asarray(ious, dtype=np.float64)
    nan = np.isnan(v)
    return (float(np.mean(v[~nan])) if (~nan).any() else float("nan")), int(nan.sum())


def accuracy_curve(ious, thresholds=THRESHOLDS):
    """fraction of samples with IoU > tau, per tau (iouenergythreshold.py:226-236)"""
    v = np.asarray(ious, dtype=np.float64)
    return np.array([float(np.mean(v > t)) for t in thresholds])


def area_under_curve(acc, thresholds=THRESHOLDS):
    """sklearn.metrics.auc on the reversed lists, as areaundercurve.py:36-40 calls it = trapezoid rule"""
    x = np.asarray(thresholds, dtype=np.float64)[::-1]
    y = np.asarray(acc, dtype=np.float64)[::-1]
    return float(abs(np.sum((x[1:] - x[:-1]) * (y[1:] + y[:-1]) * 0.5)))
