"""Energy-map localisation metric, the step right after the generator in every evaluation script of the
reference: `find_logen` on the real and the generated acoustic image, mean-threshold masks,
IoU, hit if IoU > tau (iouenergythreshold.py:213-236); accuracy over tau in {0, .1, ..., 1} integrated with the
trapezoid rule (areaundercurve.py:26-40, sklearn.metrics.auc).  The per-sample work (2 x 1728 inverse-DCT +
exp pixels, two means, two mask counts) runs on the GPU; the 11-point curve is host arithmetic.

`BoxIoU` is the Flickr-SoundNet variant (showimages_bb.py:286-320): the generated image's mask, resized to the
224 x 298 frame, against the consensus map of up to three annotators' boxes (`acimg_box_iou`).

`OverlayRenderer` draws what those scripts plot (showvideo.py:213-233, showimages.py:136-154, showimages_bb.py:240-285):
the jet-coloured energy map at alpha 0.7 over the grey frame, as RGB8 pixels on the device (`acimg_overlay_render`).

`ClipEvaluator` is the classification experiment's pass over a data set (trainer_reconstructed_class.py:262-298,
saveimagesresnet.py): loss, accuracy and the confusion matrix of clip logits, accumulated on the device
(`acimg_clip_eval`) and read back once."""
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


class OverlayRenderer(object):
    """Owns the two colour tables (device, [256,3] uint8) and the blend weight alpha = (num, den).  `base` / `over`: a
    name of `acimg.colormaps` or a [256,3] uint8 table, used as given."""

    H, W = 224, 298

    def __init__(self, device, base="gray", over="jet", alpha=(7, 10)):
        self.device = torch.device(device)
        self.fe = FrontEnd(self.device)
        self.lut_base, self.lut_over = self._table(base), self._table(over)
        self.alpha = (int(alpha[0]), int(alpha[1]))
        if not (1 <= self.alpha[1] <= 255 and 0 <= self.alpha[0] <= self.alpha[1]):
            raise ValueError("alpha = num / den wants 0 <= num <= den, 1 <= den <= 255, got %r" % (alpha,))

    def _table(self, t):
        if isinstance(t, str):
            from . import colormaps
            t = colormaps.byte_table(t)
        t = torch.as_tensor(t)
        if t.dtype != torch.uint8 or tuple(t.shape) != (256, 3):
            raise ValueError("a colour table is [256,3] uint8, got %s %s" % (t.dtype, tuple(t.shape)))
        return t.to(self.device).contiguous()

    def energy(self, generated_or_logen):
        """[n,36,48,12] MFCC image (through `FrontEnd.find_logen`) or an energy map [n,36,48] / [n,1728] as it is"""
        x = generated_or_logen.to(device=self.device, dtype=torch.float32)
        if x.dim() == 4 and x.shape[-1] == 12:
            x = self.fe.find_logen(x)
        return x.reshape(x.shape[0], 36 * 48).contiguous()

    def _render_into(self, frames, logen, boxes, out, row_bytes, image_bytes):
        n = frames.shape[0]
        if tuple(frames.shape[:3]) != (n, self.H, self.W) or frames.dim() != 4 or frames.shape[3] < 3:
            raise ValueError("frames are [n,224,298,>=3], got %s" % (tuple(frames.shape),))
        if logen.shape[0] != n:
            raise ValueError("%d frames, %d energy maps" % (n, logen.shape[0]))
        b = None
        if boxes is not None:
            b = boxes.to(device=self.device, dtype=torch.int32).reshape(n, 4, 3).contiguous()
        ops.overlay_render(self.fe.plan, frames, frames.shape[3], logen, b, self.lut_base, self.lut_over, self.alpha[0],
                           self.alpha[1], out, row_bytes, image_bytes, n)

    def _frames(self, frames):
        return frames.to(device=self.device, dtype=torch.float32).contiguous()

    def render(self, frames, generated_or_logen, boxes=None, out=None):
        """frames: float32 [n,224,298,c >= 3] (the loaders' video tensor; the first three channels are read);
        generated_or_logen: see `energy`; boxes: int32 [n,4,3] or None -> uint8 [n,224,298,3] device tensor"""
        f = self._frames(frames)
        n = f.shape[0]
        if out is None:
            out = torch.empty(n, self.H, self.W, 3, dtype=torch.uint8, device=self.device)
        if out.dtype != torch.uint8 or tuple(out.shape) != (n, self.H, self.W, 3) or not out.is_contiguous():
            raise ValueError("out is a contiguous uint8 [n,224,298,3] tensor")
        self._render_into(f, self.energy(generated_or_logen), boxes, out, self.W * 3, self.H * self.W * 3)
        return out

    def render_pair(self, frames, real, generated, gap=8, fill=255, out=None):
        """the two panels of showimages.py:136-154 on one canvas uint8 [n,224,2*298+gap,3]: the real acoustic image's
        map on the left, the generated one's on the right (the order of `namesimage`); the gap columns keep the
        canvas's fill (`fill` for a canvas made here, whatever `out` holds otherwise)"""
        f = self._frames(frames)
        n, wide = f.shape[0], 2 * self.W + int(gap)
        if out is None:
            out = torch.full((n, self.H, wide, 3), int(fill), dtype=torch.uint8, device=self.device)
        if out.dtype != torch.uint8 or tuple(out.shape) != (n, self.H, wide, 3) or not out.is_contiguous():
            raise ValueError("out is a contiguous uint8 [n,224,%d,3] tensor" % wide)
        for energy, x0 in ((self.energy(real), 0), (self.energy(generated), self.W + int(gap))):
            self._render_into(f, energy, None, out[:, :, x0:], wide * 3, self.H * wide * 3)
        return out


class ClipEvaluator(object):
    """One evaluation pass: `reset()`, `update(...)` per batch (a kernel launch, nothing read back), `result()` (the
    pass's only synchronisation).  The state's layout is that of include/acimg.h."""

    HEAD = 32         # double loss_sum, int64 clips, correct, invalid

    def __init__(self, device, num_classes, nr_frames=12):
        from . import _lib
        self.device = torch.device(device)
        self.num_classes, self.nr_frames = int(num_classes), int(nr_frames)
        nbytes = int(_lib.load().acimg_clip_eval_state_bytes(self.num_classes))
        if nbytes != self.HEAD + 4 * self.num_classes ** 2:
            raise ValueError("clip evaluation wants 1..64 classes, got %d" % self.num_classes)
        self.state = torch.zeros(nbytes, dtype=torch.uint8, device=self.device)
        self.plan = ops.Plan(self.device, eager=True)

    def reset(self):
        self.state.zero_()
        return self

    def update(self, plan, logits, ldl, clips, labels, clip_loss=None, clip_pred=None):
        """logits [clips * nr_frames, ldl] float32 and labels [clips] int32 on the device.  plan: record the call there
        (it then runs with that plan, every time); None: launch now on the current stream."""
        ops.clip_eval(self.plan if plan is None else plan, logits, ldl, clips, self.nr_frames, self.num_classes, labels,
                      self.state, clip_loss, clip_pred)

    def result(self):
        """{loss (mean over the valid clips), accuracy (correct / clips, from the integer counts), clips, correct,
        invalid, loss_sum, confusion int64 [K, K] (row = label, column = prediction)}"""
        raw = self.state.cpu().numpy()
        K = self.num_classes
        loss_sum = float(raw[:8].view(np.float64)[0])
        clips, correct, invalid = (int(v) for v in raw[8:32].view(np.int64))
        confusion = raw[32:].view(np.int32).reshape(K, K).astype(np.int64)
        return dict(loss=loss_sum / clips if clips else float("nan"), accuracy=correct / clips if clips else float("nan"),
                    clips=clips, correct=correct, invalid=invalid, loss_sum=loss_sum, confusion=confusion)


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
