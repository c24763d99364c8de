"""`Session`: what stands where the reference has a tf.Session — the device, its stream, the
parameter store and the kernel workspace shared by every model built in it — and the plumbing every
trainer shares: `Graph`, `scope_range`, `draw_noise`, `loss_dict`, `write_saver_bundle`."""
import os
from collections import OrderedDict

import numpy as np
import torch

from . import _lib, ops
from .params import ParamStore


class Session(object):
    def __init__(self, device=None):
        _lib.load()  # fail loudly, now, if the HIP extension is missing
        if device is None:
            if not torch.cuda.is_available():
                raise RuntimeError("acimg needs an MI355X (no CPU fallback exists for the hot path)")
            device = torch.device("cuda", torch.cuda.current_device())
        self.device = torch.device(device)
        self.store = ParamStore(self.device)
        self.ws = ops.Workspace(self.device)
        self._finalized = False

    def new_plan(self):
        return ops.Plan(self.device, eager=False, ws=self.ws)

    def zeros(self, *shape):
        return torch.zeros(*shape, dtype=torch.float32, device=self.device)

    def finalize(self):
        if not self._finalized:
            self.store.finalize()
            self._finalized = True

    def adam_step(self, lr, step, off=0, numel=None, grad_scale=1.0):
        """ONE Adam launch (TF-1 form, 1-based `step`) over `numel` floats at `off` of the flat trainable buffer and its
        gradient / moment twins, on the current stream; numel None: the whole buffer"""
        st = self.store
        o = 4 * off
        rc = _lib.load().acimg_adam_step(st.flat["train"].data_ptr() + o, st.grad.data_ptr() + o,
                                         st.adam_m.data_ptr() + o, st.adam_v.data_ptr() + o,
                                         st.train_numel() if numel is None else numel, ops.adam_lr_t(lr, step),
                                         0.9, 0.999, 1e-8, grad_scale, ops.current_stream_handle(self.device))
        _lib.check(rc, "adam_step")


class Graph(object):
    """Buffers + plans of a trainer for one batch size (the reference's graph has a dynamic batch dimension)."""


def scope_range(store, scope):
    """(offset, numel) of a scope's variables in the flat trainable buffer: one contiguous run"""
    rng = [(o, c) for n, o, c in store.train_ranges() if n.startswith(scope + "/")]
    return rng[0][0], rng[-1][0] + rng[-1][1] - rng[0][0]


def draw_noise(session, tensor, seed, offset):
    """fill `tensor` with N(0,1) on the device, from Philox counter `offset` on (the reference's tf.random_normal)"""
    rc = _lib.load().acimg_randn(tensor.data_ptr(), tensor.numel(), seed, offset,
                                 ops.current_stream_handle(session.device))
    _lib.check(rc, "randn")


def loss_dict(losses):
    """python floats of a trainer's loss buffer (blocks until the step that wrote it has run)"""
    v = losses[:5].tolist()
    return OrderedDict(mse=v[0], huber=v[1], latent=v[2], reg=v[3], loss=v[4])


def write_saver_bundle(store, path, global_step, saved, max_to_keep, slots_of=None, tf_shapes=None):
    """What `tf.train.Saver(max_to_keep=...).save(session, path)` leaves for a trainer whose variables live in `store`: the
    Saver-V2 bundle `path`.index + `path`.data-00000-of-00001 with every model variable under its TF name, the Adam
    slots `<var>/Adam`, `<var>/Adam_1` of the optimised variables, `beta1_power`, `beta2_power` and `global_step`; the
    oldest bundles beyond `max_to_keep` removed; and the directory's `checkpoint` state file.
    saved: the paths written so far, oldest first -> the new list.  slots_of(name) -> bool: the variables the optimiser
    holds slots for (None: every trainable variable of the store).  tf_shapes: {name: shape} of variables TensorFlow
    stores in another shape than the store does (their slots follow)."""
    from . import tfio
    tf_shapes = tf_shapes or {}

    def shaped(k, v):
        a = v.numpy()
        return a.reshape(tf_shapes[k]) if k in tf_shapes else a

    tensors = OrderedDict((k, shaped(k, v)) for k, v in store.state_dict().items())
    train = set(n for n in store.grad_dict() if slots_of is None or slots_of(n))
    for which, sfx in (("m", "/Adam"), ("v", "/Adam_1")):
        for k, v in store.slot_dict(which).items():
            if k in train:
                tensors[k + sfx] = shaped(k, v)
    t = max(int(global_step), 0)
    tensors["beta1_power"] = np.float32(0.9 ** (t + 1))     # TF-1 Adam: the powers start at beta and are
    tensors["beta2_power"] = np.float32(0.999 ** (t + 1))   # multiplied once per apply_gradients
    tensors["global_step"] = np.int64(t)
    tfio.write_checkpoint(path, tensors)
    saved = [p for p in saved if p != path] + [path]
    while len(saved) > max_to_keep:
        old = saved.pop(0)
        for f in (old + ".index", old + ".data-00000-of-00001"):
            if os.path.exists(f):
                os.remove(f)
    with open(os.path.join(os.path.dirname(path), "checkpoint"), "w") as f:   # tf.train.CheckpointState, text format
        f.write('model_checkpoint_path: "%s"\n' % os.path.basename(saved[-1]))
        for p in saved:
            f.write('all_model_checkpoint_paths: "%s"\n' % os.path.basename(p))
    return saved


_default = None


def get_default_session():
    global _default
    if _default is None:
        _default = Session()
    return _default


def set_default_session(s):
    global _default
    _default = s
