"""What every model of the package shares on the host side: `Act` (an NHWC activation inside a wider buffer), `Model`
(parameter access, scoped state loading, scratch images, gradient buffers) and `ConvModel` (the rule that puts a conv on
the split-MFMA kernels, and the recorder of the bias + ReLU U-Nets' convs and their gradients).  A selection rule is
written once, here; where two models differ, the difference is a named class attribute with its reason.
"""
import os

import numpy as np
import torch

from . import ops
from .ops import ACT_NONE, ACT_RELU, Ptr
from .params import up4
from .session import get_default_session


class Act(object):
    """An NHWC activation: logical channels C inside a buffer with pixel stride ld at channel offset."""

    def __init__(self, t, N, H, W, C, ld=None, off=0):
        self.t, self.N, self.H, self.W, self.C = t, N, H, W, C
        self.ld = up4(C) if ld is None else ld
        self.off = off

    @property
    def ptr(self):
        return Ptr(self.t, self.off)

    @property
    def Cp(self):
        return up4(self.C)

    @property
    def pixels(self):
        return self.N * self.H * self.W


def ptr_ld(a):
    """(pointer, pixel stride) arguments of an optional activation (residual, ReLU mask)"""
    return (a.ptr, a.ld) if a is not None else (None, 0)


def xavier(generator, shape, fan_in, fan_out):
    """xavier_initializer() / Glorot uniform, drawn in fp64"""
    lim = np.sqrt(6.0 / (fan_in + fan_out))
    return ((torch.rand(*shape, generator=generator, dtype=torch.float64) * 2 - 1) * lim).float()


def flat_ptr(store, group, off=0, numel=None):
    """a run of a flat parameter buffer (resolved once the buffers exist)"""
    return ops.LazyPtr(lambda: _run(store.flat[group], off, numel))


def grad_ptr(store, off, numel):
    """the same run of the flat gradient buffer"""
    return ops.LazyPtr(lambda: _run(store.grad, off, numel))


def _run(buf, off, numel):
    return buf if numel is None else buf[off:off + numel]


def load_state_file(f):
    """{TF variable name: array}: a dict, a TensorFlow checkpoint prefix, an .npz, or a torch-saved dict (possibly
    under 'model')."""
    if isinstance(f, dict):
        return f.get("model", f)
    if os.path.exists(str(f) + ".index"):
        # a TensorFlow Saver-V2 bundle prefix (the reference's own checkpoints: trainer/mfcctrainer.py:214-247)
        from . import tfio
        return tfio.read_checkpoint(str(f))
    if str(f).endswith(".npz"):
        return dict(np.load(f))
    obj = torch.load(f, map_location="cpu", weights_only=False)
    return obj.get("model", obj) if isinstance(obj, dict) else obj


class Model(object):
    """`scope` names the model's variables in the session's parameter store; `_register(store)` adds them."""
    scope = None
    session = None
    _original = None         # of a replica: the instance whose variables it shares

    def _attach(self, session):
        """first step of every `_build_model`: join the session, register the variables (a replica: adopt them)"""
        self.session = session or get_default_session()
        if self._original is None:
            self._register(self.session.store)
        else:
            self._adopt(self._original)
        return self.session

    def replica(self):
        """a second instance over the SAME variables, not yet built: another batch size (the last, partial batch) gets
        new buffers and plans from it.  Its constructor arguments are the model's own record of them (`clone_kwargs`), so
        it records the same kernel path as the original."""
        m = type(self)(**self.clone_kwargs())
        m._original = self
        return m

    def _adopt(self, original):
        """a replica takes over what `_register` created besides the store's variables (default: nothing)"""

    # weight / grad pointers (resolved once the flat buffers exist)
    def _P(self, name):
        st = self.session.store
        return ops.LazyPtr(lambda: st.p(self.scope + "/" + name))

    def _G(self, name):
        st = self.session.store
        return ops.LazyPtr(lambda: st.g(self.scope + "/" + name))

    def _load_scope(self, state, session=None):
        """load the scope's variables from a TF-named state (what every `initialize` ends with)"""
        store = (session or self.session).store
        return store.load_state(state, strict=False, only=lambda n: n.startswith(self.scope + "/"))

    def init_model(self, session, checkpoint_file):
        """Initialise every variable of the scope from a TF-named state (models/unet_acresnet.py:33-41)."""
        return self._load_scope(load_state_file(checkpoint_file), session)

    def _scope_vars(self, skip=()):
        """TF names of the scope's variables, minus those ending in one of `skip`"""
        return [n for n in self.session.store.tf_names() if n.startswith(self.scope + "/") and not n.endswith(skip)]

    def _wsplit(self, name, nbytes, kind):
        """the device image of layer `name`'s re-split kernel (kind: fwd | dgrad), allocated once"""
        bufs = self.__dict__.setdefault("_wsplit_bufs", {})
        key = (name, kind)
        if key not in bufs:
            bufs[key] = torch.zeros(int(nbytes), dtype=torch.uint8, device=self.session.device)
        return bufs[key]

    def _gbuf(self, a):
        """a gradient buffer for activation `a` (dense, channels padded to 4)"""
        return Act(self.session.zeros(a.N, a.H, a.W, up4(a.C)), a.N, a.H, a.W, a.C)


class ConvModel(Model):
    """Models whose 3x3 convs may run on the split-MFMA kernels.  `_use_split` and `_dgrad` serve every such model;
    `_conv` / `_conv_back` record one bias + ReLU conv layer (UNetAc, UNetAcNoConc: no batch norm)."""
    precision = "split"
    split_min_rows = 16384      # below this the f32 kernel (64x64 tiles + split-K) fills the chip better
    SPLIT_PRECISIONS = ("split",)    # precisions that put a layer on the split kernels (the conv-BN U-Nets add "bf16")
    # weight gradient on the bf16x3 kernel: True = only where the forward runs split (`_use_split`), False = wherever
    # precision is split, so the 12x16 layers that run f32 forward take it too (measured for UNetAc in round 3)
    WGRAD_SPLIT_NEEDS_ROWS = True
    # the kernels change every step and their split images are rebuilt: `_prep_jobs` None = one small launch in front of each
    # consumer; a PrepareJobs = ONE prepare_multi launch at the head of the forward plan does them all
    _prep_jobs = None
    PREP_JOBS_CAP = None             # jobs one batched launch takes before further ones are launched in place (None: all)
    side_lane = False                # weight gradients beside the data gradients, on the plan's second stream

    def _desc(self, x, K, stride=1, y=None, act=ACT_NONE, R=3, S=3, padding="SAME"):
        return ops.conv_desc(x.N, x.H, x.W, x.Cp if x.off == 0 and x.ld == x.Cp else x.C, K, R, S, stride, padding,
                             ldx=x.ld, ldy=(y.ld if y is not None else up4(K)), ldw=up4(K), act=act)

    def _use_split(self, d):
        """big stride-1 convs run on the split-MFMA kernels (forward f16x3, data gradient bf16x3); the 12x16 layers of the
        generators (48 row tiles: they need split-K) and the 12/133-channel layers stay f32"""
        return (self.precision in self.SPLIT_PRECISIONS and d.stride == 1 and d.C % 32 == 0 and d.K % 32 == 0 and
                d.N * d.OH * d.OW >= self.split_min_rows)

    def _prepare_job(self, plan, d, name, image, mode, jobs):
        """rebuild `image` from layer `name`'s kernel every step: mode 0 forward / 1 data gradient / 2 bf16 forward;
        a job of `jobs`' one launch, or - no batched launch, or it is full - a launch in place"""
        if jobs is None or (self.PREP_JOBS_CAP is not None and len(jobs.jobs) >= self.PREP_JOBS_CAP):
            if mode == 1:
                ops.conv2d_split3_prepare_dgrad(plan, d, self._P(name + "/kernel"), image)
            else:
                ops.conv2d_split3_prepare(plan, d, self._P(name + "/kernel"), image, bf16=mode == 2)
            return
        jobs.add(d, self._P(name + "/kernel"), image, mode)

    def _dgrad(self, plan, d, name, gy, dx, mask=None, res=None, jobs=None, bf16=False):
        """data gradient of conv `name` into dx (+ res, masked by the ReLU of `mask`): on the flipped / transposed split image
        where the forward runs split, else exact f32"""
        if self._use_split(d):
            wt = self._wsplit(name, ops.conv2d_split3_dgrad_weight_bytes(d), "dgrad")
            self._prepare_job(plan, d, name, wt, 1, jobs)
            ops.conv2d_dgrad_split3(plan, d, gy.ptr, gy.ld, wt, dx.ptr, *ptr_ld(res), *ptr_ld(mask), lddx=dx.ld, bf16=bf16)
        else:
            ops.conv2d_dgrad(plan, d, gy.ptr, gy.ld, self._P(name + "/kernel"), dx.ptr, *ptr_ld(res), *ptr_ld(mask),
                             lddx=dx.ld)

    def _conv(self, plan, name, x, y, stride=1, act=ACT_RELU):
        d = self._desc(x, y.C, stride, y, act)
        self._descs[name] = (d, x, y)
        if self._use_split(d):
            ws = self._wsplit(name, ops.conv2d_split3_weight_bytes(d), "fwd")
            self._prepare_job(plan, d, name, ws, 0, self._prep_jobs)
            ops.conv2d_fwd_split3(plan, d, x.ptr, ws, y.ptr, bias=self._P(name + "/bias"))
        else:
            ops.conv2d_fwd(plan, d, x.ptr, self._P(name + "/kernel"), self._P(name + "/bias"), y.ptr)

    def _conv_back(self, plan, name, gy, dx=None, mask=None, res=None, on_ready=None):
        """weight / bias gradient of conv `name`, and its data gradient into dx (if given); on_ready(name) is called once
        both are recorded"""
        d, x, y = self._descs[name]
        split = self._use_split(d) if self.WGRAD_SPLIT_NEEDS_ROWS else self.precision in self.SPLIT_PRECISIONS
        wg = ops.conv2d_wgrad_split3 if (split and d.K % 64 == 0) else ops.conv2d_wgrad
        # with a side lane the weight gradients run there (a second stream, in layer order) beside the chain of data
        # gradients on the main stream: a weight gradient only needs its layer's gy (fork = the side lane waits for it),
        # every gradient buffer is written once, before the fork that publishes it, and nothing on the main stream waits
        # for a weight gradient until a consumer of the parameter gradients joins.  A layer without a data gradient has
        # nothing to run beside: it stays on the main stream.
        beside = dx is not None and self.side_lane
        if beside:
            plan.fork()
        wg(plan, d, x.ptr, gy.ptr, gy.ld, self._G(name + "/kernel"), self._G(name + "/bias"), side=beside)
        if dx is not None:
            self._dgrad(plan, d, name, gy, dx, mask, res, self._prep_jobs)
        if on_ready is not None:
            on_ready(name)
