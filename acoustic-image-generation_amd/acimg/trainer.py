"""`Trainer`: the acoustic-image train / eval loop, MI355X-native (`TrainerMask` of the reference).

Mirrors trainer/mfcctrainer.py: ctor (:16-26), `_build_functions` (:28-82: tile the MFCC vector,
build image encoder + generator, MSE + Huber + latent_loss*mean(KL) + slim regularisers, Adam on
UNetAcRes/* + resnet_v1_50/conv_map/* with the BN moving-average updates), `train` (:249-398 epoch
loop, validation, best / every-10-epochs checkpoints, model.txt), `_evaluate` (:411-442),
`_retrieve_batch` (:444-467), `test` (:476-536 with the four per-3-channel MSEs), `_save_checkpoint`,
`_restore_model`, `_init_model`.  The body of the hot loop (:343-349, one session.run of
[lossmse, loss, summary_op, train_op]) is `train_step`.

One step = ONE recorded plan of C-ABI kernel launches on fixed device buffers:
  zero loss sums -> tile -> trunk forward (BN batch statistics, moving averages advance) ->
  generator forward -> reconstruction loss (+ its gradient) -> L2 regulariser -> loss scalars ->
  generator backward -> conv_map backward -> [bucketed RCCL all-reduce, overlapped] -> Adam (1 launch).
The recorded plans hold the step alone; scalars are returned as a dict.

The reference's TensorBoard log (:255-297,343-357,373-378) is written while `trainer.logger` is a `logger.Logger`
(None, the default: nothing below runs and `train()` is what it was).  On every step with step % display_freq == 0
`train()` writes, at event step = `global_step` after that batch's update: the scalars l2_loss / l1_loss / train_loss /
latent_loss (by FLAGS.MSE, FLAGS.huber_loss, --ae), the eight images mfcc0..3 (target) and reconstructed0..3 (the
training-mode forward output) of image 0 of the batch, channel groups 0-2 .. 9-11, and - `log_histograms` - one histogram
per trainable TF variable after that step's Adam update; per epoch `valid_loss` at step = epoch.  The images are
rendered and the histograms reduced ON THE DEVICE (ops.summary_images, ops.histogram_segments), behind the trained part
on its stream, for the displayed batches only, outside the recorded plans; they are read back when the batch's losses
are.  Data parallel: only the writer rank (`dp.is_writer`) is given a logger.
"""
import os
from collections import OrderedDict
from datetime import datetime

import torch

from . import _lib, dp, ops
from .flags import FLAGS
from .logger import histogram_fields
from .session import Graph, Session, draw_noise, loss_dict, write_saver_bundle
from .unet_acresnet import Z

_FRAMES_PER_SECOND = 12


class Trainer(object):

    def __init__(self, modelac, modelimages, display_freq=1,
                 learning_rate=0.0001, num_classes=14, num_epochs=1, nr_frames=12, temporal_pooling=False,
                 session=None):
        self.modelac = modelac
        self.modelimages = modelimages
        self.display_freq = display_freq
        self.learning_rate = learning_rate
        self.num_classes = num_classes
        self.num_epochs = num_epochs
        self.nr_frames = nr_frames
        self.temporal_pooling = temporal_pooling
        self.session = session
        self.global_step = 0
        self.graphs = {}
        self.comm = None
        self.group = None              # enable_data_parallel: the process group and the form of the gradient exchange
        self.exchange = "auto"
        self.noise_seed = 1237
        self._noise_calls = 0          # draws of the latent noise so far: each takes a fresh Philox counter range
        self.log = print
        self.hold_exchange = False     # True while micro-batch gradients are being accumulated (train_step_sharded)
        self._acc = None
        self._pipe = None              # state of the two-lane pipeline (train_step_pipelined)
        self._lane_cache = None        # ((caller's stream, lanes wanted), the streams measured to run beside it)
        # the lanes beside the caller's stream as high-priority streams was measured in round 3
        # (profiles/r03/pipeline_lane_priority_r03al.txt)
        self.lane_priority = 0
        self._saved = []               # the checkpoints _save_checkpoint keeps (Saver(max_to_keep=11))
        self.logger = None             # a logger.Logger: train() writes the reference's TensorBoard summaries
        self.log_histograms = False    # with a logger: also one histogram per trainable TF variable
        self._rendered = {}            # tag of a displayed batch -> what _render_summaries left on the device for it
        self._summary_plan = None      # eager plan (and workspace) of the summary launches
        self._hist_table = None        # (names, segments, limits, total elements) of the trainable variables

    # ------------------------------------------------------------------------------------------------
    # graph construction
    # ------------------------------------------------------------------------------------------------
    def _build_functions(self, data=None, batch_size=None):
        """Builds the step for `batch_size` (default: data.batch_size or FLAGS.batch_size)."""
        if batch_size is None:
            batch_size = getattr(data, "batch_size", None) or FLAGS.batch_size
        if self.session is None:
            self.session = Session()
        g = self._build_graph(int(batch_size), self.modelimages, self.modelac)
        self.session.finalize()
        self.acoustic, self.mfcc, self.video = g.acoustic, g.mfcc, g.video
        self.mfccmap = g.mfccmap
        self.primary = g
        return g

    def _build_graph(self, N, modelimages, modelac):
        sess = self.session
        z = sess.zeros
        g = Graph()
        g.N = N
        g.modelimages, g.modelac = modelimages, modelac
        g.acoustic = z(N, 36, 48, 12)
        g.mfcc = z(N, 12)
        g.video = z(N, 224, 298, 3)
        g.eps = z(N, Z)
        # self.mfccmap = tile(mfcc) -> [-1,36,48,12]   (trainer/mfcctrainer.py:38-40)
        g.mfccmap = z(N, 36, 48, 12)
        modelimages._build_model(g.video, session=sess)
        modelac._build_model(g.mfccmap, modelimages.output, session=sess, eps=g.eps)
        g.sums = z(4)          # [sum e^2, sum huber, sum w^2, -]
        g.chan = z(16)         # per-channel squared error (test)
        g.losses = z(8)        # mse, huber, latent, reg, total
        g.g_logit = z(N, 36, 48, 12)
        count = N * 36 * 48 * 12
        w_mse, w_hub = float(bool(FLAGS.MSE)), float(bool(FLAGS.huber_loss))
        ae = modelac.embedding
        kl = None if ae else modelac.kl

        def head(plan):
            ops.zero(plan, g.sums)
            ops.tile_mfcc(plan, g.mfcc, g.mfccmap, N, 36 * 48, 12)

        # ---- training step ----
        p = sess.new_plan()
        head(p)
        head_calls = len(p.calls)
        p.extend(modelimages.plan_train)
        p.extend(modelac.plan_fwd)
        ops.recon_loss(p, modelac.output, g.acoustic, g.g_logit, g.sums, count, w_mse, w_hub)
        modelimages.record_regularizer(p, ops.Ptr(g.sums, 2))
        from .vision import WEIGHT_DECAY
        ops.loss_finalize(p, g.sums, kl, N, count, FLAGS.latent_loss, 0.5 * WEIGHT_DECAY, w_mse, w_hub, g.losses)
        # gradient buckets: the flat buffer is laid out in backward-completion order; a host hook after
        # the last kernel of each bucket fires its all-reduce on the side stream (no-op on one GPU)
        s = modelac.scope
        cm = modelimages.scope + "/conv_map"
        self.bucket_boundaries = [cm + "/BatchNorm/beta", s + "/layer6/conv_1/bias", s + "/dense/bias",
                                  s + "/heads/bias"]
        ready = {"layer6/conv_1": 1, "dense": 2, "heads": 3, "layer1/conv_1": 4}

        def on_ready(name, p=p):
            if name in ready:
                # the bucket's weight gradients run on the plan's side lane: joined before an exchange reads them
                p.add_hook(lambda i=ready[name], join=p.make_join(): self._bucket_ready(i, join))

        modelac.record_backward(p, g.g_logit, modelimages.g_output, FLAGS.latent_loss / N if not ae else 0.0,
                                on_ready=on_ready)
        modelimages.record_backward(p)
        p.add_hook(lambda: self._bucket_ready(0))
        g.plan_train = p
        # the calls [head_calls, head_calls + frozen_calls) are the FROZEN trunk (train_step_pipelined's lane A)
        g.head_calls = head_calls
        g.frozen_calls = modelimages.frozen_calls
        g.stage_calls = modelimages.stage_calls            # None with one trunk stage
        g.stage_read_calls = modelimages.stage_read_calls
        # ---- evaluation step (is_training = 0: moving statistics; MSE only, :411-442) ----
        e = sess.new_plan()
        head(e)
        e.extend(modelimages.plan_eval)
        e.extend(modelac.plan_fwd)
        ops.recon_loss(e, modelac.output, g.acoustic, None, g.sums, count, 1.0, 1.0)
        ops.zero(e, g.chan)
        ops.sqerr_channels(e, modelac.output, g.acoustic, N * 36 * 48, 12, g.chan)
        ops.loss_finalize(e, g.sums, None, N, count, 0.0, 0.0, 1.0, 0.0, g.losses)
        g.plan_eval = e
        g.count = count
        self.graphs[N] = g
        return g

    def _graph_for(self, N):
        if N in self.graphs:
            return self.graphs[N]
        # a different batch size (last partial batch): same variables, new buffers + plans, the same kernel path - two-pass
        # rule included - as the primary graph (Model.replica)
        return self._build_graph(N, self.modelimages.replica(), self.modelac.replica())

    def _bucket_ready(self, i, join=None):
        if self.comm is not None and not self.hold_exchange:
            if join is not None:
                join()
            self.comm.bucket_ready(i)

    def enable_data_parallel(self, group=None, exchange="auto", force=False):
        """All-reduce the flat gradient across ranks (torch.distributed must be initialised).  exchange:
          "bucketed": five contiguous buckets, each fired from its hook in the recorded backward plan on an exchange stream
                      (the all-reduce overlaps the rest of the backward pass: BASELINE.json's north_star form);
          "whole":    ONE all-reduce of the whole flat gradient behind the backward pass;
          "auto":     bucketed on the one-stream entries (train_step), whole on the pipelined entry, whose trained part
                      already runs a pipeline tick behind the trunk stages (the slack budget).
        force: exchange even at world size 1 (rehearsal of the RCCL path on a one-GPU box)."""
        assert exchange in ("auto", "bucketed", "whole"), exchange
        store = self.session.store
        self.buckets = dp.make_buckets(store.train_ranges(), self.bucket_boundaries)
        assert len(self.buckets) == 5, self.buckets
        self.comm = dp.GradComm(store.grad, self.buckets, group, force=force)
        self.group = group
        self.exchange = exchange
        return self.comm

    def sync_moving_statistics(self):
        """collective: every rank ends up with the mean over ranks of the trunk's BN moving statistics
        (per-replica while training; one set for checkpoints and evaluation: SURVEY §8(e))"""
        self.flush_pipeline()
        store = self.session.store
        rng = [(v.offset, v.numel) for n, v in store.vars.items() if v.group == "state" and "/moving_" in n]
        dp.average_moving_statistics(store.flat["state"], rng, self.group)
        store.version += 1

    # ------------------------------------------------------------------------------------------------
    # the step
    # ------------------------------------------------------------------------------------------------
    def _feed(self, g, batch, eps):
        acoustic, mfcc, video = batch[0], batch[1], batch[2]
        g.acoustic.copy_(acoustic.reshape(g.N, 36, 48, 12), non_blocking=True)
        g.mfcc.copy_(mfcc.reshape(g.N, 12), non_blocking=True)
        g.video.copy_(video.reshape(g.N, 224, 298, 3), non_blocking=True)
        self._noise(g, eps)

    def _noise(self, g, eps):
        """eps given: copy it in (parity tests); else sample N(0,1) on the device, a fresh Philox
        counter range every step (the reference's tf.random_normal, models/unet_acresnet.py:77)"""
        if eps is not None:
            g.eps.copy_(eps.reshape(g.N, Z), non_blocking=True)
        else:
            self._noise_calls += 1
            draw_noise(self.session, g.eps, self.noise_seed, self._noise_calls * 65536)

    def train_step(self, batch=None, eps=None, sync=True, probe=None, tag=None):
        """One optimisation step (the body of the reference's hot loop, trainer/mfcctrainer.py:343-349).
        batch: (acoustic [N,36,48,12], mfcc [N,12], video [N,224,298,3], ...) or None to reuse the
        tensors already resident in the graph's input buffers.  Returns {mse, huber, latent, reg, loss}
        (python floats; sync=False returns the device tensor instead and does not block).  tag: with a logger, render
        this batch's summaries behind the step (`train()` reads them back under that tag)."""
        g = self.primary if batch is None else self._graph_for(int(batch[1].reshape(-1, 12).shape[0]))
        self.flush_pipeline()
        if batch is not None:
            self._feed(g, batch, eps)
        else:
            self._noise(g, eps)
        whole = self.comm is not None and self.exchange == "whole"
        held, self.hold_exchange = self.hold_exchange, self.hold_exchange or whole
        try:
            if probe is None:
                g.plan_train.run()      # hooks inside fire the bucketed all-reduce when data-parallel
            else:
                g.plan_train.run_probed(probe[0], probe[1])
        finally:
            self.hold_exchange = held
        scale = 1.0
        if self.comm is not None and self.comm.enabled:
            if whole:
                self.comm.allreduce_all()
            else:
                self.comm.wait()
            scale = self.comm.grad_scale
        self.global_step += 1
        self.session.adam_step(self.learning_rate, self.global_step, grad_scale=scale)
        if tag is not None and self.logger is not None:
            self._rendered[tag] = self._render_summaries(g)
        if not sync:
            return g.losses
        return self._scalars(g)

    # ---- software pipeline over HIP streams ------------------------------------------------------------------
    def _pipeline(self, g):
        """Stages: the FROZEN trunk (no trainable variable is read: trainer/mfcctrainer.py:64 keeps it out of var_list),
        as one stage or — `ResNet50Model(stages=2)`, the default — as two (units 1-8 | units 9-16, each with its own
        arena / statistics / tail workspace, a dedicated boundary tensor between them); then the TRAINED part: conv_map,
        the generator, the losses, the backward pass, the gradient exchange, Adam.  One HIP stream per stage (the first
        is the caller's); per call the stages run consecutive batches: trunk stage 1 of batch n, stage 2 of batch n - 1,
        the trained part of batch n - 2.  The arithmetic of every batch is the one-stream step's, bit for bit: a trunk
        stage's inputs (images or the boundary tensor, frozen weights, its own moving statistics, in batch order) do not
        depend on later stages, and every stage processes the batches in order on its own stream.  Buffers that cross a
        stage boundary are written by the producing stage's LAST call, which waits until the consuming stage of the
        previous batch has read them (boundary tensor: after stage 2's first unit; `xfinal`: after the whole trained
        part, whose last kernel — conv_map's weight gradient — reads it)."""
        if self._pipe is not None and self._pipe["g"] is g:
            return self._pipe
        mi = self.modelimages
        if g.frozen_calls is None or not mi._split:
            raise RuntimeError("train_step_pipelined: needs the split-MFMA trunk (precision f16x3 / f16): its frozen part "
                               "uses no shared workspace")
        assert self._pipe is None or not self._pipe["inflight"]
        dev = self.session.device
        full = g.plan_train
        lo, cut = g.head_calls, g.head_calls + g.frozen_calls
        assert full.calls[cut - 1][0] == "bn_add_relu_split", full.calls[cut - 1][0]     # the call that writes xfinal
        cur = torch.cuda.current_stream(dev)
        # one stream per stage beyond the first, one for the trained part and one for its side lane — only streams that
        # were MEASURED to run beside the caller's and beside each other (ops.concurrent_streams): the runtime maps
        # streams onto a few hardware queues (4 by default; RCCL takes some) and two streams on one queue serialise
        want = (2 if g.stage_calls is not None else 1) + 1
        key = (cur.cuda_stream, want)
        if self._lane_cache is None or self._lane_cache[0] != key:
            self._lane_cache = (key, ops.concurrent_streams(dev, cur, want, priority=self.lane_priority))
        lanes = list(self._lane_cache[1])
        side_b = lanes.pop() if len(lanes) == want else None
        while len(lanes) < want - 1:
            lanes.append(lanes[-1] if lanes else cur)      # too few queues: stages share a lane (slower, still correct)
        stages = []
        if g.stage_calls is not None:
            sc, src = g.head_calls + g.stage_calls, g.head_calls + g.stage_read_calls
            # ... the boundary tensor (a two-pass unit writes it from conv3's second pass)
            assert full.calls[sc - 1][0] in ("bn_add_relu_split", "conv2d_fwd_split3p_tail", "conv2d_fwd_split3p_tail_proj")
            stages.append(dict(parts=[(full.slice(lo, sc - 1), lo, None, None), (full.slice(sc - 1, sc), sc - 1, "x", None)],
                               stream=cur))
            stages.append(dict(parts=[(full.slice(sc, src), sc, None, "x"), (full.slice(src, cut - 1), src, None, None),
                                      (full.slice(cut - 1, cut), cut - 1, "b", None)],
                               stream=lanes[0]))
        else:
            stages.append(dict(parts=[(full.slice(lo, cut - 1), lo, None, None), (full.slice(cut - 1, cut), cut - 1, "b", None)],
                               stream=cur))
        for st in stages:
            st["done"] = torch.cuda.Event()
        pipe = dict(g=g, stages=stages, head=full.slice(0, lo), b=full.slice(cut, len(full.calls)), b_off=cut,
                    sb=lanes[-1], ev={"x": torch.cuda.Event(), "b": torch.cuda.Event()},
                    recorded=set(), inflight=[], finished=[], lanes=len(set(x.cuda_stream for x in lanes + [cur])))
        ops.set_side_lane(dev, pipe["sb"], side_b if side_b is not None else pipe["sb"])
        if pipe["sb"] != cur:
            pipe["sb"].wait_stream(cur)
        for st in stages[1:]:
            if st["stream"] != cur:
                st["stream"].wait_stream(cur)
        self._pipe = pipe
        return pipe

    def _run_trained_part(self, pipe, item, probe=None):
        """the trained part of the oldest batch on its stream (targets copied in behind the previous batch), Adam included"""
        g = pipe["g"]
        with torch.cuda.stream(pipe["sb"]):
            if item["targets"] is not None:
                ac, mf = item["targets"]
                g.acoustic.copy_(ac.reshape(g.N, 36, 48, 12), non_blocking=True)
                g.mfcc.copy_(mf.reshape(g.N, 12), non_blocking=True)
            self._noise(g, item["eps"])
            pipe["sb"].wait_event(pipe["stages"][-1]["done"])      # the trunk has written xfinal for this batch
            pipe["head"].run()
            # data parallel: ONE exchange of the whole flat gradient, issued from THIS stream after the backward pass (no
            # buckets, no separate exchange stream): the trained part has a whole tick of slack behind the trunk stages,
            # so nothing needs to overlap inside it; every collective call costs host time, and every stream beyond the
            # runtime's 4 hardware queues shares a queue with one of the lanes (RCCL's own stream is the fourth)
            bucketed = self.exchange == "bucketed" and item.get("accum") is None
            held, self.hold_exchange = self.hold_exchange, self.hold_exchange or not bucketed
            try:
                if probe is None:
                    pipe["b"].run()
                else:
                    pipe["b"].run_probed(probe[0], probe[1], offset=pipe["b_off"])
            finally:
                self.hold_exchange = held
            store = self.session.store
            scale = 1.0
            acc = item.get("accum")
            if acc is not None:
                # shard i of n of a strong-scaling step (train_step_sharded): gradients and losses are accumulated on this
                # stream; the exchange and the ONE Adam update follow the last shard
                i, n = acc
                L = _lib.load()
                sth = ops.current_stream_handle(self.session.device)
                if i == 0:
                    self._acc.copy_(store.grad)
                    self._acc_loss = g.losses[:5].clone()
                else:
                    _lib.check(L.acimg_axpy(1.0, store.grad.data_ptr(), self._acc.data_ptr(), store.grad.numel(), sth),
                               "axpy")
                    self._acc_loss = self._acc_loss + g.losses[:5]
                if i + 1 < n:
                    pipe["ev"]["b"].record(pipe["sb"])
                    pipe["recorded"].add("b")
                    return
                store.grad.copy_(self._acc)
                world = 1
                if self.comm is not None and self.comm.enabled:
                    self.comm.allreduce_all()
                    world = self.comm.world
                scale = 1.0 / (n * world)
                if item.get("tag") is not None:
                    pipe["finished"].append((item["tag"], self._acc_loss / n))
            elif self.comm is not None and self.comm.enabled:
                if bucketed:
                    self.comm.wait()
                else:
                    self.comm.allreduce_all()
                scale = self.comm.grad_scale
            self.global_step += 1
            self.session.adam_step(self.learning_rate, self.global_step, grad_scale=scale)
            if acc is None and item.get("tag") is not None:
                # a private copy of this batch's losses (the graph's buffer is rewritten by the next batch)
                pipe["finished"].append((item["tag"], g.losses[:5].clone()))
                if self.logger is not None:
                    self._rendered[item["tag"]] = self._render_summaries(g)
            pipe["ev"]["b"].record(pipe["sb"])
        pipe["recorded"].add("b")

    def _run_trunk_stage(self, pipe, k, item, probe=None):
        g, st = pipe["g"], pipe["stages"][k]
        with torch.cuda.stream(st["stream"]):
            if k == 0:
                if item["video"] is not None:
                    g.video.copy_(item["video"].reshape(g.N, 224, 298, 3), non_blocking=True)
            else:
                st["stream"].wait_event(pipe["stages"][k - 1]["done"])
            for plan, off, wait, record in st["parts"]:
                if wait is not None and wait in pipe["recorded"]:
                    st["stream"].wait_event(pipe["ev"][wait])      # the consumer of the previous batch has read it
                if probe is None:
                    plan.run()
                else:
                    plan.run_probed(probe[0], probe[1], offset=off)
                if record is not None:
                    pipe["ev"][record].record(st["stream"])
                    pipe["recorded"].add(record)
            st["done"].record(st["stream"])

    def _advance(self, pipe, new_item, probe=None):
        """one tick: every batch in flight moves one stage on (oldest first, so that an event waited on in this tick was
        recorded for the batch before); returns the loss tensor if a batch finished"""
        out, n = None, len(pipe["stages"])
        flight = pipe["inflight"]
        if flight and flight[0]["stage"] == n:
            self._run_trained_part(pipe, flight.pop(0), probe)
            out = pipe["g"].losses
        for item in flight:                      # oldest first = deepest stage first
            self._run_trunk_stage(pipe, item["stage"], item, probe)
            item["stage"] += 1
        if new_item is not None:
            new_item["stage"] = 0
            self._run_trunk_stage(pipe, 0, new_item, probe)
            new_item["stage"] = 1
            flight.append(new_item)
        return out

    def pop_finished(self):
        """[(tag, {mse, huber, latent, reg, loss})] of the batches submitted with a tag that finished since the last call,
        oldest first (reads behind the trained part's stream, not behind the trunks in flight)"""
        pipe = self._pipe
        if pipe is None or not pipe["finished"]:
            return []
        done, pipe["finished"] = pipe["finished"], []
        return [(tag, self._lane_b_scalars(t)) for tag, t in done]

    def train_step_pipelined(self, batch=None, eps=None, probe=None, tag=None):
        """One call = one batch in, one optimisation step out, in steady state: the frozen trunk of THIS batch starts on
        the caller's stream while the later stages of the previous batches run on theirs (`_pipeline`).  Returns the
        device tensor of the losses of the batch that finished in this call (None while the pipeline fills);
        `flush_pipeline()` finishes the batches in flight.  batch None: reuse the images / targets resident in the
        graph's buffers (bench.py).  tag: keep this batch's losses for `pop_finished()` (the training log)."""
        g = self.primary if batch is None else self._graph_for(int(batch[1].reshape(-1, 12).shape[0]))
        out = None
        carried = []
        if self._pipe is not None and self._pipe["g"] is not g:
            out = self.flush_pipeline()      # another batch size (the last, partial batch): finish the ones in flight
            carried, self._pipe = self._pipe["finished"], None
        pipe = self._pipeline(g)
        pipe["finished"] = carried + pipe["finished"]
        # the targets are consumed two calls later, on the trained part's stream: they are staged NOW (a device copy per
        # batch in flight), so a loader may reuse its host buffers as soon as this call returns; the images are copied
        # in this call (trunk stage 1 runs in it)
        targets = None
        if batch is not None:
            targets = (self._stage_for_lane_b(pipe, batch[0]), self._stage_for_lane_b(pipe, batch[1]))
            if eps is not None:
                eps = self._stage_for_lane_b(pipe, eps)
        item = dict(video=None if batch is None else batch[2], targets=targets, eps=eps, tag=tag)
        res = self._advance(pipe, item, probe)
        return res if res is not None else out

    def _stage_for_lane_b(self, pipe, x):
        """device copy of a host / device tensor made NOW on the caller's stream and read two ticks later by the trained
        part's stream: `record_stream` tells the caching allocator about that second stream, so the block is not handed
        to a later staging copy (on the caller's stream) before the trained part's D2D copy of it has run"""
        t = torch.as_tensor(x).to(self.session.device, torch.float32, copy=True)
        if pipe["sb"] != torch.cuda.current_stream(self.session.device):
            t.record_stream(pipe["sb"])
        return t

    def _lane_b_scalars(self, losses):
        """python floats of a loss tensor produced on lane B (read behind that lane, not behind the trunk in flight)"""
        with torch.cuda.stream(self._pipe["sb"]):
            return loss_dict(losses)

    def flush_pipeline(self):
        """finish the batches in flight (oldest first) and make the current stream wait for every lane; returns the
        losses of the last one (device tensor) or None"""
        pipe, out = self._pipe, None
        if pipe is None:
            return None
        while pipe["inflight"]:
            res = self._advance(pipe, None)
            out = res if res is not None else out
        cur = torch.cuda.current_stream(self.session.device)
        for st in pipe["stages"]:
            if st["stream"] != cur:
                cur.wait_stream(st["stream"])
        cur.wait_stream(pipe["sb"])
        return out

    def train_step_sharded(self, shards, eps=None, probe=None, pipelined=False, tag=None):
        """Strong-scaling step: `shards` = this rank's micro-batches (each of the primary graph's size: the BN group),
        run one after the other with their gradients accumulated; ONE exchange of the accumulated gradient, ONE Adam
        update with scale 1 / (shards * world).  With one shard per rank this is `train_step` (overlapped buckets).
        pipelined: the shards go through the lanes of `train_step_pipelined` - inside a step every shard sees the same
        weights and the frozen trunk reads none of them, so the trunk of shard i + 1 (and of the next step's first
        shards) runs beside the trained part of shard i; gradients and losses are accumulated on the trained part's
        stream in shard order: bit-identical to the one-stream form.  Returns None then (`flush_pipeline()` finishes the
        shards in flight; `pop_finished()` returns the mean losses of the steps submitted with a `tag`)."""
        if pipelined:
            g = self.primary
            if self._pipe is not None and self._pipe["g"] is not g:
                self.flush_pipeline()
                self._pipe = None
            pipe = self._pipeline(g)
            if self._acc is None:
                self._acc = torch.zeros_like(self.session.store.grad)
            for i, b in enumerate(shards):
                e = None if eps is None else self._stage_for_lane_b(pipe, eps[i])
                item = dict(video=b[2], targets=(self._stage_for_lane_b(pipe, b[0]), self._stage_for_lane_b(pipe, b[1])),
                            eps=e, tag=tag, accum=(i, len(shards)))
                self._advance(pipe, item, probe)
            return None
        if len(shards) == 1:
            return self.train_step(shards[0], eps=None if eps is None else eps[0], sync=probe is None, probe=probe)
        self.flush_pipeline()          # a batch in flight reads the input buffers this call is about to overwrite
        store = self.session.store
        g = self.primary
        if self._acc is None:
            self._acc = torch.zeros_like(store.grad)
        L = _lib.load()
        st = ops.current_stream_handle(self.session.device)
        self.hold_exchange = True
        tot = None
        try:
            for i, b in enumerate(shards):
                self._feed(g, b, None if eps is None else eps[i])
                if probe is None:
                    g.plan_train.run()
                else:
                    g.plan_train.run_probed(probe[0], probe[1])
                if i == 0:
                    self._acc.copy_(store.grad)
                else:
                    _lib.check(L.acimg_axpy(1.0, store.grad.data_ptr(), self._acc.data_ptr(), store.grad.numel(), st),
                               "axpy")
                tot = g.losses[:5].clone() if tot is None else tot + g.losses[:5]
        finally:
            self.hold_exchange = False
        store.grad.copy_(self._acc)
        world = 1
        if self.comm is not None and self.comm.enabled:
            self.comm.allreduce_all()
            world = self.comm.world
        self.global_step += 1
        self.session.adam_step(self.learning_rate, self.global_step, grad_scale=1.0 / (len(shards) * world))
        return loss_dict(tot / len(shards))

    def _scalars(self, g):
        return loss_dict(g.losses)

    # ---- TensorBoard summaries (trainer/mfcctrainer.py:255-297,343-357) ---------------------------------------------
    def _histogram_table(self):
        """built once: the TF names of the trainable variables and, on the device, their boxes in the flat trainable
        buffer (13 int64 each: offset, internal dims, lo, hi; a fused head is a column box of the shared matrix) and TF's
        default bucket limits"""
        if self._hist_table is None:
            from . import events
            store = self.session.store
            names, rows, total = [], [], 0

            def seg(var, lo, hi):
                dims = list(var.shape) + [1] * (4 - len(var.shape))
                return [var.offset] + dims + list(lo) + [0] * (4 - len(lo)) + list(hi) + [1] * (4 - len(hi))

            fused_internal = set()
            for h in store.fused:
                fused_internal.update((h.kernel.name, h.bias.name))
                rows_k = h.hh * h.hw * h.cp
                for i, name in enumerate(h.tf_names):          # n0 kernel, n0 bias [, n1 kernel, n1 bias]
                    c_lo = (i // 2) * h.z
                    names.append(name)
                    if i % 2 == 0:
                        rows.append([h.kernel.offset, h.hh * h.hw, h.cp, h.kernel.shape[1], 1,
                                     0, 0, c_lo, 0, h.hh * h.hw, h.cin, c_lo + h.z, 1])
                        assert h.kernel.shape[0] == rows_k, (h.kernel.shape, rows_k)
                        total += h.kernel.numel
                    else:
                        rows.append(seg(h.bias, (c_lo,), (c_lo + h.z,)))
                        total += h.bias.numel
            for name, v in store.vars.items():
                if v.group == "train" and name not in fused_internal:
                    names.append(name)
                    rows.append(seg(v, (0,) * len(v.tf_shape), v.tf_shape))
                    total += v.numel
            dev = self.session.device
            limits = events.default_bucket_limits()
            self._hist_table = (names, torch.tensor(rows, dtype=torch.int64, device=dev),
                                torch.tensor(limits, dtype=torch.float64, device=dev), int(total), limits)
        return self._hist_table

    def _render_summaries(self, g):
        """on the CURRENT stream, behind the step that just ran on it: the eight [36,48,3] images of image 0 of the batch
        (4 channel groups of the target, 4 of the generated image) into a fresh uint8 tensor and, with `log_histograms`,
        the histograms of the flat trainable buffer (after this step's Adam update) into fresh tensors.  Nothing is read
        back here."""
        dev = self.session.device
        if self._summary_plan is None:
            self._summary_plan = ops.Plan(dev, eager=True)
        plan = self._summary_plan
        images = torch.empty((8, 36, 48, 3), dtype=torch.uint8, device=dev)
        ops.summary_images(plan, g.acoustic, 12, 36 * 48, 0, 4, 1, images[:4])
        ops.summary_images(plan, g.modelac.output, 12, 36 * 48, 0, 4, 1, images[4:])
        out = dict(step=self.global_step, images=images, stream=torch.cuda.current_stream(dev), hist=None)
        if self.log_histograms:
            names, table, limits, total, _ = self._histogram_table()
            V, L = len(names), limits.numel()
            counts = torch.empty((V, L), dtype=torch.int64, device=dev)
            stats = torch.empty((V, 4), dtype=torch.float64, device=dev)
            bad = torch.empty((V,), dtype=torch.int64, device=dev)
            ops.histogram_segments(plan, self.session.store.flat["train"], table, V, limits, L, total, counts, stats, bad)
            out["hist"] = (counts, stats, bad)
        return out

    def _register_summaries(self):
        """the registrations of trainer/mfcctrainer.py:266-297 (+ the variables' histograms), merged"""
        lg = self.logger
        if lg.summary_op is not None:
            return
        if FLAGS.MSE:
            lg.log_scalar('l2 loss', "mse")
        if FLAGS.huber_loss:
            lg.log_scalar('l1 loss', "huber")
        lg.log_scalar('train_loss', "loss")
        if not FLAGS.ae:
            lg.log_scalar('latent_loss', "latent")       # losses[2]: FLAGS.latent_loss * mean KL, the weighted term
        for i in range(4):
            lg.log_image('mfcc{}'.format(i), i, max_outputs=1)
        for i in range(4):
            lg.log_image('reconstructed{}'.format(i), 4 + i, max_outputs=1)
        if self.log_histograms:
            for v, name in enumerate(self._histogram_table()[0]):
                lg.log_histogram(name + ":0", v)
        lg.merge_summary()

    def _write_summaries(self, losses, rendered):
        """read one displayed batch's images (and histograms) back behind the stream that rendered them and write the
        step's summary"""
        with torch.cuda.stream(rendered["stream"]):
            images = rendered["images"].cpu().numpy()
            hist = None if rendered["hist"] is None else [t.cpu().numpy() for t in rendered["hist"]]
        names = limits = None
        if hist is not None:
            names, _, _, _, limits = self._histogram_table()

        def fetch(kind, source):
            if kind == "scalar":
                return losses[source]
            if kind == "image":
                return images[source:source + 1]
            counts, stats, bad = hist
            return histogram_fields(names[source] + ":0", counts[source], stats[source], bad[source], limits)

        self.logger.write_summary(self.logger.summary(fetch), rendered["step"])

    def eval_step(self, batch=None, eps=None):
        """forward in inference mode (BN moving statistics); returns mse + the four per-3-channel MSEs"""
        g = self.primary if batch is None else self._graph_for(int(batch[1].reshape(-1, 12).shape[0]))
        self.flush_pipeline()
        if batch is not None:
            self._feed(g, batch, eps)
        else:
            self._noise(g, eps)
        g.plan_eval.run()
        mse = float(g.losses[0])
        ch = g.chan[:12].tolist()
        res = OrderedDict(mse=mse)
        per = g.N * 36 * 48 * 3
        for i in range(4):
            res["mse%d" % i] = sum(ch[3 * i:3 * i + 3]) / per
        return res

    def generate(self, batch, eps=None):
        """the generator output of the inference-mode forward (is_training = 0, BN moving statistics; the plan of
        `eval_step`, whose loss part runs and is ignored) for `batch` = (acoustic, mfcc [n,12], video [n,224,298,3],
        ...); the acoustic slot may hold zeros.  Returns the graph's [n,36,48,12] device buffer for that batch size
        (partial batches included): it is overwritten by the next call with the same n."""
        g = self._graph_for(int(batch[1].reshape(-1, 12).shape[0]))
        self.flush_pipeline()
        self._feed(g, batch, eps)
        g.plan_eval.run()
        return g.modelac.output

    def features(self, batch, eps=None):
        """the latent of the same inference-mode forward as `generate`: the code the decoder's dense layer consumes,
        `zbuf[:, :150]` = mean + std * eps (extract_features_unetraces.py:124-125), or the min-max normalised code
        itself when the generator is a plain auto-encoder (--ae 1).  Returns a [n,150] float32 device view of the
        graph's buffer for that batch size: it is overwritten by the next call with the same n."""
        from .unet_acresnet import Z
        g = self._graph_for(int(batch[1].reshape(-1, 12).shape[0]))
        self.flush_pipeline()
        self._feed(g, batch, eps)
        g.plan_eval.run()
        return g.modelac.zbuf[:, :Z]

    # ------------------------------------------------------------------------------------------------
    # reference protocol: loops, checkpoints
    # ------------------------------------------------------------------------------------------------
    def _retrieve_batch(self, next_batch):
        if FLAGS.model == 'UNet':
            mfcc = next_batch[1].reshape(-1, 12)
            images = next_batch[2].reshape(-1, 224, 298, 3)
            acoustic = next_batch[0].reshape(-1, 36, 48, 12)
            labels = next_batch[3].reshape(mfcc.shape[0], -1).argmax(1)
            scenario = next_batch[4].reshape(mfcc.shape[0], -1).argmax(1)
        else:
            raise ValueError('Unknown model type')
        return acoustic, mfcc, images, labels, scenario

    def _init_model(self, session):
        """random init, then optional partial restores (trainer/mfcctrainer.py:163-234)"""
        self.modelimages.initialize()
        self.modelac.initialize()
        if FLAGS.init_checkpoint is not None:
            self.modelac.init_model(session, FLAGS.init_checkpoint)
        elif FLAGS.acoustic_init_checkpoint is not None or FLAGS.visual_init_checkpoint is not None:
            if FLAGS.acoustic_init_checkpoint is not None:
                self.modelac.init_model(session, FLAGS.acoustic_init_checkpoint)
            if FLAGS.visual_init_checkpoint is not None:
                self.modelimages.init_model(session, FLAGS.visual_init_checkpoint)
        elif FLAGS.restore_checkpoint is not None:
            self._restore_model(session)

    def _restore_model(self, session):
        """model variables only: Adam slots and global_step start afresh (:236-247)"""
        from .vision import load_state_file
        state = load_state_file(FLAGS.restore_checkpoint)
        session.store.load_state(state, strict=False)

    def _save_checkpoint(self, session, epoch):
        """`self.saver.save(session, '<checkpoint_dir>/<exp_name>/epoch_<n>.ckpt')` of trainer/mfcctrainer.py:400-406,
        :81 (Saver(max_to_keep=11)): a TensorFlow Saver-V2 bundle (epoch_<n>.ckpt.index + .data-00000-of-00001 + the
        `checkpoint` state file) holding what the reference's Saver holds — every model variable under its TF name,
        the Adam slots `<var>/Adam`, `<var>/Adam_1`, `beta1_power`, `beta2_power` and `global_step` — so the
        reference's own `_restore_model` / `init_model` (:214-247) can read it.  Data-parallel: every rank calls this
        (the BN moving statistics are averaged over ranks first, a collective); only rank 0 writes."""
        self.flush_pipeline()
        if self.comm is not None and self.comm.enabled:
            self.sync_moving_statistics()
        if not dp.is_writer(self.group):
            return None
        checkpoint_dir = '{}/{}'.format(FLAGS.checkpoint_dir, FLAGS.exp_name)
        os.makedirs(checkpoint_dir, exist_ok=True)
        model_name = 'epoch_{}.ckpt'.format(epoch)
        self.log('{}: {} - Saving model to {}/{}'.format(datetime.now(), FLAGS.exp_name, checkpoint_dir, model_name))
        path = '{}/{}'.format(checkpoint_dir, model_name)
        self._saved = write_saver_bundle(session.store, path, self.global_step, self._saved, 11)   # :81
        return path

    def train(self, train_data=None, valid_data=None):
        assert train_data is not None
        assert valid_data is not None
        if not self.graphs:
            self._build_functions(train_data)
        session = self.session
        self._init_model(session)
        if FLAGS.checkpoint_dir is not None:
            self._save_checkpoint(session, 'random')
        start_epoch = int(self.global_step)
        best_epoch, best_loss = -1, 10000
        if self.logger is not None:
            self._register_summaries()
        for epoch in range(start_epoch, start_epoch + self.num_epochs):
            step = 0
            pipelined = self.modelimages._split and FLAGS.pipeline

            def report(i, r):
                if i % self.display_freq == 0:
                    self.log('{}: {} - Iteration: [{:3}]\t Training_mse_Loss: {:6f}\t Training_Loss: {:6f}'.format(
                        datetime.now(), FLAGS.exp_name, i, r["mse"], r["loss"]))
                    if self.logger is not None:
                        self._write_summaries(r, self._rendered.pop(i))

            for next_batch in train_data.data:
                acoustic, mfcc, images, _, _ = self._retrieve_batch(next_batch)
                if pipelined:
                    # this batch's trunk starts beside the later stages of the batches before it: the line of iteration
                    # i is written when that batch finishes, a few calls later (same numbers, same order)
                    self.train_step_pipelined((acoustic, mfcc, images),
                                              tag=step if step % self.display_freq == 0 else None)
                    for i, r in self.pop_finished():
                        report(i, r)
                else:
                    report(step, self.train_step((acoustic, mfcc, images),
                                                 tag=step if step % self.display_freq == 0 else None))
                step += 1
            if pipelined:
                self.flush_pipeline()
                for i, r in self.pop_finished():
                    report(i, r)
            if self.comm is not None and self.comm.enabled:
                # data parallel: validate with ONE set of BN moving statistics (their mean over ranks, a collective every
                # rank enters here, unconditionally); _evaluate reduces its sums over ranks, so `total_loss` - and with
                # it every branch below that contains a collective (_save_checkpoint) - is the same on all ranks
                self.sync_moving_statistics()
            total_loss = self._evaluate(session, 'validation', valid_data)
            self.log('{}: {} - Epoch: {}\t Validation_mse_Loss: {:6f}'.format(datetime.now(), FLAGS.exp_name, epoch,
                                                                              total_loss))
            if self.logger is not None:
                from . import events
                self.logger.write_summary([events.scalar_value("valid_loss", total_loss)], epoch)
                self.logger.flush_writer()
            if FLAGS.checkpoint_dir is not None:
                if epoch % 10 == 0:
                    self._save_checkpoint(session, epoch)
                if total_loss <= best_loss:
                    best_epoch, best_loss = epoch, total_loss
                    self._save_checkpoint(session, epoch)
                    if dp.is_writer(self.group):
                        with open('{}/{}'.format(FLAGS.checkpoint_dir, FLAGS.exp_name) + "/model.txt", "w") as outfile:
                            outfile.write('{}: {}\nBest Epoch: {}\nValidation_mse_Loss: {:6f}\n'.format(
                                datetime.now(), FLAGS.exp_name, best_epoch, best_loss))
            elif total_loss <= best_loss:
                best_epoch, best_loss = epoch, total_loss
        self.log('{}: {} - Best Epoch: {}\t Validation_mse_Loss: {:6f}'.format(datetime.now(), FLAGS.exp_name,
                                                                            best_epoch, best_loss))
        return best_loss

    def _valid(self, session, data):
        return self._evaluate(session, 'validation', data)

    def _evaluate(self, session, mod, data):
        """size-weighted mean of the per-batch MSE (trainer/mfcctrainer.py:411-442)"""
        loss_sum, data_set_size = 0.0, 0
        for next_batch in data.data:
            acoustic, mfcc, images, labels, _ = self._retrieve_batch(next_batch)
            r = self.eval_step((acoustic, mfcc, images))
            n = labels.shape[0]
            data_set_size += n
            loss_sum += r["mse"] * n
        if self.comm is not None and self.comm.enabled:     # every rank validates its own shard of `data`
            loss_sum, data_set_size = dp.allreduce_sums([loss_sum, data_set_size], self.session.device,
                                                        self.group)
        return loss_sum / data_set_size

    def test(self, test_data=None):
        assert test_data is not None
        if not self.graphs:
            self._build_functions(test_data)
        session = self.session
        self.modelimages.initialize()
        self.modelac.initialize()
        if FLAGS.restore_checkpoint is not None:
            self._restore_model(session)
        sums = [0.0] * 5
        data_set_size = 0
        for next_batch in test_data.data:
            acoustic, mfcc, images, labels, _ = self._retrieve_batch(next_batch)
            r = self.eval_step((acoustic, mfcc, images))
            n = labels.shape[0]
            data_set_size += n
            for i, k in enumerate(("mse", "mse0", "mse1", "mse2", "mse3")):
                sums[i] += r[k] * n
        test_loss, l0, l1, l2, l3 = [s / data_set_size for s in sums]
        line = '{} - Testing_Loss: {:6f}\t  Testing_Loss0: {:6f}\t Testing_Loss1: {:6f}\t Testing_Loss2: {:6f}\t ' \
               'Testing_Loss3: {:6f}'.format(datetime.now(), test_loss, l0, l1, l2, l3)
        if FLAGS.restore_checkpoint is not None and dp.is_writer(self.group):
            name_folder = str.join('/', FLAGS.restore_checkpoint.split('/')[:-1])
            tag = FLAGS.restore_checkpoint.split('/')[-1].split('.')[0].split('_')[-1]
            with open('{}'.format(name_folder) + "/test_accuracy_{}.txt".format(tag), "w") as outfile:
                outfile.write(line)
        self.log(line)
        return test_loss
