"""`ResNet50Model`: the modified ResNet-v1-50 image encoder, MI355X-native.

Mirrors the reference's model protocol (models/vision.py:8-71): `scope`, `init_model(session,
checkpoint_file)`, `_build_model(visual_images)` which sets `output`, `network`, `train_vars`
(conv_map only) and `train_vars2` (the frozen trunk).  Architecture: models/resnet50.py:75-125
(bottleneck), :205-209 (7x7/2 stem, 3x3/2 pool, conv_map 3x4 VALID 2048->12 + BN + ReLU), :261-266
(block strides 1,2,2,1 placed in each block's last unit).

MI355X design (f16x3, the default): every trunk conv is one implicit-GEMM launch on PRE-SPLIT operands (two fp16
planes per tensor in LDS-tile order, "bricks": csrc/igemm_split3d_kernel.hpp) that writes the RAW fp32 conv output
once and leaves per-row-block (sum, sum^2) partials; `bn_finalize` turns them into per-channel scale/shift (and
advances the moving averages); ONE elementwise pass per tensor (`bn_relu_split`, `bn_relu_maxpool_split`,
`bn_add_relu_split`) applies scale/shift (+ shortcut) + ReLU and writes the consumer's operand planes, so a normalised
activation is written exactly once, in the format the next K loop copies into LDS.  conv3 of a bottleneck never writes
its fp32 output when its batch statistics are known beforehand (the statistics pass of round 3, the input-side Gram
statistics of round 4): BN + shortcut + ReLU + split then run in the conv's own epilogue (`*_tail`, `*_tail_proj`).
Activations live in a few reusable arenas (about 1.2 GB at batch 32), so consecutive layers hit the 256 MiB Infinity
Cache instead of streaming 6.5 GB of distinct tensors.
"""
from collections import OrderedDict, namedtuple

import numpy as np
import torch

from . import ops
from .model import Model, flat_ptr, load_state_file  # noqa: F401  (load_state_file: imported from here by callers)
from .params import Var, up4

BLOCKS = (("block1", 64, 3, 1), ("block2", 128, 4, 2), ("block3", 256, 6, 2), ("block4", 512, 3, 1))
WEIGHT_DECAY = 5e-4   # resnet_arg_scope(weight_decay=5e-4), models/vision.py:54
BN_DECAY = 0.997
BN_EPS = 1e-5
PLANE_SLACK = 2 * 15 * 2048 * 2 + 512   # a split-format plane ends on a whole 16-pixel brick: <= 15 pixels more, twice

# The activation arenas of one pipeline stage.  a / b: the unit inputs and outputs, ping-pong (split planes; fp32 in the
# f32 trunk); p1 / p2: the split planes conv2 / conv3 read (None in the f32 trunk); r1 / r2 / r3 / sc: the raw fp32
# outputs of conv1 / conv2 / conv3 / the projection shortcut.  tag: "" or "2", the stage's part of every lane name.
Stage = namedtuple("Stage", "tag a b p1 p2 r1 r2 r3 sc")


class ResNet50Model(Model):

    def __init__(self, input_shape=None, num_classes=None, precision="f16x3", stages=None, stage_cut=8, side_lane=True,
                 two_pass=True, two_pass_max_cin=256, gram=True):
        """precision: arithmetic of the frozen trunk convs — "f16x3" (split-fp16 MFMA, fp32-class
        results, default), "f32" (exact-f32 MFMA) or "f16" (fp16 OPERAND STORAGE: the same data path, but the 52 trunk
        convs fetch and multiply only the hi fp16 plane of activations and weights — one MFMA per product, fp32
        accumulation, fp32 batch-norm statistics; BASELINE configs[4]'s "fp16 with fp32 loss accumulation").  With
        "f16x3" / "f16" the stem runs as a row-run conv and conv_map as a tap GEMM on the split-MFMA kernels
        (_stem_bn, _conv_map_tap; those two layers keep the three-term product)."""
        self.scope = 'resnet_v1_50'
        assert precision in ("f16x3", "f32", "f16")
        self.precision = precision
        self._split = precision in ("f16x3", "f16")
        self._terms = 1 if precision == "f16" else 3
        # stages = 2: the frozen trunk is recorded as TWO pipeline stages (units 1-8 | units 9-16) with an activation
        # arena, a statistics buffer and a tail workspace each and a dedicated boundary tensor, so that the trainer can
        # run stage 1 of batch t + 2 beside stage 2 of batch t + 1 (Trainer.train_step_pipelined): two trunk kernels of
        # different depth fill each other's partial last rounds.  stages = 1: one arena; the four projection shortcuts
        # then run on the plan's side lane beside conv1 .. conv3 (with two stages the stage streams take that role and
        # the 4 hardware queues are spent on the pipeline's lanes).
        if stages is None:
            stages = 2 if precision in ("f16x3", "f16") else 1
        assert stages in (1, 2)
        if precision not in ("f16x3", "f16"):
            stages = 1
        self.stages = stages
        # units in stage 1: 8 = blocks 1 + 2 + the first unit of block 3 (measured: 5: 7.53, 6: 7.30, 7: 7.18, 8: 7.06,
        # 9: 7.19 ms/step; the two trunk stages and the trained part should take about the same time)
        # (constructor arguments, not environment variables: stages, stage_cut, side_lane)
        self.STAGE_CUT = int(stage_cut)
        self.side_lane = bool(side_lane) and stages == 1
        # two_pass: conv3 of the identity units runs twice - statistics only, then again with BN + shortcut + ReLU + split
        # in its epilogue (ops.conv2d_fwd_split3p_stats / _tail) - instead of conv + bn_add_relu_split: the unit's widest
        # tensor never exists in fp32 (f16x3 only; units with a subsampled shortcut and the last unit keep the pass)
        self.two_pass = bool(two_pass) and precision == "f16x3"
        # widest conv3 INPUT that takes the two passes: with the chip to itself the second K loop pays up to 128 channels; in
        # the pipelined step, where three lanes share HBM, 256 is as fast (6.617 vs 6.632 ms, three alternating runs each:
        # profiles/r03/pipeline_two_pass_rule_r03ao.txt) and moves 1.4 GB less per step; 512 is slower (6.656 ms)
        self.two_pass_max_cin = int(two_pass_max_cin)
        # gram (round 4): the statistics of those conv3 layers come from the Gram matrix of the conv's INPUT
        # (ops.gram_stats: P C^2 MACs at two MFMAs per product + two small launches) instead of a statistics pass that
        # repeats the conv's K loop (4 P C^2 MACs at three): the conv then runs ONCE, with the fused tail.  False = round
        # 3's two K loops (kept for the A/B tables and the bit-exactness tests of the pass form).
        self.gram = bool(gram) and self.two_pass
        self._ctor = dict(input_shape=list(input_shape), num_classes=num_classes, precision=precision, stages=stages,
                          stage_cut=int(stage_cut), side_lane=bool(side_lane), two_pass=bool(two_pass),
                          two_pass_max_cin=int(two_pass_max_cin), gram=bool(gram))
        self.num_classes = num_classes
        self.height = input_shape[0]
        self.width = input_shape[1]
        self.channels = input_shape[2]
        if num_classes is not None:
            raise NotImplementedError("the logits layer is not on the acoustic-image path (num_classes=None)")
        self.session = None
        self.output = None
        self.network = None
        # marks in plan_train, set while it is recorded (the trainer's pipeline cuts the plan there): the calls
        # [0, frozen_calls) are the frozen trunk; with two stages, stage 2 begins at stage_calls and has read the boundary
        # tensor by stage_read_calls.  None: not marked (only the split trunk marks its end, only two stages a boundary)
        self.frozen_calls = None
        self.stage_calls = None
        self.stage_read_calls = None

    def clone_kwargs(self):
        """constructor arguments of a second instance that records the same plan shape (Model.replica: another batch
        size over the same variables)"""
        return dict(self._ctor)

    # ---- variable inventory (TF names) --------------------------------------------------------------
    def _units(self):
        depth_in = 64
        for name, base, n, stride in BLOCKS:
            for u in range(n):
                s = stride if u == n - 1 else 1
                yield ("%s/%s/unit_%d/bottleneck_v1" % (self.scope, name, u + 1), depth_in, base * 4, base, s)
                depth_in = base * 4

    def _conv_layers(self):
        yield (self.scope + "/conv1", 7, 7, 3, 64)
        for scope, din, d, db, s in self._units():
            if din != d:
                yield (scope + "/shortcut", 1, 1, din, d)
            yield (scope + "/conv1", 1, 1, din, db)
            yield (scope + "/conv2", 3, 3, db, db)
            yield (scope + "/conv3", 1, 1, db, d)
        yield (self.scope + "/conv_map", 3, 4, 2048, 12)

    def _register(self, store):
        cm = self.scope + "/conv_map"
        # trainable first (conv_map/* is in the optimiser's var_list, trainer/mfcctrainer.py:64)
        store.add(Var(cm + "/weights", (3, 4, 2048, 12), "conv", "train"))
        store.add(Var(cm + "/BatchNorm/gamma", (12,), "vec", "train"))
        store.add(Var(cm + "/BatchNorm/beta", (12,), "vec", "train"))
        store.add(Var(cm + "/BatchNorm/moving_mean", (12,), "vec", "state"))
        store.add(Var(cm + "/BatchNorm/moving_variance", (12,), "vec", "state"))
        for scope, kh, kw, cin, cout in self._conv_layers():
            if scope == cm:
                continue
            store.add(Var(scope + "/weights", (kh, kw, cin, cout), "conv", "trunkw"))
            for sfx in ("gamma", "beta", "moving_mean", "moving_variance"):
                store.add(Var(scope + "/BatchNorm/" + sfx, (cout,), "vec", "state"))

    # ---- reference protocol ------------------------------------------------------------------------
    def init_model(self, session, checkpoint_file):
        """Initialise from a TF-named state dict, everything except logits / conv_map
        (models/vision.py:20-42).  checkpoint_file: path to .npz / torch file, or a dict."""
        state = load_state_file(checkpoint_file)
        store = (session or self.session).store
        return store.load_state(state, strict=False,
                                only=lambda n: n.startswith(self.scope + "/") and "/logits" not in n and "/conv_map" not in n)

    def initialize(self, seed=1238):
        """slim defaults: variance_scaling_initializer conv kernels, gamma 1, beta 0, moving 0/1"""
        g = torch.Generator().manual_seed(seed)
        state = OrderedDict()
        for scope, kh, kw, cin, cout in self._conv_layers():
            fan_in = kh * kw * cin
            t = torch.randn(kh, kw, cin, cout, generator=g, dtype=torch.float64).clamp_(-2, 2)
            state[scope + "/weights"] = (t * np.sqrt(1.3 * 2.0 / fan_in)).float()
            state[scope + "/BatchNorm/gamma"] = torch.ones(cout)
            state[scope + "/BatchNorm/beta"] = torch.zeros(cout)
            state[scope + "/BatchNorm/moving_mean"] = torch.zeros(cout)
            state[scope + "/BatchNorm/moving_variance"] = torch.ones(cout)
        self._load_scope(state)

    def _build_model(self, visual_images, session=None):
        """visual_images: device buffer [N,224,298,3] float32 (the feed target).  Records the forward
        plans (training / inference BN mode) and the conv_map backward plan."""
        sess = self._attach(session)
        N = visual_images.shape[0]
        assert tuple(visual_images.shape[1:]) == (self.height, self.width, self.channels)
        self.N = N
        self._alloc(sess, visual_images)
        self.plan_train = sess.new_plan()
        self.plan_eval = sess.new_plan()
        self._record_forward(self.plan_train, True)
        self._record_forward(self.plan_eval, False)
        self._alloc_reserved()
        self.network = OrderedDict(input=visual_images, is_training=None, keep_prob=None)
        self.network[self.scope + "/conv_map"] = self.output
        cm = self.scope + "/conv_map"
        self.train_vars = [cm + "/weights", cm + "/BatchNorm/gamma", cm + "/BatchNorm/beta"]
        self.train_vars2 = [n for n, v in sess.store.vars.items()
                            if v.group == "trunkw" or (v.group == "state" and n.endswith(("gamma", "beta")))]

    # ---- buffers -------------------------------------------------------------------------------------
    def _alloc(self, sess, images):
        N, H, W = self.N, self.height, self.width
        z = sess.zeros
        self.images = images
        self.xpad = z(N, H, W, 4)
        oh1, ow1 = (H + 6 - 7) // 2 + 1, (W + 6 - 7) // 2 + 1
        self.stem_hw = (oh1, ow1)
        self.raw0 = z(N, oh1, ow1, 64)
        ph, _ = ops.same_out_pad(oh1, 3, 2)
        pw, _ = ops.same_out_pad(ow1, 3, 2)
        self.pool_hw = (ph, pw)
        # arena sizes in elements, [io, r1, r2, r3]: over all units, and over the units of stage 2 alone, which only ever
        # holds unit outputs in its io planes (its first input is the boundary tensor, `xb` elements)
        two = self.stages == 2
        h, w = ph, pw
        mx, mx2, xb = [N * h * w * 64, 0, 0, 0], [0, 0, 0, 0], 0
        nch = 64
        for k, (scope, din, d, db, s) in enumerate(self._units()):
            oh, _ = ops.same_out_pad(h, 1, s)
            ow, _ = ops.same_out_pad(w, 1, s)
            r = [N * h * w * db, N * oh * ow * db, N * oh * ow * d]
            mx = [max(a, b) for a, b in zip(mx, [max(N * h * w * din, N * oh * ow * d)] + r)]
            if two and k == self.STAGE_CUT - 1:
                xb = N * oh * ow * d
            if two and k >= self.STAGE_CUT:
                mx2 = [max(a, b) for a, b in zip(mx2, [N * oh * ow * d] + r)]
            h, w = oh, ow
            nch += (d if din != d else 0) + 2 * db + d
        self.final_hw = (h, w)
        io32 = (z(mx[0]), z(mx[0]))
        raw = [z(mx[1]), z(mx[2]), z(mx[3]), z(mx[3])]
        if not self._split:
            self.arenas = [Stage("", io32[0], io32[1], None, None, *raw)]
        else:
            # split-format arenas (two fp16 planes per tensor = the bytes of the fp32 tensor); stage 1 keeps the size of
            # the one-stage trunk, stage 2 has its own (sized for its units), the boundary tensor crosses between them
            u8 = lambda n: torch.zeros(int(4 * n + PLANE_SLACK), dtype=torch.uint8, device=sess.device)  # noqa: E731
            self._io32 = io32       # the split trunk has no fp32 unit outputs: allocated as ever, used by nothing
            self.arenas = [Stage("", u8(mx[0]), u8(mx[0]), u8(mx[1]), u8(mx[2]), *raw)]
            if two:
                self.planes_x = u8(xb)
                planes2 = [u8(mx2[0]), u8(mx2[0]), u8(mx2[1]), u8(mx2[2])]
                self.arenas.append(Stage("2", *planes2, z(mx2[1]), z(mx2[2]), z(mx2[3]), z(mx2[3])))
        self.xfinal = z(N, h, w, 2048)          # block4 output, kept for the conv_map weight gradient
        self.affine = z(2 * (nch + 64 + 16))    # scale/shift of every BN layer
        self._aff_off = 0
        self._aff_cache = {}                    # scope -> (scale, shift), slices of `affine`
        fh, fw = h - 3 + 1, w - 4 + 1
        self.feat_hw = (fh, fw)
        self.raw_cm = z(N, fh, fw, 12)
        self.output = z(N, fh, fw, 12)
        self.save_mean = z(16)
        self.save_invstd = z(16)
        self.g_output = z(N, fh, fw, 12)        # filled by the generator's backward (min-max bwd)
        self.g_raw_cm = z(N, fh, fw, 12)
        # per-lane buffers, (kind, lane) -> tensor.  A lane is what may run at the same time as another: a pipeline stage
        # ("" / "2"), its side lane ("_side" + stage), and conv_map ("cm": the first layer of the TRAINED part of the step,
        # which the two-lane pipeline of acimg/trainer.py runs beside the frozen trunk of the next batch).  Every lane has
        # a statistics buffer ("stats", floats: `_lane_stats`), a tail workspace and a Gram workspace ("tail" / "gram",
        # bytes: `_lane_ws`) of its own; two lanes never share one
        self.lane_bufs = {}
        self._stats_need = {}                   # lane -> floats its statistics buffer must hold (_alloc_reserved)
        if self._split:
            # stem as a row-run conv on the split-MFMA kernel: zero-padded 4-channel frame (+ slack for the last run),
            # kernel re-laid as [7][32 = 7 pixels x 4 channels + 4 zero rows][64]
            self.stem_frame = z(N * (H + 6) * (W + 6) * 4 + 64)
            self.stem_w = z(7, 1, 32, 64)
            self._stem_d = ops.conv_desc(N, H + 6, W + 6, 32, 64, 7, 1, 2, "VALID", ldx=4, ldy=64, ldw=64)
            self._stem_d.OH, self._stem_d.OW = oh1, ow1
            # conv_map as a tap GEMM (ops.tapconv_*): packed kernel, its split image, per-input-pixel products
            self._cm_d = ops.conv_desc(N, h, w, 2048, 12, 3, 4, 1, "VALID", ldx=2048, ldy=12, ldw=12)
            self._cm_d1 = ops.conv_desc(N, h, w, 2048, 144, 1, 1, 1, "SAME", ldx=2048, ldy=144, ldw=144)
            self.cm_wt = z(2048, 144)
            self.cm_wsplit = torch.zeros(int(ops.conv2d_split3_weight_bytes(self._cm_d1)), dtype=torch.uint8,
                                         device=sess.device)
            self.cm_z = z(N * h * w, 144)
            self.cm_gz = z(N * h * w, 144)
            self.cm_dwt = z(2048, 144)
        # f16x3: split + transposed copies of the frozen kernels (`_split_image`), refreshed when the store changes
        self._sp3 = {}
        self._sp3_bytes = 0
        self._sp3_version = -1
        self.plan_prepare = sess.new_plan()
        self.wsplit = None                      # _alloc_reserved
        # sum of squares of the frozen kernels (record_regularizer)
        self._trunk_ss = None
        self._trunk_ss_version = -1
        self._plan_reg = None

    def _alloc_reserved(self):
        """what the recorded calls reach through lazy pointers, once both forward plans have said how much they need: the
        split images of the frozen kernels and every lane's statistics buffer"""
        self.wsplit = torch.zeros(max(self._sp3_bytes, 16), dtype=torch.uint8, device=self.session.device)
        for lane, need in self._stats_need.items():
            self.lane_bufs["stats", lane] = self.session.zeros(need)

    def _lane_stats(self, lane, floats):
        """reserves `floats` floats of `lane`'s statistics buffer -> lazy pointer to it"""
        self._stats_need[lane] = max(self._stats_need.get(lane, 0), floats)
        return ops.LazyPtr(lambda: self.lane_bufs["stats", lane])

    def _lane_ws(self, kind, lane, nbytes):
        """`lane`'s workspace of `kind` ("tail" | "gram") with at least `nbytes` bytes, zero at start.  A tensor at once, not
        a lazy pointer: the call records its byte count.  One that is too small is replaced; a call recorded with the
        smaller one keeps the buffer it was recorded with."""
        ws = self.lane_bufs.get((kind, lane))
        if ws is None or ws.numel() < nbytes:
            ws = self.lane_bufs[kind, lane] = torch.zeros(nbytes, dtype=torch.uint8, device=self.session.device)
        return ws

    def _affine(self, scope, cout):
        """(scale, shift) of BN layer `scope`: two runs of `affine`, handed out on first use"""
        if scope not in self._aff_cache:
            c = up4(cout)
            self._aff_cache[scope] = (self.affine[self._aff_off:self._aff_off + c],
                                      self.affine[self._aff_off + c:self._aff_off + 2 * c])
            self._aff_off += 2 * c
            assert self._aff_off <= self.affine.numel()
        return self._aff_cache[scope]

    # ---- the steps every layer is recorded from ----------------------------------------------------------
    def _var(self, name):
        """variable `name` (full TF name) in the store's flat buffers, resolved once they exist"""
        st = self.session.store
        return ops.LazyPtr(lambda: st.p(name))

    def _grad(self, name):
        st = self.session.store
        return ops.LazyPtr(lambda: st.g(name))

    def _split_image(self, scope, d, w=None):
        """the split image of frozen kernel `scope` (w: its fp32 source, default the variable `scope`/weights): a run of
        `wsplit`, registered on first use, when its prepare launch joins `plan_prepare` -> lazy pointer"""
        if scope not in self._sp3:
            off = self._sp3[scope] = self._sp3_bytes
            self._sp3_bytes += -(-ops.conv2d_split3_weight_bytes(d) // 256) * 256
            ops.conv2d_split3_prepare(self.plan_prepare, d, w if w is not None else self._var(scope + "/weights"),
                                      ops.LazyPtr(lambda: self.wsplit[off:]))
        off = self._sp3[scope]
        return ops.LazyPtr(lambda: self.wsplit[off:])

    def _bn_finalize(self, plan, scope, cout, stats, rows, count, training, save=False, side=False):
        """statistics partials (training) or the moving statistics -> (scale, shift) of BN layer `scope`.  save: keep the
        batch mean / inverse deviation for the backward pass (conv_map); side: on the plan's side lane"""
        sc, sh = self._affine(scope, cout)
        b = scope + "/BatchNorm/"
        ops.bn_finalize(plan, stats if training else None, rows if training else 0, cout, up4(cout),
                        count if training else 0, self._var(b + "gamma"), self._var(b + "beta"),
                        self._var(b + "moving_mean"), self._var(b + "moving_variance"), sc, sh, BN_DECAY, BN_EPS, training,
                        self.save_mean if save else None, self.save_invstd if save else None, side=side)
        return sc, sh

    def _refresh_split_weights(self):
        """host hook at the head of the forward plans: re-split the frozen kernels iff they changed"""
        st = self.session.store
        if self._sp3_bytes and self._sp3_version != st.version:
            if self._split:      # [7][7][4][64] -> [7][28 of 32][64] (parameter plumbing, load time only)
                self.stem_w.view(7, 32, 64)[:, :28].copy_(st.p(self.scope + "/conv1/weights").reshape(7, 28, 64))
            self.plan_prepare.run()
            self._sp3_version = st.version

    @staticmethod
    def _lo_off(rows, c):
        """byte offset of the lo plane of a [rows, c] split-format tensor = acimg_split_plane_bytes(rows, c): planes are
        whole 16-pixel x 32-channel bricks (include/acimg.h, pre-split activation format)"""
        return -(-rows // 16) * 16 * c * 2

    # ---- plan recording ------------------------------------------------------------------------------
    def _conv_bn(self, plan, scope, x, hw, cin, kh, kw, cout, stride, padding, out, in_aff, training,
                 save=False):
        """raw conv + BN statistics -> (scale, shift) of this layer, exact f32 (the f32 trunk; the f16x3 / f16 trunk goes
        through _conv_bn_planes, _stem_bn and _conv_map_tap); returns (OH, OW, scale, shift)"""
        d = ops.conv_desc(self.N, hw[0], hw[1], cin, cout, kh, kw, stride, padding, ldx=cin, ldy=up4(cout),
                          ldw=up4(cout))
        rows = ops.conv2d_stats_rows(d)
        stats = self._lane_stats("", rows * 2 * up4(cout))
        isc, ish = (in_aff if in_aff is not None else (None, None))
        ops.conv2d_fwd(plan, d, x, self._var(scope + "/weights"), None, out, isc, ish, 1, stats if training else None)
        sc, sh = self._bn_finalize(plan, scope, cout, stats, rows, self.N * d.OH * d.OW, training, save=save)
        return d.OH, d.OW, sc, sh

    def _conv_bn_planes(self, plan, scope, xplanes, hw, cin, kh, kw, cout, stride, padding, out, training, side=False,
                        tag=""):
        """like _conv_bn, for an input in split format (pre-normalised fp16 hi/lo planes).  side: conv + finalize on the
        plan's side lane (the projection shortcut beside conv1..conv3 of its unit); tag "2": second pipeline stage.
        Every (stage, lane) pair has a statistics buffer and a tail workspace (tickets) of its own: they may run at the
        same time"""
        d = ops.conv_desc(self.N, hw[0], hw[1], cin, cout, kh, kw, stride, padding, ldx=cin, ldy=up4(cout),
                          ldw=up4(cout))
        rows = ops.conv2d_fwd_split3p_stats_rows(d) if self._terms == 3 else ops.conv2d_fwd_split3_stats_rows(d)
        lane = ("_side" if side else "") + tag
        stats = self._lane_stats(lane, rows * 2 * up4(cout))
        # partial sums + tile tickets of the trunk kernel's tail split; used by nothing else
        # (recording the staged trunk WITHOUT the tail split — the other stages fill the partial last rounds anyway —
        #  was measured: 7.21 -> 7.13 ms/step pipelined, but 8.96 -> 9.22 ms on one stream and 249 -> 223 TFLOP/s for
        #  the kernel with the chip to itself; the plan is shared by both entry points, so the split stays)
        tail_ws = self._lane_ws("tail", lane, ops.conv2d_fwd_split3p_workspace(d))
        ops.conv2d_fwd_split3p(plan, d, xplanes, self._lo_off(self.N * hw[0] * hw[1], cin), self._split_image(scope, d),
                               out, stats if training else None, tail_ws=tail_ws, terms=self._terms, side=side)
        sc, sh = self._bn_finalize(plan, scope, cout, stats, rows, self.N * d.OH * d.OW, training, side=side)
        return d.OH, d.OW, sc, sh

    def _conv3_two_pass(self, plan, scope, xplanes, hw, cin, cout, sc_planes, out_planes, training, tag="", proj=None):
        """conv3 of a unit without its raw output (include/acimg.h, acimg_conv2d_fwd_split3p_stats / _tail / _tail_proj):
        [statistics pass ->] bn_finalize -> the conv again with relu(BN + shortcut) + split in the epilogue.  In inference
        mode the affine comes from the moving statistics and the first pass is not needed.  proj = (raw fp32 output of the
        unit's shortcut conv, its scale, its shift) for a unit with a projection shortcut, else the identity shortcut is
        read from `sc_planes`."""
        d = ops.conv_desc(self.N, hw[0], hw[1], cin, cout, 1, 1, 1, "SAME", ldx=cin, ldy=cout, ldw=cout)
        M = self.N * hw[0] * hw[1]
        rows = -(-M // 128)
        stats = self._lane_stats(tag, rows * 2 * cout)
        wsplit = self._split_image(scope, d)
        tail_ws = self._lane_ws("tail", tag, ops.conv2d_fwd_split3p_workspace(d))
        lo = self._lo_off(M, cin)
        lo_out = self._lo_off(M, cout)
        if training and self.gram and ops.gram_stats_workspace(M, cin) > 0:
            # statistics from the conv's input (one workspace per pipeline stage: the stages run side by side)
            sc, sh = self._affine(scope, cout)
            b = scope + "/BatchNorm/"
            ops.gram_stats(plan, xplanes, lo, M, cin, self._var(scope + "/weights"), cout, cout, self._var(b + "gamma"),
                           self._var(b + "beta"), self._var(b + "moving_mean"), self._var(b + "moving_variance"), sc, sh,
                           self._lane_ws("gram", tag, ops.gram_stats_workspace(M, cin)), BN_DECAY, BN_EPS)
        else:
            if training:
                ops.conv2d_fwd_split3p_stats(plan, d, xplanes, lo, wsplit, stats, tail_ws=tail_ws)
            sc, sh = self._bn_finalize(plan, scope, cout, stats, rows, M, training)
        if proj is not None:
            ops.conv2d_fwd_split3p_tail_proj(plan, d, xplanes, lo, wsplit, sc, sh, proj[0], proj[1], proj[2], out_planes,
                                             lo_out, tail_ws=tail_ws)
        else:
            ops.conv2d_fwd_split3p_tail(plan, d, xplanes, lo, wsplit, sc, sh, sc_planes, lo_out, out_planes, lo_out,
                                        tail_ws=tail_ws)

    def _two_pass_ok(self, hw, cin, cout):
        """measured per shape at batch 32 (profiles/r03/op_report_two_pass_all_r03u.txt): the statistics pass costs 85-95 %
        of the conv it repeats once K >= 256 (the K loop, not the output, is its time), so the second K loop only pays
        for the short-K / large-image units: 56x75 64->256 113 -> 84 us, 128->512 247 -> 192 us per unit, against
        28x38 256->1024 130 -> 144 and 14x19 512->2048 94 -> 121"""
        M = self.N * hw[0] * hw[1]
        if not (self.two_pass and self._terms == 3 and cin <= self.two_pass_max_cin and cout % 128 == 0 and
                M * cout * 4 < 2 ** 31):
            return False
        # the library's own tile choice for this shape under the current configuration (a forced experiment tile, or
        # fewer than 200 tiles, takes the unit back to conv + bn_add_relu_split)
        d = ops.conv_desc(self.N, hw[0], hw[1], cin, cout, 1, 1, 1, "SAME", ldx=cin, ldy=cout, ldw=cout)
        return tuple(ops.conv2d_fwd_split3_tiling(d)[:2]) == (128, 128)

    def _record_forward_split(self, plan, training):
        """f16x3 trunk: activations between convs live in split format.  Per bottleneck unit:
             conv1(X) -> raw1 -> [BN+ReLU+split] -> conv2 -> raw2 -> [BN+ReLU+split] -> conv3 -> raw3
             out = relu(BN(raw3) + shortcut) written straight in split format (next unit's X)."""
        N = self.N
        H, W = self.height, self.width
        plan.add_hook(self._refresh_split_weights)
        ops.pad_image(plan, self.images, self.stem_frame, N, H, W, 3, 4, H + 6, W + 6, 3, 3)
        oh, ow, sc, sh = self._stem_bn(plan, training)
        ph, pw = self.pool_hw
        _, pt = ops.same_out_pad(oh, 3, 2)
        _, pl = ops.same_out_pad(ow, 3, 2)
        cur, nxt = self.arenas[0].a, self.arenas[0].b
        ops.bn_relu_maxpool_split(plan, self.raw0, sc, sh, cur, self._lo_off(N * ph * pw, 64), N, oh, ow, 64, ph, pw,
                                  pt, pl)
        h, w = ph, pw
        units = list(self._units())
        # (without two stages no unit is the first of stage 2 or the last of stage 1)
        first2, last1 = (self.STAGE_CUT, self.STAGE_CUT - 1) if self.stages == 2 else (None, None)
        for i, (scope, din, d, db, s) in enumerate(units):
            last = i == len(units) - 1
            st = self.arenas[1 if first2 is not None and i >= first2 else 0]
            if i == first2:
                # stage 2 starts here: it reads the boundary tensor and ping-pongs inside its own arena
                if training:
                    self.stage_calls = len(plan.calls)
                cur, nxt = self.planes_x, st.a
            nxt_out = self.planes_x if i == last1 else nxt      # the last unit of stage 1 writes the boundary tensor

            def shortcut_conv(side):
                """the unit's projection shortcut -> (its raw fp32 output, scale, shift)"""
                _, _, ssc, tsc = self._conv_bn_planes(plan, scope + "/shortcut", cur, (h, w), din, 1, 1, d, s, "SAME",
                                                      st.sc, training, side=side, tag=st.tag)
                return st.sc, ssc, tsc

            beside = din != d and self.side_lane
            if beside:
                # the projection shortcut reads the same planes as conv1 and meets the main branch only in the unit's
                # last pass: it runs on the plan's side lane beside conv1 .. conv3 (their tails leave slots)
                plan.fork()
                forked = shortcut_conv(True)

            def shortcut():
                """where the main branch needs the projection shortcut: join the side lane, or record the conv in place;
                None for an identity unit"""
                if din == d:
                    return None
                if beside:
                    plan.join()
                    return forked
                return shortcut_conv(False)

            oh1, ow1, s1, t1 = self._conv_bn_planes(plan, scope + "/conv1", cur, (h, w), din, 1, 1, db, 1, "SAME",
                                                    st.r1, training, tag=st.tag)
            ops.bn_relu_split(plan, st.r1, s1, t1, 1, st.p1, self._lo_off(N * h * w, db), N * h * w, db)
            oh2, ow2, s2, t2 = self._conv_bn_planes(plan, scope + "/conv2", st.p1, (h, w), db, 3, 3, db, s,
                                                    "SAME" if s == 1 else 1, st.r2, training, tag=st.tag)
            ops.bn_relu_split(plan, st.r2, s2, t2, 1, st.p2, self._lo_off(N * oh2 * ow2, db), N * oh2 * ow2, db)
            if s == 1 and not last and self._two_pass_ok((oh2, ow2), db, d):
                # conv3 twice: the raw [N, oh, ow, d] tensor and its BN pass never exist (the shortcut is recorded first)
                self._conv3_two_pass(plan, scope + "/conv3", st.p2, (oh2, ow2), db, d, cur, nxt_out, training, tag=st.tag,
                                     proj=shortcut())
            else:
                # (conv3 is recorded before a shortcut conv in place: the order of the recorded calls is pinned)
                _, _, s3, t3 = self._conv_bn_planes(plan, scope + "/conv3", st.p2, (oh2, ow2), db, 1, 1, d, 1, "SAME",
                                                    st.r3, training, tag=st.tag)
                out_planes = None if last else nxt_out
                out_lo = 0 if last else self._lo_off(N * oh2 * ow2, d)
                out32 = self.xfinal if last else None
                proj = shortcut()
                if proj is not None:
                    ops.bn_add_relu_split(plan, st.r3, s3, t3, proj[0], proj[1], proj[2], None, 0, out_planes, out_lo,
                                          out32, N, oh2, ow2, d, oh2, ow2, 1)
                else:
                    ops.bn_add_relu_split(plan, st.r3, s3, t3, None, None, None, cur, self._lo_off(N * h * w, din),
                                          out_planes, out_lo, out32, N, oh2, ow2, d, h, w, s)
            h, w = oh2, ow2
            if i == first2:
                if training:
                    self.stage_read_calls = len(plan.calls)  # stage 2 no longer reads the boundary tensor from here on
                cur, nxt = st.a, st.b
            else:
                cur, nxt = nxt, cur
        fh, fw = self.feat_hw
        if training:
            # everything recorded so far is the FROZEN trunk (no trainable variable is read): the trainer may run it
            # for the next batch beside the trained part of the current one; the last call writes `xfinal`
            self.frozen_calls = len(plan.calls)
        scm, tcm = self._conv_map_tap(plan, training)
        ops.bn_relu(plan, self.raw_cm, scm, tcm, self.output, N * fh * fw, 12, 12, 12)

    def _stem_bn(self, plan, training):
        """conv1 (7x7/2 after 3+3 explicit zero padding) + BN statistics as a row-run conv (include/acimg.h,
        acimg_conv2d_fwd_split3) on the split-MFMA kernel"""
        scope = self.scope + "/conv1"
        d = self._stem_d
        rows = ops.conv2d_fwd_split3_stats_rows(d)
        stats = self._lane_stats("", rows * 2 * 64)
        ops.conv2d_fwd_split3(plan, d, self.stem_frame, self._split_image(scope, d, self.stem_w), self.raw0,
                              None, None, 0, stats if training else None)
        sc, sh = self._bn_finalize(plan, scope, 64, stats, rows, self.N * d.OH * d.OW, training)
        return d.OH, d.OW, sc, sh

    def _conv_map_tap(self, plan, training):
        """conv_map (3x4 VALID, 2048 -> 12) + BN statistics on the split-MFMA path: one GEMM over the INPUT pixels
        with 12 taps x 12 channels = 144 columns, then a 12-tap gather (ops.tapconv_*); the kernel trains, so its
        packed / split image is rebuilt in the plan (two tiny launches)"""
        cm = self.scope + "/conv_map"
        d, d1 = self._cm_d, self._cm_d1
        fh, fw = self.feat_hw
        ops.tapconv_pack(plan, d, self._var(cm + "/weights"), self.cm_wt, 144)
        ops.conv2d_split3_prepare(plan, d1, self.cm_wt, self.cm_wsplit)
        ops.conv2d_fwd_split3(plan, d1, self.xfinal, self.cm_wsplit, self.cm_z)
        rows = ops.tapconv_stats_rows(d)
        stats = self._lane_stats("cm", rows * 2 * 12)       # a lane of its own: see _alloc
        ops.tapconv_gather(plan, d, self.cm_z, 144, self.raw_cm, stats if training else None)
        return self._bn_finalize(plan, cm, 12, stats, rows, self.N * fh * fw, training, save=True)

    def _record_forward(self, plan, training):
        if self._split:
            return self._record_forward_split(plan, training)
        N = self.N
        H, W = self.height, self.width
        st = self.arenas[0]
        plan.add_hook(self._refresh_split_weights)
        ops.pad_channels(plan, self.images, self.xpad, N * H * W, 3, 4)
        oh, ow, sc, sh = self._conv_bn(plan, self.scope + "/conv1", self.xpad, (H, W), 4, 7, 7, 64, 2, 3,
                                       self.raw0, None, training)
        ph, pw = self.pool_hw
        _, pt = ops.same_out_pad(oh, 3, 2)
        _, pl = ops.same_out_pad(ow, 3, 2)
        cur, nxt = st.a, st.b
        ops.bn_relu_maxpool(plan, self.raw0, sc, sh, cur, N, oh, ow, 64, ph, pw, pt, pl)
        h, w = ph, pw
        units = list(self._units())
        for i, (scope, din, d, db, s) in enumerate(units):
            last = i == len(units) - 1
            oh1, ow1, s1, t1 = self._conv_bn(plan, scope + "/conv1", cur, (h, w), din, 1, 1, db, 1, "SAME",
                                             st.r1, None, training)
            oh2, ow2, s2, t2 = self._conv_bn(plan, scope + "/conv2", st.r1, (h, w), db, 3, 3, db, s,
                                             "SAME" if s == 1 else 1, st.r2, (s1, t1), training)
            oh3, ow3, s3, t3 = self._conv_bn(plan, scope + "/conv3", st.r2, (oh2, ow2), db, 1, 1, d, 1,
                                             "SAME", st.r3, (s2, t2), training)
            out = self.xfinal if last else nxt
            if din != d:
                _, _, ssc, tsc = self._conv_bn(plan, scope + "/shortcut", cur, (h, w), din, 1, 1, d, s, "SAME",
                                               st.sc, None, training)
                ops.bn_add_relu(plan, st.r3, s3, t3, st.sc, ssc, tsc, out, N, oh3, ow3, d, oh3, ow3, 1)
            else:
                ops.bn_add_relu(plan, st.r3, s3, t3, cur, None, None, out, N, oh3, ow3, d, h, w, s)
            h, w = oh3, ow3
            if not last:
                cur, nxt = nxt, cur
        fh, fw = self.feat_hw
        _, _, scm, tcm = self._conv_bn(plan, self.scope + "/conv_map", self.xfinal, (h, w), 2048, 3, 4, 12, 1,
                                       "VALID", self.raw_cm, None, training, save=True)
        ops.bn_relu(plan, self.raw_cm, scm, tcm, self.output, N * fh * fw, 12, 12, 12)

    def record_backward(self, plan):
        """conv_map backward: g(output) -> BN/ReLU backward -> weight gradient (+ L2 term).  The trunk
        below conv_map receives no gradient (it is not in var_list, trainer/mfcctrainer.py:64)."""
        cm = self.scope + "/conv_map"
        N = self.N
        fh, fw = self.feat_hw
        h, w = self.final_hw
        ops.bn_relu_bwd(plan, self.raw_cm, self.output, self.g_output, self._var(cm + "/BatchNorm/gamma"),
                        self.save_mean, self.save_invstd, self.g_raw_cm, self._grad(cm + "/BatchNorm/gamma"),
                        self._grad(cm + "/BatchNorm/beta"), N * fh * fw, 12)
        if self._split:
            # tap-GEMM form: dWt[2048][144] = xfinal^T . (tap-scattered g_raw_cm), then back to HWIO + the L2 term
            ops.tapconv_scatter(plan, self._cm_d, self.g_raw_cm, 12, self.cm_gz, 144)
            ops.conv2d_wgrad_split3(plan, self._cm_d1, self.xfinal, self.cm_gz, 144, self.cm_dwt, None)
            ops.tapconv_unpack(plan, self._cm_d, self.cm_dwt, 144, self._var(cm + "/weights"), WEIGHT_DECAY,
                               self._grad(cm + "/weights"))
            return
        d = ops.conv_desc(N, h, w, 2048, 12, 3, 4, 1, "VALID", ldx=2048, ldy=12, ldw=12)
        ops.conv2d_wgrad(plan, d, self.xfinal, self.g_raw_cm, 12, self._grad(cm + "/weights"), None)
        ops.axpy(plan, WEIGHT_DECAY, self._var(cm + "/weights"), self._grad(cm + "/weights"), 3 * 4 * 2048 * 12)

    def record_regularizer(self, plan, accum):
        """adds sum(w^2) over every conv kernel of the scope into accum[0] (slim l2_regularizer terms
        collected by tf.losses.get_total_loss, trainer/mfcctrainer.py:60).  The trunk is frozen
        (trainer/mfcctrainer.py:64), so its 23.5 M-element sum is computed when the parameters are (re)loaded and
        only added here; conv_map trains and is summed every step."""
        st = self.session.store
        if self._trunk_ss is None:
            self._trunk_ss = self.session.zeros(4)
            self._plan_reg = self.session.new_plan()
            ops.zero(self._plan_reg, self._trunk_ss)
            ops.sumsq(self._plan_reg, flat_ptr(st, "trunkw"), st._sizes["trunkw"], self._trunk_ss)
        plan.add_hook(self._refresh_trunk_sumsq)
        ops.axpy(plan, 1.0, self._trunk_ss, accum, 1)
        ops.sumsq(plan, self._P("conv_map/weights"), 3 * 4 * 2048 * 12, accum)

    def _refresh_trunk_sumsq(self):
        st = self.session.store
        if self._trunk_ss_version != st.version:
            self._plan_reg.run()
            self._trunk_ss_version = st.version
