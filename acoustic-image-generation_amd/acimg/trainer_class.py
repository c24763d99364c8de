"""`TrainerClass`: the classification experiment of the reference, MI355X-native - DualCamNet trained and scored on
GENERATED acoustic images (trainer/trainer_reconstructed_class.py), on the REAL ones or on the tiled MFCC map
(trainer/trainer_class.py, `--mfcc 1` / `--mfcc 1 --mfccmap 1` in main.py:314-323).

source = "generated" mirrors trainer_reconstructed_class.py:14-75: ResNet-50 image encoder + `UNetAc` generator run in
inference mode (`is_training: 0`, :183-186), their output is viewed as clips of 12 frames (:44), DualCamNet
classifies each frame, logits are averaged per clip (:47-48), loss = tf.losses.softmax_cross_entropy (:49-54),
Adam on the `DualCamNet/` variables only (:58-70).  `train_step` is the body of the loop at :176-190.
source = "acoustic" / "mfccmap" mirror trainer_class.py:29-73: the same classifier, loss and optimiser on the loader's
acoustic images, or on tile(mfcc) (:39-45); no trunk or generator variable is registered or run.

One step = ONE recorded plan: [tile MFCC -> trunk forward (moving statistics) -> generator forward ->] DualCamNet
forward -> clip softmax-CE (+ gradient, + accuracy count) -> DualCamNet backward; then Adam over the contiguous
DualCamNet range of the flat parameter buffer.  A pass over a data set (`_evaluate`) runs the forward part followed by
`acimg_clip_eval`: loss sum, counters and the confusion matrix collect on the device and are read back once.
The loops, log lines, best-epoch rule and files are the reference's (:87-321 / trainer_class.py:84-314); checkpoints
are Saver-V2 bundles with the reference Saver's variable set.  Single GPU.
"""
import os
from collections import OrderedDict
from datetime import datetime

import torch

from . import ops
from .flags import FLAGS
from .params import up4
from .session import Graph, Session, draw_noise, scope_range, write_saver_bundle
from .unet_acresnet import Z

SOURCES = ("generated", "acoustic", "mfccmap")


def source_from_flags():
    """main.py:314-323: `--mfcc` selects the baseline trainer (trainer_class.py), which classifies the MFCC map under
    `--mfccmap` and the real acoustic images otherwise; without `--mfcc` the classifier sees generated images"""
    if FLAGS.mfcc:
        return "mfccmap" if FLAGS.mfccmap else "acoustic"
    return "generated"


class TrainerClass(object):

    def __init__(self, model, model_encoder_images, model_encoder_acoustic, display_freq=1, learning_rate=0.0001,
                 num_classes=14, num_epochs=1, nr_frames=12, temporal_pooling=False, session=None, source=None):
        """source: "generated" | "acoustic" | "mfccmap"; None = decided by FLAGS when the functions are built
        (`source_from_flags`: "generated" unless --mfcc).  The two encoders may be None for the baseline sources."""
        if source is not None and source not in SOURCES:
            raise ValueError("source is one of %r, got %r" % (SOURCES, source))
        self.model = model
        self.model_encoder_images = model_encoder_images
        self.model_encoder_acoustic = model_encoder_acoustic
        self.display_freq = display_freq
        self.learning_rate = learning_rate
        self.num_classes = num_classes
        self.num_epochs = num_epochs
        self.nr_frames = nr_frames
        self.temporal_pooling = temporal_pooling
        self.session = session
        self.source = source
        self.global_step = 0
        self.noise_seed = 1237
        self._noise_calls = 0           # draws of the latent noise so far: each takes a fresh Philox counter range
        self._saved = []                # the checkpoints _save_checkpoint keeps (Saver(max_to_keep=5))
        self.graphs = {}                # clips -> Graph
        self.evaluator = None
        self.last_evaluation = None     # `ClipEvaluator.result()` of the latest `_evaluate`
        self.log = print

    # ------------------------------------------------------------------------------------------------
    # graph construction
    # ------------------------------------------------------------------------------------------------
    def _build_functions(self, data=None, batch_size=None):
        """batch_size = number of FRAMES (a multiple of 12: clips of 12 consecutive frames); taken from `data` when not
        given: a clip-mode loader (embedding=0) counts clips, any other object frames"""
        if batch_size is None and getattr(data, "batch_size", None):
            batch_size = data.batch_size * (self.nr_frames if getattr(data, "embedding", 1) == 0 else 1)
        N = int(batch_size or 24)
        assert N % self.nr_frames == 0, "the frame batch must hold whole clips of %d frames" % self.nr_frames
        if self.source is None:
            self.source = source_from_flags()
        if self.source == "generated" and (self.model_encoder_images is None or self.model_encoder_acoustic is None):
            raise ValueError("source 'generated' needs the image encoder and the generator")
        if self.session is None:
            self.session = Session()
        from .evaluate import ClipEvaluator
        self.evaluator = ClipEvaluator(self.session.device, self.num_classes, self.nr_frames)
        mi, ma = (self.model_encoder_images, self.model_encoder_acoustic) if self.source == "generated" else (None, None)
        g = self._build_graph(N, self.model, mi, ma)
        self.session.finalize()
        # the DualCamNet variables are one contiguous run of the flat trainable buffer
        self.off, self.numel = scope_range(self.session.store, self.model.scope)
        g.off, g.numel = self.off, self.numel
        self.primary = g
        return g

    def _build_graph(self, N, m, mi, ma):
        sess = self.session
        z = sess.zeros
        g = Graph()
        g.N, g.clips = N, N // self.nr_frames
        g.model, g.model_encoder_images, g.model_encoder_acoustic = m, mi, ma
        g.labels = torch.zeros(g.clips, dtype=torch.int32, device=sess.device)
        fwd = sess.new_plan()           # everything up to the per-frame logits
        if self.source == "generated":
            g.mfcc = z(N, 12)
            g.video = z(N, 224, 298, 3)
            g.eps = z(N, Z)
            g.mfccmap = z(N, 36, 48, 12)
            mi._build_model(g.video, session=sess)
            ma._build_model(g.mfccmap, mi.output, session=sess, eps=g.eps)
            m._build_model(ma.output, session=sess)
            ops.tile_mfcc(fwd, g.mfcc, g.mfccmap, N, 36 * 48, 12)
            fwd.extend(mi.plan_eval)
            fwd.extend(ma.plan_fwd)
        elif self.source == "mfccmap":
            g.mfcc = z(N, 12)
            g.mfccmap = z(N, 36, 48, 12)
            m._build_model(g.mfccmap, session=sess)
            ops.tile_mfcc(fwd, g.mfcc, g.mfccmap, N, 36 * 48, 12)
        else:
            g.acoustic = z(N, 36, 48, 12)
            m._build_model(g.acoustic, session=sess)
        fwd.extend(m.plan_fwd)
        kp = up4(self.num_classes)
        g.out = z(4)                  # loss, #correct
        g.g_logits = z(N, kp)
        p = sess.new_plan()
        ops.zero(p, g.out)
        p.extend(fwd)
        e = sess.new_plan()
        e.extend(p)
        ops.clip_softmax_ce(p, m.logits, kp, g.clips, self.nr_frames, self.num_classes, g.labels, g.out, g.g_logits, kp)
        m.record_backward(p, g.g_logits)
        ops.clip_softmax_ce(e, m.logits, kp, g.clips, self.nr_frames, self.num_classes, g.labels, g.out, None, kp)
        self.evaluator.update(fwd, m.logits, kp, g.clips, g.labels)
        g.plan_train, g.plan_eval, g.plan_pass = p, e, fwd
        self.graphs[g.clips] = g
        return g

    def _graph_for(self, clips):
        """the graph of this clip count: another batch size (the last, partial batch) gets the same variables with new
        buffers and plans, as `Trainer._graph_for` does"""
        if clips in self.graphs:
            return self.graphs[clips]
        mi = ma = None
        if self.source == "generated":
            mi, ma = self.model_encoder_images.replica(), self.model_encoder_acoustic.replica()
        g = self._build_graph(clips * self.nr_frames, self.model.replica(), mi, ma)
        g.off, g.numel = self.off, self.numel
        return g

    # ------------------------------------------------------------------------------------------------
    # the step
    # ------------------------------------------------------------------------------------------------
    def _class_of(self, labels, clips):
        """int32 class per clip from class numbers [clips] or one-hot rows [clips, classes] (an all-zero row, which the
        loaders write for a class they do not know, becomes -1: no loss, no count)"""
        lab = torch.as_tensor(labels).reshape(clips, -1)
        if lab.shape[1] > 1:
            lab = torch.where(lab.sum(1) > 0, lab.argmax(1), torch.full_like(lab.argmax(1), -1))
        else:
            lab = lab[:, 0]
        return lab.to(torch.int32)

    def _split(self, batch):
        """(acoustic, mfcc, video, labels) of a step's batch: the 3-tuple (mfcc, video, labels) of the generated source,
        or what `_retrieve_batch` returns"""
        if len(batch) == 3:
            return (None,) + tuple(batch)
        acoustic, mfcc, video, labels = batch
        return acoustic, mfcc, video, labels

    def _clips_of(self, batch):
        acoustic, mfcc, _, _ = self._split(batch)
        rows = mfcc.reshape(-1, 12).shape[0] if mfcc is not None else acoustic.reshape(-1, 36, 48, 12).shape[0]
        if rows == 0 or rows % self.nr_frames:
            raise ValueError("a batch of %d frames is not whole clips of %d" % (rows, self.nr_frames))
        return rows // self.nr_frames

    def _feed(self, g, batch, eps):
        if batch is not None:
            acoustic, mfcc, video, labels = self._split(batch)
            if self.source == "acoustic":
                if acoustic is None:
                    raise ValueError("source 'acoustic' wants (acoustic, mfcc, video, labels) batches")
                g.acoustic.copy_(acoustic.reshape(g.N, 36, 48, 12), non_blocking=True)
            else:
                g.mfcc.copy_(mfcc.reshape(g.N, 12), non_blocking=True)
            if self.source == "generated":
                g.video.copy_(video.reshape(g.N, 224, 298, 3), non_blocking=True)
            g.labels.copy_(self._class_of(labels, g.clips), non_blocking=True)
        if self.source != "generated":
            return
        if eps is not None:
            g.eps.copy_(eps.reshape(g.N, Z), non_blocking=True)
        else:
            self._noise_calls += 1
            draw_noise(self.session, g.eps, self.noise_seed, self._noise_calls * 65536)

    def train_step(self, batch=None, eps=None):
        """batch: (mfcc [N,12], video [N,224,298,3], labels [clips] or one-hot [clips, classes]), or the 4-tuple of
        `_retrieve_batch`; None reuses the primary graph's resident inputs.  Returns {loss, accuracy}"""
        g = self.primary if batch is None else self._graph_for(self._clips_of(batch))
        self._feed(g, batch, eps)
        g.plan_train.run()
        self.global_step += 1
        self.session.adam_step(self.learning_rate, self.global_step, g.off, g.numel)
        v = g.out[:2].tolist()
        return OrderedDict(loss=v[0], accuracy=v[1] / g.clips)

    def eval_step(self, batch=None, eps=None):
        g = self.primary if batch is None else self._graph_for(self._clips_of(batch))
        self._feed(g, batch, eps)
        g.plan_eval.run()
        v = g.out[:2].tolist()
        return OrderedDict(loss=v[0], accuracy=v[1] / g.clips)

    # ------------------------------------------------------------------------------------------------
    # reference protocol: loops, checkpoints
    # ------------------------------------------------------------------------------------------------
    def _retrieve_batch(self, next_batch):
        """a loader tuple -> (acoustic [-1,12,36,48,12], mfcc [-1,12], images [-1,224,298,3], one-hot labels
        [-1, num_classes]) (:284-294, trainer_class.py:269-279): one label row per clip, so the loader runs in clip
        mode (embedding=0)"""
        if FLAGS.model == 'DualCamNet':
            mfcc = next_batch[1].reshape(-1, 12)
            images = next_batch[2].reshape(-1, 224, 298, 3)
            acoustic = next_batch[0].reshape(-1, 12, 36, 48, 12)
            labels = next_batch[3].reshape(-1, self.num_classes)
        else:
            raise ValueError('Unknown model type')
        if labels.shape[0] * self.nr_frames != mfcc.shape[0]:
            raise ValueError("%d label rows for %d frames: the classifier wants one row per clip of %d frames (a loader "
                             "with embedding=0)" % (labels.shape[0], mfcc.shape[0], self.nr_frames))
        return acoustic, mfcc, images, labels

    def _models(self):
        """the models whose variables this trainer's session holds, in initialisation order"""
        if self.source == "generated":
            return [self.model_encoder_images, self.model_encoder_acoustic, self.model]
        return [self.model]

    def _initialize(self):
        """`session.run(tf.global_variables_initializer())`: fresh weights, Adam slots and global_step"""
        for m in self._models():
            m.initialize()
        store = self.session.store
        store.adam_m.zero_()
        store.adam_v.zero_()
        self.global_step = 0

    def _load(self, checkpoint, models):
        from .model import load_state_file
        state = self.model._to_internal(load_state_file(checkpoint))
        scopes = tuple(m.scope + "/" for m in models)
        return self.session.store.load_state(state, strict=False, only=lambda n: n.startswith(scopes))

    def _init_model(self, session):
        """:87-109 / trainer_class.py:84-106"""
        if FLAGS.init_checkpoint is not None:
            if self.source != "generated":
                raise ValueError("--init_checkpoint holds the image encoder and the generator: source %r has neither "
                                 "(use --restore_checkpoint)" % self.source)
            self.log('{}: {} - Initializing session'.format(datetime.now(), FLAGS.exp_name))
            self._initialize()
            self._load(FLAGS.init_checkpoint, [self.model_encoder_images, self.model_encoder_acoustic])
            self.log('{}: {} - Done'.format(datetime.now(), FLAGS.exp_name))
        elif FLAGS.restore_checkpoint is not None:
            self._restore_model(session)
        else:
            self.log('{}: {} - Initializing full model'.format(datetime.now(), FLAGS.exp_name))
            self._initialize()
            self.log('{}: {} - Done'.format(datetime.now(), FLAGS.exp_name))

    def _restore_model(self, session):
        """model variables only - encoder, generator and classifier (:111-125), or the classifier alone
        (trainer_class.py:108-120); Adam slots and global_step start afresh"""
        self.log('{}: {} - Restoring session'.format(datetime.now(), FLAGS.exp_name))
        self._initialize()
        self._load(FLAGS.restore_checkpoint, self._models())
        self.log('{}: {} - Done'.format(datetime.now(), FLAGS.exp_name))

    def _save_checkpoint(self, session, epoch):
        """`self.saver.save(session, '<checkpoint_dir>/<exp_name>/epoch_<n>.ckpt')` (:237-243, Saver(max_to_keep=5),
        :75): every variable of the session under its TF name - `DualCamNet/conv1/weights` in its 5-D conv3d shape -
        the Adam slots of the DualCamNet variables, the beta powers and global_step"""
        checkpoint_dir = '{}/{}'.format(FLAGS.checkpoint_dir, FLAGS.exp_name)
        os.makedirs(checkpoint_dir, exist_ok=True)
        model_name = 'epoch_{}.ckpt'.format(epoch)
        self.log('{}: {} - Saving model to {}/{}'.format(datetime.now(), FLAGS.exp_name, checkpoint_dir, model_name))
        path = '{}/{}'.format(checkpoint_dir, model_name)
        scope = self.model.scope + "/"
        conv1 = scope + "conv1/weights"
        shapes = {conv1: tuple(self.model.state_dict_tf()[conv1].shape)}
        self._saved = write_saver_bundle(session.store, path, self.global_step, self._saved, 5,
                                         slots_of=lambda n: n.startswith(scope), tf_shapes=shapes)
        return path

    def train(self, train_data=None, valid_data=None):
        assert train_data is not None
        assert valid_data is not None
        if not self.graphs:
            self._build_functions(train_data)
        session = self.session
        self._init_model(session)
        self._save_checkpoint(session, 'random')
        start_epoch = int(self.global_step)
        best_epoch = -1
        best_accuracy = -1.0
        best_loss = 10000
        for epoch in range(start_epoch, start_epoch + self.num_epochs):
            step = 0
            for next_batch in train_data.data:
                r = self.train_step(self._retrieve_batch(next_batch))
                if step % self.display_freq == 0:
                    self.log('{}: {} - Iteration: [{:3}]\t Training_Loss: {:6f}\t Training_Accuracy: {:6f}'.format(
                        datetime.now(), FLAGS.exp_name, step, r["loss"], r["accuracy"]))
                step += 1
            total_loss, total_accuracy = self._evaluate(session, 'validation', valid_data)
            self.log('{}: {} - Epoch: {}\t Validation_Loss: {:6f}\t Validation_Accuracy: {:6f}'.format(
                datetime.now(), FLAGS.exp_name, epoch, total_loss, total_accuracy))
            # if accuracy or loss decrease save model
            if total_accuracy > best_accuracy or (total_accuracy == best_accuracy and total_loss <= best_loss):
                best_epoch = epoch
                best_accuracy = total_accuracy
                best_loss = total_loss
                self._save_checkpoint(session, epoch)
                with open('{}/{}'.format(FLAGS.checkpoint_dir, FLAGS.exp_name) + "/model.txt", "w") as outfile:
                    outfile.write('{}: {}\nBest Epoch: {}\nValidation_Loss: {:6f}\nValidation_Accuracy: {:6f}\n'.format(
                        datetime.now(), FLAGS.exp_name, best_epoch, best_loss, best_accuracy))
        self.log('{}: {} - Best Epoch: {}\t Validation_Loss: {:6f}\t Validation_Accuracy: {:6f}'.format(
            datetime.now(), FLAGS.exp_name, best_epoch, best_loss, best_accuracy))
        return best_loss, best_accuracy

    def _valid(self, session, data):
        return self._evaluate(session, 'validation', data)

    def _evaluate(self, session, mod, data):
        """(loss, accuracy) over `data` (:248-282): the mean of the per-clip losses and the fraction of clips predicted
        right - what the reference's size-weighted means of the per-batch values are.  Every batch is the forward plan
        followed by `acimg_clip_eval` into the evaluator's state; `result()` is the pass's one read-back and stays in
        `last_evaluation` (confusion matrix included)."""
        self._begin_pass()
        for next_batch in data.data:
            self._pass_batch(next_batch)
        r = self._end_pass()
        return r["loss"], r["accuracy"]

    def _begin_pass(self):
        self.evaluator.reset()

    def _pass_batch(self, next_batch):
        """one loader batch of a pass: inputs in, forward plan + `acimg_clip_eval` enqueued, nothing read back"""
        batch = self._retrieve_batch(next_batch)
        g = self._graph_for(self._clips_of(batch))
        self._feed(g, batch, None)
        g.plan_pass.run()

    def _end_pass(self):
        self.last_evaluation = self.evaluator.result()
        return self.last_evaluation

    def test(self, test_data=None):
        assert test_data is not None
        if not self.graphs:
            self._build_functions(test_data)
        session = self.session
        self._restore_model(session)
        test_loss, test_accuracy = self._evaluate(session, 'test', test_data)
        if self.source == "generated":
            name = '{}/{}'.format(FLAGS.checkpoint_dir, FLAGS.exp_name) + "/test_accuracy.txt"
        else:
            name_folder = str.join('/', FLAGS.restore_checkpoint.split('/')[:-1])
            tag = FLAGS.restore_checkpoint.split('/')[-1].split('.')[0].split('_')[1]
            name = '{}'.format(name_folder) + ("/test_accuracy_mfccmap_{}.txt" if self.source == "mfccmap"
                                              else "/test_accuracy_{}.txt").format(tag)
        line = '{}: {} - Testing_Loss: {:6f}\nTesting_Accuracy: {:6f}'.format(datetime.now(), FLAGS.exp_name, test_loss,
                                                                               test_accuracy)
        with open(name, "w") as outfile:
            outfile.write(line)
        self.log(line)
        return test_loss
