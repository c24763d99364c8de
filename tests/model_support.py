"""Trainers on the device as several model-level tests (and tools/debug) build them, the activations and ReLU patterns
they hand to the oracle, and the loss lines of a training log."""
import re


def make(device, lr=1e-3, epochs=1):
    """the UNet trainer of the trainer-surface, loader and classification tests -> (trainer, session)"""
    from acimg.flags import FLAGS
    from acimg.session import Session
    from acimg.trainer import Trainer
    from acimg.unet_acresnet import UNetAc
    from acimg.vision import ResNet50Model

    FLAGS.model, FLAGS.ae, FLAGS.latent_loss = "UNet", 0, 1e-6
    sess = Session(device)
    tr = Trainer(UNetAc(input_shape=[36, 48, 12], embedding=False, num_skip=1),
                 ResNet50Model(input_shape=[224, 298, 3], num_classes=None), display_freq=1, learning_rate=lr,
                 num_epochs=epochs, session=sess)
    return tr, sess


def build(device, num_skip, embedding, batch, lr=1e-3, precision="f16x3", bench_defaults=False, side_lane=True, stages=None):
    """the train step and the oracle on identical weights -> (trainer, oracle, session)"""
    from acimg.flags import FLAGS
    from acimg.session import Session
    from acimg.trainer import Trainer
    from acimg.unet_acresnet import UNetAc
    from acimg.vision import ResNet50Model
    from oracle import trainer as otr

    FLAGS.model = "UNet"
    FLAGS.ae = int(embedding)
    # larger than the default 1e-6 so the KL path is visible in the gradients (bench_defaults: the bench's own 1e-6)
    FLAGS.latent_loss = 1e-6 if bench_defaults else 1e-3
    orc = otr.Oracle(num_skip=num_skip, embedding=embedding, learning_rate=lr, latent_loss=FLAGS.latent_loss,
                     randomize=True)
    sess = Session(device)
    mi = ResNet50Model(input_shape=[224, 298, 3], num_classes=None, precision=precision, stages=stages, side_lane=side_lane)
    ma = UNetAc(input_shape=[36, 48, 12], embedding=embedding, num_skip=num_skip,
                precision="split" if precision == "f16x3" else "f32", side_lane=side_lane)
    if not bench_defaults:
        ma.split_min_rows = 0   # exercise the split-MFMA generator convs even at the tiny test batch
    tr = Trainer(ma, mi, learning_rate=lr, session=sess)
    tr._build_functions(batch_size=batch)
    loaded = sess.store.load_state(orc.state_dict(), strict=True)
    assert len(loaded) == len(orc.state_dict())
    return tr, orc, sess


MASK_PAIRS = [("c11", "layer1/conv_1"), ("conv1", "layer1/conv_2"), ("pool1", "layer1/pool_2"),
              ("c21", "layer2/conv_1"), ("conv2_0", "layer2/conv_2"), ("dns", "dense"), ("net", "conv2d"),
              ("c41", "layer4/conv_1"), ("conv4", "layer4/conv_2"), ("c51", "layer5/conv_1"),
              ("conv5", "layer5/conv_2"), ("c61", "layer6/conv_1"), ("conv6", "layer6/conv_2"),
              ("c71", "layer7/conv_1"), ("conv7", "layer7/conv_2")]


def saved_activations(g):
    """{oracle layer name: post-ReLU activation saved by the HIP forward} (+ the ResNet feature)"""
    out = {}
    for attr, key in MASK_PAIRS:
        a = getattr(g.modelac, attr)
        out[key] = a.t.cpu().reshape(a.N, a.H, a.W, -1)[..., a.off:a.off + a.C]
    out["conv_map"] = g.modelimages.output.cpu()
    return out


def noconc_masks(m):
    """the ReLU patterns of a UNetAcNoConc forward, under the oracle's layer names"""
    acts = {"layer1/conv_1": m.c11, "layer1/conv_2": m.conv1, "layer1/pool_2": m.pool1, "layer3/conv_1": m.c31,
            "layer3/conv_2": m.conv2, "conv2d": m.net, "layer4/conv_1": m.c41, "layer4/conv_2": m.conv4,
            "layer5/conv_1": m.c51, "layer5/conv_2": m.conv5}
    out = {k: (a.t[..., :a.C] > 0).cpu() for k, a in acts.items()}
    out["dense"] = (m.dns.t > 0).cpu()
    return out


def loss_lines(log, validation):
    """the iteration lines of a training log, cut to their loss fields; validation: the epochs' validation losses after them"""
    lines = [re.search(r"Iteration: \[ *\d+\]\t Training_mse_Loss: [0-9.]+\t Training_Loss: [0-9.]+", ln).group(0)
             for ln in log if "Training_mse_Loss" in ln]
    return lines + [ln.split("Validation_mse_Loss:")[1] for ln in log if "- Epoch:" in ln] if validation else lines
