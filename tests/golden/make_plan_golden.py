"""Generates tests/golden/plan_signatures.json: what every trainer RECORDS - the sequence of C-ABI calls of its train (and
eval) plan with their descriptors, scalars and buffer wiring - on a CPU session, so that a change to the host layer that
moves a layer onto another kernel, reorders a launch or rewires a buffer shows up without a GPU.  Reads nothing outside the
package; tests/test_plan_signatures_cpu.py rebuilds the same configurations with `record()` and compares.

One entry per `plan.calls` item: [call name, on the side lane?, arguments], an argument being
  a ConvDesc                   -> {"desc": [every field]}
  a Python int / float / None  -> itself
  a tensor, Ptr or LazyPtr     -> {"buf": ordinal of first appearance of its resolved address within the plan}
  workspace pointer / tickets  -> "ws" | "side_ws" | "tickets";  workspace bytes -> {"ws_bytes": resolved number}
  a prepare_multi job table    -> {"jobs": [[descriptor fields, kernel ordinal, image ordinal, mode], ...]} (on its first
                                  argument; the four table pointers are tags)
and a host hook (no arguments) its name: fork / join / hook.  Per configuration (they do not depend on the batch size)
also the store's tf_names(), its train_ranges(), the size of the flat trainable buffer and its CRC-32C after every
model's initialize() at its default seed (the order of the random draws).

The lists are some 6 MB, so the committed file holds what pins them and names a difference: per plan the call names in clear
(`rle`: a repeated block written once; a list many plans share stored once), three hex digits of SHA-256 per call and one
SHA-256 of the whole serialised list; of each variable list its length and SHA-256.  `--full` writes the lists themselves:
run it on two trees and diff the files to see what a failing hash hides.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_plan_golden.py
    ... make_plan_golden.py --device cuda --full --out PATH     (the Trainer configurations at N = 16, with lanes)
"""
import argparse
import ctypes
import hashlib
import json
import os
import re
import sys
from collections import OrderedDict

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for _p in (ROOT, os.path.join(ROOT, "acoustic-image-generation_amd")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

GOLDEN = os.path.join(HERE, "plan_signatures.json")


# ---- the configurations ---------------------------------------------------------------------------------------------
def configurations(gpu=False):
    """[(key, kind, keyword arguments, batch sizes)].  N = 8 / 16 put the 36x48 layers on either side of the 16384-row
    split rule (13824 / 27648 rows)."""
    gen = [dict(num_skip=0), dict(num_skip=1), dict(num_skip=2), dict(num_skip=1, embedding=True),
           dict(num_skip=1, precision="f32"), dict(num_skip=1, side_lane=False)]
    # the trunk's variants (ResNet50Model keyword sets) under one generator.  N = 7 / 8: at 7 the 56x75 and 28x38 layers
    # have row counts that are 8 mod 16, so every brick round-up of a split-format plane is exercised; 8 is the aligned case
    trunk = [dict(num_skip=1, trunk=t) for t in (
        dict(precision="f32"), dict(precision="f16"), dict(stages=1), dict(stages=1, side_lane=False), dict(gram=False),
        dict(two_pass=False), dict(stage_cut=5), dict(two_pass_max_cin=128))]
    if gpu:       # the lanes are what a CPU session cannot see: the generator's and the trunk's configurations alone
        return [_keyed("trainer", kw, (16,)) for kw in gen + trunk]
    out = [_keyed("trainer", kw, (8, 16)) for kw in gen]
    for model in ("UNet", "UNetSound"):
        for precision in ("split", "bf16", "f32"):
            for defer_bn in (True, False):
                out.append(_keyed("vae", dict(model=model, precision=precision, defer_bn=defer_bn), (2, 16)))
    for precision in ("split", "f32"):
        out.append(_keyed("vae", dict(model="UNetAcNoConc", precision=precision), (8, 16)))
    for assoc in ("AssociatorVideoAc", "AssociatorAudioAc", "AssociatorAudio"):
        out.append(_keyed("associator", dict(associator=assoc), (8, 16)))
    out.append(_keyed("class", dict(), (12, 24)))
    for mode in ("all", "fusion", "onlyaudiovideo"):
        out.append(_keyed("multi", dict(mode=mode), (2, 16)))
    out += [_keyed("trainer", kw, (7, 8)) for kw in trunk]
    return out


def _keyed(kind, kw, Ns):
    return ("%s(%s)" % (kind, ", ".join("%s=%s" % kv for kv in sorted(kw.items()))), kind, kw, Ns)


def build(kind, kw, N, device):
    """-> (trainer, session, graph, [models in initialisation order])"""
    from acimg import multimodal, unet_acoustic, unet_joint, unet_vae
    from acimg.dualcamnet import DualCamHybridModel
    from acimg.flags import FLAGS, _Flags
    from acimg.session import Session
    from acimg.trainer import Trainer
    from acimg.trainer_associator import TrainerAssociator
    from acimg.trainer_class import TrainerClass
    from acimg.trainer_multi import TrainerMulti
    from acimg.trainer_vae import TrainerVAE
    from acimg.unet_acresnet import UNetAc
    from acimg.vision import ResNet50Model

    FLAGS.__dict__.update(_Flags().__dict__)          # every flag at its default, whatever ran before
    sess = Session(torch.device(device))
    if kind == "trainer":
        kw = dict(kw)
        trunk = kw.pop("trunk", {})
        FLAGS.model, FLAGS.ae = "UNet", int(kw.get("embedding", False))
        ma = UNetAc(input_shape=[36, 48, 12], **kw)
        mi = ResNet50Model(input_shape=[224, 298, 3], num_classes=None, **trunk)
        tr, models = Trainer(ma, mi, session=sess), [mi, ma]
    elif kind == "vae":
        kw = dict(kw)
        cls = kw.pop("model")
        m = (unet_acoustic.UNetAcNoConc if cls == "UNetAcNoConc" else getattr(unet_vae, cls))(**kw)
        tr, models = TrainerVAE(m, session=sess), [m]
    elif kind == "associator":
        ma, md = getattr(multimodal, kw["associator"])(), unet_acoustic.UNetAcZ()
        tr, models = TrainerAssociator(ma, md, session=sess), [ma, md]
    elif kind == "class":
        m = DualCamHybridModel(input_shape=[36, 48, 12], num_classes=14)
        mi = ResNet50Model(input_shape=[224, 298, 3], num_classes=None)
        ma = UNetAc(input_shape=[36, 48, 12], embedding=False, num_skip=1)
        tr, models = TrainerClass(m, mi, ma, session=sess), [mi, ma, m]
    else:
        mode = kw["mode"]
        assoc = {"all": multimodal.Jointmvae, "fusion": multimodal.JointTwomvae2,
                 "onlyaudiovideo": multimodal.Jointmvae}[mode]()
        assoc1 = multimodal.JointTwomvae() if mode == "onlyaudiovideo" else None
        mac, mau, mvi = unet_joint.UNetAc2([36, 48, 12]), unet_joint.UNetSound22([193, 257, 1]), unet_joint.Unet2([224, 298, 3])
        tr = TrainerMulti(mac, mau, mvi, assoc, assoc1, session=sess, mode=mode, moddrop=mode == "all")
        models = [mac, mau, mvi, assoc] + ([assoc1] if assoc1 is not None else [])
    g = tr._build_functions(batch_size=N)
    sess.finalize()
    return tr, sess, g, models


# ---- the signature ---------------------------------------------------------------------------------------------------
def _desc_fields(d):
    return [getattr(d, f[0]) for f in d._fields_]


def signature(plan):
    """the plan's call list as JSON-able values (see the module docstring); the session must be finalised"""
    from acimg import ops

    plan.ws.allocate()
    plan.side_ws.allocate()
    seen = {}

    def buf(a):
        addr = ops._resolve(a)
        return seen.setdefault(addr, len(seen))

    def arg(a):
        if a is None or isinstance(a, (int, float)):
            return a
        if isinstance(a, (torch.Tensor, ops.Ptr, ops.LazyPtr)):
            return {"buf": buf(a)}
        if isinstance(a, ops._WsPtr):
            return "ws" if a.ws is plan.ws else "side_ws"
        if isinstance(a, ops._WsBytes):
            return {"ws_bytes" if a.ws is plan.ws else "side_ws_bytes": int(a.ws.nbytes)}
        if isinstance(a, ops._Tickets):
            return "tickets_off" if a.off else "tickets"
        if isinstance(a, ops._JobsArg):
            if a.which != "n":
                return "jobs." + a.which
            return {"jobs": [[_desc_fields(d), buf(w), buf(o), mode] for d, w, o, mode in a.jobs.jobs]}
        if hasattr(a, "_obj") and isinstance(a._obj, ops.ConvDesc):          # ctypes.byref(descriptor)
            return {"desc": _desc_fields(a._obj)}
        if isinstance(a, (ctypes.c_void_p, ctypes.c_int)):
            return a.value
        raise TypeError("plan argument of a kind the signature does not know: %r" % (a,))

    out = []
    for i, (name, fn, args) in enumerate(plan.calls):
        out.append(name if args is None else [name, i in plan.side, [arg(a) for a in args]])
    return out


def _dump(v):
    return json.dumps(v, sort_keys=True, separators=(",", ":"))


HEX = 3        # hex digits of SHA-256 kept per call: enough to name the first call that differs; `sha256` decides equality


def rle(names):
    """call names in clear, an immediately repeated block of up to 12 calls written once, as in (a b c)x4"""
    out, i = [], 0
    while i < len(names):
        best = (0, 1, 1)        # (calls saved, block length, repeats)
        for L in range(1, 13):
            n = 1
            while names[i + n * L:i + (n + 1) * L] == names[i:i + L]:
                n += 1
            if (n - 1) * L > best[0]:
                best = ((n - 1) * L, L, n)
        _, L, n = best
        out.append(" ".join(names[i:i + L]) if n == 1 else "(%s)x%d" % (" ".join(names[i:i + L]), n))
        i += L * n
    return " ".join(out)


def unrle(text):
    names = []
    for block, n, single in re.findall(r"\(([^)]*)\)x(\d+)|(\S+)", text):
        names += [single] if single else block.split() * int(n)
    return names


def digest(sig):
    """the committed form of a signature: names in clear, HEX hex digits per call, one SHA-256 over the whole list"""
    names = [c if isinstance(c, str) else c[0] for c in sig]
    assert unrle(rle(names)) == names
    calls = "".join(hashlib.sha256(_dump(c).encode()).hexdigest()[:HEX] for c in sig)
    return OrderedDict(names=rle(names), calls=calls, sha256=hashlib.sha256(_dump(sig).encode()).hexdigest())


def listed(v):
    """the committed form of a variable list: its length and the SHA-256 of its serialisation"""
    return [len(v), hashlib.sha256(_dump(v).encode()).hexdigest()]


_CRC = {}


def record(kind, kw, N, device="cpu", full=False):
    """-> (the store's record, {plan name: committed form}, {plan name: full signature}) of one configuration at batch N"""
    from acimg import tfio

    tr, sess, g, models = build(kind, kw, N, device)
    plans = OrderedDict(plan_train=signature(g.plan_train))
    if getattr(g, "plan_eval", None) is not None:
        plans["plan_eval"] = signature(g.plan_eval)
    key = (kind, _dump(kw))            # the initial weights do not depend on the batch size: drawn once per model set
    if key not in _CRC:
        for m in models:
            m.initialize()
        _CRC[key] = tfio.crc32c_array(sess.store.flat["train"].cpu().numpy())
    names, ranges = list(sess.store.tf_names()), [list(r) for r in sess.store.train_ranges()]
    store = OrderedDict(tf_names=names if full else listed(names), train_ranges=ranges if full else listed(ranges),
                        train_numel=sess.store.train_numel(), init_crc32c=_CRC[key])
    return store, OrderedDict((k, sig if full else digest(sig)) for k, sig in plans.items()), plans


def load_golden(path=GOLDEN):
    """{configuration: record} with every plan's shared name list put back in place"""
    with open(path) as f:
        g = json.load(f)
    for rec in g["configurations"].values():
        for plans in rec["plans"].values():
            for p in plans.values():
                p["names"] = g["names"][p["names"]]
    return g["configurations"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--device", default="cpu")
    ap.add_argument("--out", default=GOLDEN)
    ap.add_argument("--full", action="store_true", help="write the lists themselves, not their digests")
    a = ap.parse_args()
    out, shared = OrderedDict(), OrderedDict()
    for key, kind, kw, Ns in configurations(gpu=a.device != "cpu"):
        for N in Ns:
            store, plans, sigs = record(kind, kw, N, a.device, a.full)
            rec = out.setdefault(key, OrderedDict(store, plans=OrderedDict()))
            assert all(rec[k] == v for k, v in store.items()), "the variables of %s depend on the batch size" % key
            for p in ([] if a.full else plans.values()):       # many plans launch the same kernels in the same order
                p["names"] = shared.setdefault(p["names"], "n%d" % len(shared))
            rec["plans"][str(N)] = plans
            print(key, "N=%d" % N, " ".join("%s: %d calls" % (k, len(v)) for k, v in sigs.items()), flush=True)
    with open(a.out, "w") as f:
        if a.full:
            json.dump(out, f, indent=1)
        else:                                                   # one line per name list and per configuration
            f.write('{"names": {\n%s\n},\n"configurations": {\n%s\n}}' % (
                ",\n".join("%s: %s" % (json.dumps(i), json.dumps(n)) for n, i in shared.items()),
                ",\n".join("%s: %s" % (json.dumps(k), json.dumps(r)) for k, r in out.items())))
        f.write("\n")
    print("wrote", a.out, os.path.getsize(a.out), "bytes")


if __name__ == "__main__":
    main()
