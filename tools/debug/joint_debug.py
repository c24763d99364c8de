"""diagnostics of the joint-latent step against its oracle: relative errors stage by stage"""
import functools, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "acoustic-image-generation_amd"), os.path.join(ROOT, "tests")]
import torch
from acimg.multimodal import Jointmvae
from acimg.session import Session
from acimg.trainer_multi import TrainerMulti
from acimg.unet_joint import UNetAc2, UNetSound22, Unet2
from oracle import joint
from op_support import rel_err

rel = functools.partial(rel_err, floor=1e-30, same_shape=False)

dev = torch.device("cuda:0")
N = 2
orc = joint.Oracle(learning_rate=1e-3)
sess = Session(dev)
tr = TrainerMulti(UNetAc2([36, 48, 12]), UNetSound22([193, 257, 1]), Unet2([224, 298, 3]), Jointmvae(), learning_rate=1e-3, session=sess)
g = tr._build_functions(batch_size=N)
sess.store.load_state(orc.state_dict(), strict=True)
batch, eps = joint.synthetic_batch(N)
got = tr.train_step((batch["ac"], batch["audio"], batch["video"]), eps=eps, apply=False)
torch.cuda.synchronize()
ref = orc.train_step(batch, eps, apply=False)
print({k: (round(got[k], 6), round(ref["losses"][k], 6)) for k in got})
for key, (m, _, attr) in g.mods.items():
    print(key, "features", rel(m.features, ref["feats"][key]), "head", rel(getattr(tr.modelassociator, attr), ref["heads"][attr]),
          "mean", rel(m.mean, ref["outs"][key]["mean"]), "std", rel(m.std, ref["outs"][key]["std"]),
          "z", rel(m.zbuf[:, :m.Z], ref["outs"][key]["z"]), "out", rel(m.output[..., :m.channels], ref["outs"][key]["output"]))
