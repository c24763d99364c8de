"""Triplet losses (trainer/trainer_three.py:551-732) through the C ABI vs the fp64 oracle: loss,
fraction of positive triplets, counts and the gradients w.r.t. both embedding sets, batch-all and batch-hard."""
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "acoustic-image-generation_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


SENTINEL = -12345.0


def _run(e0, e1, labels, scenario, margin, hard, weight=1.0, ld=None):
    """ld: one leading dimension for all four matrices, or (lde0, lde1, ldg0, ldg1).  The pad columns hold NaN in the
    embeddings and SENTINEL in the gradients: nothing may read the former, and the latter must survive"""
    from acimg import ops
    B, D = e0.shape
    lde0, lde1, ldg0, ldg1 = ld if isinstance(ld, tuple) else (ld or D,) * 4
    a = torch.full((B, lde0), float("nan"), device=DEV)
    b = torch.full((B, lde1), float("nan"), device=DEV)
    a[:, :D] = e0.float().to(DEV)
    b[:, :D] = e1.float().to(DEV)
    lab, sc = labels.int().to(DEV), scenario.int().to(DEV)
    ws = torch.zeros(ops.triplet_loss_workspace(B), dtype=torch.uint8, device=DEV)
    out = torch.zeros(4, device=DEV)
    g0, g1 = torch.full((B, ldg0), SENTINEL, device=DEV), torch.full((B, ldg1), SENTINEL, device=DEV)
    g0[:, :D] = 0
    g1[:, :D] = 0
    plan = ops.Plan(DEV, eager=True)
    ops.triplet_loss_fwd(plan, a, lde0, b, lde1, lab, sc, B, D, margin, hard, ws, out)
    ops.triplet_loss_bwd(plan, a, lde0, b, lde1, B, D, weight, ws, g0, ldg0, g1, ldg1)
    torch.cuda.synchronize()
    assert bool((g0[:, D:] == SENTINEL).all()) and bool((g1[:, D:] == SENTINEL).all()), "gradient pad columns written"
    return out.cpu(), g0[:, :D].cpu().double(), g1[:, :D].cpu().double(), (a, b, ws, plan)


def _oracle(e0, e1, labels, scenario, margin, hard):
    from oracle import triplet as ot
    a, b = e0.clone().requires_grad_(True), e1.clone().requires_grad_(True)
    loss, frac, npos, nvalid = (ot.mix_data_hard if hard else ot.mix_all)(a, b, labels, scenario, margin)
    z = torch.zeros_like(a)
    if not loss.requires_grad:
        return float(loss), float(frac), float(npos), float(nvalid), z, z
    ga, gb = torch.autograd.grad(loss, [a, b], allow_unused=True)
    return float(loss), float(frac), float(npos), float(nvalid), z if ga is None else ga, z if gb is None else gb


def _rel(a, b):
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))


@pytest.mark.parametrize("hard", [0, 1])
@pytest.mark.parametrize("B,D,ld", [(48, 150, 152), (7, 12, 12), (300, 64, 64), (9, 300, (300, 304, 308, 312))])
def test_triplet_random(hard, B, D, ld):
    """(9, 300): triplet_grad_kernel walks D in strides of 256, so a second pass of 44 columns; four different leading
    dimensions, so an ld taken from the wrong matrix shows"""
    g = torch.Generator().manual_seed(100 + B)
    e0 = 0.05 * torch.randn(B, D, generator=g, dtype=torch.float64)
    e1 = 0.05 * torch.randn(B, D, generator=g, dtype=torch.float64)
    labels = torch.randint(0, 5, (B,), generator=g)
    scenario = torch.randint(0, 3, (B,), generator=g)
    margin = 0.2
    # the device works in fp32: give the oracle the fp32-rounded inputs
    e0, e1 = e0.float().double(), e1.float().double()
    out, g0, g1, _ = _run(e0, e1, labels, scenario, margin, hard, weight=0.5, ld=ld)
    loss, frac, npos, nvalid, ga, gb = _oracle(e0, e1, labels, scenario, margin, hard)
    assert float(out[3]) == nvalid
    # a triplet within fp32 rounding of the hinge may fall on either side
    assert abs(float(out[2]) - npos) <= max(2.0, 2e-5 * npos), (float(out[2]), npos)
    assert abs(float(out[0]) - loss) <= 1e-4 * abs(loss) + 1e-7, (float(out[0]), loss)
    assert abs(float(out[1]) - frac) <= 1e-4 * frac + 1e-7
    assert _rel(g0, 0.5 * ga) < 1e-3 and _rel(g1, 0.5 * gb) < 1e-3, (_rel(g0, 0.5 * ga), _rel(g1, 0.5 * gb))


@pytest.mark.parametrize("hard", [0, 1])
def test_triplet_exact_ties(hard):
    """small-integer embeddings with repeated rows: every distance is exact in fp32 and fp64, so the hinge at exactly
    zero and the tied maxima / minima take TensorFlow's conventions or the gradients differ visibly"""
    g = torch.Generator().manual_seed(7)
    base0 = torch.randint(-2, 3, (4, 6), generator=g).double()
    base1 = torch.randint(-2, 3, (4, 6), generator=g).double()
    idx = torch.tensor([0, 1, 2, 3, 0, 1, 2, 3, 0, 0])
    e0, e1 = base0[idx], base1[idx]
    labels = torch.tensor([0, 1, 0, 1, 0, 1, 2, 2, 0, 0])
    scenario = torch.tensor([0, 0, 0, 1, 0, 0, 1, 1, 0, 0])
    for margin in (1.0, 0.0, 4.0):
        out, g0, g1, _ = _run(e0, e1, labels, scenario, margin, hard)
        loss, frac, npos, nvalid, ga, gb = _oracle(e0, e1, labels, scenario, margin, hard)
        assert float(out[2]) == npos and float(out[3]) == nvalid
        assert abs(float(out[0]) - loss) <= 1e-6 * abs(loss) + 1e-9
        assert (g0 - ga).abs().max() <= 1e-5 * ga.abs().max().clamp_min(1.0), (margin, (g0 - ga).abs().max())
        assert (g1 - gb).abs().max() <= 1e-5 * gb.abs().max().clamp_min(1.0), (margin, (g1 - gb).abs().max())


def test_triplet_no_valid_triplet_and_accumulate():
    from acimg import ops
    g = torch.Generator().manual_seed(3)
    e0 = torch.randn(6, 8, generator=g, dtype=torch.float64).float().double()
    e1 = torch.randn(6, 8, generator=g, dtype=torch.float64).float().double()
    same = torch.zeros(6, dtype=torch.long)
    out, g0, g1, _ = _run(e0, e1, same, same, 0.3, 0)        # one video: no negatives, 0 / 1e-16 = 0
    assert out.tolist() == [0.0, 0.0, 0.0, 0.0] and float(g0.abs().max()) == 0.0 and float(g1.abs().max()) == 0.0
    labels = torch.tensor([0, 0, 1, 1, 2, 2])
    out, g0, g1, (a, b, ws, plan) = _run(e0, e1, labels, same, 0.3, 0)
    acc = torch.ones(6, 8, device=DEV)
    ops.triplet_loss_bwd(plan, a, 8, b, 8, 6, 8, 2.0, ws, acc, 8, None, 0, accumulate=True)
    torch.cuda.synchronize()
    assert torch.allclose(acc.cpu().double(), 1.0 + 2.0 * g0, atol=1e-6)
    twice = _run(e0, e1, labels, same, 0.3, 0)
    assert torch.equal(twice[1], g0) and torch.equal(twice[0], out)            # bit-reproducible


def test_triplet_errors():
    from acimg import _lib, ops
    L = _lib.load()
    x = torch.zeros(4, 8, device=DEV)
    lab = torch.zeros(4, dtype=torch.int32, device=DEV)
    out = torch.zeros(4, device=DEV)
    ws = torch.zeros(ops.triplet_loss_workspace(4), dtype=torch.uint8, device=DEV)
    assert L.acimg_triplet_loss_fwd(x.data_ptr(), 8, x.data_ptr(), 8, lab.data_ptr(), lab.data_ptr(), 4, 8, 0.1, 0,
                                    ws.data_ptr(), 16, out.data_ptr(), None) != 0
    assert L.acimg_triplet_loss_fwd(x.data_ptr(), 4, x.data_ptr(), 8, lab.data_ptr(), lab.data_ptr(), 4, 8, 0.1, 0,
                                    ws.data_ptr(), ws.numel(), out.data_ptr(), None) != 0
    assert L.acimg_triplet_loss_fwd(x.data_ptr(), 8, x.data_ptr(), 8, lab.data_ptr(), lab.data_ptr(), 4096, 8, 0.1, 0,
                                    ws.data_ptr(), ws.numel(), out.data_ptr(), None) != 0
    assert L.acimg_triplet_loss_bwd(x.data_ptr(), 8, x.data_ptr(), 8, 4, 8, 1.0, ws.data_ptr(), ws.numel(), None, 0,
                                    None, 0, 0, None) != 0
