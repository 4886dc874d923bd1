"""Disparity supervision end to end at B = 1 on the seeded model: the encoder's gradients under DisparityLoss on the full-resolution soft
read-out against torch's float64 autograd of the oracle encoder followed by a plain torch formulation of the read-out and the loss, and
a three-step SGD loop on Stereo2Voxel under VoxelBCELoss + 0.1 * DisparityLoss run twice.

Method, helpers and tolerance are tests/test_encoder_training_gpu.py's, imported as they are: ReLU gates inside the window E take the
gate of the path under test, and the yardstick is FACTOR times torch's float32 CPU autograd of the same graph, per tensor in relative
L2.  The read-out adds no gate of its own that needs mending: the loss's two branches meet with one derivative, and |L - R| has its
kink where two features are equal, which in a ReLU tower means both are 0 — a gate the window already covers."""
import numpy as np
import pytest
import torch

from tests import _dispbwd64 as R
from tests import test_encoder_training_gpu as T

pytestmark = pytest.mark.gpu
DEV = T.DEV


def _ground_truth(s3r, seed):
    """(1,224,224) synthetic disparity in render pixels: a smooth positive map with planted invalid pixels (inf, -1, NaN)"""
    g = torch.Generator().manual_seed(seed)
    y, x = torch.meshgrid(torch.arange(224.0), torch.arange(224.0), indexing="ij")
    gt = 60 + 50 * torch.sin(x / 37) * torch.cos(y / 53) + 3 * torch.rand(224, 224, generator=g)
    u = torch.rand(224, 224, generator=g)
    gt[u < 0.30] = float("inf")
    gt[(u >= 0.30) & (u < 0.35)] = -1.0
    gt[(u >= 0.35) & (u < 0.36)] = float("nan")
    return gt[None]


def _torch_readout(feats, max_disp, tau, scale):
    """(disp_l, disp_r) (B,224,224) in feats.dtype: costs via abs, a min-shifted softmax, the bilinear blend as the explicit matrix of
    tests/_dispbwd64.py (the fp32 index rule), times scale"""
    dt = feats.dtype
    b = feats.shape[0] // 2
    L, Rt = feats[:b], feats[b:]
    H, W = L.shape[2:]
    dm = min(max_disp, W)
    wts = R.weights64 if dt == torch.float64 else R.weights32
    wy, wx = torch.from_numpy(wts(H, 224)).to(dt), torch.from_numpy(wts(W, 224)).to(dt)
    d = torch.arange(dm, dtype=dt)
    out = []
    for right in (False, True):
        cols = []
        for k in range(dm):
            c = (Rt[..., :W - k] - L[..., k:]).abs().sum(1) if right else (L[..., k:] - Rt[..., :W - k]).abs().sum(1)
            pad = torch.full(c.shape[:-1] + (k,), float("inf"), dtype=dt)
            cols.append(torch.cat([c, pad], -1) if right else torch.cat([pad, c], -1))
        c = torch.stack(cols, -1)                                    # (b,H,W,dm), +inf where d >= n(w)
        p = torch.softmax((c.min(-1, keepdim=True).values.detach() - c) / tau, -1)
        disp = (p * d).sum(-1)
        out.append(torch.einsum("oh,bhw,pw->bop", wy, disp, wx) * scale)
    return out


def _torch_loss(pred, gt, beta=1.0):
    ok = torch.isfinite(gt) & (gt >= 0)
    l = torch.nn.functional.smooth_l1_loss(pred[ok], gt[ok].to(pred.dtype), beta=beta, reduction="sum")
    return l / max(int(ok.sum()), 1)


def test_encoder_gradients_under_the_disparity_loss_against_float64(s3r, oracle):
    state, left, right = T._problem("voxel")
    model = T._model(s3r, "voxel")
    enc = model.encoder
    gtl, gtr = _ground_truth(s3r, 1), _ground_truth(s3r, 2)
    dl, dr = model.differentiable_disparity(left, right, full_resolution=True)
    assert dl.shape == dr.shape == (1, 224, 224) and dl.grad_fn is not None
    crit = s3r.DisparityLoss()
    loss = crit(dl, gtl.to(DEV)) + crit(dr, gtr.to(DEV))
    with torch.no_grad():                                          # the scaling rules of disparity(readout="soft"): x8, 224 x 224
        f = enc.differentiable_pair(left, right)
        pl, pr = s3r.disparity_soft(f[:1], f[1:], model.cost_volume.max_disp, model.disparity_temperature, (224, 224), 8.0)
        ql, qr = model.disparity(left, right, readout="soft", full_resolution=True)
    assert torch.equal(pl.view(torch.int32), dl.detach().view(torch.int32)) and torch.equal(pr.view(torch.int32), dr.detach().view(torch.int32))
    print(f"against disparity(readout='soft') on the fused forward's features: max |d| {(ql - pl).abs().max().item():.3e} px")
    acts = T._saved_activations(loss)
    loss.backward()
    torch.cuda.synchronize()
    params = dict(enc.named_parameters())
    names = T._trained(enc)
    assert len(names) == 3 * 8 and set(acts) == set(enc.names)
    for n, p in params.items():
        assert (p.grad is None) == n.endswith("bn.weight"), n
    tau, D = float(np.float32(model.disparity_temperature)), model.cost_volume.max_disp

    def tail(orc, h, ctx):
        a, b = _torch_readout(h, D, tau, 8.0)
        return _torch_loss(a, gtl) + _torch_loss(b, gtr)

    ref = T._references(lambda dt: T._oracle_encoder(oracle, state, dt), "encoder", left, right, tail, acts)
    print(f"loss {loss.item():.7g}; float64 {ref['losses'][0]:.7g}; float32 on the CPU {ref['losses'][1]:.7g}")
    assert abs(loss.item() - ref["losses"][0]) <= 1e-4 * abs(ref["losses"][0])
    T._compare({n: params[n].grad for n in names}, ref, names)


def test_three_sgd_steps_under_both_losses_are_deterministic(s3r):
    """three SGD steps on every trained parameter of Stereo2Voxel under VoxelBCELoss + 0.1 * DisparityLoss (left and right maps), twice
    from the same state: identical losses and identical bits in every parameter; every encoder parameter moved"""
    state, left, right = T._problem("voxel")
    gt = (torch.rand(1, 32, 32, 32, generator=torch.Generator().manual_seed(2)) < 0.3).float().to(DEV)
    gtl, gtr = _ground_truth(s3r, 1).to(DEV), _ground_truth(s3r, 2).to(DEV)

    def three_steps():
        model = T._model(s3r, "voxel")
        params = dict(model.named_parameters())
        opt = torch.optim.SGD([params[n] for n in T._trained(model)], lr=T.LR)
        bce, dsp = s3r.VoxelBCELoss(), s3r.DisparityLoss()
        losses = []
        for _ in range(3):
            opt.zero_grad()
            dl, dr = model.differentiable_disparity(left, right, full_resolution=True)
            loss = bce(model.differentiable(left, right), gt) + 0.1 * (dsp(dl, gtl) + dsp(dr, gtr))
            loss.backward()
            opt.step()
            losses.append(loss.item())
        return {n: p.detach().clone() for n, p in model.named_parameters()}, losses

    a, la = three_steps()
    b, lb = three_steps()
    print(f"losses {la}")
    assert la == lb and all(np.isfinite(la))
    for n in a:
        assert torch.equal(a[n].view(torch.int32), b[n].view(torch.int32)), n
    for n in T._trained(s3r.Stereo2Voxel()):
        assert not torch.equal(a[n].cpu(), state[n]), f"{n} did not move"
