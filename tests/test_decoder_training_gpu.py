"""The whole decoder under autograd from the stereo feature maps — `start="v1"` of Decoder.differentiable_tail and of
VolumeEncoder.differentiable_features behind CostVolume.differentiable — at B = 1 on a seeded model and synthetic pairs: every
gradient against torch's float64 autograd of the oracle's graph, the forward value against the fused inference path, and a three-step
SGD loop run twice.

The tolerance of the gradient tests is not a measured number of the code under test.  The yardstick is torch's own float32 CPU
autograd of the SAME oracle graph against the same float64 result, computed here, per tensor in relative L2.  The HIP path may exceed
it by FACTOR = 8: DESIGN.md §2 documents the per-layer forward error of the kernels against float64 as 3e-7 .. 1e-6 for the direct
form and up to 4.7e-6 for the Winograd forms (tools/wino_numerics.py), and the activations the backward saves come from those
kernels.  Worst against worst that is 4.7e-6 / 1e-6 = 4.7, rounded up to a power of two.

ReLU gates: where this file departs from a plain float64 comparison, and why.  The derivative of a ReLU is a step, and a
pre-activation nearer to zero than the forward's own rounding error has no defined side: whichever way a path rounds it decides
whether that element's whole gradient passes.  ONE such element moves every gradient upstream of it by 1e-4 .. 1e-3 in relative L2.
Measured on an MI355X (docs/LAB_NOTES.md, "Cost-volume backward", has the table): against the plain float64 autograd every tensor from
d2 upstream was off by 3.0e-4 (d2.bn.bias) .. 2.2e-3 (fl), d3 and d4 by 1e-7 .. 4e-7; exactly two gates of 5.1 million differed, one
in d2 (float64 pre-activation 2.4e-6 at a mean |t| of 0.57) and one in v3 (1.0e-6), both inside the HIP forward's error; with those
two gates taken from the HIP path the same comparison gave 1.1e-7 .. 2.3e-6, at most 4.4 times the yardstick.  The float32 yardstick
happened to round all of them as float64 does; nothing makes it.  So the reference here is the float64 autograd of the oracle's graph
in which a ReLU whose float64 pre-activation lies within E of zero takes the gate of the path under test, and every other gate is
float64's own.  E, per layer AND channel (the folded BatchNorm scale sets a channel's error scale) = FACTOR times the largest
difference between the float32 CPU oracle's pre-activation and float64's in that channel: the same yardstick and the same factor,
applied to the forward.  tests/test_conv_backward_gpu.py's d3 test treats its gate the same way ("where the reference pre-activation
is within E_a of 0 the device may gate the other way").  Inside that window the reference is not independent of the code under test;
what keeps the window from hiding a defect: a gate that differs anywhere outside it fails the test outright, the window must hold
less than one element in 1000 of a layer, and the plain float64 figures are printed beside the asserted ones."""
import functools

import numpy as np
import pytest
import torch

from tests import _head64 as H64

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FACTOR = 8.0
LR = 0.05            # the learning rate of tests/test_conv_backward_gpu.py's d3 + d4 loop


def _rel(a, ref):
    return ((a.double() - ref).norm() / ref.norm()).item()


def _trained(module):
    return [n for n, _ in module.named_parameters() if not n.endswith("bn.weight")]


def _saved_activations(out):
    """layer name -> the output y that each differentiable_conv behind `out` saved for its backward (what its ReLU gate reads)"""
    ys, todo, seen = {}, [out.grad_fn], set()
    while todo:
        node = todo.pop()
        if node is None or node in seen:
            continue
        seen.add(node)
        if type(node).__name__ == "_ConvFunctionBackward":
            ys[node.layer.name] = node.saved_tensors[2].detach().cpu()
        todo.extend(f for f, _ in node.next_functions)
    return ys


def _oracle_pass(blocks, tail, fl, fr, dtype, gates=None, E=None):
    """the oracle's graph in `dtype` on the CPU: cost volume, the conv + BatchNorm + ReLU `blocks`, then `tail` (a scalar loss).
    gates / E: a ReLU whose pre-activation lies within E[name] of zero takes gates[name] (a bool tensor) instead of its own sign.
    Returns (loss, gradients by name, pre-activations by name, how many gates were undefined / differed inside / differed outside)"""
    from oracle import s2v_oracle as O
    a, b = fl.to(dtype).clone().requires_grad_(), fr.to(dtype).clone().requires_grad_()
    h = O.cost_volume(a, b)
    pre, counts = {}, {}
    for name, blk in blocks:
        t = blk.bn(blk.conv(h))
        pre[name] = t.detach()
        own = t.detach() > 0
        if gates is None:
            h = torch.relu(t)
        else:
            near = t.detach().abs() <= E[name]
            differ = own != gates[name]
            counts[name] = (int(near.sum()), int((differ & near).sum()), int((differ & ~near).sum()), t.numel())
            h = t * torch.where(near, gates[name], own).to(dtype)
    loss = tail(h)
    loss.backward()
    return loss.item(), {"fl": a.grad, "fr": b.grad}, pre, counts


def _references(module64, module32, blocks_of, tail_of, params_of, fl, fr, hip_activations):
    """(unmended float64 gradients, mended float64 gradients, float32 gradients, losses, gate counts): see the module docstring"""
    fl, fr = fl.cpu(), fr.cpu()
    l64, g64, pre64, _ = _oracle_pass(blocks_of(module64), tail_of(module64, torch.float64), fl, fr, torch.float64)
    g64.update({n: p.grad.clone() for n, p in params_of(module64)})
    l32, g32, pre32, _ = _oracle_pass(blocks_of(module32), tail_of(module32, torch.float32), fl, fr, torch.float32)
    g32.update({n: p.grad.clone() for n, p in params_of(module32)})
    E = {n: FACTOR * (pre32[n].double() - pre64[n]).abs().amax(dim=(0, 2, 3, 4), keepdim=True) for n in pre64}      # per channel
    gates = {n: hip_activations[n] > 0 for n in pre64}
    module64.zero_grad()
    _, m64, _, counts = _oracle_pass(blocks_of(module64), tail_of(module64, torch.float64), fl, fr, torch.float64, gates, E)
    m64.update({n: p.grad.clone() for n, p in params_of(module64)})
    return g64, m64, g32, (l64, l32), counts, E


def _compare(got, g64, m64, g32, counts, E, names):
    """per tensor: the HIP path's relative L2 error against the (gate-mended) float64 reference within FACTOR times the float32 CPU
    autograd's against float64"""
    for n, (near, inside, outside, total) in counts.items():
        print(f"{n}: E {E[n].min().item():.3e} .. {E[n].max().item():.3e} by channel; {near} of {total} pre-activations within E of zero, "
              f"{inside} of them gated the other way; {outside} gates differ outside")
        assert outside == 0, f"{n}: a ReLU gate differs where float64 is more than E away from zero"
        assert near <= 1e-3 * total, n
    bad = []
    for n in names:
        hip, cpu, raw = _rel(got[n].cpu(), m64[n]), _rel(g32[n], g64[n]), _rel(got[n].cpu(), g64[n])
        print(f"{n}: HIP {hip:.3e} (unmended float64: {raw:.3e}), torch float32 on the CPU {cpu:.3e}, ratio {hip / cpu:.2f}")
        assert g64[n].norm().item() > 0 and cpu < 1e-2, n           # the yardstick itself is a gradient
        if not hip <= FACTOR * cpu:
            bad.append((n, hip, cpu))
    assert not bad, bad


# ---------------------------------------------------------------- the voxel branch
@functools.lru_cache(maxsize=None)
def _voxel_problem():
    """the seeded model's state, one synthetic pair, its stereo features and a target grid, computed once and shared (left unchanged)"""
    import s3r
    model = s3r.Stereo2Voxel()
    s3r.seed_module(model, seed=0)
    state = {k: v.clone() for k, v in model.state_dict().items()}
    model.to(DEV)
    left, right = s3r.synthetic_pairs(1, seed=0, device=DEV)
    fl, fr = model.stereo_features(left, right)
    gt = (torch.rand(1, 32, 32, 32, generator=torch.Generator().manual_seed(2)) < 0.3).float()
    return state, (left, right), (fl, fr), gt


def _voxel_model(s3r):
    model = s3r.Stereo2Voxel()
    model.load_state_dict(_voxel_problem()[0])
    return model.to(DEV)


def test_voxel_decoder_gradients_from_the_features_against_float64(s3r, oracle):
    state, _, (fl, fr), gt = _voxel_problem()
    model = _voxel_model(s3r)
    a, b = fl.clone().requires_grad_(), fr.clone().requires_grad_()
    occ = model.decoder.differentiable_tail(model.cost_volume.differentiable(a, b), start="v1")
    loss = s3r.VoxelBCELoss()(occ, gt.to(DEV))
    acts = _saved_activations(loss)
    loss.backward()
    torch.cuda.synchronize()
    params = dict(model.decoder.named_parameters())
    names = _trained(model.decoder)
    assert len(names) == 3 * 9 + 2                                  # conv.weight, conv.bias, bn.bias of v1 .. d3; d4 has no BatchNorm
    assert list(acts) and set(acts) == set(model.decoder.names[:-1])
    for n, p in params.items():
        assert (p.grad is None) == n.endswith("bn.weight"), n
    assert all(p.grad is None for p in model.encoder.parameters())

    def make(dtype):
        dec = oracle.OracleDecoder().eval()
        dec.load_state_dict({k[len("decoder."):]: v for k, v in state.items() if k.startswith("decoder.")})
        return dec.to(dtype)

    blocks_of = lambda dec: [(n, getattr(dec, n)) for n in dec.names[:-1]]
    tail_of = lambda dec, dtype: lambda h: torch.nn.BCELoss()(dec.d4(h).squeeze(1), gt.to(dtype))
    g64, m64, g32, (l64, l32), counts, E = _references(make(torch.float64), make(torch.float32), blocks_of, tail_of,
                                                       lambda dec: dec.named_parameters(), fl, fr, acts)
    print(f"loss {loss.item():.7g}; float64 {l64:.7g}; float32 on the CPU {l32:.7g}")
    got = {"fl": a.grad, "fr": b.grad}
    got.update({n: params[n].grad for n in names})
    _compare(got, g64, m64, g32, counts, E, ["fl", "fr"] + names)


def test_value_from_v1_agrees_with_the_fused_forward(s3r):
    """differentiable_tail(cost_volume.differentiable(fl, fr), start="v1") against model(l, r), per voxel within tests/_head64.py's
    forward_bound — the bound tests/test_head_backward_gpu.py applies to the standalone head against the fused d3 + d4 pass — evaluated
    on the d3 activation of the v1 path.  Bit equality is not promised."""
    _, (left, right), (fl, fr), _ = _voxel_problem()
    model = _voxel_model(s3r)
    with torch.no_grad():
        feats = model.decoder.differentiable_features(model.cost_volume.differentiable(fl, fr), start="v1")
        head = model.decoder.differentiable_head(feats)
        fused = model(left, right)
        chain = model.head_features(left, right)
    torch.cuda.synchronize()
    assert head.shape == fused.shape == (1, 32, 32, 32)
    w, bias = model.decoder.d4.conv.weight.detach().cpu().numpy().reshape(-1), model.decoder.d4.conv.bias.item()
    y64, z, mag = H64.forward64(feats.cpu().numpy(), w, bias, "sigmoid")
    lim = H64.forward_bound(z, mag, y64)
    err = np.abs(head.cpu().numpy().astype(np.float64) - fused.cpu().numpy().astype(np.float64))
    print(f"v1 path vs fused forward: max |d| {err.max():.3e}, max err / bound {(err / lim).max():.4f}; d3 activation bit-identical to the "
          f"chain's: {torch.equal(feats.view(torch.int32), chain.view(torch.int32))}, max |d| {(feats - chain).abs().max().item():.3e}")
    assert (err <= lim).all()


def test_three_sgd_steps_on_the_whole_decoder_are_deterministic_and_descend(s3r):
    """three SGD steps on every trainable decoder parameter plus an additive perturbation of the two feature maps, twice from the same
    state: identical bits, and the loss after the third step is below the loss before the first"""
    state, _, (fl, fr), gt = _voxel_problem()
    gt = gt.to(DEV)

    def three_steps():
        model = _voxel_model(s3r)
        params = dict(model.decoder.named_parameters())
        names = _trained(model.decoder)
        dl, dr = torch.zeros_like(fl).requires_grad_(), torch.zeros_like(fr).requires_grad_()
        opt = torch.optim.SGD([params[n] for n in names] + [dl, dr], lr=LR)
        bce = s3r.VoxelBCELoss()
        run = lambda: bce(model.decoder.differentiable_tail(model.cost_volume.differentiable(fl + dl, fr + dr), start="v1"), gt)
        losses = []
        for _ in range(3):
            opt.zero_grad()
            loss = run()
            loss.backward()
            opt.step()
            losses.append(loss.item())
        with torch.no_grad():
            losses.append(run().item())
        out = {n: p.detach().clone() for n, p in model.decoder.named_parameters()}
        out.update({"dl": dl.detach().clone(), "dr": dr.detach().clone()})
        return out, losses

    a, la = three_steps()
    b, lb = three_steps()
    print(f"losses {la}")
    assert la == lb and all(np.isfinite(la))
    assert la[3] < la[0]
    for n in a:
        assert torch.equal(a[n].view(torch.int32), b[n].view(torch.int32)), n
    for n in _trained(s3r.Decoder()):
        assert not torch.equal(a[n].cpu(), state["decoder." + n]), f"{n} did not move"
    assert bool(a["dl"].abs().max() > 0) and bool(a["dr"].abs().max() > 0)


# ---------------------------------------------------------------- the point branch
def test_point_branch_gradients_from_the_features_against_float64(s3r, oracle):
    model = s3r.Stereo2Point()
    s3r.seed_module(model, seed=0)
    state = {k: v.clone() for k, v in model.state_dict().items()}
    model.to(DEV)
    left, right = s3r.synthetic_pairs(1, seed=0, device=DEV)
    fl, fr = model.stereo_features(left, right)
    target = torch.rand(1, 2048, 3, generator=torch.Generator().manual_seed(8)) - 0.5
    a, b = fl.clone().requires_grad_(), fr.clone().requires_grad_()
    latent = model.decoder.differentiable_features(model.cost_volume.differentiable(a, b), start="v1")
    assert latent.shape == (1, 512, 4, 4, 4)
    loss = s3r.ChamferDistance()(model.point_head.differentiable(latent), target.to(DEV))
    acts = _saved_activations(loss)
    loss.backward()
    torch.cuda.synchronize()
    names = ["decoder." + n for n in _trained(model.decoder)] + ["point_head." + n for n in _trained(model.point_head)]
    params = dict(model.named_parameters())
    assert len(names) == 3 * 6 + 2 * 3 and set(acts) == set(model.decoder.names)
    for n, p in params.items():
        assert (p.grad is None) == (n.endswith("bn.weight") or n.startswith("encoder.")), n

    def make(dtype):
        orc = oracle.OracleStereo2Point().eval()
        orc.load_state_dict(state)
        return orc.to(dtype)

    blocks_of = lambda orc: [(n, getattr(orc.decoder, n)) for n in orc.decoder.names]
    tail_of = lambda orc, dtype: lambda h: oracle.chamfer_loss(orc.point_head(h), target.to(dtype))
    params_of = lambda orc: [(n, p) for n, p in orc.named_parameters() if not n.startswith("encoder.")]
    g64, m64, g32, (l64, l32), counts, E = _references(make(torch.float64), make(torch.float32), blocks_of, tail_of, params_of, fl, fr, acts)
    print(f"loss {loss.item():.7g}; float64 {l64:.7g}; float32 on the CPU {l32:.7g}")
    got = {"fl": a.grad, "fr": b.grad}
    got.update({n: params[n].grad for n in names})
    _compare(got, g64, m64, g32, counts, E, ["fl", "fr"] + names)
