"""The stand-alone ops of the package: one C-ABI entry point each behind a functional form (`linear`, `conv_forward`, `voxel_bce`, ...),
its deterministic backward (`*_backward`), the `torch.autograd.Function` that joins the two (`differentiable_*`) and the loss modules
built on them (`ChamferDistance`, `VoxelBCELoss`, `DisparityLoss`), plus the metrics and disparity read-outs.  PyTorch is plumbing here
(device memory, streams, the autograd graph); every value and every gradient comes from a HIP kernel of libs3r_hip.so, and nothing
falls back to the CPU.  The networks (modules.py) are built from these; this file never imports them.

Every `*_backward` follows one order: validate (`_grad_and_output`: an activation's derivative needs the layer's output), allocate the
sides asked for (`_out`), give an empty batch its zero sums (`_zero_sums`), then query and allocate the scratch (`_scratch`) and call
the entry point with `None` for what is absent (`_ptrs`).
"""
from __future__ import annotations

import collections
import ctypes as C
import dataclasses
import weakref
from math import prod as _prod
from typing import Optional, Sequence

import torch
import torch.nn as nn

from . import _lib
from . import arch_spec as spec
from ._tensors import _aligned16, _check_channel_vector, _check_input, _check_input_cl, _stream_ptr
from .augment import augment_pair      # noqa: F401  (the augmentation's functional form lives with its config: augment.py)

_LINEAR_ACTS = ("none", "relu", "sigmoid")


def _out(shape, device, need=True, dtype=torch.float32):
    """an uninitialised result tensor, or None for a side that is not asked for"""
    return torch.empty(shape, dtype=dtype, device=device) if need else None


def _ptrs(*tensors):
    """the addresses the C-ABI takes; NULL for a tensor that is absent"""
    return [None if t is None else t.data_ptr() for t in tensors]


def _scratch(need, what, device):
    """the scratch of one call: `need` is the entry point's size answer (checked as `what`), at least one float is allocated"""
    return torch.empty(max(_lib.check(need, what), 1), dtype=torch.float32, device=device)


def _zero_sums(*sums):
    """an empty batch: the sums over it are zero, and no kernel runs"""
    for t in sums:
        if t is not None:
            t.zero_()


def _holds(B, shape_tail, unit="samples"):
    """a check(t, name) for `_grad_and_output`: t as a contiguous fp32 (B, *shape_tail) tensor (unit None: `linear_backward`'s wording)"""
    def check(t, name):
        t = _check_input(t, name, shape_tail)
        if t.shape[0] != B:
            raise RuntimeError(f"{name} must hold {B} {unit}, got {t.shape[0]}" if unit else
                               f"{name} must have batch {B}, got {tuple(t.shape)}")
        return t
    return check


def _grad_and_output(who, act, y, grad_y, check, detach_y=True):
    """(grad_y, y) of a backward, each through `check`: an act other than "none" needs the layer's output y, of grad_y's shape and batch
    (detached first where the op always detached it: conv, stem, batchnorm)"""
    gy = check(grad_y, "grad_y")
    if act == "none":
        return gy, None
    if y is None:
        raise RuntimeError(f"{who}: act {act!r} needs the layer's output y")
    return gy, check(y.detach() if detach_y else y, "y")


def _check_linear(x, weight, act, who):
    if act not in _LINEAR_ACTS:
        raise RuntimeError(f"{who}: act must be one of {_LINEAR_ACTS}, got {act!r}")
    if x.dim() != 2 or weight.dim() != 2 or x.shape[1] != weight.shape[1]:
        raise RuntimeError(f"{who} expects x (B,Cin) and weight (Cout,Cin), got {tuple(x.shape)} and {tuple(weight.shape)}")
    x = _check_input(x, "x", (weight.shape[1],))
    w = weight.detach()
    if w.device != x.device or w.dtype != torch.float32 or not w.is_contiguous():
        raise RuntimeError(f"{who}: weight must be a contiguous fp32 tensor on {x.device}")
    if w.numel() == 0:
        raise RuntimeError(f"{who} needs a non-empty weight")
    return x, w


@torch.no_grad()
def linear(x: torch.Tensor, weight: torch.Tensor, bias: Optional[torch.Tensor], act: str = "none") -> torch.Tensor:
    """act(x weight^T + bias) on the HIP linear kernels (`s3r_linear_forward`): x (B,Cin), weight (Cout,Cin) in torch layout,
    bias (Cout) or None; act "none", "relu" or "sigmoid".  Records no graph (`differentiable_linear` does)."""
    x, w = _check_linear(x, weight, act, "linear")
    B, cin, cout = x.shape[0], w.shape[1], w.shape[0]
    b = None
    if bias is not None:
        b = bias.detach()
        if b.shape != (cout,) or b.device != x.device or b.dtype != torch.float32 or not b.is_contiguous():
            raise RuntimeError(f"linear: bias must be a contiguous fp32 ({cout},) tensor on {x.device}")
    y = _out((B, cout), x.device)
    if B:
        lib = _lib.load()
        scratch = _scratch(lib.s3r_linear_scratch_elems(B, cin, cout), "linear scratch query", x.device)
        _lib.check(lib.s3r_linear_forward(x.data_ptr(), w.data_ptr(), *_ptrs(b), y.data_ptr(), B, cin, cout,
                                          _lib.ACT[act], scratch.data_ptr(), scratch.numel(), _stream_ptr(x.device)), "linear")
    return y


@torch.no_grad()
def linear_backward(x: torch.Tensor, weight: torch.Tensor, y: Optional[torch.Tensor], grad_y: torch.Tensor, act: str,
                    need_x: bool = True, need_w: bool = True, need_b: bool = True):
    """(grad_x (B,Cin), grad_w (Cout,Cin), grad_bias (Cout)) of y = act(x weight^T + bias) for the output gradient grad_y (B,Cout),
    `None` for the sides not asked for (`s3r_linear_backward`).  y is the layer's output (it may be None when act is "none").  Fixed
    summation orders, no atomics: the same bits on every run.  A side that is not needed costs neither its GEMM nor its traffic."""
    x, w = _check_linear(x, weight, act, "linear_backward")
    if not (need_x or need_w or need_b):
        raise RuntimeError("linear_backward needs need_x, need_w or need_b")
    B, cin, cout = x.shape[0], w.shape[1], w.shape[0]
    gy, yy = _grad_and_output("linear_backward", act, y, grad_y, _holds(B, (cout,), None), detach_y=False)
    dev = x.device
    gx, gw, gb = _out((B, cin), dev, need_x), _out((cout, cin), dev, need_w), _out((cout,), dev, need_b)
    if B == 0:
        _zero_sums(gw, gb)
        return gx, gw, gb
    lib = _lib.load()
    scratch = _scratch(lib.s3r_linear_backward_scratch_elems(B, cin, cout), "linear backward scratch query", dev)
    _lib.check(lib.s3r_linear_backward(x.data_ptr(), w.data_ptr(), *_ptrs(yy, gy, gx, gw, gb), B, cin, cout, _lib.ACT[act],
                                       scratch.data_ptr(), scratch.numel(), _stream_ptr(dev)), "linear backward")
    return gx, gw, gb


class _LinearFunction(torch.autograd.Function):
    """`linear` with `linear_backward` as its derivative; saves x, weight and y"""

    @staticmethod
    def forward(ctx, x, weight, bias, act):
        y = linear(x, weight, bias, act)
        ctx.act = act
        ctx.save_for_backward(x, weight, y)
        return y

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_y):
        x, weight, y = ctx.saved_tensors
        need_x, need_w, need_b = ctx.needs_input_grad[:3]
        if not (need_x or need_w or need_b):
            return None, None, None, None
        gx, gw, gb = linear_backward(x, weight, y, grad_y.contiguous().float(), ctx.act, need_x, need_w, need_b)
        return gx, gw, gb, None


def differentiable_linear(x: torch.Tensor, weight: torch.Tensor, bias: Optional[torch.Tensor], act: str = "none") -> torch.Tensor:
    """`linear` recorded for autograd: the same bits, with the deterministic backward `linear_backward`, called with exactly the
    sides autograd needs (`needs_input_grad`).  A B = 0 input gives zero gradients without a kernel call."""
    return _LinearFunction.apply(x, weight, bias, act)


@torch.no_grad()
def chamfer_distance(p: torch.Tensor, q: torch.Tensor):
    """(dist1 (B,N), dist2 (B,M), idx1 (B,N) int32, idx2 (B,M) int32): squared-L2 nearest neighbours (`s3r_chamfer_forward`).
    The distance is ((dx*dx + dy*dy) + dz*dz) in fp32, each operation rounded once.  idx is the FIRST minimum: the lowest index
    holding the smallest distance, as one sequential scan with a strict `<` finds it.  Minima are taken over the distances that are
    not NaN (IEEE minNum); a query with no candidate below +inf gets dist = +inf, idx = 0.  Inputs are expected finite: a
    non-finite point has the distance +inf itself, so it shows up as a non-finite loss and never hides behind a finite one."""
    if p.dim() != 3 or q.dim() != 3 or p.shape[-1] != 3 or q.shape[-1] != 3 or p.shape[0] != q.shape[0]:
        raise RuntimeError(f"chamfer_distance expects (B,N,3) and (B,M,3), got {tuple(p.shape)} and {tuple(q.shape)}")
    p = _check_input(p, "p", p.shape[1:])
    q = _check_input(q, "q", q.shape[1:])
    B, N, M = p.shape[0], p.shape[1], q.shape[1]
    if N == 0 or M == 0:
        raise RuntimeError("chamfer_distance needs non-empty point clouds")
    d1, d2 = _out((B, N), p.device), _out((B, M), p.device)
    i1, i2 = _out((B, N), p.device, dtype=torch.int32), _out((B, M), p.device, dtype=torch.int32)
    if B:
        _lib.check(_lib.load().s3r_chamfer_forward(p.data_ptr(), q.data_ptr(), d1.data_ptr(), d2.data_ptr(),
                                                   i1.data_ptr(), i2.data_ptr(), B, N, M, _stream_ptr(p.device)),
                   "chamfer")
    return d1, d2, i1, i2


@torch.no_grad()
def chamfer_distance_backward(p: torch.Tensor, q: torch.Tensor, idx1: torch.Tensor, idx2: torch.Tensor, grad_dist1, grad_dist2,
                              need_p: bool = True, need_q: bool = True):
    """(grad_p (B,N,3) or None, grad_q (B,M,3) or None) of sum(grad_dist1 * dist1) + sum(grad_dist2 * dist2), the indices of
    `chamfer_distance` held fixed (`s3r_chamfer_backward`): a gather with a fixed summation order — own term first, then the
    scattered terms in ascending source index, fp32, no fused multiply-adds, no atomics — so the bits do not depend on the run or on
    the batch split.  grad_dist1 / grad_dist2: (B,N) / (B,M) fp32, or None for zeros (not both); need_p / need_q: the sides to compute."""
    if p.dim() != 3 or q.dim() != 3 or p.shape[-1] != 3 or q.shape[-1] != 3 or p.shape[0] != q.shape[0]:
        raise RuntimeError(f"chamfer_distance_backward expects (B,N,3) and (B,M,3), got {tuple(p.shape)} and {tuple(q.shape)}")
    p = _check_input(p, "p", p.shape[1:])
    q = _check_input(q, "q", q.shape[1:])
    B, N, M = p.shape[0], p.shape[1], q.shape[1]
    if N == 0 or M == 0:
        raise RuntimeError("chamfer_distance_backward needs non-empty point clouds")
    if grad_dist1 is None and grad_dist2 is None:
        raise RuntimeError("chamfer_distance_backward needs grad_dist1 or grad_dist2")
    if not (need_p or need_q):
        raise RuntimeError("chamfer_distance_backward needs need_p or need_q")
    idx1 = _check_input(idx1, "idx1", (N,), torch.int32)
    idx2 = _check_input(idx2, "idx2", (M,), torch.int32)
    g1 = None if grad_dist1 is None else _check_input(grad_dist1, "grad_dist1", (N,))
    g2 = None if grad_dist2 is None else _check_input(grad_dist2, "grad_dist2", (M,))
    for t, name in ((idx1, "idx1"), (idx2, "idx2"), (g1, "grad_dist1"), (g2, "grad_dist2")):
        if t is not None and t.shape[0] != B:
            raise RuntimeError(f"{name} must have batch {B}, got {tuple(t.shape)}")
    gp, gq = _out((B, N, 3), p.device, need_p), _out((B, M, 3), p.device, need_q)
    if B:
        _lib.check(_lib.load().s3r_chamfer_backward(p.data_ptr(), q.data_ptr(), idx1.data_ptr(), idx2.data_ptr(),
                                                    *_ptrs(g1, g2, gp, gq), B, N, M, _stream_ptr(p.device)), "chamfer backward")
    return gp, gq


class _ChamferFunction(torch.autograd.Function):
    """`chamfer_distance` with `chamfer_distance_backward` as its derivative (the indices are constants of the graph)"""

    @staticmethod
    def forward(ctx, p, q):
        d1, d2, i1, i2 = chamfer_distance(p, q)
        ctx.mark_non_differentiable(i1, i2)
        ctx.set_materialize_grads(False)                           # an unused dist1 / dist2 arrives as None: NULL, not a zero tensor
        ctx.save_for_backward(p, q, i1, i2)
        return d1, d2, i1, i2

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g1, g2, _gi1, _gi2):
        p, q, i1, i2 = ctx.saved_tensors
        need_p, need_q = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        if (g1 is None and g2 is None) or not (need_p or need_q):
            return None, None
        g1 = None if g1 is None else g1.contiguous().float()
        g2 = None if g2 is None else g2.contiguous().float()
        return chamfer_distance_backward(p, q, i1, i2, g1, g2, need_p, need_q)


def differentiable_chamfer_distance(p: torch.Tensor, q: torch.Tensor):
    """`chamfer_distance` recorded for autograd: (dist1, dist2, idx1, idx2), the same bits; dist1 / dist2 carry the deterministic
    backward `chamfer_distance_backward`, idx1 / idx2 are non-differentiable."""
    return _ChamferFunction.apply(p, q)


class ChamferDistance(nn.Module):
    """Drop-in for the reference's extensions/chamfer_dist module (README.md:64-65): forward(p, q)
    returns mean(dist1) + mean(dist2).  (Whether the reference reduces with mean or sum, squared or
    not, is unknown — SURVEY.md §8a row 5; `chamfer_distance` exposes the unreduced tensors.)
    A loss as well as a metric: with grad mode on and p or q requiring grad the value (the same bits) is recorded for autograd
    through `differentiable_chamfer_distance`; otherwise nothing is recorded."""

    def forward(self, p, q):
        if torch.is_grad_enabled() and (p.requires_grad or q.requires_grad):
            d1, d2, _, _ = differentiable_chamfer_distance(p, q)
        else:
            d1, d2, _, _ = chamfer_distance(p, q)
        return d1.mean() + d2.mean()


def _check_bce(pred, target, who):
    if not isinstance(pred, torch.Tensor) or not isinstance(target, torch.Tensor):
        raise TypeError(f"{who}: pred and target must be torch.Tensors")
    if pred.dim() < 2 or pred.shape != target.shape:
        raise RuntimeError(f"{who} expects pred and target of one shape (B, ...), got {tuple(pred.shape)} and {tuple(target.shape)}")
    p = _check_input(pred.detach(), "pred", pred.shape[1:])
    t = _check_input(target.detach(), "target", target.shape[1:])
    voxels = _prod(pred.shape[1:])
    if voxels == 0:
        raise RuntimeError(f"{who} needs non-empty samples")
    return p, t, pred.shape[0], voxels


@torch.no_grad()
def voxel_bce(pred: torch.Tensor, target: torch.Tensor, elements: bool = False):
    """(loss_sum (B), loss_elem or None) of torch.nn.BCELoss's per-element rule on pred, target (B, ...) (`s3r_voxel_bce_forward`):
    l = -(t * clamp(log p) + (1 - t) * clamp(log(1 - p))), the logs clamped at -100 before the multiplication; loss_sum[b] is the fp32
    sum of sample b's losses in a fixed order that depends on the sample size only (include/s3r.h), so it has the same bits in every
    batch split; loss_elem (the shape of pred) is returned with `elements=True`.  A NaN or out-of-range pred makes that sample's sum
    NaN (torch raises instead).  Records no graph (`differentiable_voxel_bce` does)."""
    p, t, B, V = _check_bce(pred, target, "voxel_bce")
    s, e = _out((B,), p.device), _out(p.shape, p.device, elements)
    if B:
        _lib.check(_lib.load().s3r_voxel_bce_forward(p.data_ptr(), t.data_ptr(), s.data_ptr(), *_ptrs(e), B, V, _stream_ptr(p.device)),
                   "voxel_bce")
    return s, e


@torch.no_grad()
def voxel_bce_backward(pred: torch.Tensor, target: torch.Tensor, grad_scale: torch.Tensor) -> torch.Tensor:
    """grad_pred (the shape of pred) of sum_b grad_scale[b] * loss_sum[b] (`s3r_voxel_bce_backward`): grad_scale[b] * (p - t) /
    max((1 - p) * p, 1e-12), each operation rounded once — torch's binary_cross_entropy_backward, elementwise and bit for bit."""
    p, t, B, V = _check_bce(pred, target, "voxel_bce_backward")
    gs = _check_input(grad_scale, "grad_scale", ())
    if gs.shape[0] != B:
        raise RuntimeError(f"grad_scale must have shape ({B},), got {tuple(gs.shape)}")
    g = _out(p.shape, p.device)
    if B:
        _lib.check(_lib.load().s3r_voxel_bce_backward(p.data_ptr(), t.data_ptr(), gs.data_ptr(), g.data_ptr(), B, V, _stream_ptr(p.device)),
                   "voxel_bce backward")
    return g


class _VoxelBCEFunction(torch.autograd.Function):
    """`voxel_bce`'s loss_sum with `voxel_bce_backward` as its derivative; the gradient goes to pred only"""

    @staticmethod
    def forward(ctx, pred, target):
        s, _ = voxel_bce(pred, target)
        ctx.save_for_backward(pred, target)
        return s

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_sum):
        pred, target = ctx.saved_tensors
        if not ctx.needs_input_grad[0]:
            return None, None
        return voxel_bce_backward(pred, target, grad_sum.contiguous().float()), None


def differentiable_voxel_bce(pred: torch.Tensor, target: torch.Tensor) -> torch.Tensor:
    """`voxel_bce`'s loss_sum (B) recorded for autograd: the same bits, with the elementwise backward `voxel_bce_backward`.  The
    gradient goes to pred only (a target is a constant of the loss)."""
    return _VoxelBCEFunction.apply(pred, target)


class VoxelBCELoss(nn.Module):
    """torch.nn.BCELoss (mean reduction) on occupancy grids: forward(pred, target) with pred, target (B,32,32,32) or any (B, ...)
    returns the mean over all elements, `loss_sum.double().sum() / (B V)` cast to fp32 — the per-sample sums are the HIP kernel's,
    in its fixed order.  With grad mode on and pred requiring grad the value (the same bits) is recorded for autograd through
    `differentiable_voxel_bce`; otherwise nothing is recorded (as `ChamferDistance`)."""

    def forward(self, pred, target):
        if torch.is_grad_enabled() and pred.requires_grad:
            s = differentiable_voxel_bce(pred, target)
        else:
            s, _ = voxel_bce(pred, target)
        return (s.double().sum() / max(pred.numel(), 1)).float()


def _check_head(x, weight, act, who):
    if act not in _LINEAR_ACTS:
        raise RuntimeError(f"{who}: act must be one of {_LINEAR_ACTS}, got {act!r}")
    if not isinstance(x, torch.Tensor) or x.dim() < 3:
        raise RuntimeError(f"{who} expects x (B, C, ...), got {tuple(getattr(x, 'shape', ()))}")
    if weight.numel() != x.shape[1]:
        raise RuntimeError(f"{who} expects a weight of {x.shape[1]} elements (Conv(C -> 1, k = 1)), got {tuple(weight.shape)}")
    x = _check_input(x.detach(), "x", x.shape[1:])
    w = weight.detach()
    if w.device != x.device or w.dtype != torch.float32 or not w.is_contiguous():
        raise RuntimeError(f"{who}: weight must be a contiguous fp32 tensor on {x.device}")
    positions = _prod(x.shape[2:])
    if x.shape[1] == 0 or positions == 0:
        raise RuntimeError(f"{who} needs non-empty channels and positions")
    return x, w.view(-1), positions


def _check_head_bias(bias, device, who):
    if bias is None:
        return None
    b = bias.detach()
    if b.numel() != 1 or b.device != device or b.dtype != torch.float32:
        raise RuntimeError(f"{who}: bias must be one fp32 element on {device}")
    return b.reshape(1)


@torch.no_grad()
def head(x: torch.Tensor, weight: torch.Tensor, bias: Optional[torch.Tensor], act: str = "sigmoid") -> torch.Tensor:
    """The pointwise head act(sum_c x[:, c] weight[c] + bias) as `s3r_conv_forward` runs a Conv(C -> 1, k = 1) layer ALONE: x
    (B,C,n,n) or (B,C,n,n,n) with one edge n, weight any shape of C elements (an nn.Conv's (1,C,1,1,1)), bias one element or None;
    act "none", "relu" or "sigmoid".  Returns (B,n,n[,n]).  Records no graph (`differentiable_head` does)."""
    x, w, _ = _check_head(x, weight, act, "head")
    b = _check_head_bias(bias, x.device, "head")
    nd = x.dim() - 2
    n = x.shape[2]
    if nd not in (2, 3) or any(e != n for e in x.shape[2:]):
        raise RuntimeError(f"head expects x (B,C,n,n) or (B,C,n,n,n) with one edge n, got {tuple(x.shape)}")
    B, cin = x.shape[0], x.shape[1]
    y = _out((B,) + tuple(x.shape[2:]), x.device)
    if B == 0:
        return y
    lib = _lib.load()
    desc = _lib.ConvDesc(_lib.OP_CONV, nd, B, cin, 1, n, 1, 1, 0, _lib.ACT[act], 0, -1, 0, 0, 0, 0, 0, 0, 0, 1, 0, 0.0)
    stream = _stream_ptr(x.device)
    elems = C.c_int64(0)
    _lib.check(lib.s3r_conv_packed_elems(C.byref(desc), C.byref(elems)), "head: packed_elems")
    pw = _out(elems.value, x.device)
    _lib.check(lib.s3r_conv_pack_weights(C.byref(desc), w.data_ptr(), pw.data_ptr(), stream), "head: pack_weights")
    scratch = _scratch(lib.s3r_conv_scratch_elems(C.byref(desc)), "head: scratch query", x.device)
    _lib.check(lib.s3r_conv_forward(C.byref(desc), x.data_ptr(), pw.data_ptr(), None, *_ptrs(b), y.data_ptr(),
                                    scratch.data_ptr(), scratch.numel(), stream), "head")
    return y


@torch.no_grad()
def head_backward(x: torch.Tensor, weight: torch.Tensor, y: Optional[torch.Tensor], grad_y: torch.Tensor, act: str,
                  need_x: bool = True, need_w: bool = True, need_b: bool = True, scale: Optional[torch.Tensor] = None):
    """(grad_x (the shape of x), grad_w (C), grad_bias (1)) of y = act((sum_c x[:, c] weight[c]) * scale + bias) for the output
    gradient grad_y (B, ...), `None` for the sides not asked for (`s3r_head_backward`).  x (B,C,...) with any positions per sample, y
    the layer's output (it may be None when act is "none"), scale one frozen fp32 element or None for 1.  One streaming pass, fixed
    summation orders, no atomics: the same bits on every run.  Without need_x grad_x is not written, without need_w x is not read."""
    x, w, S = _check_head(x, weight, act, "head_backward")
    if not (need_x or need_w or need_b):
        raise RuntimeError("head_backward needs need_x, need_w or need_b")
    B, cin, dev = x.shape[0], x.shape[1], x.device

    def flat(t, name):
        t = _check_input(t, name, t.shape[1:])
        if t.shape[0] != B or t.numel() != B * S:
            raise RuntimeError(f"{name} must hold (B, positions) = ({B}, {S}) elements, got {tuple(t.shape)}")
        return t

    gy, yy = _grad_and_output("head_backward", act, y, grad_y, flat, detach_y=False)
    sc = _check_head_bias(scale, dev, "head_backward (scale)")
    gx, gw, gb = _out(x.shape, dev, need_x), _out((cin,), dev, need_w), _out((1,), dev, need_b)
    if B == 0:
        _zero_sums(gw, gb)
        return gx, gw, gb
    lib = _lib.load()
    scratch = _scratch(lib.s3r_head_backward_scratch_elems(B, cin, S), "head backward scratch query", dev)
    _lib.check(lib.s3r_head_backward(x.data_ptr(), w.data_ptr(), *_ptrs(sc, yy, gy, gx, gw, gb), B, cin, S, _lib.ACT[act],
                                     scratch.data_ptr(), scratch.numel(), _stream_ptr(dev)), "head backward")
    return gx, gw, gb


class _HeadFunction(torch.autograd.Function):
    """`head` with `head_backward` as its derivative; saves x, weight and y"""

    @staticmethod
    def forward(ctx, x, weight, bias, act):
        y = head(x, weight, bias, act)
        ctx.act = act
        ctx.save_for_backward(x, weight, y)
        return y

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_y):
        x, weight, y = ctx.saved_tensors
        need_x, need_w, need_b = ctx.needs_input_grad[:3]
        if not (need_x or need_w or need_b):
            return None, None, None, None
        gx, gw, gb = head_backward(x, weight, y, grad_y.contiguous().float(), ctx.act, need_x, need_w, need_b)
        return gx, None if gw is None else gw.view(weight.shape), gb, None


def differentiable_head(x: torch.Tensor, weight: torch.Tensor, bias: Optional[torch.Tensor], act: str = "sigmoid") -> torch.Tensor:
    """`head` recorded for autograd: the same bits (the value of `s3r_conv_forward` on the head layer alone), with the deterministic
    backward `head_backward`, called with exactly the sides autograd needs (`needs_input_grad`); gradients come back in the
    parameters' own shapes.  A B = 0 input gives zero gradients without a kernel call."""
    return _HeadFunction.apply(x, weight, bias, act)


# ---------------------------------------------------------------------------------------------------------------------------------
# One convolution layer under autograd: the forward as a one-layer chain, the backward as s3r_conv_backward + the adjoint layer's forward
_CONV_OPS = ("conv2d", "conv3d", "deconv2d", "deconv3d")
_PACKED_FOR = collections.OrderedDict()      # (id(weight), device, descriptor) -> (weakref to the weight, version, packed image)
_PACKED_MAX = 32


def _packed_for(weight: torch.Tensor, desc) -> torch.Tensor:
    """`weight` (torch layout) packed for `desc`: ONE image per (weight object, layer), valid for the `_version` it was packed at — what
    `_HipChain._ensure_packed` keys on too.  An in-place update of the parameter (an optimizer step) bumps `_version`, and the new image
    REPLACES the old one.  The weak reference tells a live tensor from another one that got a dead one's `id` (an address is no
    identity either: the allocator hands a freed block to the next tensor of the same size)."""
    sig = tuple(getattr(desc, n) for n in ("op", "ndim", "cin", "cout", "in_size", "k", "stride", "pad", "out_pad", "dtype", "algo"))
    key = (id(weight), str(weight.device), sig)
    hit = _PACKED_FOR.get(key)
    if hit is not None and hit[0]() is weight and hit[1] == weight._version:
        _PACKED_FOR.move_to_end(key)
        return hit[2]
    lib = _lib.load()
    one = _lib.ConvDesc.from_buffer_copy(desc)
    one.batch = 1
    n = C.c_int64(0)
    _lib.check(lib.s3r_conv_packed_elems(C.byref(one), C.byref(n)), "packed_elems")
    w = weight.detach().float().contiguous()
    pw = _out(n.value, w.device)
    _lib.check(lib.s3r_conv_pack_weights(C.byref(one), w.data_ptr(), pw.data_ptr(), _stream_ptr(w.device)), "pack_weights")
    _PACKED_FOR[key] = (weakref.ref(weight), weight._version, pw)
    _PACKED_FOR.move_to_end(key)
    for k in [k for k, v in _PACKED_FOR.items() if v[0]() is None]:      # images of tensors that are gone
        del _PACKED_FOR[k]
    while len(_PACKED_FOR) > _PACKED_MAX:
        _PACKED_FOR.popitem(last=False)
    return pw


def _run_one_layer(desc, x: torch.Tensor, pw: torch.Tensor, scale, shift, y: torch.Tensor) -> torch.Tensor:
    """One layer through `s3r_chain_forward`: `s3r_conv_forward` behind the halo-padded copy of an unpadded input that the layer's
    kernel may read its zero padding from (the chain plans that copy itself; a single `s3r_conv_forward` call refuses such a layer)."""
    lib = _lib.load()
    arr = (_lib.Layer * 1)()
    arr[0].desc = desc
    arr[0].packed_w = pw.data_ptr()
    arr[0].scale = scale.data_ptr() if scale is not None else None
    arr[0].shift = shift.data_ptr() if shift is not None else None
    ws = _scratch(lib.s3r_chain_workspace_elems(arr, 1), "workspace query", x.device)
    _lib.check(lib.s3r_chain_forward(arr, 1, x.data_ptr(), y.data_ptr(), ws.data_ptr(), ws.numel(), 1, _stream_ptr(x.device)),
               "one-layer chain")
    return y


def _check_conv(x, weight, layer, who):
    if layer.op not in _CONV_OPS:
        raise RuntimeError(f"{who} takes a conv2d / conv3d / deconv2d / deconv3d layer, got {layer.op!r}")
    if layer.act not in _LINEAR_ACTS:
        raise RuntimeError(f"{who}: act must be one of {_LINEAR_ACTS}, got {layer.act!r}")
    if layer.dil != 1:
        raise RuntimeError(f"{who}: dilation 1 only")
    nd = spec.ndim(layer)
    if not isinstance(x, torch.Tensor) or x.dim() != nd + 2 or x.shape[1] != layer.cin or any(e != x.shape[2] for e in x.shape[2:]):
        raise RuntimeError(f"{who} expects x (B, {layer.cin}, n{', n' * (nd - 1)}) with one edge n, got {tuple(getattr(x, 'shape', ()))}")
    x = _check_input(x.detach(), "x", x.shape[1:])
    want = ((layer.cin, layer.cout) if layer.op.startswith("deconv") else (layer.cout, layer.cin)) + (layer.k,) * nd
    w = weight.detach()
    if tuple(w.shape) != want or w.device != x.device or w.dtype != torch.float32 or not w.is_contiguous():
        raise RuntimeError(f"{who}: weight must be a contiguous fp32 tensor of shape {want} on {x.device}, got {tuple(w.shape)}")
    n = x.shape[2]
    m = spec.out_size(layer, n)
    if m <= 0:
        raise RuntimeError(f"{who}: the layer has no output over an edge of {n}")
    return x, w, n, (x.shape[0], layer.cout) + (m,) * nd


@torch.no_grad()
def conv_forward(x: torch.Tensor, weight: torch.Tensor, scale: Optional[torch.Tensor], shift: Optional[torch.Tensor],
                 layer: spec.Layer) -> torch.Tensor:
    """act(conv(x, weight) * scale + shift) of ONE arch_spec layer (conv2d / conv3d / deconv2d / deconv3d, dilation 1, act none /
    relu / sigmoid) under the library's AUTO algorithm, as a one-layer `s3r_chain_forward`.  Records no graph."""
    x, w, n, yshape = _check_conv(x, weight, layer, "conv_forward")
    sc = _check_channel_vector(scale, layer.cout, x.device, "conv_forward", "scale")
    sh = _check_channel_vector(shift, layer.cout, x.device, "conv_forward", "shift")
    y = _out(yshape, x.device)
    if x.shape[0] == 0:
        return y
    desc = _lib.make_desc(layer, x.shape[0], n)
    return _run_one_layer(desc, x, _packed_for(weight, desc), sc, sh, y)


@torch.no_grad()
def conv_backward(x: torch.Tensor, weight: torch.Tensor, y: Optional[torch.Tensor], grad_y: torch.Tensor, layer: spec.Layer,
                  scale: Optional[torch.Tensor] = None, need_x: bool = True, need_w: bool = True, need_shift: bool = True):
    """(grad_x, grad_w, grad_shift) of y = act(conv(x, weight) * scale + shift) for the output gradient grad_y, `None` for the sides not
    asked for.  ONE `s3r_conv_backward` call (gs = g * scale, grad_w in the weight's torch shape, grad_shift (cout): fixed summation
    orders, no atomics, the same bits on every run and for every batch a sample appears in) and then, when need_x, the forward of the
    adjoint layer (`s3r_conv_adjoint_desc`) on gs with this layer's own weight tensor, packed once per weight tensor and `_version`.  y may
    be None when the layer's act is "none"; scale (cout) is frozen: it gets no gradient."""
    x, w, n, yshape = _check_conv(x, weight, layer, "conv_backward")
    if not (need_x or need_w or need_shift):
        raise RuntimeError("conv_backward needs need_x, need_w or need_shift")
    B, dev = x.shape[0], x.device
    gy, yy = _grad_and_output("conv_backward", layer.act, y, grad_y, _holds(B, yshape[1:]))
    sc = _check_channel_vector(scale, layer.cout, dev, "conv_backward", "scale")
    gx, gs = _out(x.shape, dev, need_x), _out(yshape, dev, need_x)
    gw, gb = _out(w.shape, dev, need_w), _out((layer.cout,), dev, need_shift)
    if B == 0:
        _zero_sums(gw, gb)
        return gx, gw, gb
    lib = _lib.load()
    desc = _lib.make_desc(layer, B, n)
    scratch = _scratch(lib.s3r_conv_backward_scratch_elems(C.byref(desc)), "conv backward scratch query", dev)
    _lib.check(lib.s3r_conv_backward(C.byref(desc), *_ptrs(x if need_w else None, yy, gy, sc, gs, gw, gb), scratch.data_ptr(),
                                     scratch.numel(), _stream_ptr(dev)), "conv backward")
    if need_x:
        adj = _lib.ConvDesc()
        _lib.check(lib.s3r_conv_adjoint_desc(C.byref(desc), C.byref(adj)), "conv adjoint descriptor")
        _run_one_layer(adj, gs, _packed_for(weight, adj), None, None, gx)
    return gx, gw, gb


class _ConvFunction(torch.autograd.Function):
    """`conv_forward` with `conv_backward` as its derivative; saves x, weight, scale and y"""

    @staticmethod
    def forward(ctx, x, weight, scale, shift, layer):
        y = conv_forward(x, weight, scale, shift, layer)
        ctx.layer = layer
        ctx.has_scale = scale is not None
        ctx.save_for_backward(x, weight, y, *((scale,) if scale is not None else ()))
        return y

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_y):
        x, weight, y = ctx.saved_tensors[:3]
        scale = ctx.saved_tensors[3] if ctx.has_scale else None
        need_x, need_w, need_shift = ctx.needs_input_grad[0], ctx.needs_input_grad[1], ctx.needs_input_grad[3]
        if not (need_x or need_w or need_shift):
            return None, None, None, None, None
        gx, gw, gb = conv_backward(x, weight, y, grad_y.contiguous().float(), ctx.layer, scale, need_x, need_w, need_shift)
        return gx, gw, None, gb, None


def differentiable_conv(x: torch.Tensor, weight: torch.Tensor, scale: Optional[torch.Tensor], shift: Optional[torch.Tensor],
                        layer: spec.Layer) -> torch.Tensor:
    """`conv_forward` recorded for autograd: the value of the layer's kernel under the AUTO algorithm, with the deterministic backward
    `conv_backward`, called with exactly the sides autograd needs (`needs_input_grad` of x, weight and shift).  `scale` is frozen: its
    gradient is `None` (a folded BatchNorm scale: `bn.weight` is not trained through this path)."""
    return _ConvFunction.apply(x, weight, scale, shift, layer)


# ---------------------------------------------------------------------------------------------------------------------------------
# The stem's backward: s3r_stem_backward
def _check_stem_render(x, name):
    if not isinstance(x, torch.Tensor) or x.dim() != 4 or x.shape[1] != 3 or x.shape[2] != x.shape[3] or x.shape[2] < 1:
        raise RuntimeError(f"{name} must be renders (N, 3, n, n), got {tuple(getattr(x, 'shape', ()))}")
    dt = torch.uint8 if x.dtype == torch.uint8 else torch.float32
    return _aligned16(_check_input(x.detach(), name, x.shape[1:], dt))


@torch.no_grad()
def stem_backward(left: torch.Tensor, right: Optional[torch.Tensor], y: Optional[torch.Tensor], grad_y: torch.Tensor,
                  scale: Optional[torch.Tensor] = None, act: str = "relu", need_w: bool = True, need_shift: bool = True):
    """(grad_w, grad_shift) of the stem y = act(conv2d(X, w; 3 -> 32, k 3, s 2, p 1) * scale + shift) for the output gradient grad_y
    (N,32,m,m), `None` for the side not asked for: ONE `s3r_stem_backward` call.  X are the renders as the forward reads them, float32
    or uint8 (scaled by 1/255 as they are read), `left` then `right` (None: one tensor) — no conversion, no concatenation.  Fixed
    summation orders, no atomics: the same bits for one tensor or two, for uint8 renders and their host conversion, and grad_w of a batch
    is the ascending sum of its images' results.  y may be None when act is "none"; scale (32) is frozen."""
    if act not in ("none", "relu"):
        raise RuntimeError(f"stem_backward: act must be 'none' or 'relu', got {act!r}")
    if not (need_w or need_shift):
        raise RuntimeError("stem_backward needs need_w or need_shift")
    left = _check_stem_render(left, "left")
    n, dev = left.shape[2], left.device
    if right is not None:
        right = _check_stem_render(right, "right")
        if tuple(right.shape[1:]) != tuple(left.shape[1:]) or right.dtype != left.dtype or right.device != dev:
            raise RuntimeError("left and right renders must share one edge, dtype and device")
        if right.shape[0] == 0:
            right = None
        elif left.shape[0] == 0:
            left, right = right, None
    N = left.shape[0] + (right.shape[0] if right is not None else 0)
    m = (n - 1) // 2 + 1
    gy, yy = _grad_and_output("stem_backward", act, y, grad_y, _holds(N, (32, m, m), "images"))
    sc = _check_channel_vector(scale, 32, dev, "stem_backward", "scale")
    gw, gb = _out((32, 3, 3, 3), dev, need_w), _out((32,), dev, need_shift)
    if N == 0:
        _zero_sums(gw, gb)
        return gw, gb
    lib = _lib.load()
    scratch = _scratch(lib.s3r_stem_backward_scratch_elems(N, n), "stem backward scratch query", dev)
    _lib.check(lib.s3r_stem_backward(left.data_ptr(), *_ptrs(right), left.shape[0], int(left.dtype == torch.uint8),
                                     *_ptrs(yy, gy, sc, gw, gb), N, n, _lib.ACT[act], scratch.data_ptr(), scratch.numel(),
                                     _stream_ptr(dev)), "stem backward")
    return gw, gb


class _StemFunction(torch.autograd.Function):
    """The encoder's first block with `stem_backward` as its derivative with respect to (weight, shift); the renders get no gradient.
    act "relu": the stem kernel itself on the renders as given — the one-layer chain `encoder._run(left, "e1", 0, right)`, which reads the
    encoder's own e1 parameters (`weight`, `shift` and `scale` ARE those, handed in so that autograd sees them).  act "none" (the
    batch-statistics form; scale None, shift = conv.bias): the stem kernel has no form without its activation, so the forward is
    `conv_forward` on the fp32 conversion of the concatenated renders; the backward reads the renders as given either way."""

    @staticmethod
    def forward(ctx, weight, shift, scale, encoder, left, right, act):
        if act == "none":
            x = left if right is None else torch.cat([left, right], 0)
            if x.dtype == torch.uint8:                             # IEEE division by a device tensor: the kernels' correctly rounded u / 255
                x = x.float() / torch.full((), 255.0, device=x.device)     # (a Python-scalar divisor may be turned into a reciprocal)
            y = conv_forward(x, weight, None, shift, dataclasses.replace(encoder._layers[0], act="none"))
        else:
            y = encoder._run(left, encoder.names[0], 0, right)
        ctx.act, ctx.has_scale, ctx.has_right = act, scale is not None, right is not None
        ctx.save_for_backward(left, y, *((right,) if right is not None else ()), *((scale,) if scale is not None else ()))
        return y

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_y):
        saved = list(ctx.saved_tensors)
        left, y = saved[0], saved[1]
        right = saved[2] if ctx.has_right else None
        scale = saved[-1] if ctx.has_scale else None
        need_w, need_shift = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        if not (need_w or need_shift):
            return (None,) * 7
        gw, gb = stem_backward(left, right, y if ctx.act != "none" else None, grad_y.contiguous().float(), scale, ctx.act, need_w,
                               need_shift)
        return gw, gb, None, None, None, None, None


# ---------------------------------------------------------------------------------------------------------------------------------
# Train-mode BatchNorm (batch statistics) + activation: s3r_batchnorm_train_forward / _backward
def _check_bn(z, who):
    if not isinstance(z, torch.Tensor) or z.dim() < 2:
        raise RuntimeError(f"{who} expects z (B, C, ...), got {tuple(getattr(z, 'shape', ()))}")
    z = _check_input(z.detach(), "z", z.shape[1:])
    S = _prod(z.shape[2:])
    if z.shape[1] == 0 or S == 0:
        raise RuntimeError(f"{who} needs non-empty channels and positions")
    if z.shape[0] * S < 2:
        raise RuntimeError(f"{who}: batch statistics need more than one value per channel, got z {tuple(z.shape)}")
    return z, S


@torch.no_grad()
def batchnorm_train_forward(z: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, eps: float, act: str = "none"):
    """(y, mean, var, invstd) of train-mode BatchNorm + activation on z (B,C,...) (`s3r_batchnorm_train_forward`): per channel the batch
    mean and the BIASED variance in two passes, invstd = 1 / sqrt(var + eps), y = act(((z - mean) * invstd) * gamma + beta) with nothing
    fused; gamma, beta (C); act "none", "relu" or "sigmoid".  Fixed summation orders, no atomics: the same bits on every run.  A sample's
    result depends on the batch it is in.  Records no graph (`differentiable_batchnorm` does)."""
    if act not in _LINEAR_ACTS:
        raise RuntimeError(f"batchnorm_train_forward: act must be one of {_LINEAR_ACTS}, got {act!r}")
    z, S = _check_bn(z, "batchnorm_train_forward")
    B, ch, dev = z.shape[0], z.shape[1], z.device
    ga = _check_channel_vector(gamma, ch, dev, "batchnorm_train_forward", "gamma")
    be = _check_channel_vector(beta, ch, dev, "batchnorm_train_forward", "beta")
    y = torch.empty_like(z)
    mean, var, invstd = (_out((ch,), dev) for _ in range(3))
    lib = _lib.load()
    scratch = _scratch(lib.s3r_batchnorm_train_forward_scratch_elems(B, ch, S), "batchnorm forward scratch query", dev)
    _lib.check(lib.s3r_batchnorm_train_forward(z.data_ptr(), ga.data_ptr(), be.data_ptr(), float(eps), _lib.ACT[act], y.data_ptr(),
                                               mean.data_ptr(), var.data_ptr(), invstd.data_ptr(), B, ch, S, scratch.data_ptr(),
                                               scratch.numel(), _stream_ptr(dev)), "batchnorm forward")
    return y, mean, var, invstd


@torch.no_grad()
def batchnorm_train_backward(z: torch.Tensor, y: Optional[torch.Tensor], grad_y: torch.Tensor, gamma: torch.Tensor, mean: torch.Tensor,
                             invstd: torch.Tensor, act: str, need_z: bool = True, need_gamma: bool = True, need_beta: bool = True):
    """(grad_z, grad_gamma, grad_beta) of `batchnorm_train_forward` for the output gradient grad_y (the shape of z), `None` for the sides
    not asked for (`s3r_batchnorm_train_backward`): z, y, mean and invstd are the forward's (y may be None when act is "none").  One pass
    for the two sums, a finish, one pass for grad_z; fixed summation orders, no atomics.  A side that is not asked for is not written."""
    if act not in _LINEAR_ACTS:
        raise RuntimeError(f"batchnorm_train_backward: act must be one of {_LINEAR_ACTS}, got {act!r}")
    if not (need_z or need_gamma or need_beta):
        raise RuntimeError("batchnorm_train_backward needs need_z, need_gamma or need_beta")
    z, S = _check_bn(z, "batchnorm_train_backward")
    B, ch, dev = z.shape[0], z.shape[1], z.device
    gy, yy = _grad_and_output("batchnorm_train_backward", act, y, grad_y, _holds(B, z.shape[1:]))
    ga, mu, iv = (_check_channel_vector(v, ch, dev, "batchnorm_train_backward", n)
                  for v, n in ((gamma, "gamma"), (mean, "mean"), (invstd, "invstd")))
    gz, gg, gb = _out(z.shape, dev, need_z), _out((ch,), dev, need_gamma), _out((ch,), dev, need_beta)
    lib = _lib.load()
    scratch = _scratch(lib.s3r_batchnorm_train_backward_scratch_elems(B, ch, S), "batchnorm backward scratch query", dev)
    _lib.check(lib.s3r_batchnorm_train_backward(z.data_ptr(), *_ptrs(yy), gy.data_ptr(), ga.data_ptr(), mu.data_ptr(), iv.data_ptr(),
                                                _lib.ACT[act], *_ptrs(gz, gg, gb), B, ch, S, scratch.data_ptr(), scratch.numel(),
                                                _stream_ptr(dev)), "batchnorm backward")
    return gz, gg, gb


class _BatchNormTrainFunction(torch.autograd.Function):
    """`batchnorm_train_forward` with `batchnorm_train_backward` as its derivative; saves z, gamma, y, mean and invstd.  mean and var
    are returned for the running statistics and carry no gradient."""

    @staticmethod
    def forward(ctx, z, gamma, beta, eps, act):
        y, mean, var, invstd = batchnorm_train_forward(z, gamma, beta, eps, act)
        ctx.act = act
        ctx.save_for_backward(z, gamma, y, mean, invstd)
        ctx.mark_non_differentiable(mean, var)
        return y, mean, var

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_y, _gmean, _gvar):
        z, gamma, y, mean, invstd = ctx.saved_tensors
        need_z, need_gamma, need_beta = ctx.needs_input_grad[:3]
        if not (need_z or need_gamma or need_beta):
            return None, None, None, None, None
        gz, gg, gb = batchnorm_train_backward(z, y, grad_y.contiguous().float(), gamma, mean, invstd, ctx.act, need_z, need_gamma, need_beta)
        return gz, gg, gb, None, None


def differentiable_batchnorm(z: torch.Tensor, bn: nn.Module, act: str = "none") -> torch.Tensor:
    """act(bn(z)) of an affine `nn.BatchNorm2d` / `nn.BatchNorm3d` (any `_BatchNorm`) with BATCH statistics — torch's training mode,
    whatever `bn.training` says — recorded for autograd: `batchnorm_train_forward`'s bits, with the deterministic backward
    `batchnorm_train_backward` called with exactly the sides autograd needs (`needs_input_grad` of z, `bn.weight`, `bn.bias`).  When
    `bn.track_running_stats` is set the running statistics and `num_batches_tracked` are updated as torch updates them: with
    `bn.momentum` (None: the cumulative average 1 / num_batches_tracked) and the UNBIASED variance var * N / (N - 1), in torch operations
    on the (C) vectors under no_grad."""
    if not isinstance(bn, nn.modules.batchnorm._BatchNorm) or bn.weight is None or bn.bias is None:
        raise RuntimeError("differentiable_batchnorm takes an affine nn.BatchNorm1d / 2d / 3d module")
    if not isinstance(z, torch.Tensor) or z.dim() < 2 or z.shape[1] != bn.num_features:
        raise RuntimeError(f"differentiable_batchnorm expects z (B, {bn.num_features}, ...), got {tuple(getattr(z, 'shape', ()))}")
    y, mean, var = _BatchNormTrainFunction.apply(z, bn.weight, bn.bias, float(bn.eps), act)
    if bn.track_running_stats and bn.running_mean is not None:
        with torch.no_grad():
            n = z.numel() // z.shape[1]
            bn.num_batches_tracked += 1
            f = 1.0 / float(bn.num_batches_tracked) if bn.momentum is None else float(bn.momentum)
            bn.running_mean.mul_(1.0 - f).add_(mean, alpha=f)
            bn.running_var.mul_(1.0 - f).add_(var * (n / (n - 1.0)), alpha=f)
    return y


@torch.no_grad()
def cost_volume_backward(grad_volume: torch.Tensor, need_left: bool = True, need_right: bool = True):
    """(grad_left, grad_right), (B,C,H,W) each and `None` for the side not asked for, of the plain cost volume for its output gradient
    grad_volume (B,2C,D,H,W): ONE `s3r_cost_volume_backward` call.  Every element is its own sequential fp32 sum in ascending d (no
    atomics: the same bits on every run and for every batch a sample appears in); the volume's structural zeros are never read."""
    if not (need_left or need_right):
        raise RuntimeError("cost_volume_backward needs need_left or need_right")
    if not isinstance(grad_volume, torch.Tensor) or grad_volume.dim() != 5 or grad_volume.shape[1] % 2 or grad_volume.shape[1] == 0:
        raise RuntimeError(f"cost_volume_backward expects grad_volume (B, 2C, D, H, W), got {tuple(getattr(grad_volume, 'shape', ()))}")
    gv = _check_input(grad_volume.detach(), "grad_volume", grad_volume.shape[1:])
    B, C2, D, H, W = gv.shape
    if min(D, H, W) < 1:
        raise RuntimeError(f"cost_volume_backward: D, H and W must be positive, got {tuple(gv.shape)}")
    gl, gr = _out((B, C2 // 2, H, W), gv.device, need_left), _out((B, C2 // 2, H, W), gv.device, need_right)
    if B == 0:
        return gl, gr
    _lib.check(_lib.load().s3r_cost_volume_backward(gv.data_ptr(), *_ptrs(gl, gr), B, C2 // 2, D, H, W, _stream_ptr(gv.device)),
               "cost volume backward")
    return gl, gr


class _CostVolumeFunction(torch.autograd.Function):
    """the plain `s3r_cost_volume_forward` (halo 0) with `cost_volume_backward` as its derivative; saves nothing (the operator is linear)"""

    @staticmethod
    def forward(ctx, feat_left, feat_right, max_disp):
        if feat_left.shape != feat_right.shape or feat_left.dim() != 4:
            raise RuntimeError(f"feature maps must both be (B,C,H,W), got {tuple(feat_left.shape)} and {tuple(feat_right.shape)}")
        fl = _check_input(feat_left.detach(), "feat_left", feat_left.shape[1:])
        fr = _check_input(feat_right.detach(), "feat_right", feat_left.shape[1:])
        B, Cc, H, W = fl.shape
        vol = _out((B, 2 * Cc, int(max_disp), H, W), fl.device)
        if B:
            _lib.check(_lib.load().s3r_cost_volume_forward(fl.data_ptr(), fr.data_ptr(), vol.data_ptr(), B, Cc, int(max_disp), H, W, 0,
                                                           _stream_ptr(fl.device)), "cost_volume")
        return vol

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_volume):
        need_l, need_r = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        if not (need_l or need_r):
            return None, None, None
        gl, gr = cost_volume_backward(grad_volume.contiguous().float(), need_l, need_r)
        return gl, gr, None


def differentiable_cost_volume(feat_left: torch.Tensor, feat_right: torch.Tensor, max_disp: int = spec.MAX_DISP) -> torch.Tensor:
    """The plain fp32 cost volume (B,2C,D,H,W) recorded for autograd: the value has the bits of `CostVolume.forward` (the same kernel call),
    the backward is `cost_volume_backward`, called with exactly the sides autograd needs (`needs_input_grad` of the two maps)."""
    return _CostVolumeFunction.apply(feat_left, feat_right, max_disp)


@torch.no_grad()
def voxel_iou(pred: torch.Tensor, gt: torch.Tensor, threshold: float = 0.5) -> torch.Tensor:
    """Per-sample IoU of (pred > th) vs (gt > th), computed on the device: (B,...) -> (B,) (`s3r_voxel_iou`).  Occupied means
    strictly greater than the threshold ROUNDED TO fp32, compared in fp32 (a voxel holding float32(0.3) is not occupied at 0.3);
    NaN is not occupied.  The counts are exact; the result is float32(intersection) / float32(union), conversions
    round-to-nearest-even, 1 for an empty union."""
    if pred.shape != gt.shape:
        raise RuntimeError("pred and gt shapes differ")
    pred = _check_input(pred, "pred", pred.shape[1:])
    gt = _check_input(gt, "gt", gt.shape[1:])
    B = pred.shape[0]
    out = torch.empty((B,), dtype=torch.float32, device=pred.device)
    if B:
        _lib.check(_lib.load().s3r_voxel_iou(pred.data_ptr(), gt.data_ptr(), float(threshold), out.data_ptr(), B,
                                             pred[0].numel(), _stream_ptr(pred.device)), "voxel_iou")
    return out


@torch.no_grad()
def disparity_wta(feat_l: torch.Tensor, feat_r: torch.Tensor, max_disp: int = spec.MAX_DISP):
    """Predicted left / right disparity maps (ground truth: disp_%02d_{l,r}.exr,
    /root/reference/README.md:75-76): winner-take-all over the shift-and-diff costs the cost volume holds, read
    straight from the two feature maps.  (B,C,H,W) x2 fp32 -> two (B,H,W) fp32 maps, integer-valued, in
    feature-resolution pixels; disp_l[b,h,w] = first argmin_d sum_c |L[b,c,h,w] - R[b,c,h,w-d]|, disp_r mirrored."""
    if feat_l.shape != feat_r.shape or feat_l.dim() != 4:
        raise RuntimeError("feat_l / feat_r must be two (B,C,H,W) tensors of one shape")
    feat_l = _check_input(feat_l.float(), "feat_l", feat_l.shape[1:])
    feat_r = _check_input(feat_r.float(), "feat_r", feat_r.shape[1:])
    B, Cc, H, W = feat_l.shape
    dl = torch.empty((B, H, W), dtype=torch.float32, device=feat_l.device)
    dr = torch.empty_like(dl)
    if B:
        _lib.check(_lib.load().s3r_disparity_wta(feat_l.data_ptr(), feat_r.data_ptr(), dl.data_ptr(), dr.data_ptr(), B,
                                                 Cc, H, W, int(max_disp), _stream_ptr(feat_l.device)), "disparity_wta")
    return dl, dr


@torch.no_grad()
def disparity_soft(feat_l: torch.Tensor, feat_r: torch.Tensor, max_disp: int = spec.MAX_DISP, temperature: float = 1.0,
                   out_size: Optional[Sequence[int]] = None, scale: float = 1.0, confidence: bool = False):
    """Sub-pixel disparity read-out (`s3r_disparity_soft`; a stand-in like `disparity_wta`, not a learned head): per pixel the
    soft-argmin sum_d d p_d, p_d = softmax_d(-c(d) / temperature), over the SAME shift-and-diff costs c(d) the WTA takes the argmin
    of, and the confidence p_best = 1 / sum_d exp((min c - c(d)) / temperature).  Features: fp32 (B,C,H,W), or the bf16 encoder's
    logical (B,C,H,W) channels-last tensors as they are (no conversion pass; same bits as the fp32 call on `channels_last_to_f32`).
    out_size=None: (B,H,W) maps; else (B,*out_size), upsampled bilinearly (torch's align_corners=False).  Disparities are
    multiplied by `scale` (8: render pixels).  Returns (dl, dr), or (dl, dr, cl, cr) with confidence=True.  One kernel launch; torch
    only allocates."""
    if feat_l.dim() != 4 or feat_l.shape != feat_r.shape:
        raise RuntimeError("feat_l / feat_r must be two (B,C,H,W) tensors of one shape")
    if feat_l.dtype != feat_r.dtype or feat_l.dtype not in (torch.float32, torch.bfloat16):
        raise RuntimeError(f"features must both be float32 (NCHW) or bfloat16 (channels-last), got {feat_l.dtype} / {feat_r.dtype}")
    bf16 = feat_l.dtype == torch.bfloat16
    chk = _check_input_cl if bf16 else _check_input
    pl, pr = chk(feat_l, "feat_l", feat_l.shape[1:], feat_l.dtype), chk(feat_r, "feat_r", feat_r.shape[1:], feat_r.dtype)
    # (bf16: the kernel reads rows in 16-byte pieces; _check_input_cl copies a view at an odd storage offset once)
    B, Cc, H, W = feat_l.shape
    OH, OW = (H, W) if out_size is None else (int(out_size[0]), int(out_size[1]))
    dev = feat_l.device
    outs = [_out((B, OH, OW), dev) for _ in range(4 if confidence else 2)]
    if B:
        ptr = _ptrs(*outs) + [None] * (4 - len(outs))
        _lib.check(_lib.load().s3r_disparity_soft(pl.data_ptr(), pr.data_ptr(), _lib.DTYPE["bf16" if bf16 else "fp32"], *ptr, B,
                                                  Cc, H, W, int(max_disp), float(temperature), OH, OW, float(scale),
                                                  _stream_ptr(dev)), "disparity_soft")
    return tuple(outs)


def _check_soft_features(feat_l, feat_r, who):
    if not isinstance(feat_l, torch.Tensor) or not isinstance(feat_r, torch.Tensor) or feat_l.dim() != 4 or feat_l.shape != feat_r.shape:
        raise RuntimeError(f"{who}: feat_l / feat_r must be two (B,C,H,W) tensors of one shape")
    if feat_l.dtype != torch.float32 or feat_r.dtype != torch.float32:
        raise RuntimeError(f"{who} reads float32 (NCHW) features only (no bf16 backward exists), got {feat_l.dtype} / {feat_r.dtype}")
    return (_check_input(feat_l.detach(), "feat_l", feat_l.shape[1:]), _check_input(feat_r.detach(), "feat_r", feat_r.shape[1:]))


@torch.no_grad()
def disparity_soft_backward(feat_l: torch.Tensor, feat_r: torch.Tensor, grad_disp_l: Optional[torch.Tensor],
                            grad_disp_r: Optional[torch.Tensor], max_disp: int = spec.MAX_DISP, temperature: float = 1.0,
                            out_size: Optional[Sequence[int]] = None, scale: float = 1.0, need_left: bool = True,
                            need_right: bool = True):
    """(grad_left, grad_right), (B,C,H,W) each and `None` for the side not asked for, of `disparity_soft`'s two disparity maps for their
    gradients grad_disp_l / grad_disp_r (B,*out_size) (either may be None: zeros): ONE `s3r_disparity_soft_backward` call with the
    forward's max_disp, temperature, out_size and scale.  Nothing is saved by the forward: the kernel recomputes the costs and the softmax.
    Every output element is its own sequential fp32 sum in ascending d and the upsample's adjoint is a gather in a fixed order (no
    atomics: the same bits on every run and for every batch a sample appears in).  fp32 features only."""
    if not (need_left or need_right):
        raise RuntimeError("disparity_soft_backward needs need_left or need_right")
    if grad_disp_l is None and grad_disp_r is None:
        raise RuntimeError("disparity_soft_backward needs grad_disp_l or grad_disp_r")
    fl, fr = _check_soft_features(feat_l, feat_r, "disparity_soft_backward")
    B, Cc, H, W = fl.shape
    OH, OW = (H, W) if out_size is None else (int(out_size[0]), int(out_size[1]))
    grads = [None if g is None else _check_input(g.detach(), name, (OH, OW))
             for g, name in ((grad_disp_l, "grad_disp_l"), (grad_disp_r, "grad_disp_r"))]
    if any(g is not None and g.shape[0] != B for g in grads):
        raise RuntimeError(f"disparity_soft_backward: the disparity gradients must be ({B},{OH},{OW})")
    gl, gr = _out(fl.shape, fl.device, need_left), _out(fl.shape, fl.device, need_right)
    if B:
        _lib.check(_lib.load().s3r_disparity_soft_backward(fl.data_ptr(), fr.data_ptr(), _lib.DTYPE["fp32"], *_ptrs(*grads, gl, gr), B, Cc, H, W,
                                                           int(max_disp), float(temperature), OH, OW, float(scale),
                                                           _stream_ptr(fl.device)), "disparity_soft backward")
    return gl, gr


class _DisparitySoftFunction(torch.autograd.Function):
    """`disparity_soft`'s two disparity maps with `disparity_soft_backward` as their derivative; saves the two feature maps only"""

    @staticmethod
    def forward(ctx, feat_l, feat_r, max_disp, temperature, size, scale):
        fl, fr = _check_soft_features(feat_l, feat_r, "differentiable_disparity_soft")
        ctx.save_for_backward(feat_l, feat_r)
        ctx.args = (int(max_disp), float(temperature), None if size is None else (int(size[0]), int(size[1])), float(scale))
        dl, dr = disparity_soft(fl, fr, ctx.args[0], ctx.args[1], ctx.args[2], ctx.args[3])
        return dl, dr

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_l, grad_r):
        need_l, need_r = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        if not (need_l or need_r):
            return None, None, None, None, None, None
        feat_l, feat_r = ctx.saved_tensors
        max_disp, tau, size, scale = ctx.args
        gl, gr = disparity_soft_backward(feat_l, feat_r, grad_l.contiguous().float(), grad_r.contiguous().float(), max_disp, tau, size,
                                         scale, need_l, need_r)
        return gl, gr, None, None, None, None


def differentiable_disparity_soft(feat_l: torch.Tensor, feat_r: torch.Tensor, max_disp: int = spec.MAX_DISP, temperature: float = 1.0,
                                  size: Optional[Sequence[int]] = None, scale: float = 1.0):
    """`disparity_soft`'s (disp_l, disp_r) recorded for autograd: the values have the bits of `disparity_soft` (the same kernel call), the
    backward is `disparity_soft_backward`, called with exactly the sides autograd needs (`needs_input_grad` of the two maps).  fp32
    features (B,C,H,W); size=None: (B,H,W) maps, else (B,*size) upsampled bilinearly; disparities are multiplied by `scale`.  The
    confidence maps are not returned (they get no gradient), and the temperature is a constant."""
    return _DisparitySoftFunction.apply(feat_l, feat_r, max_disp, temperature, size, scale)


def _check_disparity_loss(pred, gt, beta, who):
    if not isinstance(pred, torch.Tensor) or not isinstance(gt, torch.Tensor):
        raise TypeError(f"{who}: pred and gt must be torch.Tensors")
    if pred.dim() < 2 or pred.shape != gt.shape:
        raise RuntimeError(f"{who} expects pred and gt of one shape (B, ...), got {tuple(pred.shape)} and {tuple(gt.shape)}")
    beta = float(beta)
    if not (beta >= 0.0) or beta == float("inf"):
        raise ValueError(f"{who}: beta must be finite and >= 0, got {beta}")
    p = _check_input(pred.detach(), "pred", pred.shape[1:])
    t = _check_input(gt.detach(), "gt", gt.shape[1:])
    pixels = _prod(pred.shape[1:])
    if pixels == 0:
        raise RuntimeError(f"{who} needs non-empty samples")
    return p, t, pred.shape[0], pixels, beta


@torch.no_grad()
def disparity_loss(pred: torch.Tensor, gt: torch.Tensor, beta: float = 1.0, elements: bool = False):
    """(loss_sum (B), count (B) int32, loss_elem or None) of the smooth-L1 loss on the pixels whose ground truth is valid (finite and
    >= 0, as `disparity_metrics`) (`s3r_disparity_loss_forward`): with e = pred - gt, l = 0.5 e^2 / beta where |e| < beta, else
    |e| - 0.5 beta (beta = 0: plain L1); an invalid pixel counts as +0.0 and its values never enter arithmetic.  loss_sum[b] is the fp32
    sum in `voxel_bce`'s fixed order (a function of the sample size only: the same bits in every batch split), count[b] the valid
    pixels; loss_elem (the shape of pred) is returned with `elements=True`.  Records no graph (`differentiable_disparity_loss` does)."""
    p, t, B, P, beta = _check_disparity_loss(pred, gt, beta, "disparity_loss")
    s, n, e = _out((B,), p.device), _out((B,), p.device, dtype=torch.int32), _out(p.shape, p.device, elements)
    if B:
        _lib.check(_lib.load().s3r_disparity_loss_forward(p.data_ptr(), t.data_ptr(), beta, s.data_ptr(), n.data_ptr(), *_ptrs(e), B, P,
                                                          _stream_ptr(p.device)), "disparity_loss")
    return s, n, e


@torch.no_grad()
def disparity_loss_backward(pred: torch.Tensor, gt: torch.Tensor, grad_scale: torch.Tensor, beta: float = 1.0) -> torch.Tensor:
    """grad_pred (the shape of pred) of sum_b grad_scale[b] * loss_sum[b] (`s3r_disparity_loss_backward`): grad_scale[b] *
    clamp((pred - gt) / beta, -1, 1) at a valid pixel (grad_scale[b] * sgn(pred - gt) at beta = 0), exactly +0.0 at an invalid one —
    elementwise and bit for bit."""
    p, t, B, P, beta = _check_disparity_loss(pred, gt, beta, "disparity_loss_backward")
    gs = _check_input(grad_scale, "grad_scale", ())
    if gs.shape[0] != B:
        raise RuntimeError(f"grad_scale must have shape ({B},), got {tuple(gs.shape)}")
    g = _out(p.shape, p.device)
    if B:
        _lib.check(_lib.load().s3r_disparity_loss_backward(p.data_ptr(), t.data_ptr(), gs.data_ptr(), beta, g.data_ptr(), B, P,
                                                           _stream_ptr(p.device)), "disparity_loss backward")
    return g


class _DisparityLossFunction(torch.autograd.Function):
    """`disparity_loss`'s loss_sum with `disparity_loss_backward` as its derivative; the gradient goes to pred only.  count is returned
    beside it as a constant."""

    @staticmethod
    def forward(ctx, pred, gt, beta):
        s, n, _ = disparity_loss(pred, gt, beta)
        ctx.save_for_backward(pred, gt)
        ctx.beta = float(beta)
        ctx.mark_non_differentiable(n)
        return s, n

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_sum, _grad_count):
        pred, gt = ctx.saved_tensors
        if not ctx.needs_input_grad[0]:
            return None, None, None
        return disparity_loss_backward(pred, gt, grad_sum.contiguous().float(), ctx.beta), None, None


def differentiable_disparity_loss(pred: torch.Tensor, gt: torch.Tensor, beta: float = 1.0):
    """`disparity_loss`'s (loss_sum (B), count (B)) with loss_sum recorded for autograd: the same bits, with the elementwise backward
    `disparity_loss_backward`.  The gradient goes to pred only (a ground truth is a constant of the loss)."""
    return _DisparityLossFunction.apply(pred, gt, beta)


class DisparityLoss(nn.Module):
    """Smooth-L1 loss (torch.nn.SmoothL1Loss's rule with `beta`; beta = 0 is L1) of a disparity map against a ground truth with invalid
    pixels: forward(pred, gt) with pred, gt (B,H,W) or any (B, ...) returns the mean over the VALID pixels of the batch (ground truth
    finite and >= 0: the EXR maps mark background as inf or negative), `loss_sum.double().sum() / max(count.sum(), 1)` cast to fp32 —
    the per-sample sums and counts are the HIP kernel's, the sums in its fixed order.  A batch without a valid pixel gives 0 and a
    zero gradient.  With grad mode on and pred requiring grad the value (the same bits) is recorded for autograd through
    `differentiable_disparity_loss`; otherwise nothing is recorded (as `VoxelBCELoss`)."""

    def __init__(self, beta: float = 1.0):
        super().__init__()
        beta = float(beta)
        if not (beta >= 0.0) or beta == float("inf"):
            raise ValueError(f"DisparityLoss: beta must be finite and >= 0, got {beta}")
        self.beta = beta

    def forward(self, pred, gt):
        if torch.is_grad_enabled() and isinstance(pred, torch.Tensor) and pred.requires_grad:
            s, n = differentiable_disparity_loss(pred, gt, self.beta)
        else:
            s, n, _ = disparity_loss(pred, gt, self.beta)
        return (s.double().sum() / n.sum().clamp(min=1).double()).float()


@torch.no_grad()
def disparity_metrics(pred: torch.Tensor, gt: torch.Tensor):
    """Stereo metrics per sample (`s3r_disparity_metrics`) over the pixels whose ground truth is valid (finite, >= 0):
    (B,...) x2 fp32 -> (epe (B,) fp32, equal bit for bit to `disparity_epe`; counts (B,4) int32 = valid pixels, |err| > 1,
    |err| > 3, D1 = |err| > 3 and |err| > 0.05 gt).  Integer counts: rates pool exactly over samples and ranks."""
    if pred.shape != gt.shape:
        raise RuntimeError("pred and gt shapes differ")
    pred = _check_input(pred, "pred", pred.shape[1:])
    gt = _check_input(gt, "gt", gt.shape[1:])
    B = pred.shape[0]
    epe = torch.empty((B,), dtype=torch.float32, device=pred.device)
    counts = torch.empty((B, 4), dtype=torch.int32, device=pred.device)
    if B:
        _lib.check(_lib.load().s3r_disparity_metrics(pred.data_ptr(), gt.data_ptr(), epe.data_ptr(), counts.data_ptr(), B,
                                                     pred[0].numel(), _stream_ptr(pred.device)), "disparity_metrics")
    return epe, counts


@torch.no_grad()
def disparity_epe(pred: torch.Tensor, gt: torch.Tensor):
    """Per-sample end-point error mean|pred - gt| over the pixels whose ground truth is valid (finite and >= 0 — EXR
    disparity maps mark background with inf / negative values), reduced on the device: (B,...) x2 ->
    (epe (B,) fp32, valid pixel count (B,) int32)."""
    if pred.shape != gt.shape:
        raise RuntimeError("pred and gt shapes differ")
    pred = _check_input(pred, "pred", pred.shape[1:])
    gt = _check_input(gt, "gt", gt.shape[1:])
    B = pred.shape[0]
    epe = torch.empty((B,), dtype=torch.float32, device=pred.device)
    cnt = torch.empty((B,), dtype=torch.int32, device=pred.device)
    if B:
        _lib.check(_lib.load().s3r_disparity_epe(pred.data_ptr(), gt.data_ptr(), epe.data_ptr(), cnt.data_ptr(), B,
                                                 pred[0].numel(), _stream_ptr(pred.device)), "disparity_epe")
    return epe, cnt


def _check_surface(volume, sample_ids, n_points, seed):
    if not isinstance(volume, torch.Tensor) or volume.dim() != 4:
        raise RuntimeError("volume must be a (B, D, H, W) fp32 tensor")
    volume = _check_input(volume, "volume", volume.shape[1:])
    B = volume.shape[0]
    if not isinstance(sample_ids, torch.Tensor) or sample_ids.dtype != torch.int64 or tuple(sample_ids.shape) != (B,) \
            or sample_ids.device != volume.device or not sample_ids.is_contiguous():
        raise RuntimeError(f"sample_ids must be a contiguous ({B},) int64 tensor on {volume.device}")
    if int(n_points) < 1:
        raise ValueError(f"n_points must be positive, got {n_points!r}")
    if not 0 <= int(seed) < 2 ** 64:
        raise ValueError(f"seed must be in [0, 2^64), got {seed!r}")
    return volume


@torch.no_grad()
def voxel_surface_points(volume: torch.Tensor, sample_ids: torch.Tensor, n_points: int = 2048, seed: int = 0, threshold: float = 0.5,
                         return_counts: bool = False, out=None, scratch=None):
    """(B, n_points, 3) clouds in [-0.5, 0.5]^3 drawn on the exposed faces of the (B, D, H, W) fp32 occupancy grids
    (`s3r_voxel_surface_points`, include/s3r.h: a sampling rule INVENTED by this build).  sample_ids (B,) int64 ON THE DEVICE: a
    sample's cloud depends on (seed, its id, its grid, threshold, n_points) only, and an empty grid gives zeros.  return_counts: also
    the (B,) int32 exposed-face counts.  `out` is (points[, counts]) to write into, `scratch` a float buffer of at least
    `s3r_voxel_surface_points_scratch_elems` floats.  No autograd: ground truth is data."""
    volume = _check_surface(volume, sample_ids, n_points, seed)
    B, D, H, W = volume.shape
    dev = volume.device
    if out is None:
        out = (torch.empty((B, int(n_points), 3), dtype=torch.float32, device=dev),
               torch.empty((B,), dtype=torch.int32, device=dev) if return_counts else None)
    points, counts = out
    if B:
        lib = _lib.load()
        need = lib.s3r_voxel_surface_points_scratch_elems(B, D, H, W)
        if scratch is None:
            scratch = _scratch(need, "voxel_surface_points scratch query", dev)
        with torch.cuda.device(dev):
            _lib.check(lib.s3r_voxel_surface_points(volume.data_ptr(), float(threshold), sample_ids.data_ptr(), int(seed), points.data_ptr(),
                                                    *_ptrs(counts), B, D, H, W, int(n_points), scratch.data_ptr(), scratch.numel(),
                                                    _stream_ptr(dev)), "voxel_surface_points")
    return (points, counts) if return_counts else points


class SurfacePoints(nn.Module):
    """`voxel_surface_points` with its cloud and scratch kept between calls, keyed on the batch's shape: the same addresses at every call,
    so it can sit inside a captured training step (the graph replays with fresh clouds from the new grids and ids).  `forward` returns
    the kept tensor: copy what must outlive the next call."""

    def __init__(self, n_points: int = 2048, seed: int = 0, threshold: float = 0.5):
        super().__init__()
        self.n_points, self.seed, self.threshold = int(n_points), int(seed), float(threshold)
        self._key = None
        self._out = None
        self._scratch = None

    def forward(self, volume: torch.Tensor, sample_ids: torch.Tensor) -> torch.Tensor:
        volume = _check_surface(volume, sample_ids, self.n_points, self.seed)
        key = (tuple(volume.shape), volume.device)
        if self._key != key:
            if torch.cuda.is_current_stream_capturing():
                raise RuntimeError("SurfacePoints met a new batch shape under stream capture: run one batch of this shape before capturing")
            B = volume.shape[0]
            self._out = (torch.empty((B, self.n_points, 3), dtype=torch.float32, device=volume.device), None)
            self._scratch = _scratch(_lib.load().s3r_voxel_surface_points_scratch_elems(*volume.shape), "SurfacePoints scratch query",
                                     volume.device) if B else None
            self._key = key
        return voxel_surface_points(volume, sample_ids, self.n_points, self.seed, self.threshold, out=self._out, scratch=self._scratch)
