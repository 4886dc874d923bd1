"""numpy / float64 restatements of s3r_conv_backward and s3r_conv_adjoint_desc (include/s3r.h) for tests/test_conv_backward_{cpu,gpu}.py.

The layer is y = act(conv(x, w) * scale[o] + shift[o]), a Conv or ConvTranspose in 2D or 3D with dilation 1.

  g32, gs32, reduce32     tests/_linear64.py's and tests/_head64.py's restatements, unchanged: the pre-activation gradient, g * scale rounded
                          once (scale broadcast per channel), the head backward's summation order over a channel's positions
  grad_shift32(g)         reduce32 over g viewed as (B, cout, S): bit for bit
  grad_w64(case, x, gs)   the header's formula  grad_w[a][f][t] = sum_{b,q} A[b][a][q] F[b][f][q s - p + t]  in float64 from fp32 inputs as given
                          (Conv: A = gs, F = x; ConvTranspose: A = x, F = gs), with per element the number K of terms whose fine position lies
                          inside the grid (the others are exact zeros) and mag = sum |term|.  `mutant=` builds the wrong formulas the cases
                          must tell apart: "swap" (the two channel axes exchanged), "flip" (the kernel flipped on every axis)
  grad_x64(case, w, gs)   the adjoint layer's forward in float64 on the layer's own weight tensor: a Conv's grad_x is
                          ConvTranspose(out_pad = (n + 2 p - k) mod s)(gs), a ConvTranspose's is Conv(gs) — no flip, no re-layout
  bound32(K, mag)         tests/_linear64.py's any-order bound, unchanged

Cases are (op, ndim, cin, cout, k, s, p, out_pad, n, B): the issue's nine, d3's own geometry at B = 1 and 2, and one whose coarse rows
are longer than the 64 positions a staged chunk holds (the kernel then walks a row in segments: another path).
"""
from collections import namedtuple

import numpy as np
import torch
import torch.nn.functional as TF

from tests._head64 import gs32 as _gs32, reduce32
from tests._linear64 import ACTS, EPS64, U32, bits, bound32, g32, gamma      # noqa: F401  (re-exported)

F = np.float32
Case = namedtuple("Case", "op nd cin cout k s p opad n B")

CASES = [
    Case("conv", 3, 5, 7, 3, 1, 1, 0, 5, 3),
    Case("conv", 3, 16, 33, 3, 2, 1, 0, 6, 2),            # adjoint has out_pad 1
    Case("conv", 3, 32, 48, 4, 1, 0, 0, 7, 2),            # v6's form
    Case("conv", 2, 33, 31, 3, 2, 1, 0, 9, 5),
    Case("conv", 2, 64, 16, 1, 1, 0, 0, 23, 1),           # S = 529: crosses a 512 chunk with a tail
    Case("deconv", 3, 32, 16, 4, 2, 1, 0, 4, 3),          # S = 512 exactly
    Case("deconv", 3, 7, 5, 4, 2, 1, 0, 3, 2),
    Case("deconv", 2, 16, 16, 3, 2, 1, 1, 5, 2),
    Case("deconv", 3, 8, 24, 2, 2, 0, 0, 3, 2),           # k = stride
]
D3 = [Case("deconv", 3, 128, 64, 4, 2, 1, 0, 16, 1), Case("deconv", 3, 128, 64, 4, 2, 1, 0, 16, 2)]
LONG_ROWS = [Case("conv", 2, 3, 4, 3, 1, 1, 0, 70, 1)]    # 70 coarse positions per row: two segments, the second short
SIGMOID_CASES = (0, 5)                                    # cases 1 and 6 also run with sigmoid


def case_id(c):
    return f"{c.op}{c.nd}d-{c.cin}to{c.cout}-k{c.k}s{c.s}p{c.p}o{c.opad}-n{c.n}-B{c.B}"


def acts_of(i):
    return ACTS if i in SIGMOID_CASES else ACTS[:2]


def out_edge(c):
    if c.op == "deconv":
        return (c.n - 1) * c.s - 2 * c.p + c.k + c.opad
    return (c.n + 2 * c.p - c.k) // c.s + 1


def weight_shape(c):
    return ((c.cin, c.cout) if c.op == "deconv" else (c.cout, c.cin)) + (c.k,) * c.nd


def x_shape(c, B=None):
    return (c.B if B is None else B, c.cin) + (c.n,) * c.nd


def y_shape(c, B=None):
    return (c.B if B is None else B, c.cout) + (out_edge(c),) * c.nd


def adjoint_out_pad(c):
    return (c.n + 2 * c.p - c.k) % c.s if c.op == "conv" else 0


def linmap(c, x, w):
    """the layer's linear part in x's dtype (torch)"""
    if c.op == "deconv":
        f = TF.conv_transpose3d if c.nd == 3 else TF.conv_transpose2d
        return f(x, w, None, c.s, c.p, c.opad)
    f = TF.conv3d if c.nd == 3 else TF.conv2d
    return f(x, w, None, c.s, c.p)


def _bc(v, nd):
    return v.reshape((1, -1) + (1,) * nd)


def activate(t, act):
    return {"none": t, "relu": torch.relu(t), "sigmoid": torch.sigmoid(t)}[act]


def make(c, seed, act="none", scale=True, lattice=False):
    """fp32 numpy (x, w, scale, shift, y, gy) of a case; y is the layer's own output (float64, rounded once).  lattice=True: small integers
    in x, gy and scale (y is then a sign pattern: the backward only gates on it)"""
    g = torch.Generator().manual_seed(seed)
    if lattice:
        x = torch.randint(-3, 4, x_shape(c), generator=g).float()
        gy = torch.randint(-3, 4, y_shape(c), generator=g).float()
        sc = torch.randint(1, 3, (c.cout,), generator=g).float() if scale else None
        y = torch.randint(0, 2, y_shape(c), generator=g).float() * 2 - 1
        w = torch.randint(-2, 3, weight_shape(c), generator=g).float()
        return x.numpy(), w.numpy(), None if sc is None else sc.numpy(), np.zeros(c.cout, F), y.numpy(), gy.numpy()
    x = torch.randn(x_shape(c), generator=g)
    fan = (c.cin * max(1, c.k // c.s) ** c.nd) if c.op == "deconv" else c.cin * c.k ** c.nd
    w = torch.randn(weight_shape(c), generator=g) / fan ** 0.5
    sc = (0.5 + torch.rand(c.cout, generator=g)) if scale else None
    sh = 0.1 * torch.randn(c.cout, generator=g)
    gy = torch.randn(y_shape(c), generator=g)
    z = linmap(c, x.double(), w.double())
    if sc is not None:
        z = z * _bc(sc.double(), c.nd)
    y = activate(z + _bc(sh.double(), c.nd), act).float()
    return x.numpy(), w.numpy(), None if sc is None else sc.numpy(), sh.numpy(), y.numpy(), gy.numpy()


def gs32(g, scale):
    """g (B, cout, ...) * scale[o], rounded once; g itself when scale is None"""
    g = np.asarray(g, F)
    if scale is None:
        return g.copy()
    return _gs32(g, np.asarray(scale, F).reshape((1, -1) + (1,) * (g.ndim - 2)))


def grad_shift32(g, batch_order="ascending"):
    g = np.asarray(g, F)
    return reduce32(g.reshape(g.shape[0], g.shape[1], -1), batch_order)


def autograd64(c, x, w, scale, shift, act, gy):
    """torch's own float64 autograd of sum(gy * act(linmap(x, w) * scale + shift)): (grad_x, grad_w, grad_shift) as numpy float64"""
    xd = torch.from_numpy(np.asarray(x)).double().requires_grad_()
    wd = torch.from_numpy(np.asarray(w)).double().requires_grad_()
    sh = torch.from_numpy(np.asarray(shift)).double().requires_grad_()
    z = linmap(c, xd, wd)
    if scale is not None:
        z = z * _bc(torch.from_numpy(np.asarray(scale)).double(), c.nd)
    y = activate(z + _bc(sh, c.nd), act)
    gx, gw, gb = torch.autograd.grad((torch.from_numpy(np.asarray(gy)).double() * y).sum(), (xd, wd, sh))
    return gx.numpy(), gw.numpy(), gb.numpy(), y.detach().numpy()


def grad_w64(c, x, gs, mutant=None):
    """(grad_w, K, mag) in float64 from x (B,cin,n..) and gs (B,cout,m..) as given"""
    x64, gs64 = np.asarray(x).astype(np.float64), np.asarray(gs).astype(np.float64)
    A, Fi = (x64, gs64) if c.op == "deconv" else (gs64, x64)
    mc, nf, nd, k, s, p = A.shape[2], Fi.shape[2], c.nd, c.k, c.s, c.p
    B, Ca, Cf = A.shape[0], A.shape[1], Fi.shape[1]
    size = max(nf + p, (mc - 1) * s + k)                              # padded coordinate u = fine index + p, read at q s + t
    Fp = np.zeros((B, Cf) + (size,) * nd)
    inside = np.zeros((size,) * nd)
    core = (slice(p, p + nf),) * nd
    Fp[(slice(None), slice(None)) + core] = Fi
    inside[core] = 1.0
    gw, mag = np.zeros((Ca, Cf) + (k,) * nd), np.zeros((Ca, Cf) + (k,) * nd)
    K = np.zeros((k,) * nd, np.int64)
    A2 = np.ascontiguousarray(np.moveaxis(A.reshape(B, Ca, -1), 1, 0)).reshape(Ca, -1)          # [a][(b, q)]
    for t in np.ndindex(*(k,) * nd):
        win = tuple(slice(ti, ti + s * (mc - 1) + 1, s) for ti in t)
        tt = tuple(k - 1 - ti for ti in t) if mutant == "flip" else t
        W2 = np.ascontiguousarray(np.moveaxis(Fp[(slice(None), slice(None)) + win].reshape(B, Cf, -1), 1, 0)).reshape(Cf, -1)
        gw[(slice(None), slice(None)) + tt] = A2 @ W2.T                 # sum over (b, q) of A[b][a][q] F[b][f][q s - p + t]
        mag[(slice(None), slice(None)) + tt] = np.abs(A2) @ np.abs(W2).T
        K[tt] = B * int(inside[win].sum())
    if mutant == "swap":
        gw = np.ascontiguousarray(np.swapaxes(gw, 0, 1)).reshape(gw.shape)
    K = np.broadcast_to(K, gw.shape)
    return gw, K, mag


def grad_x64(c, w, gs):
    """the adjoint layer's forward on gs in float64, on the layer's own weight tensor"""
    w64 = torch.from_numpy(np.asarray(w)).double()
    g64 = torch.from_numpy(np.asarray(gs)).double()
    if c.op == "conv":
        f = TF.conv_transpose3d if c.nd == 3 else TF.conv_transpose2d
        return f(g64, w64, None, c.s, c.p, adjoint_out_pad(c)).numpy()
    f = TF.conv3d if c.nd == 3 else TF.conv2d
    return f(g64, w64, None, c.s, c.p).numpy()


def lim64(K, mag):
    """two float64 evaluations of the same K-term sums in different orders: each within gamma_{K+1} mag of the real value"""
    return 2 * (K + 1) * EPS64 / (1 - (K + 1) * EPS64) * mag + 1e-300
