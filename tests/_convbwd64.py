"""numpy / float64 restatements of s3r_conv_backward and s3r_conv_adjoint_desc (include/s3r.h) for tests/test_conv_backward_{cpu,gpu}.py.

The layer is y = act(conv(x, w) * scale[o] + shift[o]), a Conv or ConvTranspose in 2D or 3D with dilation 1.

  g32, gs32, reduce32     tests/_linear64.py's and tests/_head64.py's restatements, unchanged: the pre-activation gradient, g * scale rounded
                          once (scale broadcast per channel), the head backward's summation order over a channel's positions
  grad_shift32(g)         reduce32 over g viewed as (B, cout, S): bit for bit
  grad_w64(case, x, gs)   the header's formula  grad_w[a][f][t] = sum_{b,q} A[b][a][q] F[b][f][q s - p + t]  in float64 from fp32 inputs as given
                          (Conv: A = gs, F = x; ConvTranspose: A = x, F = gs), with per element the number K of terms whose fine position lies
                          inside the grid (the others are exact zeros) and mag = sum |term|.  `mutant=` builds the wrong formulas the cases
                          must tell apart: "swap" (the two channel axes exchanged), "flip" (the kernel flipped on every axis), and two
                          tiling mistakes built from geo(): "drop_tail_slice" (the coarse positions of each sample's last K slice
                          contribute nothing), "drop_tap_group" (the taps t_w >= 4, the second tap group along W, are zero)
  grad_x64(case, w, gs)   the adjoint layer's forward in float64 on the layer's own weight tensor: a Conv's grad_x is
                          ConvTranspose(out_pad = (n + 2 p - k) mod s)(gs), a ConvTranspose's is Conv(gs) — no flip, no re-layout
  bound32(K, mag)         tests/_linear64.py's any-order bound, unchanged
  geo(case)               csrc/s3r_conv_bwd.hip's convbwd_geo restated: the weight-gradient GEMM's tiling, chunking and K slicing
  nan_taps(case, pos)     the taps of grad_w that read the fine position `pos`, from the header's formula alone

Cases are (op, ndim, cin, cout, k, s, p, out_pad, n, B): the issue's nine, d3's own geometry at B = 1 and 2, and one whose coarse rows
are longer than the 64 positions a staged chunk holds (the kernel then walks a row in segments: another path).  SHAPES is the tiling
sweep: the smallest geometries at which each branch of convbwd_geo / convbwd_gw_kernel / convbwd_shift_finish_kernel is taken that
the twelve above never reach (tests/test_conv_backward_cpu.py::test_shapes_cover_the_tiling names the branches through geo()).
"""
from collections import namedtuple
from types import SimpleNamespace

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
SHAPES = [
    Case("conv", 2, 3, 130, 5, 2, 2, 0, 11, 2),           # ntg 2 with a one-tap second group; nag 2 (130 = 128 + 2)
    Case("conv", 3, 6, 130, 3, 2, 1, 0, 7, 2),            # nag 2 in 3D, R = 16 whole rows
    Case("conv", 2, 40, 260, 3, 1, 1, 0, 6, 1),           # nag 3 with a 4-row last group; nft 2 with 8 channels in the last
    Case("conv", 2, 3, 4, 6, 2, 2, 0, 40, 1),             # ntg 2 (taps 4, 5); 7 chunks in 4 slices of 2: ragged last slice, short last chunk
    Case("conv", 2, 8, 8, 7, 3, 3, 0, 12, 2),             # stride 3, k 7 (a second group of 3 taps)
    Case("conv", 3, 3, 4, 4, 4, 0, 0, 16, 2),             # run halved to 32 in whole-row form (R 8)
    Case("conv", 3, 2, 3, 7, 3, 3, 0, 10, 1),             # run halved and ntg 2
    Case("deconv", 3, 3, 2, 4, 4, 0, 0, 4, 2),            # the same halving with the ConvTranspose roles (A = x)
    Case("conv", 2, 3, 4, 8, 4, 2, 0, 252, 1),            # run halved into segment form (WL 32, nseg 2, short second segment), ntg 2
    Case("conv", 2, 5, 4, 5, 4, 2, 0, 131, 1),            # mc 33 (odd, WLP 34), R 1
    Case("deconv", 2, 4, 3, 4, 2, 1, 0, 70, 1),           # segments with a ConvTranspose at stride 2
    Case("conv", 2, 2, 3, 3, 2, 1, 0, 141, 1),            # segments with a stride-2 Conv (mc 71)
    Case("conv", 3, 1, 2, 3, 1, 1, 0, 66, 1),             # segments in 3D
    Case("conv", 2, 2, 3, 3, 1, 1, 0, 64, 1),             # mc = 64: the last whole-row shape
    Case("conv", 2, 2, 3, 3, 1, 1, 0, 65, 1),             # mc = 65: a second segment of ONE position
    Case("deconv", 2, 6, 5, 2, 3, 0, 1, 5, 2),            # k < stride with output padding
    Case("deconv", 3, 5, 3, 5, 3, 2, 2, 3, 1),            # k5 s3 out_pad 2 in 3D, ntg 2
    Case("conv", 2, 4, 4, 1, 2, 0, 0, 8, 2),              # k1 at stride 2: one tile in all
    Case("conv", 2, 3, 2, 3, 1, 1, 0, 1, 2),              # coarse edge 1 (WLP 2, one real column)
    Case("conv", 2, 2, 3, 3, 1, 1, 0, 4, 70),             # B = 70: the finish kernels' second 64-sample block
]
SHAPES_SIGMOID = (3, 10)                                  # these two of SHAPES also run with sigmoid
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


def make(c, seed, act="none", scale=True, lattice=False, mean=0.0):
    """fp32 numpy (x, w, scale, shift, y, gy) of a case; y is the layer's own output (float64, rounded once).  lattice=True: small integers
    in x, gy and scale (y is then a sign pattern: the backward only gates on it).  mean: added to the normal draws of x and grad_y (the
    draws themselves do not change: data_mean)"""
    g = torch.Generator().manual_seed(seed)
    if lattice:
        x = torch.randint(-3, 4, x_shape(c), generator=g).float()
        gy = torch.randint(-3, 4, y_shape(c), generator=g).float()
        sc = torch.randint(1, 3, (c.cout,), generator=g).float() if scale else None
        y = torch.randint(0, 2, y_shape(c), generator=g).float() * 2 - 1
        w = torch.randint(-2, 3, weight_shape(c), generator=g).float()
        return x.numpy(), w.numpy(), None if sc is None else sc.numpy(), np.zeros(c.cout, F), y.numpy(), gy.numpy()
    x = torch.randn(x_shape(c), generator=g) + mean
    fan = (c.cin * max(1, c.k // c.s) ** c.nd) if c.op == "deconv" else c.cin * c.k ** c.nd
    w = torch.randn(weight_shape(c), generator=g) / fan ** 0.5
    sc = (0.5 + torch.rand(c.cout, generator=g)) if scale else None
    sh = 0.1 * torch.randn(c.cout, generator=g)
    gy = torch.randn(y_shape(c), generator=g) + mean
    z = linmap(c, x.double(), w.double())
    if sc is not None:
        z = z * _bc(sc.double(), c.nd)
    y = activate(z + _bc(sh.double(), c.nd), act).float()
    return x.numpy(), w.numpy(), None if sc is None else sc.numpy(), sh.numpy(), y.numpy(), gy.numpy()


def data_mean(c):
    """The mean of the random x and grad_y of a case: 0 for the twelve layer geometries (their data are what they always were), 1 for
    the sweep.  Why: an element of grad_w is a sum of K products.  On zero-mean data it is a random walk of size about sqrt(K) sigma^2,
    while the any-order bound gamma_{K+1} sum|term| grows like K^2 u: from K of about (1 / u)^(2/3) ~ 10^5 on the bound exceeds the
    gradient itself and the comparison can see no mistake, not even a missing slice (a 3D segment case has K >= 65^3 = 274625).  With
    mean 1 the sum grows like K, a part r of the terms that goes missing moves an element by about r K against a bound of about
    1.4 K^2 u, i.e. by r / (1.4 K u) bounds: 5 bounds for one slice of eight at K = 66^3, more everywhere else."""
    return 1.0 if any(c._replace(B=s.B) == s for s in SHAPES) else 0.0


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


CB_AG, CB_FT, CB_RUN, CB_LDS_MAX = 128, 32, 64, 64 * 1024


def geo(c):
    """convbwd_geo (csrc/s3r_conv_bwd.hip) restated line by line: it MIRRORS the kernel file and must move with it.  The CPU test pins
    it against the library through s3r_conv_backward_scratch_elems (which shows nsl) for every case.  None where no tiling fits."""
    deconv = c.op == "deconv"
    o = out_edge(c)
    g = SimpleNamespace(nd=c.nd, k=c.k, s=c.s, p=c.p)
    g.Ca, g.Cf = (c.cin, c.cout) if deconv else (c.cout, c.cin)
    g.mc, g.nf = (c.n, o) if deconv else (o, c.n)
    g.Q, g.Pf, g.T, g.To = g.mc ** c.nd, g.nf ** c.nd, c.k ** c.nd, c.k ** (c.nd - 1)
    g.NT = min(c.k, 4)
    g.ntg = (c.k + g.NT - 1) // g.NT
    g.nrows = g.mc ** (c.nd - 1)
    run = CB_RUN
    while True:
        if run < 2:
            return None
        if g.mc <= run:
            g.WL, g.nseg = g.mc, 1
            g.WLP = (g.WL + 1) & ~1
            g.R = min(max(1, run // g.WLP), g.nrows)
        else:
            g.WL, g.WLP, g.R = run, run, 1
            g.nseg = (g.mc + run - 1) // run
        g.FL = (g.WLP - 1) * c.s + g.ntg * g.NT
        g.astr, g.fstr = (g.R * g.WLP) | 1, (g.R * g.FL) | 1
        g.lds_bytes = 4 * (CB_AG * g.astr + CB_FT * g.fstr)
        if g.lds_bytes <= CB_LDS_MAX:
            break
        run //= 2
    g.run = run
    g.nchunks = (g.nrows + g.R - 1) // g.R if g.nseg == 1 else g.nrows * g.nseg
    g.nag, g.nft = (g.Ca + CB_AG - 1) // CB_AG, (g.Cf + CB_FT - 1) // CB_FT
    g.tiles = g.nag * g.nft * g.To * g.ntg
    if g.tiles >= 1 << 24:
        return None
    want = max(1, min((64 + g.tiles - 1) // g.tiles, g.nchunks))
    g.cps = (g.nchunks + want - 1) // want
    g.nsl = (g.nchunks + g.cps - 1) // g.cps
    g.slab = g.Ca * g.Cf * g.T
    return g


def scratch_elems(c, B=None):
    """conv_backward_scratch_elems restated: [gs][chunk sums of g][slabs when there is more than one]"""
    B, g, S = c.B if B is None else B, geo(c), out_edge(c) ** c.nd
    return B * c.cout * S + c.cout * B * ((S + 511) // 512) + (B * g.nsl * g.slab if B * g.nsl > 1 else 0)


def tail_slice_mask(c):
    """True at the coarse positions (nrows, mc) that the chunks of a sample's LAST K slice cover (geo()'s chunk walk)"""
    g = geo(c)
    m = np.zeros((g.nrows, g.mc), bool)
    for ch in range((g.nsl - 1) * g.cps, g.nchunks):
        if g.nseg == 1:
            m[ch * g.R:(ch + 1) * g.R] = True
        else:
            row, w0 = ch // g.nseg, (ch % g.nseg) * g.WL
            m[row, w0:w0 + g.WL] = True
    return m.reshape((g.mc,) * c.nd)


def slice_index(c):
    """int (mc,)*nd: the K slice (0 .. nsl - 1) whose chunks cover each coarse position of a sample (geo()'s chunk walk)"""
    g = geo(c)
    m = np.zeros((g.nrows, g.mc), np.int64)
    for ch in range(g.nchunks):
        if g.nseg == 1:
            m[ch * g.R:(ch + 1) * g.R] = ch // g.cps
        else:
            row, w0 = ch // g.nseg, (ch % g.nseg) * g.WL
            m[row, w0:w0 + g.WL] = ch // g.cps
    return m.reshape((g.mc,) * c.nd)


def nan_taps(c, pos):
    """bool (k,)*nd: the taps t for which, on every axis, pos + p - t is a multiple of s whose quotient lies in [0, mc) — the terms
    A[b][a][q] F[b][f][q s - p + t] of the header's formula that read the fine position `pos`"""
    mc = c.n if c.op == "deconv" else out_edge(c)
    hit = np.ones((c.k,) * c.nd, bool)
    for ax, x in enumerate(pos):
        t = np.arange(c.k)
        d = x + c.p - t
        ok = (d % c.s == 0) & (d >= 0) & (d // c.s < mc)
        hit &= ok.reshape(tuple(-1 if i == ax else 1 for i in range(c.nd)))
    return hit


def grad_w64(c, x, gs, mutant=None):
    """(grad_w, K, mag) in float64 from x (B,cin,n..) and gs (B,cout,m..) as given"""
    x64, gs64 = np.asarray(x).astype(np.float64), np.asarray(gs).astype(np.float64)
    A, Fi = (x64, gs64) if c.op == "deconv" else (gs64, x64)
    if mutant == "drop_tail_slice":
        A = np.where(tail_slice_mask(c), 0.0, A)
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
    if mutant == "drop_tap_group":
        gw[..., 4:] = 0.0
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
