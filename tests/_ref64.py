"""Per-element fp64 reference and error bounds for the convolution / linear layers of the C-ABI (tests/test_buffers_*.py).

ref64(layer, x, p)   the layer in float64 from its own parameters: conv / transposed conv / linear, then the folded BatchNorm
                     (y * scale + shift), then the activation; also `mag`, the same layer on |x| with |w|, times |scale|, plus |shift|
bound(...)           the largest |got - ref| an fp32 kernel may show at each element

Direct kernel, residue classes, depth-to-space, staged, unfolded and linear layers (form "direct"):

    |got - ref| <= c_K u L mag + a_act + tiny,     u = 2^-24,  c_K = 1.01 (K + 3)

Derivation.  Before the activation an output element is s = sum_{i<=K} w_i x_i, with K the number of NON-ZERO terms that can meet
one output (cin * k^nd for a convolution; cin * ceil(k / stride)^nd for a residue-class transposed convolution: a class sees only its
own taps; cin for a linear layer).  Zero padding, zero-padded channels and zero-stuffed positions add exact zeros, which never round.
Whatever the order of the summation (MFMA blocks, split-K partial slabs summed in any tree, rounded or exact products), the
computed sum obeys |s^ - s| <= gamma_K sum |w_i x_i|, gamma_K = K u / (1 - K u) (Higham, Accuracy and Stability of Numerical
Algorithms, 2nd ed., eqs. 3.4-3.5).  The epilogue t = s^ scale + shift adds at most two roundings, u (1 + u) each of
|s^ scale| + |shift| <= mag (1 + gamma_K), so |t^ - t| <= (gamma_K + 2 u + O(u^2)) mag.  K <= 2^16 here, so 1 / (1 - K u) < 1.004
and (K + 3) u (1.01) covers both terms.  The activation is L-Lipschitz (ReLU / none / Tanh 1, sigmoid 1/4, LeakyReLU max(1, slope),
ELU max(1, alpha)), and its own evaluation in fp32 adds a_act: 0 for ReLU / none, u |ref| for LeakyReLU, 8 u (|ref| + max(1, alpha))
for the transcendental ones (a few ulp of expf / tanhf / the divide).  `tiny` = 2^-120 covers the underflow range.

This is a worst-case (not a statistical) bound, so it is safe; it is also tight enough to see one missing or doubled TAP (all cin
terms of it): the mutation self-test in tests/test_buffers_cpu.py builds those errors in fp32 for every case and requires the
checker to flag them.  It cannot see one TERM — a single (channel, tap) product is about mag / K and the bound grows with K, so
from a few thousand terms on a dropped or doubled one is inside it (tests/test_exact_cpu.py asserts that for K >= 16384).  Single
terms are held bit for bit, on integer-lattice data, by tests/test_exact_gpu.py (tests/_lattice.py).

Winograd forms (one-, two-, three-axis; form "wino"): the transforms mix a tile, so an element's error follows its neighbours'
magnitudes.  The bound is 5e-5 L max_{neighbourhood}(mag) + a_act + tiny — the constant of tests/test_wino_gpu.py::
test_winograd_on_offset_and_heavy_tailed_inputs (largest error < 5e-5 of the problem's own scale), with the scale taken over the
(2 * 4 + 1)-wide window around the element along every spatial axis (an F(4, 3) tile and the kernel's reach) in its own channel.

bf16 layers (form "bf16") keep tests/test_bf16_gpu.py's per-layer tolerance: the reference is computed from the bf16-rounded input
and weights, and |got - ref| <= 2^-7 |ref| + 1e-3 max |ref|.

A chain's bound (chain_ref64) adds to each layer's own bound the previous layers' error carried through it: L |scale| (|w| * e_in).
"""
from __future__ import annotations

import math

import torch
import torch.nn.functional as F

U = 2.0 ** -24
TINY = 2.0 ** -120
WINO_C = 5e-5


def ndim(layer):
    return {"conv2d": 2, "conv3d": 3, "deconv2d": 2, "deconv3d": 3, "linear": 0}[layer.op]


def act_param(layer):
    if layer.act_param is not None:
        return float(layer.act_param)
    return {"leaky_relu": 0.01, "elu": 1.0}.get(layer.act, 0.0)


def make_params(layer, seed, device="cpu"):
    """weights in torch layout, folded (scale, shift) — scale None without BatchNorm; fp32, seeded"""
    g = torch.Generator().manual_seed(seed)
    nd = ndim(layer)
    if layer.op == "linear":
        shape = (layer.cout, layer.cin)
        fan = layer.cin
    elif layer.op.startswith("deconv"):
        shape = (layer.cin, layer.cout) + (layer.k,) * nd
        fan = layer.cin * max(1, (layer.k // layer.s)) ** nd
    else:
        shape = (layer.cout, layer.cin) + (layer.k,) * nd
        fan = layer.cin * layer.k ** nd
    w = torch.randn(shape, generator=g) / math.sqrt(fan)
    shift = 0.1 * torch.randn(layer.cout, generator=g)
    scale = (0.5 + torch.rand(layer.cout, generator=g)) if layer.bn else None
    return {"w": w.to(device), "scale": None if scale is None else scale.to(device), "shift": shift.to(device)}


def linmap(layer, x, w):
    """the layer's linear part (no bias) in x's dtype"""
    nd = ndim(layer)
    if layer.op == "linear":
        return x.reshape(x.shape[0], -1) @ w.t()
    if layer.op.startswith("deconv"):
        f = F.conv_transpose3d if nd == 3 else F.conv_transpose2d
        return f(x, w, None, layer.s, layer.p, layer.opad, 1, layer.dil)
    f = F.conv3d if nd == 3 else F.conv2d
    return f(x, w, None, layer.s, layer.p, layer.dil)


def _bc(v, y):
    return v.reshape((1, -1) + (1,) * (y.dim() - 2))


def epilogue(layer, t, scale, shift):
    """y * scale + shift; either vector may be None (include/s3r.h: a NULL scale is 1, a NULL shift is 0)"""
    if scale is not None:
        t = t * _bc(scale.to(t.dtype), t)
    return t if shift is None else t + _bc(shift.to(t.dtype), t)


def activate(layer, t):
    a = layer.act
    if a == "relu":
        return t.clamp_min(0)
    if a == "sigmoid":
        return torch.sigmoid(t)
    if a == "leaky_relu":
        return F.leaky_relu(t, act_param(layer))
    if a == "elu":
        return F.elu(t, act_param(layer))
    if a == "tanh":
        return torch.tanh(t)
    return t


def lipschitz(layer):
    return {"sigmoid": 0.25, "leaky_relu": max(1.0, abs(act_param(layer))), "elu": max(1.0, act_param(layer))}.get(layer.act, 1.0)


def act_err(layer, ref):
    if layer.act in ("relu", "none"):
        return torch.zeros_like(ref)
    if layer.act == "leaky_relu":
        return U * ref.abs()
    return 8 * U * (ref.abs() + max(1.0, act_param(layer)))


def k_terms(layer):
    """non-zero products that can meet one output element (the K of the bound)"""
    nd = ndim(layer)
    if layer.op == "linear":
        return layer.cin
    if layer.op.startswith("deconv") and layer.dil == 1:
        return layer.cin * (-(-layer.k // layer.s)) ** nd
    return layer.cin * layer.k ** nd


def ref64(layer, x, p):
    """(ref, mag) in float64 on x's device; x is the logical (unpadded) input"""
    x64 = x.double()
    w64 = p["w"].double().to(x.device)
    sc = None if p["scale"] is None else p["scale"].double().to(x.device)
    sh = None if p["shift"] is None else p["shift"].double().to(x.device)
    pre = epilogue(layer, linmap(layer, x64, w64), sc, sh)
    mag = linmap(layer, x64.abs(), w64.abs())
    mag = epilogue(layer, mag, None if sc is None else sc.abs(), None if sh is None else sh.abs())
    return activate(layer, pre), mag


def nbhd_max(layer, mag):
    nd = ndim(layer)
    if nd == 0:
        return mag
    f = F.max_pool3d if nd == 3 else F.max_pool2d
    return f(mag, 9, 1, 4)


def bound(layer, ref, mag, form):
    if form == "bf16":
        return 2.0 ** -7 * ref.abs() + 1e-3 * float(ref.abs().max()) + TINY
    L = lipschitz(layer)
    if form == "wino":
        core = WINO_C * L * nbhd_max(layer, mag)
    else:
        core = 1.01 * (k_terms(layer) + 3) * U * L * mag
    return core + act_err(layer, ref) + TINY


def carried(layer, p, err_in):
    """the previous layers' error bound carried through this layer: L |scale| (|w| * e_in)"""
    w64 = p["w"].double().to(err_in.device).abs()
    t = linmap(layer, err_in, w64)
    if p["scale"] is not None:
        t = t * _bc(p["scale"].double().to(t.device).abs(), t)
    return lipschitz(layer) * t


def chain_ref64(layers, forms, x, params):
    """(ref, bound) of a chain, reshaping between layers the way the library does (flat per sample)"""
    h, err = x.double(), torch.zeros_like(x, dtype=torch.float64)
    for i, (l, f, p) in enumerate(zip(layers, forms, params)):
        if l.op != "linear":
            n = round((h[0].numel() // l.cin) ** (1.0 / ndim(l)))
            h = h.reshape((h.shape[0], l.cin) + (n,) * ndim(l))
            err = err.reshape(h.shape)
        ref, mag = ref64(l, h, p)
        e = bound(l, ref, mag, f)
        if i:
            e = e + carried(l, p, err if l.op != "linear" else err.reshape(err.shape[0], -1))
        h, err = ref, e
    return h, err


def worst(got, ref, bnd):
    """largest |got - ref| / bound, with the index where it occurs (NaN in got: inf)"""
    got = got.double().to(ref.device)
    if bool(torch.isnan(got).any()):
        i = int(torch.isnan(got).reshape(-1).nonzero()[0, 0])
        return math.inf, i
    r = ((got - ref).abs() / bnd).reshape(-1)
    i = int(r.argmax())
    return float(r[i]), i
