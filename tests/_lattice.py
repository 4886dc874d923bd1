"""Integer-lattice data for the bit-exact tests (tests/test_exact_cpu.py, tests/test_exact_gpu.py).

The argument.  When the input, the weights and the folded epilogue of a layer are integers (or dyadic rationals with a few
fractional bits), every product and every partial sum of the layer IN ANY SUMMATION ORDER is a multiple of 2^-f of magnitude at
most `mag` (the same layer on |x| with |w|, times |scale|, plus |shift|).  If mag * 2^f < 2^24, each of them is an fp32 number, no
fp32 operation on them rounds, and a kernel's output equals the float64 reference bit for bit — MFMA block order, split-K slabs,
residue classes, staging, unfolding and launch forms included.  There is no tolerance and hence no floor: one missing (channel,
tap) term at K = 32768 is a mismatch, where tests/_ref64.py's bound (which grows with K) cannot see it.  On the bf16 path the
inputs (|v| <= 256) are exact in bf16, the fp32 accumulator is exact, so the output must be RNE_bf16(exact value) bit for bit;
outputs above 256 are often exact ties, which pins the rounding mode.

lattice_case(layer, B, n_in, seed, form, ...)   x, {"w", "scale", "shift"} on the lattice of `form`
expected(layer, x, p, dtype)                      _ref64.ref64 cast to fp32 (exact), and `.to(bfloat16)` of that (RNE) for bf16
exactness(layer, x, p, form, dtype)               the conditions that make "exact" true, computed from the reference alone

Lattice.  x and w are integers; `scale` (layers with a folded BatchNorm) is one of 1/4, 1/2, 1, 2 per channel; `shift` is an integer
in [-8, 32] plus, where the channel's scale is < 1, a multiple of 1/4.  Activations are restricted to the exact ones: none, ReLU,
LeakyReLU with a power-of-two slope (1/4 and 1/2: fused in the kernels' epilogue; 2: above 1, the separate pass).  Sigmoid, ELU
and Tanh evaluate transcendental functions and cannot be exact: they stay with tests/_ref64.py's bound; `exact_act` substitutes
an exact activation in the cases taken from tests/_buffer_cases.py.

Winograd forms.  The kernels fold G into the packed weights in fp32 (s3r_wino_axis1.hip: pack_wino_kernel, and s3r_wino.h: wax_g, constants
1/4, 1/6, 1/12, 1/24 for F(4, 3) and 1/2, 1/6, 1/3, 2/3, 4/3 for F(2, 4) with the points 0, +-1, 2, inf; the F(2, 2) classes of a
transposed layer use sums of taps only).  Per transformed axis the lattice step is the lcm of G's denominators, from
tools/wino_matrices.py's construction in exact arithmetic: F(4, 3) 24, F(2, 4) 6, F(2, 2) 1 (`wino_step`).  B^T and A^T are
integer matrices and no other constant touches the data.  A weight k * step times the fp32 constant c = fl(n / step) is
k n (1 + delta) with |delta| <= 2^-24, which rounds to the integer k n whenever that integer has fewer than 24 bits — but ONLY as a
single product: `g0 * (1 / 24) + g2 * (1 / 6)` may be contracted into one fused multiply-add, whose single rounding sees
k0 (1 + delta) + 4 k2 and, under cancellation, keeps the delta.  So a Winograd case has ONE non-zero tap per (cout, cin) fibre along
every transformed axis (the tap varies from fibre to fibre, so every row of G meets data); then each entry of G g is a single product
and the packed weights are the exact integers whatever the compiler fuses.  `exactness` checks that property of the data too.
The flow of a Winograd case is the direct layer's AND the form's own: sum_{k, l} T[j][l][k] |g_k| |x_l| per transformed axis with
T = sum_i |A^T[j][i]| |G[i][k]| |B^T[i][l]| from the exact matrices (`wino_gain`, `_wino_flow`) — input transform, class GEMM and
finish in the kernels' order.  The 576 step makes the two-axis flow large (about 9e4 per channel and remaining tap with dense
x in {-1, 0, 1}), so those cases thin x and w until it fits (tests/_exact_cases.py::_wino_data).
"""
from __future__ import annotations

import dataclasses
import math
from fractions import Fraction as Fr
from functools import lru_cache

import torch

from tests import _ref64 as R

TWO24 = float(2 ** 24)
EXACT_ACTS = ("none", "relu", "leaky_relu")
SCALES = (0.25, 0.5, 1.0, 2.0)


def exact_act(layer, slope=0.25):
    """the layer with an exact activation in place of a transcendental one, and a power-of-two slope for LeakyReLU"""
    if layer.act in ("none", "relu"):
        return layer
    if layer.act == "leaky_relu":
        return dataclasses.replace(layer, act_param=slope)
    return dataclasses.replace(layer, act="leaky_relu" if layer.act == "elu" else "relu", act_param=slope if layer.act == "elu" else None)


# ---------------------------------------------------------------- Winograd matrices in exact arithmetic (tools/wino_matrices.py)
def cook_toom(m, r, pts):
    """(A^T, G, B^T) of F(m, r) for the finite points `pts` and infinity, as Fractions"""
    pts = [Fr(p) for p in pts]
    n = m + r - 1
    assert len(pts) == n - 1

    def polymul(a, b):
        out = [Fr(0)] * (len(a) + len(b) - 1)
        for i, u in enumerate(a):
            for j, v in enumerate(b):
                out[i + j] += u * v
        return out

    f = [math.prod([a - b for j, b in enumerate(pts) if j != i], start=Fr(1)) for i, a in enumerate(pts)]
    AT = [[(pts[i] ** j if i < n - 1 else Fr(int(j == m - 1))) for i in range(n)] for j in range(m)]
    G = [[pts[i] ** k / f[i] for k in range(r)] for i in range(n - 1)] + [[Fr(0)] * (r - 1) + [Fr(1)]]
    BT = []
    for i in range(n - 1):
        poly = [Fr(1)]
        for j, b in enumerate(pts):
            if j != i:
                poly = polymul(poly, [-b, Fr(1)])
        BT.append(poly + [Fr(0)] * (n - len(poly)))
    poly = [Fr(1)]
    for b in pts:
        poly = polymul(poly, [-b, Fr(1)])
    BT.append(poly)
    return AT, G, BT


WINO_POINTS = {"f43": (4, 3, (0, 1, -1, 2, -2)), "f24": (2, 4, (0, 1, -1, 2))}


@lru_cache(None)
def wino_matrices(kind):
    m, r, pts = WINO_POINTS[kind]
    return cook_toom(m, r, pts)


def wino_step(kind):
    """lcm of the denominators of G: the weights' lattice step per transformed axis"""
    if kind == "f22":
        return 1
    return math.lcm(*[v.denominator for row in wino_matrices(kind)[1] for v in row])


# form -> (matrix kind, number of transformed axes)
#   f43-h    one-axis F(4, 3) along H (Conv2d / Conv3d k3 s1 p1)
#   f43x2    two-axis F(4, 3) x F(4, 3): over (H, W) for Conv2d, over (D, H) for Conv3d
#   f24x2    two-axis F(2, 4) x F(2, 4) over (D, H) (Conv3d k4 valid)
#   f22x2    ConvTranspose3d k4 s2 p1: F(2, 2) along D and H inside every output-parity class
#   f22x3    the same along D, H and W (the three-axis form)
FORMS = {"direct": None, "f43-h": ("f43", 1), "f43x2": ("f43", 2), "f24x2": ("f24", 2), "f22x2": ("f22", 2), "f22x3": ("f22", 3)}


def _fibre_axes(layer, form):
    """the weight tensor's kernel axes (indices into w.shape) along which the form applies a NON-INTEGER G"""
    nd = R.ndim(layer)
    if form == "f43-h":
        return (nd,)                                   # kh: w[cout][cin][kh][kw] / w[cout][cin][kd][kh][kw]
    if form in ("f43x2", "f24x2"):
        return (2, 3)                                  # Conv2d: (kh, kw); Conv3d: (kd, kh)
    return ()


def wino_gain(kind):
    """T[j][l][k] = sum_i |A^T[j][i]| |G[i][k]| |B^T[i][l]|: the weight with which the product |x_l| |g_k| enters the absolute-value flow
    of output j of a tile along one axis (input transform, class product, finish), as a float64 tensor (m, n, r)"""
    AT, G, BT = wino_matrices(kind)
    n, m, r = len(BT), len(AT), len(G[0])
    return torch.tensor([[[float(sum(abs(AT[j][i]) * abs(G[i][k]) * abs(BT[i][l]) for i in range(n))) for k in range(r)]
                          for l in range(n)] for j in range(m)], dtype=torch.float64)


# ---------------------------------------------------------------- data
EP_FORMS = ("ss", "0s", "s0", "00")


def lattice_case(layer, B, n_in, seed, form="direct", xmax=2, wmax=1, density=1.0, xdensity=1.0, ep="ss"):
    """x (B, cin, n_in, ...) and {"w", "scale", "shift"} on the lattice of `form`, fp32 on the CPU, seeded.  ep: the epilogue's vector
    form, (scale, shift) each given `s` or NULL `0` — "ss": what the layer has (a scale where it folds a BatchNorm, and a shift);
    "0s" / "s0" / "00" drop the scale, the shift or both (None: the test bodies pass a NULL pointer).  x, w and the vectors that
    remain are the SAME numbers in all four forms (a shift without a scale keeps its integer part only)"""
    assert ep in EP_FORMS and (layer.bn or ep[0] == "0" or ep == "ss"), (ep, "a given scale needs a layer with bn=True")
    assert layer.act in EXACT_ACTS, f"{layer.act} cannot be exact"
    if layer.act == "leaky_relu":
        s = R.act_param(layer)
        assert s > 0 and math.log2(s) == int(math.log2(s)), "LeakyReLU needs a power-of-two slope"
    g = torch.Generator().manual_seed(seed)                # the parameters: the same for every batch size
    nd = R.ndim(layer)
    x = torch.randint(-xmax, xmax + 1, (B, layer.cin) + (n_in,) * nd, generator=torch.Generator().manual_seed(seed + 7919)).float()
    if xdensity < 1.0:
        x = x * (torch.rand(x.shape, generator=torch.Generator().manual_seed(seed + 104729)) < xdensity).float()
    if layer.op == "linear":
        shape = (layer.cout, layer.cin)
    elif layer.op.startswith("deconv"):
        shape = (layer.cin, layer.cout) + (layer.k,) * nd
    else:
        shape = (layer.cout, layer.cin) + (layer.k,) * nd
    w = torch.randint(-wmax, wmax + 1, shape, generator=g).float()
    if density < 1.0:
        w = w * (torch.rand(shape, generator=g) < density).float()
    axes = _fibre_axes(layer, form)
    if axes:                                           # ONE non-zero tap per fibre of the transformed axes (jointly, for two axes)
        keep = torch.ones(shape)
        for a in axes:
            pick = torch.randint(0, shape[a], [1 if i in axes else s for i, s in enumerate(shape)], generator=g)
            keep = keep * (torch.arange(shape[a]).reshape([-1 if i == a else 1 for i in range(len(shape))]) == pick).float()
        w = w * keep * float(wino_step(FORMS[form][0]) ** len(axes))
    if layer.bn:
        scale = torch.tensor(SCALES)[torch.randint(0, 4, (layer.cout,), generator=g)]
    else:
        scale = None
    shift = torch.randint(-8, 33, (layer.cout,), generator=g).float()
    if ep[0] == "0":
        scale = None
    if scale is not None:
        shift = shift + (scale < 1).float() * torch.randint(0, 4, (layer.cout,), generator=g).float() * 0.25
    return x, {"w": w, "scale": scale, "shift": None if ep[1] == "0" else shift}


def expected(layer, x, p, dtype="fp32"):
    """the exact output: float64 reference cast to fp32 (exact under `exactness`), rounded to bf16 (RNE) for bf16 outputs"""
    ref, _ = R.ref64(layer, x, p)
    out = ref.float()
    return out.to(torch.bfloat16) if dtype == "bf16" else out


def frac_bits(layer, p):
    """fractional bits the epilogue and the activation bring: 2 for a scale < 1 (and its dyadic shift), log2(1 / slope) for LeakyReLU"""
    f = 0
    if p["scale"] is not None and bool((p["scale"] < 1).any()):
        f += 2
    if layer.act == "leaky_relu" and R.act_param(layer) < 1:
        f += int(round(-math.log2(R.act_param(layer))))
    return f


def fp32_layer(layer, x, p):
    """the layer in fp32 on the CPU: torch's own reduction, an independent summation order"""
    return R.activate(layer, R.epilogue(layer, R.linmap(layer, x.float(), p["w"].float()), p["scale"], p["shift"]))


def bf16_shares(ref32):
    """(share of exact ties, share of inexact non-ties) among fp32 values about to be rounded to bf16"""
    low = ref32.contiguous().view(torch.int32) & 0xFFFF
    n = ref32.numel()
    return float((low == 0x8000).sum()) / n, float(((low != 0) & (low != 0x8000)).sum()) / n


def _wino_flow(layer, x, p, form):
    """the absolute-value flow through a Winograd form in the kernels' order (|B^T| over the input tile, the class GEMM's sum over
    channels and remaining taps with |G g|, |A^T| over the class sums), before the epilogue: its largest value per output channel.

    F(m, r) forms: along a transformed axis, output j of tile q is sum_i A^T[j][i] (sum_k G[i][k] g_k) (sum_l B^T[i][l] x_{m q + l}), and
    every intermediate of it is bounded by sum_{k, l} T[j][l][k] |g_k| |x_{m q + l}| with T = wino_gain: a convolution of |x| with
    stride m over the tile's n = m + r - 1 inputs, one output channel per (cout, j); the other axes keep their own taps.
    F(2, 2) classes of a transposed layer: y = (x0 - x1) g0 + x1 (g0 + g1), every product |x_l| |g_k| enters at most twice per
    transformed axis: 2^axes times the direct layer's flow."""
    kind, nax = FORMS[form]
    nd = R.ndim(layer)
    if kind == "f22":
        out = R.linmap(layer, x.double().abs(), p["w"].double().abs())
        return out.transpose(0, 1).reshape(layer.cout, -1).amax(1) * 2.0 ** nax
    T = wino_gain(kind)
    m, n, r = T.shape
    axes = _fibre_axes(layer, form)
    w = p["w"].double().abs().movedim(axes, tuple(range(-len(axes), 0)))           # (cout, cin, rest..., k [, K])
    if len(axes) == 1:
        w = torch.einsum("jlk,...k->j...l", T, w)
    else:
        w = torch.einsum("jlk,JLK,...kK->jJ...lL", T, T, w)
        w = w.reshape((-1,) + w.shape[2:])
    w = w.movedim(tuple(range(-len(axes), 0)), tuple(a + 1 for a in axes))          # (j, cout, cin, kernel axes with n in place of r)
    w = w.reshape((-1,) + w.shape[2:])
    n_in = x.shape[-1]
    tiles = -(-(n_in + 2 * layer.p - r + 1) // m)
    pads = []
    for sp_axis in reversed(range(nd)):                # F.pad lists the last axis first
        pads += [layer.p, (m * tiles + r - 1 - n_in - layer.p) if sp_axis + 2 in axes else layer.p]
    xa = torch.nn.functional.pad(x.double().abs(), pads)
    stride = [m if i + 2 in axes else 1 for i in range(nd)]
    f = torch.nn.functional.conv3d if nd == 3 else torch.nn.functional.conv2d
    out = f(xa, w.contiguous(), None, stride)           # channels: (j [, J], cout)
    return out.transpose(0, 1).reshape(out.shape[1] // layer.cout, layer.cout, -1).amax((0, 2))


def exactness(layer, x, p, form="direct", dtype="fp32"):
    """the record of the conditions under which the case is exact and able to see a mistake (see the module docstring):
    flow        largest absolute-value flow (direct: `mag` of ref64; Winograd: through |B^T|, |G|, the channel sum, |A^T|)
    bits        flow * 2^f < 2^24, f the fractional bits in play; and every reference value is a multiple of 2^-f
    independent torch's CPU fp32 evaluation equals the float64 one bit for bit
    nonzero     share of non-zero outputs after the activation
    ties, inexact   (bf16 outputs) shares of exact ties and of inexact non-ties
    fibres      (Winograd) one non-zero tap per fibre of the transformed axes, weights multiples of the lattice step"""
    ref, mag = R.ref64(layer, x, p)
    L = R.lipschitz(layer)
    sc = torch.ones(layer.cout, dtype=torch.float64) if p["scale"] is None else p["scale"].double().abs()
    sh = torch.zeros(layer.cout, dtype=torch.float64) if p["shift"] is None else p["shift"].double().abs()
    # fractional bits per channel: 2 where the scale is < 1 (1/4, 1/2 and the shift's quarters), plus the LeakyReLU slope's
    fc = 2.0 * (sc < 1).double() + (frac_bits(layer, {"scale": None}) if layer.act == "leaky_relu" else 0)
    per_ch = mag.transpose(0, 1).reshape(layer.cout, -1).amax(1).cpu() if layer.op != "linear" else mag.amax(0).cpu()
    rec = {"f": frac_bits(layer, p), "mag": float(per_ch.max())}
    if FORMS[form] is not None:
        per_ch = torch.maximum(per_ch, _wino_flow(layer, x.cpu(), {k: None if v is None else v.cpu() for k, v in p.items()}, form) * sc + sh)
        axes = _fibre_axes(layer, form)
        step = wino_step(FORMS[form][0]) ** len(axes)
        nz = (p["w"] != 0).float()
        for a in axes:
            nz = nz.sum(a, keepdim=True)
        rec["fibres"] = bool((nz <= 1).all()) and bool((p["w"] % step == 0).all())
    rec["flow"] = float(per_ch.max())
    rec["bits24"] = float((per_ch * L * 2.0 ** fc).max()) / TWO24           # < 1: 24 significant bits hold every intermediate
    scaled = ref * 2.0 ** rec["f"]
    rec["bits"] = rec["bits24"] < 1 and bool((scaled == scaled.round()).all())
    ref32 = ref.float()
    got32 = fp32_layer(layer, x, p)
    rec["independent"] = bool((ref32.double() == ref).all()) and torch.equal(got32.view(torch.int32), ref32.view(torch.int32))
    rec["nonzero"] = float((ref != 0).sum()) / ref.numel()
    rec["neg_zero"] = bool((ref32.view(torch.int32) == -2 ** 31).any())
    if dtype == "bf16":
        rec["ties"], rec["inexact"] = bf16_shares(ref32)
    return rec


def admissible(rec, bf16_out=False):
    """None, or the name of the first condition the case misses"""
    if not rec["bits"]:
        return "bits"
    if not rec.get("fibres", True):
        return "fibres"
    if not rec["independent"]:
        return "independent"
    if rec["neg_zero"]:
        return "neg_zero"
    if rec["nonzero"] < 0.25:
        return "nonzero"
    if bf16_out and (rec["ties"] < 0.01 or rec["inexact"] < 0.01):
        return "bf16 shares"
    return None


def bf16_magnitudes(K):
    """(xmax, wmax) for a bf16 case of reduction depth K.  bf16 keeps 8 significant bits, so an integer output is inexact only above
    256: the spread of the sum, sqrt(K E[x^2] E[w^2]) with E[v^2] = a (a + 1) / 3 for integers uniform in [-a, a], is brought to at
    least 400; |x| <= 64 and |w| <= 4 stay exact in bf16"""
    for a, b in ((2, 1), (4, 1), (4, 2), (8, 2), (16, 2), (16, 4), (32, 4), (64, 4)):
        if math.sqrt(K * a * (a + 1) / 3 * b * (b + 1) / 3) >= 400:
            return a, b
    return 64, 4
