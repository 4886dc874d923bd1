"""numpy / float64 restatements of s3r_stem_backward (include/s3r.h) for tests/test_stem_backward_{cpu,gpu}.py.

The layer is the stem  y = act(conv2d(X, w; 3 -> 32, k 3, stride 2, pad 1) * scale[o] + shift[o]), X the render as the forward reads it:
fp32 as it is, uint8 as float32(u) / float32(255).

  render32(r)             the render as fp32: the host conversion the kernel's scaling must equal bit for bit
  g32, gs32, grad_shift32 tests/_convbwd64.py's, unchanged: s3r_conv_backward's rule and order over (image, channel) rows of m^2 positions
  grad_w64(x, gs)         the header's formula in float64 through tests/_convbwd64.py's grad_w64 on the stem's geometry; returns
                          (grad_w, K, mag) with K = n_images m^2, the number of terms the issue's bound counts, and mag = sum |gs| |X|
  grad_w_ordered32(...)   the header's slice / image order restated in fp32 with float64 partial dot products rounded once per slice:
                          NOT the kernel's bits (inside a slice the kernel is an fp32 fmaf chain) — only a vehicle for the order mutants
                          of tests/test_stem_backward_cpu.py, which must move its result on the device table's data
  slices(m)               csrc/s3r_stem_bwd.hip's slicing restated: r = ceil(m / 32) rows per slice, ceil(m / r) slices
  scratch_elems(n, s)     stem_backward_scratch_elems restated: [32 n ceil(m^2 / 512)][n nsl 864][n 864]
  bound32(K, mag)         tests/_linear64.py's any-order bound, unchanged

CASES are the issue's (n_images, in_size) table.
"""
import numpy as np
import torch

from tests import _convbwd64 as R
from tests._convbwd64 import bits, bound32, g32, grad_shift32, gs32      # noqa: F401  (re-exported)

F = np.float32
CO, CI, K3 = 32, 3, 3

CASES = [(1, 1), (2, 2), (3, 7), (2, 8), (2, 46), (3, 64), (1, 130), (5, 20), (70, 4), (1, 224), (2, 224)]
SMALL = [c for c in CASES if c[1] <= 64 and c[0] <= 5]                     # every run / address / split variant runs on these
ACTS = ("relu", "none")


def case_id(c):
    return f"n{c[0]}-s{c[1]}"


def out_edge(s):
    return (s - 1) // 2 + 1


def conv_case(n_images, in_size):
    """the stem over an edge of in_size as a tests/_convbwd64.py case"""
    return R.Case("conv", 2, CI, CO, K3, 2, 1, 0, in_size, n_images)


def render32(r):
    """fp32 renders as they are; uint8 renders as float32(u) / float32(255), correctly rounded (numpy's fp32 division is)"""
    r = np.asarray(r)
    if r.dtype == np.uint8:
        return (r.astype(F) / F(255)).astype(F)
    assert r.dtype == F
    return r


def slices(m):
    rps = (m + 31) // 32
    return rps, (m + rps - 1) // rps


def scratch_elems(n_images, in_size):
    if n_images == 0:
        return 0
    m = out_edge(in_size)
    return CO * n_images * ((m * m + 511) // 512) + n_images * slices(m)[1] * CO * 27 + n_images * CO * 27


def make(n_images, in_size, seed, act="relu", u8=False, lattice=False, scale=True):
    """(renders, scale, y, grad_y): renders fp32 in [0, 1) or uint8; y the layer's own output for random weights (float64, rounded once;
    None for act none); lattice=True: small integers in grad_y and scale, renders small integers (fp32) or drawn from {0, 255} (uint8:
    X is then exactly 0 or 1), y a sign pattern"""
    g = torch.Generator().manual_seed(seed)
    m = out_edge(in_size)
    shape, yshape = (n_images, CI, in_size, in_size), (n_images, CO, m, m)
    if lattice:
        if u8:
            x = (torch.randint(0, 2, shape, generator=g) * 255).to(torch.uint8)
        else:
            x = torch.randint(-3, 4, shape, generator=g).float()
        gy = torch.randint(-3, 4, yshape, generator=g).float()
        sc = torch.randint(1, 3, (CO,), generator=g).float() if scale else None
        y = torch.randint(0, 2, yshape, generator=g).float() * 2 - 1
    else:
        x = torch.randint(0, 256, shape, generator=g).to(torch.uint8) if u8 else torch.rand(shape, generator=g)
        gy = torch.randn(yshape, generator=g)
        sc = (0.5 + torch.rand(CO, generator=g)) if scale else None
        w = torch.randn((CO, CI, K3, K3), generator=g) / 27 ** 0.5
        sh = 0.1 * torch.randn(CO, generator=g)
        x64 = torch.from_numpy(render32(x.numpy())).double() - 0.5         # (centred: about half of the ReLU gates are open)
        z = torch.nn.functional.conv2d(x64, w.double(), None, 2, 1)
        if sc is not None:
            z = z * sc.double().view(1, -1, 1, 1)
        y = torch.relu(z + sh.double().view(1, -1, 1, 1)).float()
    return x.numpy(), None if sc is None else sc.numpy(), (None if act == "none" else y.numpy()), gy.numpy()


def grad_w64(x32, gs):
    """(grad_w (32,3,3,3), K, mag): float64 from the fp32 X and gs as given; K = n_images m^2"""
    x32, gs = np.asarray(x32, F), np.asarray(gs, F)
    gw, _, mag = R.grad_w64(conv_case(x32.shape[0], x32.shape[2]), x32, gs)
    return gw, gs.shape[0] * gs.shape[2] * gs.shape[3], mag


def grad_w_ordered32(x32, gs, slice_order="ascending", image_order="ascending"):
    """the header's order around float64 slice sums: per image, the slices' sums (each rounded to fp32 once) added in `slice_order`
    starting from the first; the images' partials added in `image_order` starting from the first"""
    x32, gs = np.asarray(x32, F), np.asarray(gs, F)
    n, m = x32.shape[0], gs.shape[2]
    rps, nsl = slices(m)
    parts = []
    for b in range(n):
        sums = []
        for z in range(nsl):
            rows = np.zeros((1, CO, m, m), F)
            rows[0, :, z * rps:(z + 1) * rps] = gs[b, :, z * rps:(z + 1) * rps]
            sums.append(R.grad_w64(conv_case(1, x32.shape[2]), x32[b:b + 1], rows)[0].astype(F))
        if slice_order == "descending":
            sums = sums[::-1]
        p = sums[0].copy()
        for t in sums[1:]:
            p = (p + t).astype(F)
        parts.append(p)
    if image_order == "descending":
        parts = parts[::-1]
    acc = parts[0].copy()
    for p in parts[1:]:
        acc = (acc + p).astype(F)
    return acc
