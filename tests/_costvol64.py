"""The cost volume's backward (s3r_cost_volume_backward, include/s3r.h) restated in numpy: the defined fp32 order, the same sums in
float64 with a derived bound, the case table and data sets that tests/test_cost_volume_backward_cpu.py and _gpu.py share, and the
mutants of the order that those data sets must tell from it.

With gv = grad_volume (B, 2C, D, H, W), n_L(w) = min(D, w + 1), n_R(w) = min(D, W - w):
  grad_left [b,c,h,w] = sum_{d < n_L(w)} ( gv[b,  c,d,h,w] - gv[b,C+c,d,h,w-d] )
  grad_right[b,c,h,w] = sum_{d < n_R(w)} ( gv[b,C+c,d,h,w] - gv[b,  c,d,h,w+d] )
Order: t_d is one fp32 subtraction; the accumulator starts AS t_0; t_1, t_2, ... are added in ascending d, each add rounded once.
A position that is in neither sum (left slab w < d, right slab w + d >= W, any plane d >= W: the forward's structural zeros) is
never an operand of anything — here through np.where, a select.

The bound.  u = 2^-24.  Per element, with a_d, b_d the two operands of term d, n terms, mag = sum_d (|a_d| + |b_d|):
  - the computed difference is t^_d = (a_d - b_d)(1 + e_d), |e_d| <= u (one rounding; a subtraction has no underflow error: a result in
    the subnormal range is exact), so sum_d |t^_d - t_d| <= u mag and sum_d |t^_d| <= (1 + u) mag;
  - the n - 1 sequential adds of the t^_d err by at most gamma_{n-1} sum_d |t^_d|, gamma_k = k u / (1 - k u) (Higham, Accuracy and
    Stability of Numerical Algorithms, 2nd ed., eq. 4.4), again with no underflow term;
  - together |fp32 - exact| <= (u + gamma_{n-1} (1 + u)) mag <= (n + 1) u mag whenever (n - 1)(n + 1) u <= 1, i.e. for every n < 4096
    (asserted): gamma_{n-1} (1 + u) <= n u  <=>  (n - 1)(1 + u) <= n (1 - (n - 1) u)  <=>  (n - 1) u + n (n - 1) u <= 1.
  The float64 reference's own error is below 2^-29 of that.  2^-149 (half the smallest subnormal's spacing would do) keeps the
  comparison meaningful where mag is 0.  This is the constant the feature's description proposes; the derivation confirms it.
"""
from __future__ import annotations

import functools

import numpy as np

U32 = 2.0 ** -24

# (B, C, D, H, W): the smallest shapes at which each path of the kernel can go wrong (one thread per (b, c, h, w), 256 per workgroup,
# the flat index cut at workgroup boundaries wherever they fall; no row bands, so no band-boundary case)
CASES = [
    (2, 2, 5, 3, 4),        # W < D: the planes d >= W contribute nothing
    (1, 3, 4, 2, 4),        # W = D
    (2, 1, 1, 1, 7),        # D = 1, C = 1, H = 1, an odd row length
    (1, 2, 3, 2, 9),        # rows that are no multiple of 4 floats
    (3, 2, 6, 5, 13),       # H W = 65: across a wavefront boundary; B = 3 for the batch tests; 390 elements: a partial second workgroup
    (1, 1, 4, 23, 23),      # H W = 529: more than two workgroups of 256
    (1, 32, 28, 28, 28),    # the network's own shape
    (2, 32, 28, 28, 28),
]
SMALL = CASES[:6]


def case_id(c):
    return "B%d-C%d-D%d-H%d-W%d" % tuple(c)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


# ---------------------------------------------------------------- data
@functools.lru_cache(maxsize=None)
def random_gv(case, seed=0):
    """dense normal data: the gradient of a loss with respect to the volume is dense, also where the forward wrote constants"""
    B, C, D, H, W = case
    g = np.random.default_rng(1000 * seed + 7 * B + 31 * C + D + 3 * H + W)
    a = g.standard_normal((B, 2 * C, D, H, W)).astype(np.float32)
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def lattice_gv(case, seed=0):
    """integers in [-8, 8]: every difference and every partial sum is an integer far below 2^24, exact in any order"""
    B, C, D, H, W = case
    g = np.random.default_rng(50 + seed + B + C + D + H + W)
    a = g.integers(-8, 9, (B, 2 * C, D, H, W)).astype(np.float32)
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def signed_zero_gv(case):
    """-0.0 throughout the left slab, +0.0 throughout the right one: every term of grad_left is -0.0 - +0.0 = -0.0 and their sum is
    -0.0 — unless the accumulator starts as +0.0 (+0.0 + -0.0 = +0.0); every term of grad_right is +0.0 - -0.0 = +0.0"""
    B, C, D, H, W = case
    a = np.zeros((B, 2 * C, D, H, W), np.float32)
    a[:, :C] = -0.0
    a.setflags(write=False)
    return a


def structural_zero_masks(case):
    """the three classes of positions of gv that are in neither sum, as bool masks of gv's shape (a class may be empty for a case):
    left slab w < d (planes d < W only), right slab w + d >= W (planes d < W only), every plane d >= W of both slabs"""
    B, C, D, H, W = case
    d = np.arange(D).reshape(1, 1, D, 1, 1)
    w = np.arange(W).reshape(1, 1, 1, 1, W)
    left = np.zeros((B, 2 * C, D, H, W), bool)
    right = np.zeros_like(left)
    plane = np.zeros_like(left)
    left[:, :C] = (w < d) & (d < W)
    right[:, C:] = (w + d >= W) & (d < W)
    plane[:] = d >= W
    return {"left slab w < d": left, "right slab w + d >= W": right, "plane d >= W": plane}


def live_mask(case):
    m = structural_zero_masks(case)
    return ~(m["left slab w < d"] | m["right slab w + d >= W"] | m["plane d >= W"])


# ---------------------------------------------------------------- the defined order, and its mutants
MUTANTS = ("descending d", "start from +0.0", "n_L off by one", "slabs swapped", "mask by multiplication")


def _side32(A, S, sign, D, W, mutant):
    """one side: A the aligned slab (B,C,D,H,W), S the shifted one; term d of position w is A[d][w] - S[d][w - sign d], live iff
    0 <= w - sign d < W (left: sign +1, right: sign -1)"""
    Dn = min(D, W)
    w = np.arange(W)
    order = range(Dn - 1, -1, -1) if mutant == "descending d" else range(Dn)
    acc = np.zeros(A[:, :, 0].shape, np.float32)
    if mutant != "start from +0.0":
        started = np.zeros(W, bool)
    else:
        started = np.ones(W, bool)                                # the accumulator exists from the start, as +0.0
    with np.errstate(invalid="ignore", over="ignore"):
        for d in order:
            a = A[:, :, d]
            b = np.zeros_like(a)
            if sign > 0:
                b[..., d:] = S[:, :, d][..., :W - d]
                live = w >= d
                if mutant == "n_L off by one":
                    live = w > d                                  # n_L(w) = min(D, w): the last term of every sum is dropped
            else:
                b[..., :W - d] = S[:, :, d][..., d:]
                live = w + d < W
            if mutant == "mask by multiplication":
                t = ((a - b).astype(np.float32) * live.astype(np.float32)).astype(np.float32)
                acc = np.where(started, (acc + t).astype(np.float32), t)
                started = np.ones(W, bool)
                continue
            t = (a - b).astype(np.float32)                        # ONE fp32 subtraction
            acc = np.where(live & started, (acc + t).astype(np.float32), np.where(live, t, acc))
            started = started | live
    return acc


def backward32(gv, mutant=None):
    """(grad_left, grad_right) in the defined fp32 order, every operation one np.float32 operation; `mutant` names a deliberate
    departure from it (MUTANTS)"""
    assert mutant is None or mutant in MUTANTS, mutant
    gv = np.asarray(gv, np.float32)
    B, C2, D, H, W = gv.shape
    C = C2 // 2
    L, R = gv[:, :C], gv[:, C:]
    if mutant == "slabs swapped":
        L, R = R, L
    return _side32(L, R, +1, D, W, mutant), _side32(R, L, -1, D, W, mutant)


def backward64(gv):
    """the same sums in float64: (grad_left, grad_right, n_left, n_right, mag_left, mag_right); n the number of terms of each element
    (broadcastable over (B,C,H,W)), mag = sum over its terms of |a| + |b|"""
    g = np.asarray(gv, np.float64)
    B, C2, D, H, W = g.shape
    C = C2 // 2
    L, R = g[:, :C], g[:, C:]
    gl, gr = np.zeros((B, C, H, W)), np.zeros((B, C, H, W))
    ml, mr = np.zeros((B, C, H, W)), np.zeros((B, C, H, W))
    for d in range(min(D, W)):
        gl[..., d:] += L[:, :, d][..., d:] - R[:, :, d][..., :W - d]
        ml[..., d:] += np.abs(L[:, :, d][..., d:]) + np.abs(R[:, :, d][..., :W - d])
        gr[..., :W - d] += R[:, :, d][..., :W - d] - L[:, :, d][..., d:]
        mr[..., :W - d] += np.abs(R[:, :, d][..., :W - d]) + np.abs(L[:, :, d][..., d:])
    w = np.arange(W)
    nl = np.minimum(D, w + 1).reshape(1, 1, 1, W)
    nr = np.minimum(D, W - w).reshape(1, 1, 1, W)
    return gl, gr, nl, nr, ml, mr


def bound32(n, mag):
    """|fp32 in the defined order - float64| per element (module docstring)"""
    assert np.max(n) < 4096
    return (np.asarray(n, np.float64) + 1.0) * U32 * mag + 2.0 ** -149


def oracle_backward64(gv, oracle):
    """torch's float64 autograd through the oracle's own formulation of the forward (oracle.s2v_oracle.cost_volume), for the output
    gradient gv: the reference backward64 is checked against"""
    import torch
    B, C2, D, H, W = gv.shape
    fl = torch.zeros(B, C2 // 2, H, W, dtype=torch.float64, requires_grad=True)
    fr = torch.zeros(B, C2 // 2, H, W, dtype=torch.float64, requires_grad=True)
    vol = oracle.cost_volume(fl, fr, D)
    gl, gr = torch.autograd.grad(vol, (fl, fr), torch.from_numpy(np.asarray(gv, np.float64)))
    return gl.numpy(), gr.numpy()
