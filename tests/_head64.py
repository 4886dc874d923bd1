"""numpy restatements of s3r_head_backward (include/s3r.h) for tests/test_head_backward_{cpu,gpu}.py.

The layer is y[b][s] = act(fmaf(sum_c x[b][c][s] w[c], scale, shift)): x (B,C,S), w (C), scale one float or None, y and grad_y (B,S).

  g32(y, gy, act)          s3r_linear_backward's rule word for word (tests/_linear64.py)
  gs32(g, scale)           g * scale rounded once; g itself when scale is None
  grad_x32(gs, w)          gs[b][s] * w[c]: one multiplication, bit for bit
  chunk_sums32(terms)      the header's order inside a sample: chunks of 512 positions; lane L owns positions 256 j + 4 L + i (j = 0, 1;
                           i = 0..3) and adds its terms in ascending position to a partial that starts as +0.0; halving tree over the
                           64 lanes.  `terms` are gs * x ROUNDED (the product and the add are not fused) or g
  reduce32(terms)          chunk sums -> per-sample partial (ascending chunk, starting from chunk 0's) -> ONE accumulator in ascending
                           b starting from sample 0's.  `batch_order=` builds the wrong orders the cases must catch
  grad_w32 / grad_shift32  the two outputs, bit for bit
  backward64(x, gs, g)     ((grad_w, K, mag), (grad_shift, K, mag)) in float64 from the fp32 gs / g as given: K = B S terms per element
  bound32(K, mag)          tests/_linear64.py's any-order bound gamma_{K+1} mag + K 2^-149, used unchanged

Agreement of the standalone head with the fused d3 + d4 path (forward_bound).  Both evaluate z = sum_{c<64} x_c w_c + bias in fp32 in some
order with or without fused multiply-adds, from the SAME x: each is within bound32(65, sum|x_c w_c| + |bias|) of the real z (65
terms: the bias add is one more), so they are within twice that of each other.  The sigmoid's slope is at most 1/4, so that becomes
at most half of bound32 in y.  Each side then evaluates the sigmoid itself as 1 / (1 + exp(-z)) with the fast exponential: the
exponent z * log2(e) carries two relative roundings (the constant and the product), i.e. 2 |z| u relative in e = exp(-z); the
exp2 instruction is specified to 1 ulp (2 u); the add rounds once (u) and the reciprocal or division to 1 ulp (2 u): to first order
(2 |z| + 5) u relative in y per side; (2 |z| + 6) u is taken to absorb the second-order terms.  In all:
  |y_a - y_b| <= bound32(65, mag) / 2 + 2 (2 |z| + 6) u y
Derived, not measured.
"""
import numpy as np

from tests._linear64 import ACTS, EPS64, U32, bits, bound32, g32, gamma      # noqa: F401  (re-exported)

CHUNK = 512
F = np.float32


def gs32(g, scale):
    g = np.asarray(g, F)
    if scale is None:
        return g.copy()
    with np.errstate(all="ignore"):
        return (g * F(scale)).astype(F)


def grad_x32(gs, w):
    with np.errstate(all="ignore"):
        return (np.asarray(gs, F)[:, None, :] * np.asarray(w, F)[None, :, None]).astype(F)


def chunk_sums32(terms):
    """(..., S) fp32 terms -> (..., ceil(S / 512)) chunk sums"""
    t = np.asarray(terms, F)
    S = t.shape[-1]
    nch = (S + CHUNK - 1) // CHUNK
    x = np.zeros(t.shape[:-1] + (nch * CHUNK,), F)
    x[..., :S] = t
    x = x.reshape(t.shape[:-1] + (nch, 2, 64, 4))                          # [chunk][j][lane][i]: position 256 j + 4 lane + i
    with np.errstate(all="ignore"):
        v = np.zeros(t.shape[:-1] + (nch, 64), F)
        for j in range(2):
            for i in range(4):
                v = (v + x[..., j, :, i]).astype(F)
        for o in (32, 16, 8, 4, 2, 1):
            v = (v[..., :o] + v[..., o:2 * o]).astype(F)
    return v[..., 0]


def reduce32(terms, batch_order="ascending"):
    """terms (B, ..., S) -> (...): the full order.  batch_order "descending" and "pairwise" are mutants"""
    cs = chunk_sums32(terms)
    with np.errstate(all="ignore"):
        p = cs[..., 0].copy()
        for k in range(1, cs.shape[-1]):
            p = (p + cs[..., k]).astype(F)
        if batch_order == "descending":
            p = p[::-1]
        if batch_order == "pairwise" and p.shape[0] > 2:
            half = p.shape[0] // 2
            return (reduce_rows(p[:half]) + reduce_rows(p[half:])).astype(F)
        return reduce_rows(p)


def reduce_rows(p):
    with np.errstate(all="ignore"):
        s = p[0].copy()
        for b in range(1, p.shape[0]):
            s = (s + p[b]).astype(F)
    return s


def grad_w32(gs, x, batch_order="ascending"):
    with np.errstate(all="ignore"):
        terms = (np.asarray(gs, F)[:, None, :] * np.asarray(x, F)).astype(F)
    return reduce32(terms, batch_order)


def grad_shift32(g, batch_order="ascending"):
    return reduce32(np.asarray(g, F), batch_order)


def boundaries():
    """positions per sample at which the order takes another path: a short quad, a full row of lanes, a chunk, two chunks"""
    out = set()
    for n in (4, 256, CHUNK, 2 * CHUNK):
        out |= {n - 1, n, n + 1}
    return sorted(out)


def backward64(x, gs, g):
    x64, gs64, g64 = (np.asarray(a, F).astype(np.float64) for a in (x, gs, g))
    K = g64.size
    gw = np.einsum("bs,bcs->c", gs64, x64)
    gw_mag = np.einsum("bs,bcs->c", np.abs(gs64), np.abs(x64))
    return (gw, K, gw_mag), (g64.sum(), K, np.abs(g64).sum())


def forward64(x, w, bias, act, scale=None):
    """(y, z, mag) in float64: z the pre-activation, mag = sum_c |x_c w_c| * |scale| + |bias|"""
    x64, w64 = np.asarray(x, F).astype(np.float64), np.asarray(w, F).astype(np.float64).reshape(-1)
    sc = 1.0 if scale is None else float(F(scale))
    z = np.einsum("bc...,c->b...", x64, w64) * sc + float(bias)
    mag = np.einsum("bc...,c->b...", np.abs(x64), np.abs(w64)) * abs(sc) + abs(float(bias))
    with np.errstate(all="ignore"):
        y = {"none": z, "relu": np.maximum(z, 0.0), "sigmoid": 1.0 / (1.0 + np.exp(-z))}[act]
    return y, z, mag


def forward_bound(z, mag, y, K=65):
    return bound32(K, mag) / 2 + 2 * (2 * np.abs(z) + 6) * U32 * np.abs(y)


# (B, C, S) of the device tests: the issue's list, then the boundaries of the order above (tests/test_head_backward_cpu.py checks
# that every boundary is here)
SHAPES = [(1, 1, 1), (1, 1, 4), (2, 3, 5), (1, 64, 256), (2, 64, 257), (3, 17, 1023), (2, 64, 4096), (33, 2, 64), (1, 5, 65537),
          (2, 64, 32768), (2, 3, 3), (3, 5, 255), (2, 7, 511), (2, 5, 512), (3, 4, 513), (65, 3, 1024), (2, 6, 1025)]
BIG = {(1, 5, 65537): "relu", (2, 64, 32768): "sigmoid"}                  # the largest shapes run one activation each
