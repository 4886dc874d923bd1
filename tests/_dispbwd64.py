"""Restatement of the soft read-out's backward and of the disparity loss (s3r_disparity_soft_backward, s3r_disparity_loss_forward /
_backward) in numpy: the fp32 ORDER include/s3r.h states (backward32, loss32, loss_grad32, loss_sum32) and the same sums in float64
(backward64, which also returns the per-element bound between the two).  tests/_disp64.py is imported as it is: the costs are its costs
(fp32, the kernel's order: exact) and the bilinear source rule below is the one inside its `bilinear`, restated as index arrays
(tests/test_disparity_backward_cpu.py checks the two against each other).

The bound.  u = 2^-24.  backward64 forms everything in float64 from the TRUE costs (float64 sums of |a - m|); the fp32 arithmetic differs
from it, per (direction, pixel) with n disparities and largest cost cmax, by
  - the costs: a sequential fp32 sum of C non-negative terms, each a rounded difference: |dc| <= (C + 1) u cmax for every d and the minimum;
  - the exponent x_d = (min - c_d) / tau: |dx_d| <= 2 (C + 1) u cmax / tau + 3 u |x_d|  (two cost errors; the subtraction and the division);
  - e_d = expf(x_d), documented 2 ulp = 4 u: relative error rho_d <= |dx_d| + 4 u; rho = max_d rho_d.  (A flushed weight is below 2^-126.)
  - Z and S, sums of n non-negative terms in any order: relative error <= rho + (n + 1) u; disp = S / Z: |ddisp| <= disp (2 rho + (2 n + 3) u);
  - p_d = e_d / Z: relative error <= 2 rho + (n + 2) u; t_d = p_d (disp - d):
        |dt_d| <= p_d ((2 rho + (n + 3) u) |disp - d| + |ddisp|) + u |t_d|;
  - G: at the feature size one rounded product, |dG| <= u |G|; otherwise a sum of N terms ((g s) wy) wx — three rounded products and two
    weights of up to two roundings each, <= 7 u per term — in any order: |dG| <= (N + 6) u sum |terms|; k = G / tau: |dk| <= |dG| / tau + u |k|;
  - q_d = t_d k: |dq_d| <= |dt_d| |k| + |t_d| |dk| + u |q_d|;
  - an output, the sum over n terms +-(q^own_d + q^other_d) in any order: |dgrad| <= sum_d (|dq^own_d| + |dq^other_d|) + n u sum_d |q^own_d + q^other_d|.
Everything on the right is evaluated in float64 from the float64 magnitudes; second-order terms are covered by the factor 1.01 and an
absolute 2^-120 stands in for the flushed weights.  Nothing here comes from what the kernel returns.
"""
from __future__ import annotations

import numpy as np

from tests import _disp64 as D64

U = 2.0 ** -24
F = np.float32
FLT_MIN = np.float32(np.finfo(np.float32).tiny)


def bits(a):
    return np.ascontiguousarray(np.asarray(a, np.float32)).view(np.int32)


# ---------------------------------------------------------------- the bilinear source rule (fp32, as tests/_disp64.bilinear forms it)
def src32(n_in: int, n_out: int):
    """(i0, i1, lam fp32) per output index: src = scale (dst + 0.5) - 0.5 clamped at 0, scale = in / out in fp32"""
    dst = np.arange(n_out, dtype=np.float32)
    s = F(n_in) / F(n_out) * (dst + F(0.5)) - F(0.5)
    s = np.maximum(s, F(0)).astype(np.float32)
    i0 = np.minimum(s.astype(np.int64), n_in - 1)
    i1 = np.where(i0 < n_in - 1, i0 + 1, i0)
    return i0, i1, (s - i0.astype(np.float32)).astype(np.float32)


def weights32(n_in: int, n_out: int) -> np.ndarray:
    """wt[o, i] fp32 = (i0 == i ? 1 - lam : 0) + (i1 == i ? lam : 0): the weight with which output index o reads source index i"""
    i0, i1, lam = src32(n_in, n_out)
    wt = np.zeros((n_out, n_in), np.float32)
    o = np.arange(n_out)
    a = np.zeros_like(wt)
    b = np.zeros_like(wt)
    a[o, i0] = F(1) - lam
    b[o, i1] = lam
    return (a + b).astype(np.float32)


def weights64(n_in: int, n_out: int) -> np.ndarray:
    """the same matrix in float64 from the fp32 lam (1 - lam formed in float64): the matrix of tests/_disp64.bilinear along one axis"""
    i0, i1, lam = src32(n_in, n_out)
    wt = np.zeros((n_out, n_in))
    o = np.arange(n_out)
    np.add.at(wt, (o, i0), 1.0 - lam.astype(np.float64))
    np.add.at(wt, (o, i1), lam.astype(np.float64))
    return wt


def gather32(g, H: int, W: int, scale) -> np.ndarray:
    """G (B,H,W) fp32 from grad_disp (B,OH,OW) in the stated order: rows ascending, columns ascending within a row, one accumulator
    that starts as +0.0.  An output pixel outside a feature pixel's window has weight 0 and adds +0.0 here (finite data: no bit
    changes; the kernel does not visit it)."""
    g = np.asarray(g, np.float32)
    B, OH, OW = g.shape
    s = F(scale)
    if (OH, OW) == (H, W):
        return (g * s).astype(np.float32)
    wy, wx = weights32(H, OH), weights32(W, OW)
    acc = np.zeros((B, H, W), np.float32)
    for oy in range(OH):
        hs = np.nonzero(wy[oy])[0]
        for ox in range(OW):
            ws = np.nonzero(wx[ox])[0]
            if ws.size == 0:
                continue
            gs = (g[:, oy, ox] * s).astype(np.float32)
            for h in hs:
                t = (gs * wy[oy, h]).astype(np.float32)
                for w in ws:
                    acc[:, h, w] = (acc[:, h, w] + (t * wx[ox, w]).astype(np.float32)).astype(np.float32)
    return acc


def gather64(g, H: int, W: int, scale):
    """(G float64, sum of |terms| float64, N terms per pixel) — the adjoint of tests/_disp64.bilinear times the fp32 scale"""
    g = np.asarray(g, np.float64)
    B, OH, OW = g.shape
    s = float(F(scale))
    if (OH, OW) == (H, W):
        return g * s, np.abs(g * s), np.ones((H, W))
    wy, wx = weights64(H, OH), weights64(W, OW)
    G = np.einsum("oh,bop,pw->bhw", wy, g * s, wx)
    mag = np.einsum("oh,bop,pw->bhw", wy, np.abs(g * s), wx)
    # the window holds every output whose i0 is i - 1 or i, a zero lam included
    ny = np.array([np.isin(src32(H, OH)[0], (h - 1, h)).sum() for h in range(H)])
    nx = np.array([np.isin(src32(W, OW)[0], (w - 1, w)).sum() for w in range(W)])
    return G, mag, np.outer(ny, nx).astype(np.float64)


# ---------------------------------------------------------------- q: d loss / d cost
def _q32(c, G, tau):
    """c (B,H,W,dm) fp32 costs (+inf outside [0, n)), G (B,H,W) fp32 -> q (B,H,W,dm) fp32, the kernel's operations in its order"""
    tau = F(tau)
    dm = c.shape[-1]
    with np.errstate(invalid="ignore", over="ignore"):
        mn = c[..., 0].copy()
        for d in range(1, dm):
            mn = np.fmin(mn, c[..., d])
        e = np.exp(((mn[..., None] - c).astype(np.float32) / tau).astype(np.float32)).astype(np.float32)
        e = np.where(e < FLT_MIN, F(0), e).astype(np.float32)
        z = np.zeros(c.shape[:-1], np.float32)
        s = np.zeros(c.shape[:-1], np.float32)
        for d in range(dm):
            z = (z + e[..., d]).astype(np.float32)
            s = (s + (F(d) * e[..., d]).astype(np.float32)).astype(np.float32)
        disp = (s / z).astype(np.float32)
        k = (np.asarray(G, np.float32) / tau).astype(np.float32)
        q = np.empty_like(c)
        for d in range(dm):
            p = (e[..., d] / z).astype(np.float32)
            t = (p * (disp - F(d)).astype(np.float32)).astype(np.float32)
            q[..., d] = (t * k).astype(np.float32)
    return q


def _dsum32(own, oth, qo, qx, right: bool, order: str = "contract"):
    """the ascending-d sum of one tensor: own, oth (B,C,H,W) fp32; qo, qx (B,H,W,dm) fp32.  `order` names the contract or a mutant of
    it: "descending" (d from n - 1 down), "from-zero-subtracting" (the accumulator starts as 0.0 and the terms are subtracted),
    "q-separately" (the two q's are not added first: two adds per d)."""
    B, C, H, W = own.shape
    dm = qo.shape[-1]
    out = np.zeros((B, C, H, W), np.float32)
    started = np.zeros(W, bool)
    ds = range(dm - 1, -1, -1) if order == "descending" else range(dm)
    for d in ds:
        ws = np.arange(W - d) if right else np.arange(d, W)       # outputs that have a term d
        wm = ws + d if right else ws - d
        a, m = own[..., ws], oth[..., wm]
        sign = np.where(a > m, F(1), np.where(a < m, F(-1), F(0))).astype(np.float32)

        def signed(v):
            return np.where(sign > 0, v, np.where(sign < 0, -v, F(0))).astype(np.float32)

        if order == "q-separately":
            parts = [signed(qo[:, None, :, ws, d]), signed(qx[:, None, :, wm, d])]
        else:
            parts = [signed((qo[:, None, :, ws, d] + qx[:, None, :, wm, d]).astype(np.float32))]
        for t in parts:
            t = np.broadcast_to(t, a.shape)
            if order == "from-zero-subtracting":
                out[..., ws] = (out[..., ws] - t).astype(np.float32)
                continue
            first = ~started[ws]
            cur = out[..., ws]
            out[..., ws] = np.where(first, t, (cur + t).astype(np.float32))
            started[ws] = True
    return out


def backward32(fl, fr, gdl, gdr, max_disp: int, tau, out_size=None, scale=1.0, order: str = "contract"):
    """(grad_left, grad_right) fp32 in the order include/s3r.h states; gdl or gdr None: zeros"""
    fl, fr = np.asarray(fl, np.float32), np.asarray(fr, np.float32)
    B, C, H, W = fl.shape
    OH, OW = (H, W) if out_size is None else out_size
    q = []
    for right, g in ((False, gdl), (True, gdr)):
        G = np.zeros((B, H, W), np.float32) if g is None else gather32(g, H, W, scale)
        q.append(_q32(D64.costs(fl, fr, max_disp, right), G, tau))
    return (_dsum32(fl, fr, q[0], q[1], False, order), _dsum32(fr, fl, q[1], q[0], True, order))


def _costs64(fl, fr, max_disp, right):
    """the TRUE costs: float64 sums of |a - m|; +inf where d >= n(w)"""
    fl, fr = np.asarray(fl, np.float64), np.asarray(fr, np.float64)
    B, C, H, W = fl.shape
    dm = min(max_disp, W)
    a, m = (fr, fl) if right else (fl, fr)
    out = np.full((B, H, W, dm), np.inf)
    for d in range(dm):
        ws = np.arange(W - d) if right else np.arange(d, W)
        wm = ws + d if right else ws - d
        out[:, :, ws, d] = np.abs(a[..., ws] - m[..., wm]).sum(1)
    return out


def backward64(fl, fr, gdl, gdr, max_disp: int, tau, out_size=None, scale=1.0):
    """((grad_left, grad_right) float64, (bound_left, bound_right)): the same sums in float64 and the per-element bound of the module
    docstring for an fp32 evaluation in any order"""
    fl32, fr32 = np.asarray(fl, np.float32), np.asarray(fr, np.float32)
    B, C, H, W = fl32.shape
    tau = float(F(tau))
    q, dq = [], []
    for right, g in ((False, gdl), (True, gdr)):
        c = _costs64(fl32, fr32, max_disp, right)
        dm = c.shape[-1]
        valid = np.isfinite(c)
        n = valid.sum(-1).astype(np.float64)
        cmax = np.where(valid, c, 0).max(-1)
        mn = c.min(-1, keepdims=True)
        x = (mn - c) / tau
        e = np.exp(x)
        d = np.arange(dm, dtype=np.float64)
        z = e.sum(-1)
        disp = (e * d).sum(-1) / z
        p = e / z[..., None]
        t = p * (disp[..., None] - d)
        if g is None:
            G, gmag, N = np.zeros((B, H, W)), np.zeros((B, H, W)), np.ones((H, W))
        else:
            G, gmag, N = gather64(g, H, W, scale)
        k = G / tau
        q.append(t * k[..., None])
        # the bound's pieces
        dx = 2 * (C + 1) * U * cmax[..., None] / tau + 3 * U * np.abs(np.where(valid, x, 0))
        rho = (np.where(valid, dx, 0) + 4 * U).max(-1)
        ddisp = disp * (2 * rho + (2 * n + 3) * U)
        dt = p * ((2 * rho + (n + 3) * U)[..., None] * np.abs(np.where(valid, disp[..., None] - d, 0)) + ddisp[..., None]) + U * np.abs(t)
        same = out_size is None or tuple(out_size) == (H, W)
        dG = U * np.abs(G) if same else (N + 6) * U * gmag
        dk = dG / tau + U * np.abs(k)
        dq.append(dt * np.abs(k)[..., None] + np.abs(t) * dk[..., None] + U * np.abs(t * k[..., None]) + 2.0 ** -120)
    res, bounds = [], []
    for right in (False, True):
        own, oth = (fr32, fl32) if right else (fl32, fr32)
        qo, qx = (q[1], q[0]) if right else (q[0], q[1])
        eo, ex = (dq[1], dq[0]) if right else (dq[0], dq[1])
        dm = qo.shape[-1]
        out, err, mag, cnt = (np.zeros((B, C, H, W)) for _ in range(4))
        for d in range(dm):
            ws = np.arange(W - d) if right else np.arange(d, W)
            wm = ws + d if right else ws - d
            sign = np.sign(own[..., ws].astype(np.float64) - oth[..., wm].astype(np.float64))
            u = (qo[:, None, :, ws, d] + qx[:, None, :, wm, d])
            out[..., ws] += sign * u
            mag[..., ws] += np.abs(sign * u)
            err[..., ws] += np.abs(sign) * (eo[:, None, :, ws, d] + ex[:, None, :, wm, d])
            cnt[..., ws] += 1
        res.append(out)
        bounds.append(1.01 * (err + cnt * U * mag) + 2.0 ** -120)
    return tuple(res), tuple(bounds)


# ---------------------------------------------------------------- data
# (B, C, H, W, D, OH, OW): the smallest shapes that reach every branch, and the network's own
CASES = [(2, 3, 3, 5, 4, 3, 5), (2, 3, 3, 5, 7, 3, 5), (2, 5, 3, 5, 4, 7, 12), (1, 4, 6, 10, 3, 4, 7), (1, 2, 2, 1, 3, 2, 1)]
NETWORK = (2, 32, 28, 28, 28, 224, 224)
UPSAMPLED = CASES[2]


def case_id(case):
    B, C, H, W, D, OH, OW = case
    return f"B{B}-C{C}-{H}x{W}-D{D}-to-{OH}x{OW}"


def out_size(case):
    B, C, H, W, D, OH, OW = case
    return None if (OH, OW) == (H, W) else (OH, OW)


def random_case(case, seed: int = 0):
    """(feat_l, feat_r, grad_disp_l, grad_disp_r) fp32: features of the network's magnitude (a ReLU output), unit gradients"""
    B, C, H, W, D, OH, OW = case
    rng = np.random.default_rng(seed + 17 * C + W)
    fl = np.maximum(rng.standard_normal((B, C, H, W)), 0).astype(np.float32)
    fr = np.maximum(rng.standard_normal((B, C, H, W)), 0).astype(np.float32)
    return fl, fr, rng.standard_normal((B, OH, OW)).astype(np.float32), rng.standard_normal((B, OH, OW)).astype(np.float32)


def equal_cost_case(case, seed: int = 0):
    """per-channel constant integer features a_c != b_c with ONE channel where a_c == b_c: every cost of every pixel is equal, so every
    weight is expf(0) = 1 and the whole backward is defined bit for bit"""
    B, C, H, W, D, OH, OW = case
    rng = np.random.default_rng(seed + 5)
    a = rng.integers(-4, 5, size=(B, C)).astype(np.float32)
    b = a + rng.choice([-3, -2, -1, 1, 2, 3], size=(B, C)).astype(np.float32)
    b[:, C // 2] = a[:, C // 2]
    fl = np.broadcast_to(a[:, :, None, None], (B, C, H, W)).copy()
    fr = np.broadcast_to(b[:, :, None, None], (B, C, H, W)).copy()
    return fl, fr, rng.standard_normal((B, OH, OW)).astype(np.float32), rng.standard_normal((B, OH, OW)).astype(np.float32)


# ---------------------------------------------------------------- the loss
def valid(gt):
    gt = np.asarray(gt, np.float32)
    with np.errstate(invalid="ignore"):
        return np.isfinite(gt) & (gt >= 0)


def loss32(pred, gt, beta):
    """loss_elem fp32 (+0.0 at invalid pixels) and the valid mask: e = p - t; |e| < beta: ((0.5 e) e) / beta, else |e| - 0.5 beta"""
    pred, gt, beta = np.asarray(pred, np.float32), np.asarray(gt, np.float32), F(beta)
    ok = valid(gt)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        e = (np.where(ok, pred, F(0)) - np.where(ok, gt, F(0))).astype(np.float32)
        a = np.abs(e)
        quad = (((F(0.5) * e).astype(np.float32) * e).astype(np.float32) / beta).astype(np.float32)
        lin = (a - (F(0.5) * beta)).astype(np.float32)
        l = np.where(a < beta, quad, lin).astype(np.float32)
    return np.where(ok, l, F(0)).astype(np.float32), ok


def loss_grad32(pred, gt, grad_scale, beta):
    """grad_pred fp32: grad_scale[b] * clamp(e / beta, -1, 1) (beta == 0: grad_scale[b] * sgn(e)); +0.0 at invalid pixels"""
    pred, gt, beta = np.asarray(pred, np.float32), np.asarray(gt, np.float32), F(beta)
    ok = valid(gt)
    gs = np.asarray(grad_scale, np.float32).reshape((-1,) + (1,) * (pred.ndim - 1))
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        e = (np.where(ok, pred, F(0)) - np.where(ok, gt, F(0))).astype(np.float32)
        if beta > 0:
            v = (e / beta).astype(np.float32)
            c = np.where(v < F(-1), F(-1), np.where(v > F(1), F(1), v)).astype(np.float32)
        else:
            c = np.where(e > 0, F(1), np.where(e < 0, F(-1), np.where(e == 0, F(0), e))).astype(np.float32)
        g = (gs * c).astype(np.float32)
    return np.where(ok, g, F(0)).astype(np.float32)


def loss_sum32(elem):
    """(B, P) fp32 -> (B,) fp32 in s3r_voxel_bce_forward's order: chunks of 1024, lane L owns 256 j + 4 L + i in ascending order from
    +0.0, the halving tree over the 64 partials, the chunk sums in ascending chunk order starting from chunk 0's"""
    elem = np.asarray(elem, np.float32)
    B, P = elem.shape
    nch = -(-P // 1024)
    x = np.zeros((B, nch * 1024), np.float32)
    x[:, :P] = elem
    x = x.reshape(B, nch, 4, 64, 4)                                   # [chunk][j][lane][i]
    part = np.zeros((B, nch, 64), np.float32)
    for j in range(4):
        for i in range(4):
            part = (part + x[:, :, j, :, i]).astype(np.float32)
    o = 32
    while o:
        part[:, :, :o] = (part[:, :, :o] + part[:, :, o:2 * o]).astype(np.float32)
        o //= 2
    total = part[:, 0, 0].copy()
    for c in range(1, nch):
        total = (total + part[:, c, 0]).astype(np.float32)
    return total
