"""Restatement of the soft disparity read-out and the stereo metrics (s3r_disparity_soft, s3r_disparity_metrics) in numpy.

The matching costs are formed in fp32 in the kernel's order (channel by channel, |a - b| then add), so they are exact; the softmax,
the upsampling and the metric sums run in fp64.  tests/test_disparity_soft_cpu.py pins these functions against hand-computed
cases; tests/test_disparity_soft_gpu.py measures the kernels against them.
"""
from __future__ import annotations

import numpy as np


def costs(fl: np.ndarray, fr: np.ndarray, max_disp: int, right: bool) -> np.ndarray:
    """(B,C,H,W) fp32 x2 -> (B,H,W,Dm) fp32 costs, Dm = min(max_disp, W); +inf where d >= n(w)"""
    fl, fr = np.asarray(fl, np.float32), np.asarray(fr, np.float32)
    B, C, H, W = fl.shape
    dm = min(max_disp, W)
    a, m = (fr, fl) if right else (fl, fr)
    out = np.full((B, H, W, dm), np.inf, np.float32)
    for d in range(dm):
        ws = np.arange(W - d) if right else np.arange(d, W)        # reference pixels with a partner at distance d
        wm = ws + d if right else ws - d
        c = np.zeros((B, H, ws.size), np.float32)
        for k in range(C):
            c = (c + np.abs(a[:, k][:, :, ws] - m[:, k][:, :, wm])).astype(np.float32)
        out[:, :, ws, d] = c
    return out


def soft(fl, fr, max_disp: int, tau: float):
    """feature-resolution soft read-out: ((disp_l, disp_r), (conf_l, conf_r)), each (B,H,W) fp64"""
    tau = float(np.float32(tau))
    disp, conf = [], []
    for right in (False, True):
        c = costs(fl, fr, max_disp, right).astype(np.float64)
        mn = c.min(-1, keepdims=True)
        e = np.exp((mn - c) / tau)                                  # exp(-inf) = 0 outside [0, n)
        d = np.arange(c.shape[-1], dtype=np.float64)
        z = e.sum(-1)
        disp.append((e * d).sum(-1) / z)
        conf.append(1.0 / z)
    return tuple(disp), tuple(conf)


def bilinear(x: np.ndarray, oh: int, ow: int) -> np.ndarray:
    """(B,H,W) -> (B,oh,ow) in fp64 with torch's align_corners=False rule (source index in fp32, as torch and the kernel form it)"""
    x = np.asarray(x, np.float64)
    B, H, W = x.shape

    def src(n_in, n_out):
        dst = np.arange(n_out, dtype=np.float32)
        s = np.float32(n_in) / np.float32(n_out) * (dst + np.float32(0.5)) - np.float32(0.5)
        s = np.maximum(s, np.float32(0)).astype(np.float32)
        i0 = np.minimum(s.astype(np.int64), n_in - 1)
        i1 = np.where(i0 < n_in - 1, i0 + 1, i0)
        return i0, i1, (s - i0.astype(np.float32)).astype(np.float64)

    h0, h1, lh = src(H, oh)
    w0, w1, lw = src(W, ow)
    top = x[:, h0][:, :, w0] * (1 - lw) + x[:, h0][:, :, w1] * lw
    bot = x[:, h1][:, :, w0] * (1 - lw) + x[:, h1][:, :, w1] * lw
    return top * (1 - lh)[:, None] + bot * lh[:, None]


def metrics(pred: np.ndarray, gt: np.ndarray):
    """(B,...) x2 fp32 -> (epe (B,) fp64, counts (B,4) int64: valid, |err| > 1, |err| > 3, D1); |err| formed in fp32 as the kernel
    forms it, 0.05 gt in fp64"""
    pred = np.asarray(pred, np.float32).reshape(len(pred), -1)
    gt = np.asarray(gt, np.float32).reshape(len(gt), -1)
    with np.errstate(invalid="ignore"):
        valid = np.isfinite(gt) & (gt >= 0)
        err = np.abs(pred - gt).astype(np.float64)
    err = np.where(valid, err, 0.0)
    n = valid.sum(1)
    epe = np.where(n > 0, err.sum(1) / np.maximum(n, 1), 0.0)
    g64 = np.where(valid, gt, 0).astype(np.float64)
    counts = np.stack([n, (valid & (err > 1)).sum(1), (valid & (err > 3)).sum(1),
                       (valid & (err > 3) & (err > 0.05 * g64)).sum(1)], 1)
    return epe, counts
