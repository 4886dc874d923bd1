"""Plain sequential references of the kernels that take a discrete decision (tests/test_selection_{cpu,gpu}.py): the Chamfer
nearest-neighbour search and the thresholded voxel IoU.  numpy only, and no library routine takes a decision here: no min, argmin,
nanmin or sort — a candidate replaces the running best on a strict `<` written out below, so what a tie, a NaN or an infinity does is
readable from these few lines.  (The winner-take-all read-out already has such a reference, oracle.disparity_wta; the soft read-out
and the metrics have tests/_disp64.py.)

The contract these functions state (include/s3r.h, s3r_chamfer_forward and s3r_voxel_iou):

  distance   ((dx*dx + dy*dy) + dz*dz) in fp32, dx = p.x - q.x ..., every operation rounded once, nothing fused;
  minimum    the smallest distance that is not NaN (IEEE minNum); its index is the LOWEST index holding that distance;
  no finite  a query none of whose distances is below +inf (every one +inf or NaN) gets dist = +inf, idx = 0;
  IoU        a voxel is occupied iff value > float32(threshold), compared in fp32 (NaN is not occupied, -0.0 and +0.0 compare
             equal); the two counts are exact integers; the result is float32(inter) / float32(union), both conversions
             round-to-nearest-even, one fp32 division; 1 when the union is empty.
"""
from __future__ import annotations

import numpy as np

CH_TILE = 2048      # candidates per staging pass of chamfer_kernel (csrc/s3r_chamfer.hip)
SLICES = 4          # wave slices of a pass, each ceil(count / 4) candidates
CBLK = 8            # candidates per block of a slice


def dist3(px, py, pz, qx, qy, qz):
    """((dx*dx + dy*dy) + dz*dz), each of the eight operations one float32 operation (numpy never fuses)"""
    dx, dy, dz = px - qx, py - qy, pz - qz
    d = (dx * dx + dy * dy) + dz * dz
    assert d.dtype == np.float32
    return d


def _scan_one_way(a, c):
    """queries a (B,Q,3) against candidates c (B,K,3), both float32 -> (dist (B,Q) float32, idx (B,Q) int32)"""
    B, Q, K = a.shape[0], a.shape[1], c.shape[1]
    ax, ay, az = a[:, :, 0], a[:, :, 1], a[:, :, 2]
    best = np.full((B, Q), np.inf, np.float32)
    idx = np.zeros((B, Q), np.int32)
    for j in range(K):                                   # candidates in ascending index
        d = dist3(ax, ay, az, c[:, j, 0][:, None], c[:, j, 1][:, None], c[:, j, 2][:, None])
        upd = d < best                                   # strict: an equal distance later never replaces; NaN compares false
        best[upd] = d[upd]
        idx[upd] = j
    return best, idx


def chamfer_scan(p, q):
    """p (B,N,3), q (B,M,3) -> (dist1 (B,N), dist2 (B,M), idx1 (B,N), idx2 (B,M)), float32 / int32: per query a scan of the other
    cloud in ascending index from best = +inf, idx = 0, updating only on d < best"""
    p, q = np.ascontiguousarray(p, np.float32), np.ascontiguousarray(q, np.float32)
    with np.errstate(all="ignore"):
        d1, i1 = _scan_one_way(p, q)
        d2, i2 = _scan_one_way(q, p)
    return d1, d2, i1, i2


def chamfer_tie_stats(p, q, dist1):
    """for direction 0 (queries p, candidates q) and the scan's dist1: per query the number of candidates AT the minimum (B,N) and
    the number of staging passes that hold one (B,N).  Dense, one pass of CH_TILE candidates at a time."""
    p, q = np.ascontiguousarray(p, np.float32), np.ascontiguousarray(q, np.float32)
    B, N, M = p.shape[0], p.shape[1], q.shape[1]
    count = np.zeros((B, N), np.int64)
    passes = np.zeros((B, N), np.int64)
    with np.errstate(all="ignore"):
        for j0 in range(0, M, CH_TILE):
            c = q[:, None, j0:j0 + CH_TILE]
            d = dist3(p[:, :, None, 0], p[:, :, None, 1], p[:, :, None, 2], c[..., 0], c[..., 1], c[..., 2])
            eq = d == dist1[:, :, None]
            count += eq.sum(-1)
            passes += eq.any(-1)
    return count, passes


def iou_ref(pred, gt, th):
    """(B,V) float32 x2 -> (B,) float32 by the contract above"""
    pred = np.ascontiguousarray(pred, np.float32).reshape(len(pred), -1)
    gt = np.ascontiguousarray(gt, np.float32).reshape(len(gt), -1)
    t = np.float32(th)
    with np.errstate(invalid="ignore"):
        a, b = pred > t, gt > t                          # float32 against float32
    assert np.result_type(pred, t) == np.float32 and np.result_type(gt, t) == np.float32
    inter = np.count_nonzero(a & b, axis=1)              # exact integers
    union = np.count_nonzero(a | b, axis=1)
    out = np.ones(len(pred), np.float32)
    for s in range(len(pred)):
        if union[s]:
            out[s] = np.float32(int(inter[s])) / np.float32(int(union[s]))     # int -> float32 is round-to-nearest-even
    return out


def bits(x):
    x = np.ascontiguousarray(x)
    return x.view(np.int32) if x.dtype == np.float32 else x


def assert_same(got, want, what, case):
    """bit-for-bit; a failure names the first differing element: `case what: query (1, 1731): got 2100, want 1600`"""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, f"{case} {what}: {got.dtype}{got.shape} against {want.dtype}{want.shape}"
    bad = np.argwhere(bits(got) != bits(want))
    if bad.size:
        at = tuple(int(v) for v in bad[0])
        raise AssertionError(f"{case} {what}: {len(bad)} of {got.size} differ, first at {at}: got {got[at]!r}, want {want[at]!r}")
