"""numpy restatements of s3r_chamfer_backward (include/s3r.h) for tests/test_chamfer_backward_{cpu,gpu}.py.

Per sample, with a_i = 2 grad_dist1[i] and c_j = 2 grad_dist2[j], per component:
    grad_p[i] = a_i (p_i - q_idx1[i])  +  sum_{j ascending, idx2[j] == i}  c_j (p_i - q_j)
    grad_q[j] = c_j (q_j - p_idx2[j])  +  sum_{i ascending, idx1[i] == j}  a_i (q_j - p_i)

backward32   (a) the DEFINED fp32 order: every difference, product and add is one np.float32 operation (numpy's float32 arithmetic
             is IEEE round-to-nearest-even and never fused), the accumulator starts as the own term, the scattered terms are
             added one at a time in ascending source index.  The kernel must give these bits.
backward64   (b) the same sum in float64, and per element the number k of scattered terms and sum|term| (own term included): the
             data of the bound |fp32 - fp64| <= (k + 3) 2^-24 sum|term| + 2^-149 (one rounding for the difference, one for the
             product, k adds each bounded by sum|term|, +1 for second order; one subnormal for underflow).

A grad_dist of None is a zero tensor.  The own-term index is clamped into the other cloud, an out-of-range scatter index matches no
target — as the header states for garbage indices.  Both functions loop over the sources (ascending) and are vectorised over the
batch: within one source index every sample scatters to ONE target, so a fancy-indexed read-modify-write never collides.
"""
import numpy as np

EPS32 = 2.0 ** -24
EPS64 = 2.0 ** -53
TINY32 = 2.0 ** -149


def _direction(t, s, own, sct, w_own, w_sct, dtype):
    """targets t (B,T,3), sources s (B,S,3), own (B,T) into s, sct (B,S) into t, weights already doubled.
    -> grad (B,T,3) in `dtype`, k (B,T) scattered-term counts, mag (B,T,3) float64 sum of |term|"""
    B, T, S = t.shape[0], t.shape[1], s.shape[1]
    rows = np.arange(B)
    t, s = t.astype(dtype), s.astype(dtype)
    w_own, w_sct = w_own.astype(dtype), w_sct.astype(dtype)
    o = np.clip(own.astype(np.int64), 0, S - 1)
    diff = (t - s[rows[:, None], o]).astype(dtype)                  # rounded once
    acc = (w_own[:, :, None] * diff).astype(dtype)                  # rounded once: the accumulator starts as the own term
    mag = np.abs(acc.astype(np.float64))
    k = np.zeros((B, T), np.int64)
    sct = sct.astype(np.int64)
    for j in range(S):
        tgt = sct[:, j]
        ok = (tgt >= 0) & (tgt < T)
        if not ok.any():
            continue
        r, i = rows[ok], tgt[ok]
        d = (t[r, i] - s[r, j]).astype(dtype)
        term = (w_sct[r, j][:, None] * d).astype(dtype)
        acc[r, i] = (acc[r, i] + term).astype(dtype)
        mag[r, i] += np.abs(term.astype(np.float64))
        k[r, i] += 1
    return acc, k, mag


def _weights(g, shape):
    g = np.zeros(shape, np.float32) if g is None else np.asarray(g, np.float32)
    return g + g                                                    # 2 g: exact


def _both(p, q, idx1, idx2, g1, g2, dtype):
    p, q = np.asarray(p, np.float32), np.asarray(q, np.float32)
    a, c = _weights(g1, p.shape[:2]), _weights(g2, q.shape[:2])
    gp = _direction(p, q, np.asarray(idx1), np.asarray(idx2), a, c, dtype)
    gq = _direction(q, p, np.asarray(idx2), np.asarray(idx1), c, a, dtype)
    return gp, gq


def backward32(p, q, idx1, idx2, g1, g2):
    """(a): (grad_p, grad_q) float32, in the defined order"""
    with np.errstate(all="ignore"):
        gp, gq = _both(p, q, idx1, idx2, g1, g2, np.float32)
    assert gp[0].dtype == np.float32 and gq[0].dtype == np.float32
    return gp[0], gq[0]


def backward64(p, q, idx1, idx2, g1, g2):
    """(b): ((grad_p, k_p, mag_p), (grad_q, k_q, mag_q)) — float64 values, term counts (B,T), sum|term| (B,T,3)"""
    with np.errstate(all="ignore"):
        return _both(p, q, idx1, idx2, g1, g2, np.float64)


def bound32(k, mag):
    """the derived bound of an fp32 result in the defined order against the float64 sum, per element"""
    return (k[:, :, None] + 3) * EPS32 * mag + TINY32


def bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.int32)
