"""numpy restatements of s3r_linear_backward (include/s3r.h) for tests/test_linear_backward_{cpu,gpu}.py.

The layer is y = act(x W^T + bias): x (B,Cin), w (Cout,Cin), y and grad_y (B,Cout).

  g32(y, gy, act)       the pre-activation gradient as the header defines it, in fp32, nothing fused:
                          none g = gy;  relu g = (y > 0) ? gy : 0 (a NaN y gives 0);  sigmoid t = 1 - y, u = y * t, g = gy * u
  grad_bias32(g)        one fp32 accumulator that starts as g[0], plain adds in ascending b: the defined order, bit for bit
  backward64(x, w, g)   grad_w = g^T x and grad_x = g w in float64 from the inputs as given (fp32 values are exact in it), and per element the term count K and
                        sum|term|
  bound32(K, mag)       gamma_{K+1} mag + K 2^-149, gamma_n = n 2^-24 / (1 - n 2^-24): the standard bound for a length-K fp32 dot
                        product summed in ANY order (Higham, Accuracy and Stability of Numerical Algorithms, §3.1: gamma_K for
                        the K products and K - 1 adds; one more factor covers a final add of split-K partial sums and the float64
                        reference's own rounding, which is 2^-29 times smaller), with or without fused multiply-adds (an fma
                        drops a rounding), plus one subnormal ulp per term for products that underflow.  Derived, not measured.
"""
import numpy as np

ACTS = ("none", "relu", "sigmoid")
U32 = 2.0 ** -24
EPS64 = 2.0 ** -53


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def g32(y, gy, act):
    gy = np.asarray(gy, np.float32)
    if act == "none":
        return gy.copy()
    y = np.asarray(y, np.float32)
    if act == "relu":
        return np.where(y > np.float32(0), gy, np.float32(0)).astype(np.float32)
    if act == "sigmoid":
        with np.errstate(all="ignore"):
            t = (np.float32(1) - y).astype(np.float32)
            u = (y * t).astype(np.float32)
            return (gy * u).astype(np.float32)
    raise ValueError(act)


def grad_bias32(g):
    g = np.asarray(g, np.float32)
    s = g[0].copy()
    with np.errstate(all="ignore"):
        for b in range(1, g.shape[0]):
            s = (s + g[b]).astype(np.float32)
    return s


def backward64(x, w, g):
    """((grad_w, K, mag), (grad_x, K, mag)): float64 values, the number of terms of each element's sum, and sum|term|"""
    x64, w64, g64 = (np.asarray(a).astype(np.float64) for a in (x, w, g))
    gw = g64.T @ x64
    gw_mag = np.abs(g64).T @ np.abs(x64)
    gx = g64 @ w64
    gx_mag = np.abs(g64) @ np.abs(w64)
    return (gw, x64.shape[0], gw_mag), (gx, w64.shape[0], gx_mag)


def gamma(n):
    return n * U32 / (1.0 - n * U32)


def bound32(K, mag):
    return gamma(K + 1) * mag + K * 2.0 ** -149


def forward32(x, w, bias, act):
    """a plain fp32 forward for the tests that need SOME y consistent with the layer (its bits are not a contract here)"""
    z = (np.asarray(x, np.float64) @ np.asarray(w, np.float64).T + np.asarray(bias, np.float64)).astype(np.float32)
    if act == "relu":
        return np.maximum(z, np.float32(0))
    if act == "sigmoid":
        return (1.0 / (1.0 + np.exp(-z.astype(np.float64)))).astype(np.float32)
    return z
