"""numpy restatements of s3r_voxel_bce_forward / s3r_voxel_bce_backward (include/s3r.h) for tests/test_voxel_loss_{cpu,gpu}.py.

pred and target are (B, V) fp32.

  loss_elem32(p, t)      the per-element rule in fp32 with numpy's own float32 log.  The clamp and the order of operations are the
                         header's; the log is NOT the device's (neither is correctly rounded), so this is bit-exact only where both
                         logs are exact or clamped: the planted corners.  `mutant=` builds the wrong rules the cases must catch.
  loss_elem64(p, t)      the same rule in float64 from the fp32 inputs: log(p) and log1p(-p), i.e. the real l of the real 1 - p
  elem_bound(p, t)       per-element bound on |device l - loss_elem64|, derived below
  sum_order32(l)         the header's summation order of one sample, bit for bit: chunks of 1024, lane partials over the 16 elements
                         256 j + 4 L + i in ascending order from +0.0, halving tree, chunk sums in ascending order
  sum_bound(l)           gamma_{V-1} sum|l|: any order of V - 1 fp32 additions (Higham, Accuracy and Stability, §4.2)
  grad32(p, t, scale)    grad_pred in fp32, every operation rounded once: elementwise, so bit for bit
  grad64(p, t, scale)    the same in float64

The bound on loss_elem.  u = 2^-24.  L = 3: the ROCm install this was written against ships no HIP math accuracy table, so L is
the OpenCL full-profile limit of log, 3 ulp, which OCML's logf is specified to (not a figure from such a table).  An ulp of a normal
fp32 v is at most 2 u |v|.
  a:  |logf(p) - log p| <= 2 L u |log p|; the clamp is monotone and 1-Lipschitz, so E_a = 2 L u |log p| (0 where p = 0: logf(0) is -inf
      exactly, clamped to -100 on both sides).
  c:  q = fl(1 - p) = (1 - p)(1 + d), |d| <= u, so log q = log(1 - p) + log(1 + d) with |log(1 + d)| <= u / (1 - u): an ABSOLUTE error,
      which is what dominates for small p; then logf(q) within 2 L u |log q|:  E_c = u/(1-u) + 2 L u (|log(1 - p)| + u/(1-u)).
  l = -(t a + fl(1 - t) c): term 1 carries two roundings (product, add), term 2 three (1 - t, product, add); the negation is exact:
      |l - l64| <= t E_a + (1 - t) E_c + gamma_2 t (|a| + E_a) + gamma_3 (1 - t)(|c| + E_c) + 3 * 2^-149
with gamma_n = n u / (1 - n u), and one subnormal ulp per rounding that can underflow.  The float64 reference's own error is 2^-29
times smaller than any of these terms.  Derived, not measured.
"""
import numpy as np

CHUNK = 1024
L_ULP = 3
U32 = 2.0 ** -24
F = np.float32


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def gamma(n):
    return n * U32 / (1.0 - n * U32)


def clamp(v):
    """(v < -100) ? -100 : v — a NaN compares false and passes"""
    return np.where(v < -100, np.asarray(-100, v.dtype), v)


def loss_elem32(p, t, mutant=None):
    p, t = np.asarray(p, F), np.asarray(t, F)
    with np.errstate(all="ignore"):
        la, lc = np.log(p).astype(F), np.log((F(1) - p).astype(F)).astype(F)
        if mutant == "clamp-after-multiply":
            return (-(clamp((t * la).astype(F)) + clamp(((F(1) - t).astype(F) * lc).astype(F))).astype(F)).astype(F)
        if mutant == "fmax-clamp":                                         # fmaxf(v, -100) returns -100 for a NaN v
            a, c = np.fmax(la, F(-100)), np.fmax(lc, F(-100))
        else:
            a, c = clamp(la), clamp(lc)
        return (-((t * a).astype(F) + ((F(1) - t).astype(F) * c).astype(F)).astype(F)).astype(F)


def _logs64(p):
    p = np.asarray(p, F).astype(np.float64)
    with np.errstate(all="ignore"):
        return np.log(p), np.log1p(-p)


def loss_elem64(p, t):
    t = np.asarray(t, F).astype(np.float64)
    la, lc = _logs64(p)
    with np.errstate(all="ignore"):
        return -(t * clamp(la) + (1.0 - t) * clamp(lc))


def elem_bound(p, t):
    t = np.asarray(t, F).astype(np.float64)
    la, lc = _logs64(p)
    ua = U32 / (1.0 - U32)
    with np.errstate(all="ignore"):
        ea = np.where(np.isfinite(la), 2 * L_ULP * U32 * np.abs(la), 0.0)
        ec = np.where(np.isfinite(lc), ua + 2 * L_ULP * U32 * (np.abs(lc) + ua), 0.0)
        a, c = np.abs(clamp(la)), np.abs(clamp(lc))
        return t * ea + (1 - t) * ec + gamma(2) * t * (a + ea) + gamma(3) * (1 - t) * (c + ec) + 3 * 2.0 ** -149


def sum_order32(l):
    """one sample's loss_sum from its V losses, in the header's order"""
    l = np.asarray(l, F).reshape(-1)
    nch = (l.size + CHUNK - 1) // CHUNK
    x = np.zeros(nch * CHUNK, F)
    x[:l.size] = l
    x = x.reshape(nch, 4, 64, 4)                                           # [chunk][j][lane][i]: element 256 j + 4 lane + i
    with np.errstate(all="ignore"):
        v = np.zeros((nch, 64), F)
        for j in range(4):
            for i in range(4):
                v = (v + x[:, j, :, i]).astype(F)
        for o in (32, 16, 8, 4, 2, 1):
            v = (v[:, :o] + v[:, o:2 * o]).astype(F)
        s = v[0, 0]
        for k in range(1, nch):
            s = F(s + v[k, 0])
    return F(s)


def boundaries():
    """sample sizes at which the order takes another path: a short quad, a full 256-element row of lanes, a chunk, a round of 16 chunks"""
    out = set()
    for n in (4, 256, CHUNK, 16 * CHUNK):
        out |= {n - 1, n, n + 1}
    return sorted(out)


def sum_bound(l):
    l = np.asarray(l, np.float64).reshape(-1)
    return gamma(max(l.size - 1, 0)) * np.abs(l).sum()


def grad32(p, t, scale):
    p, t, scale = np.asarray(p, F), np.asarray(t, F), np.asarray(scale, F).reshape(-1, 1)
    with np.errstate(all="ignore"):
        n = (scale * (p - t).astype(F)).astype(F)
        d = np.maximum(((F(1) - p).astype(F) * p).astype(F), F(1e-12))
        return (n / d).astype(F)


def grad64(p, t, scale, eps=float(F(1e-12))):
    """eps: the fp32 number nearest 1e-12, in the kernel and in torch's kernels alike (torch's float64 one too: its constant is a float)"""
    p, t = np.asarray(p, F).astype(np.float64), np.asarray(t, F).astype(np.float64)
    return np.asarray(scale, np.float64).reshape(-1, 1) * (p - t) / np.maximum((1.0 - p) * p, eps)


# (B, V) of the device tests: the issue's list, then the boundaries of the order above (tests/test_voxel_loss_cpu.py checks that
# every boundary is here)
SHAPES = [(1, 1), (1, 3), (2, 4), (1, 255), (1, 256), (1, 257), (3, 1023), (2, 1024), (2, 1025), (2, 4099), (2, 32768),
          (1, 2 ** 20 + 5), (2, 5), (1, 16383), (1, 16384), (2, 16385)]

# the planted grid: every p against every t
PLANTED_P = [0.0, 2.0 ** -149, 1e-12, 0.5, 1.0 - 2.0 ** -24, 1.0]
PLANTED_T = [0.0, 0.5, 1.0]


def planted():
    p = np.repeat(np.array(PLANTED_P, F), len(PLANTED_T))
    t = np.tile(np.array(PLANTED_T, F), len(PLANTED_P))
    return p, t
