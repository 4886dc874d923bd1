"""numpy restatements of s3r_batchnorm_train_forward / s3r_batchnorm_train_backward (include/s3r.h) for
tests/test_batchnorm_train_{cpu,gpu,streams_gpu}.py.

z, y, grad_y, grad_z are (B, C, S); gamma, beta and the statistics (C); N = B S, nf = float32(N).  Everything below the "32" names is fp32
operation by operation, in the header's order:

  total32(terms)            (B, C, S) -> (C): tests/_head64.py's chunk_sums32 per (b, c) row (chunks of 512; lane L owns positions
                            256 j + 4 L + i and adds them in ascending position to a partial that starts as +0.0; halving tree), the chunk
                            sums in ascending chunk order starting AS chunk 0's sum, the rows' partials in ascending b starting AS sample
                            0's.  `mutant=` builds the wrong orders the bit-for-bit comparison must catch
  stats32(z, eps)           mean = total(z) / nf;  d = z - mean;  var = total(d * d) / nf (two passes, d * d rounded before the add);
                            invstd = 1 / sqrt(var + eps) — numpy's float32 division and square root are correctly rounded
  xhat32, y32               xhat = (z - mean) * invstd;  t = xhat * gamma;  u = t + beta;  none: u;  relu: u < 0 ? 0 : u;  sigmoid has no
                            bit-exact restatement (the kernel's exponential is the fast one): y32 returns float64 of the fp32 u there
  backward32                g = tests/_linear64.py's g32;  grad_beta = total(g);  grad_gamma = total(g * xhat), the product rounded;
                            m1 = grad_beta / nf;  m2 = grad_gamma / nf;  a = gamma * invstd;  grad_z = a * ((g - m1) - xhat * m2)
  one_pass_var32            the MUTANT  sum(z^2) / N - mean^2  in sequential fp32 (the cancellation test's foil)

The float64 references and the bounds (u = 2^-24, gamma_n = n u / (1 - n u), bound32 = tests/_linear64.py's any-order sum bound
gamma_{K+1} mag + K 2^-149, used unchanged).  All derived, none measured.

  mean      the sum is within bound32(N, sum|z|) of the real one; the division rounds once and nf once (N > 2^24):
              E_m = bound32(N, sum|z|) / N * (1 + 4u) + 4u |mean64| + 2^-149
  var       with m the fp32 mean and mean64 the real one, sum (z - m)^2 / N = var64 + (m - mean64)^2 EXACTLY (the cross term sums to
            zero), so evaluating at m instead of mean64 costs at most E_m^2.  Every term fl(fl(z - m)^2) carries three roundings and the
            sum is any-order over N terms, the division rounds once, nf once:
              E_v = E_m^2 + gamma_{N+8} (var64 + E_m^2) + (N + 1) 2^-149
  invstd    f(v) = (v + eps)^(-1/2), |f'| = f^3 / 2, largest at the low end var64 - E_v of the interval (premise: var64 + eps > E_v).
            fl(eps), the add, the square root and the division round once each (the first two enter through the square root: halved):
              E_i = E_v (var64 + eps - E_v)^(-3/2) / 2 + 5u invstd64
  y         xhat: |xhat32 - xhat64| <= E_x = |z - mean64| E_i + E_m (invstd64 + E_i) + gamma_3 (|z - mean64| + E_m) (invstd64 + E_i)
            (the subtraction and the product round once each); then the product with gamma and the add of beta:
              E_y = |gamma| E_x + gamma_3 (|gamma| (|xhat64| + E_x) + |beta|)
            ReLU is 1-Lipschitz: the same.  Sigmoid: slope <= 1/4 and tests/_head64.py's evaluation term: E_y / 4 + (2 |u64| + 6) u y64.
  backward  against float64 of the SAME formula on the SAME fp32 inputs (z, y, grad_y, gamma and the device's fp32 mean and invstd, as
            tests/_head64.py's backward64 takes gs and g "as given"): only the roundings of the formula remain.
              g: exact for none / relu; three roundings for sigmoid: E_g = gamma_3 |g64|
              xhat: two roundings: E_h = gamma_2 |xhat64|
              grad_beta:  E_b = sum E_g + bound32(N, sum(|g64| + E_g))
              grad_gamma: E_c = sum(E_g |xhat64| + (|g64| + E_g) E_h) + gamma_{N+2} sum (|g64| + E_g)(|xhat64| + E_h) + N 2^-149
              m1, m2: E_1 = E_b / N (1 + 4u) + 4u |m1|, E_2 likewise
              r = (g - m1) - xhat m2:  E_r = E_g + E_1 + |xhat64| E_2 + E_h (|m2| + E_2) + gamma_3 (|g64| + |m1| + |xhat64 m2|) + 2^-149
              grad_z = a r, a = fl(gamma invstd):  E_z = |a| (E_r + gamma_3 (|r64| + E_r)) + 2^-149
"""
import numpy as np

from tests._head64 import CHUNK, chunk_sums32
from tests._linear64 import ACTS, U32, bits, bound32, g32, gamma      # noqa: F401  (re-exported)

F = np.float32
TINY = 2.0 ** -149


def _fma32(a, b, c):
    """fl(a * b + c) with ONE rounding (the product of two fp32 values is exact in float64; the float64 add is rounded to 53 bits
    first, which can differ from a true fma in a double-rounding tie only: a mutant does not need more)"""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(F)


def chunk_sums_mutant32(a, b, how):
    """chunk sums of a * b (b None: of a) in the header's lane / tree layout with one thing wrong: "fma": partial = fma(a, b, partial);
    "first-term": the lane partial starts AS its first term, not as +0.0 (a row of -0.0 then sums to -0.0)"""
    a = np.asarray(a, F)
    S = a.shape[-1]
    nch = (S + CHUNK - 1) // CHUNK

    def lay(t):
        x = np.zeros(t.shape[:-1] + (nch * CHUNK,), F)
        x[..., :S] = t
        return x.reshape(t.shape[:-1] + (nch, 2, 64, 4))

    xa = lay(a)
    xb = lay(np.asarray(b, F)) if b is not None else None
    with np.errstate(all="ignore"):
        v = np.zeros(a.shape[:-1] + (nch, 64), F)
        first = True
        for j in range(2):
            for i in range(4):
                if how == "fma":
                    v = _fma32(xa[..., j, :, i], xb[..., j, :, i], v)
                else:
                    t = xa[..., j, :, i] if xb is None else (xa[..., j, :, i] * xb[..., j, :, i]).astype(F)
                    v = t.copy() if first else (v + t).astype(F)
                first = False
        for o in (32, 16, 8, 4, 2, 1):
            v = (v[..., :o] + v[..., o:2 * o]).astype(F)
    return v[..., 0]


def finish32(cs, mutant=None):
    """(B, C, nch) chunk sums -> (C).  mutants: "descending-chunks", "descending-batch" """
    cs = np.asarray(cs, F)
    if mutant == "descending-chunks":
        cs = cs[..., ::-1]
    with np.errstate(all="ignore"):
        p = cs[..., 0].copy()
        for k in range(1, cs.shape[-1]):
            p = (p + cs[..., k]).astype(F)
        if mutant == "descending-batch":
            p = p[::-1]
        s = p[0].copy()
        for b in range(1, p.shape[0]):
            s = (s + p[b]).astype(F)
    return s


def total32(terms, mutant=None):
    return finish32(chunk_sums32(terms), mutant)


def nf32(B, S):
    return F(B * S)


def stats32(z, eps, mutant=None):
    """(mean, var, invstd) fp32 (C).  mutant "fma": d * d fused into the add; the finish mutants of finish32"""
    z = np.asarray(z, F)
    B, _, S = z.shape
    nf = nf32(B, S)
    with np.errstate(all="ignore"):
        mean = (total32(z, mutant if mutant != "fma" else None) / nf).astype(F)
        d = (z - mean[None, :, None]).astype(F)
        if mutant == "fma":
            tot = finish32(chunk_sums_mutant32(d, d, "fma"))
        else:
            tot = total32((d * d).astype(F), mutant)
        var = (tot / nf).astype(F)
        invstd = invstd32(var, eps)
    return mean, var, invstd


def invstd32(var, eps):
    with np.errstate(all="ignore"):
        e = (np.asarray(var, F) + F(eps)).astype(F)
        return (F(1) / np.sqrt(e).astype(F)).astype(F)


def xhat32(z, mean, invstd):
    with np.errstate(all="ignore"):
        d = (np.asarray(z, F) - np.asarray(mean, F)[None, :, None]).astype(F)
        return (d * np.asarray(invstd, F)[None, :, None]).astype(F)


def u32(z, mean, invstd, gam, beta):
    with np.errstate(all="ignore"):
        t = (xhat32(z, mean, invstd) * np.asarray(gam, F)[None, :, None]).astype(F)
        return (t + np.asarray(beta, F)[None, :, None]).astype(F)


def y32(z, mean, invstd, gam, beta, act):
    """fp32 bits for none / relu; for sigmoid the float64 sigmoid of the fp32 pre-activation (compare with sigmoid_bound)"""
    u = u32(z, mean, invstd, gam, beta)
    if act == "none":
        return u
    if act == "relu":
        return np.where(u < F(0), F(0), u).astype(F)
    with np.errstate(all="ignore"):
        return 1.0 / (1.0 + np.exp(-u.astype(np.float64)))


def sigmoid_bound(u, y64):
    """the kernel's 1 / (1 + exp(-u)) against the real sigmoid of the SAME fp32 u: tests/_head64.py's evaluation term"""
    return (2 * np.abs(np.asarray(u, np.float64)) + 6) * U32 * np.abs(y64) + TINY


def backward32(z, y, gy, gam, mean, invstd, act, mutant=None):
    """(grad_z, grad_gamma, grad_beta) fp32.  mutant "fma": g * xhat fused into the add; the finish mutants of finish32"""
    z = np.asarray(z, F)
    B, _, S = z.shape
    nf = nf32(B, S)
    g = g32(y, gy, act)
    xh = xhat32(z, mean, invstd)
    with np.errstate(all="ignore"):
        gb = total32(g, mutant if mutant != "fma" else None)
        if mutant == "fma":
            gg = finish32(chunk_sums_mutant32(g, xh, "fma"))
        else:
            gg = total32((g * xh).astype(F), mutant)
        m1 = (gb / nf).astype(F)[None, :, None]
        m2 = (gg / nf).astype(F)[None, :, None]
        a = (np.asarray(gam, F) * np.asarray(invstd, F)).astype(F)[None, :, None]
        p = (xh * m2).astype(F)
        q = (g - m1).astype(F)
        r = (q - p).astype(F)
        gz = (a * r).astype(F)
    return gz, gg, gb


def one_pass_var32(z):
    """the mutant sum(z^2) / N - mean^2 per channel with plain sequential fp32 sums (b, then s ascending)"""
    z = np.asarray(z, F)
    B, ch, S = z.shape
    rows = z.transpose(1, 0, 2).reshape(ch, B * S)
    s1, s2 = np.zeros(ch, F), np.zeros(ch, F)
    for k in range(B * S):
        s1 = (s1 + rows[:, k]).astype(F)
        s2 = (s2 + (rows[:, k] * rows[:, k]).astype(F)).astype(F)
    nf = nf32(B, S)
    mean = (s1 / nf).astype(F)
    return ((s2 / nf).astype(F) - (mean * mean).astype(F)).astype(F)


# ---------------------------------------------------------------- float64 references and the derived bounds
def forward64(z, gam, beta, eps, act):
    """dict of float64 references (mean, var, invstd, xhat, u, y) and bounds (E_m, E_v, E_i, E_y) from the fp32 inputs as given"""
    z64 = np.asarray(z, F).astype(np.float64)
    B, _, S = z64.shape
    N = B * S
    g64, b64 = np.asarray(gam, F).astype(np.float64), np.asarray(beta, F).astype(np.float64)
    e = float(F(eps))
    mean = z64.mean(axis=(0, 2))
    d = z64 - mean[None, :, None]
    var = (d * d).mean(axis=(0, 2))
    inv = 1.0 / np.sqrt(var + e)
    xh = d * inv[None, :, None]
    u = xh * g64[None, :, None] + b64[None, :, None]
    with np.errstate(all="ignore"):
        y = {"none": u, "relu": np.maximum(u, 0.0), "sigmoid": 1.0 / (1.0 + np.exp(-u))}[act]
    E_m = bound32(N, np.abs(z64).sum(axis=(0, 2))) / N * (1 + 4 * U32) + 4 * U32 * np.abs(mean) + TINY
    E_v = E_m ** 2 + gamma(N + 8) * (var + E_m ** 2) + (N + 1) * TINY
    low = var + e - E_v
    assert (low > 0).all(), "premise of the invstd bound: var64 + eps > E_v"
    E_i = 0.5 * E_v * low ** -1.5 + 5 * U32 * inv
    ad = np.abs(d)
    E_x = ad * E_i[None, :, None] + (E_m * (inv + E_i))[None, :, None] + gamma(3) * (ad + E_m[None, :, None]) * (inv + E_i)[None, :, None]
    ag = np.abs(g64)[None, :, None]
    E_y = ag * E_x + gamma(3) * (ag * (np.abs(xh) + E_x) + np.abs(b64)[None, :, None]) + TINY
    if act == "sigmoid":
        E_y = E_y / 4 + sigmoid_bound(u, y)
    return dict(mean=mean, var=var, invstd=inv, xhat=xh, u=u, y=y, E_m=E_m, E_v=E_v, E_i=E_i, E_y=E_y)


def backward64(z, y, gy, gam, mean, invstd, act):
    """dict of float64 values (grad_z, grad_gamma, grad_beta) of the header's formula on the fp32 inputs AS GIVEN (mean and invstd are the
    fp32 statistics the backward is handed) and the bounds E_z, E_c (grad_gamma), E_b (grad_beta)"""
    z64, gy64 = np.asarray(z, F).astype(np.float64), np.asarray(gy, F).astype(np.float64)
    B, _, S = z64.shape
    N = B * S
    m64, i64, ga64 = (np.asarray(v, F).astype(np.float64)[None, :, None] for v in (mean, invstd, gam))
    if act == "none":
        g = gy64
    else:
        y64 = np.asarray(y, F).astype(np.float64)
        g = np.where(y64 > 0, gy64, 0.0) if act == "relu" else gy64 * (y64 * (1.0 - y64))
    xh = (z64 - m64) * i64
    gb = g.sum(axis=(0, 2))
    gg = (g * xh).sum(axis=(0, 2))
    m1, m2 = (gb / N)[None, :, None], (gg / N)[None, :, None]
    r = g - m1 - xh * m2
    a = ga64 * i64
    gz = a * r
    ag, ax = np.abs(g), np.abs(xh)
    E_g = gamma(3) * ag if act == "sigmoid" else np.zeros_like(ag)
    E_h = gamma(2) * ax
    E_b = E_g.sum(axis=(0, 2)) + bound32(N, (ag + E_g).sum(axis=(0, 2)))
    E_c = (E_g * ax + (ag + E_g) * E_h).sum(axis=(0, 2)) + gamma(N + 2) * ((ag + E_g) * (ax + E_h)).sum(axis=(0, 2)) + N * TINY
    E_1 = (E_b / N * (1 + 4 * U32))[None, :, None] + 4 * U32 * np.abs(m1)
    E_2 = (E_c / N * (1 + 4 * U32))[None, :, None] + 4 * U32 * np.abs(m2)
    E_r = E_g + E_1 + ax * E_2 + E_h * (np.abs(m2) + E_2) + gamma(3) * (ag + np.abs(m1) + np.abs(xh * m2)) + TINY
    E_z = np.abs(a) * (E_r + gamma(3) * (np.abs(r) + E_r)) + TINY
    return dict(grad_z=gz, grad_gamma=gg, grad_beta=gb, E_z=E_z, E_c=E_c, E_b=E_b)


# (B, C, S) of the device tests: S in {1, 5, 511, 512, 513, 1029} (a short single chunk, a row that is no multiple of 4, an exact chunk,
# a one-element second chunk, two chunks and a short third), B in {1, 2, 3, 65} (65 crosses the finish kernel's 64-sample step), C in
# {1, 3, 5}, and N = 2, the minimum
SHAPES = [(2, 1, 1), (1, 3, 5), (2, 5, 5), (65, 3, 5), (3, 1, 511), (1, 5, 512), (2, 3, 512), (3, 5, 513), (2, 3, 1029), (1, 1, 1029)]
CANCEL = [(65, 1, 5), (3, 1, 513), (2, 1, 1029)]      # N = 65 * 5, 3 * 513, 2 * 1029: z = 100 + 0.1 randn


def cancel_data(shape, seed):
    rng = np.random.default_rng(seed)
    return (F(100) + F(0.1) * rng.standard_normal(shape).astype(F)).astype(F)
