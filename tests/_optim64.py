"""numpy restatements of s3r_optim_step / s3r_optim_state_init (include/s3r.h) for tests/test_optimizer_{cpu,gpu,streams_gpu,training_gpu}.py.

  Desc                      the descriptor: kind "sgd" / "adam", the four flags, the baked hyper-parameters
  fresh_state(lr)           s3r_optim_state_init's eight dwords as a dict; state_words(st) packs them as int32 bits
  norm32(grads)             the ordered gradient norm: tests/_head64.chunk_sums32 per tensor (a tensor in place of a row) on the ROUNDED
                            g * g, the chunk sums of a tensor in ascending order from chunk 0's, the tensor totals in ascending tensor
                            order from tensor 0's, one sqrt.  It knows nothing of launches.
  coef32(norm, max_norm)    d = norm + 1e-6f; c = max_norm / d; (c > 1) ? 1 : c  — a NaN stays a NaN
  step32(desc, ts, st)      one step, fp32, ONE ROUNDED OPERATION PER LINE, the header's order word for word; `mutant=` builds the wrong
                            rules the bit-for-bit comparison must catch (MUTANTS)
  step64(desc, ts, st)      the same rule in float64 (powers as beta ** step, the norm as a plain float64 sum)
  bound_step(...)           a per-element bound of |step32 - step64|, propagated through the rule operation by operation

The bound (derived, not measured).  u = 2^-24 (U; the float64 side's own error enters with u = 2^-53 through the same function).  Every
fp32 operation returns its exact result times (1 + d), |d| <= u, or — a product that underflows — is off by at most TINY = 2^-149.  Every
quantity x of the rule therefore carries an absolute error E[x], and the rule's statements propagate it:
    z = x * y   (y a constant of the step, exact in both forms):   E[z] = |y| E[x] + u |z| + TINY
    z = x + y, z = x - y:                                          E[z] = E[x] + E[y] + u |z|
    z = x * x:                                                     E[z] = 2 |x| E[x] + E[x]^2 + u |z| + TINY
    z = x / c   (c = 1 - beta_pow, itself uncertain by E[c]):      E[z] = (E[x] + |z| E[c]) / (|c| - E[c]) + u |z| + TINY
    z = sqrt(x):                                                   E[z] = min(sqrt(E[x]), E[x] / sqrt(x)) + u |z|
        (|sqrt a - sqrt b| = |a - b| / (sqrt a + sqrt b) <= |a - b| / sqrt(max(a, b)), and <= sqrt|a - b|)
    z = x / y:                                                     E[z] = (E[x] + |z| E[y]) / (|y| - E[y]) + u |z| + TINY
The inputs of a step carry E[p], E[m], E[v] from the step before (zero at the first): that is how the bound compounds over steps.  The
running powers: beta_pow after k steps is k rounded multiplications, |beta_pow32 - beta ** k| <= gamma(k) beta_pow, gamma(k) = k u / (1 - k u),
and 1 - beta_pow rounds once more: E[c] = gamma(k) beta_pow + u c.  The clip coefficient: the norm is a sum of N non-negative rounded
products in SOME order, relative error gamma(N + 1) whatever the order, halved by the sqrt and rounded (u), then one add (u), one division
(u): the coefficient's relative error is at most gamma(N + 1) / 2 + 3 u + (the 1e-6f against 1e-6: below u of d); gamma(N + 5) is taken.
The clamp to 1 only shrinks it.  |x| is taken from the float64 form; the fp32 value differs from it by E[x] itself, a second-order term,
which the final factor (1 + 2^-10) absorbs.
"""
from dataclasses import dataclass, replace
from typing import Optional

import numpy as np

from tests import _head64 as H

F = np.float32
U = 2.0 ** -24
U64 = 2.0 ** -53
TINY = 2.0 ** -149
SIZES = (1, 3, 4, 511, 512, 513, 2047, 2048, 2049, 4099)      # the chunk, workgroup and ragged-tail boundaries
STEPS = 5
LR = 1e-3


@dataclass(frozen=True)
class Desc:
    kind: str = "adam"
    beta1: float = 0.9           # SGD: momentum
    beta2: float = 0.999
    eps: float = 1e-8
    wd: float = 0.0
    decoupled: bool = False
    nesterov: bool = False
    clip: Optional[float] = None  # max_norm
    skip: bool = False

    @property
    def with_norm(self):
        return self.clip is not None or self.skip

    @property
    def flags(self):
        return (1 if self.decoupled else 0) | (2 if self.nesterov else 0) | (4 if self.clip is not None else 0) | (8 if self.skip else 0)

    @property
    def has_m(self):
        return self.kind == "adam" or self.beta1 != 0

    @property
    def has_v(self):
        return self.kind == "adam"


RULES = {
    "sgd": Desc("sgd", beta1=0.0),
    "sgd_momentum": Desc("sgd", beta1=0.9),
    "sgd_nesterov_wd": Desc("sgd", beta1=0.9, nesterov=True, wd=0.01),
    "adam": Desc("adam"),
    "adam_l2": Desc("adam", wd=0.01),
    "adamw": Desc("adam", wd=0.01, decoupled=True),
}
# max_norm 1: every list below has norm > 1 (the coefficient scales); 2^100: norm < max_norm (the coefficient clamps to exactly 1)
NORMS = {"plain": {}, "clip": dict(clip=1.0), "clip_loose": dict(clip=2.0 ** 100), "skip": dict(skip=True), "clip_skip": dict(clip=1.0, skip=True)}
CASES = {f"{r}-{n}": replace(d, **kw) for r, d in RULES.items() for n, kw in NORMS.items()}


def bits(a):
    return np.ascontiguousarray(np.asarray(a, F)).view(np.int32)


# ---------------------------------------------------------------- data
def values(n, rng):
    """normal deviates times powers of two from 2^-70 to 2^20: g * g lands on denormals, normals and large values"""
    return (rng.standard_normal(n) * np.exp2(rng.integers(-70, 21, n))).astype(F)


def tensor_list(sizes=SIZES, seed=0, nan_m=False):
    """[{p, m, v}] of fresh parameters and zero moments; nan_m: the momentum buffer starts as NaN (SGD's first step sets m = g and
    never reads it: a rule that computes mu * m + g there shows)"""
    rng = np.random.default_rng(1000 + seed)
    return [dict(p=values(n, rng), m=np.full(n, np.nan if nan_m else 0.0, F), v=np.zeros(n, F)) for n in sizes]


def grads(sizes=SIZES, seed=0, step=0):
    rng = np.random.default_rng(77 * seed + 5 + step)
    return [values(n, rng) for n in sizes]


def boundary_sizes(n_tensors):
    """n_tensors tensors of 1 to 40 elements (lists of TPL - 1, TPL, TPL + 1 and 2 TPL + 1 tensors: the launch boundaries)"""
    return tuple(int(x) for x in np.random.default_rng(n_tensors).integers(1, 41, n_tensors))


def scratch_elems(sizes):
    return sum((n + H.CHUNK - 1) // H.CHUNK for n in sizes) + len(sizes)


# ---------------------------------------------------------------- state
def fresh_state(lr):
    return dict(step=0, b1p=F(1), b2p=F(1), lr=F(lr), norm=F(0), coef=F(1), skipped=0, reserved=0)


def state_words(st):
    w = np.zeros(8, np.int32)
    w[0], w[6], w[7] = st["step"], st["skipped"], st["reserved"]
    w[1:6] = bits(np.array([st["b1p"], st["b2p"], st["lr"], st["norm"], st["coef"]], F))
    return w


# ---------------------------------------------------------------- the norm
def norm32(gs, chunk_order="ascending"):
    with np.errstate(all="ignore"):
        total = None
        for g in gs:
            g = np.asarray(g, F).reshape(-1)
            cs = H.chunk_sums32((g * g).astype(F))
            if chunk_order == "descending":
                cs = cs[::-1]
            p = cs[0]
            for k in range(1, cs.shape[0]):
                p = F(p + cs[k])
            total = p if total is None else F(total + p)
        return F(np.sqrt(total))


def coef32(norm, max_norm, clamp=True):
    with np.errstate(all="ignore"):
        d = F(norm + F(1e-6))
        c = F(F(max_norm) / d)
        return F(1) if (clamp and c > F(1)) else c


# ---------------------------------------------------------------- one step, fp32
MUTANTS = ("no_bias_correction", "decay_swapped", "eps_in_sqrt", "no_nesterov", "first_step_mu_times_nan", "descending_chunks",
           "unclamped", "count_on_skip")


def step32(d, ts, gs, st, mutant=None):
    """ts: [{p, m, v}], gs: the gradients; returns (new ts, new st); the inputs are not changed"""
    assert mutant is None or mutant in MUTANTS
    st = dict(st)
    ts = [{k: a.copy() for k, a in t.items()} for t in ts]
    b1, b2, eps, wd = F(d.beta1), F(d.beta2), F(d.eps), F(d.wd)
    decoupled = d.decoupled != (mutant == "decay_swapped")
    with np.errstate(all="ignore"):
        if d.with_norm:
            st["norm"] = norm32(gs, "descending" if mutant == "descending_chunks" else "ascending")
            st["coef"] = coef32(st["norm"], d.clip, clamp=mutant != "unclamped") if d.clip is not None else F(1)
            if d.skip and not np.isfinite(st["norm"]):
                st["skipped"] += 1
                if mutant == "count_on_skip":
                    st["step"] += 1
                return ts, st
        st["step"] += 1
        if d.kind == "adam":
            st["b1p"] = F(st["b1p"] * b1)
            st["b2p"] = F(st["b2p"] * b2)
        lr, coef = st["lr"], st["coef"]
        first = st["step"] == 1
        bc1 = F(F(1) - st["b1p"])
        bc2 = F(F(1) - st["b2p"])
        if mutant == "no_bias_correction":
            bc1 = bc2 = F(1)
        omb1 = F(F(1) - b1)
        omb2 = F(F(1) - b2)
        lrwd = F(lr * wd)
        for t, g in zip(ts, gs):
            p, m, v = t["p"], t["m"], t["v"]
            g = np.asarray(g, F).copy()
            if d.clip is not None:
                g = (g * coef).astype(F)
            if d.kind == "sgd":
                if wd != 0:
                    x = (wd * p).astype(F)
                    g = (g + x).astype(F)
                if b1 != 0:
                    if first and mutant != "first_step_mu_times_nan":
                        m = g.copy()
                    else:
                        a = (b1 * m).astype(F)
                        m = (a + g).astype(F)
                    if d.nesterov and mutant != "no_nesterov":
                        x = (b1 * m).astype(F)
                        g = (g + x).astype(F)
                    else:
                        g = m
                x = (lr * g).astype(F)
                p = (p - x).astype(F)
            else:
                if wd != 0:
                    if decoupled:
                        s = (lrwd * p).astype(F)
                        p = (p - s).astype(F)
                    else:
                        x = (wd * p).astype(F)
                        g = (g + x).astype(F)
                a = (b1 * m).astype(F)
                b = (omb1 * g).astype(F)
                m = (a + b).astype(F)
                a = (b2 * v).astype(F)
                q = (g * g).astype(F)
                b = (omb2 * q).astype(F)
                v = (a + b).astype(F)
                mh = (m / bc1).astype(F)
                vh = (v / bc2).astype(F)
                if mutant == "eps_in_sqrt":
                    dn = np.sqrt((vh + eps).astype(F)).astype(F)
                else:
                    r = np.sqrt(vh).astype(F)
                    dn = (r + eps).astype(F)
                x = (mh / dn).astype(F)
                x = (lr * x).astype(F)
                p = (p - x).astype(F)
            t["p"] = p
            if d.has_m:
                t["m"] = m
            if d.has_v:
                t["v"] = v
    return ts, st


# ---------------------------------------------------------------- one step, float64, and the bound
def gamma(k, u=U):
    return k * u / (1 - k * u)


def step64(d, ts, gs, st, E=None, u=U):
    """The rule in float64 from the state as given (ts float64 or fp32 arrays; st: step, lr, skipped as the fp32 state's).  Returns
    (new ts (float64), new st, new E): E = [{p, m, v}] absolute error bounds of an evaluation with unit round-off u against this one,
    from the incoming bounds E (None: zeros).  A skipped step returns its inputs."""
    st = dict(st)
    ts = [{k: np.asarray(a, np.float64).copy() for k, a in t.items()} for t in ts]
    E = [{k: np.zeros(t["p"].shape) for k in "pmv"} for t in ts] if E is None else [{k: a.copy() for k, a in e.items()} for e in E]
    b1, b2, eps, wd = (float(F(x)) for x in (d.beta1, d.beta2, d.eps, d.wd))
    lr = float(st["lr"])
    gs = [np.asarray(g, np.float64) for g in gs]
    coef, rel_c = 1.0, 0.0
    with np.errstate(all="ignore"):
        if d.with_norm:
            norm = np.sqrt(sum(float((g * g).sum()) for g in gs))
            st["norm"] = norm
            if d.skip and not np.isfinite(norm):
                st["skipped"] += 1
                return ts, st, E
            if d.clip is not None:
                coef = min(float(F(d.clip)) / (norm + 1e-6), 1.0)
                rel_c = gamma(sum(g.size for g in gs) + 5, u)
            st["coef"] = coef
        st["step"] += 1
        k = st["step"]
        c1, c2 = 1 - b1 ** k, 1 - b2 ** k
        Ec1, Ec2 = gamma(k, u) * b1 ** k + u * c1, gamma(k, u) * b2 ** k + u * c2
        for t, e, g in zip(ts, E, gs):
            p, m, v = t["p"], t["m"], t["v"]
            Ep, Em, Ev = e["p"], e["m"], e["v"]
            Eg = np.zeros(g.shape)
            if d.clip is not None:
                g = g * coef
                Eg = np.abs(g) * (rel_c + u) + TINY
            if d.kind == "sgd":
                if wd != 0:
                    x = wd * p
                    Ex = wd * Ep + u * np.abs(x) + TINY
                    g = g + x
                    Eg = Eg + Ex + u * np.abs(g)
                if b1 != 0:
                    if k == 1:
                        m, Em = g.copy(), Eg.copy()
                    else:
                        a = b1 * m
                        Ea = b1 * Em + u * np.abs(a) + TINY
                        m = a + g
                        Em = Ea + Eg + u * np.abs(m)
                    if d.nesterov:
                        x = b1 * m
                        Ex = b1 * Em + u * np.abs(x) + TINY
                        g = g + x
                        Eg = Eg + Ex + u * np.abs(g)
                    else:
                        g, Eg = m, Em
                x = lr * g
                Ex = lr * Eg + u * np.abs(x) + TINY
                p = p - x
                Ep = Ep + Ex + u * np.abs(p)
            else:
                if wd != 0:
                    if d.decoupled:
                        w = lr * wd
                        s = w * p
                        Es = w * Ep + 2 * u * np.abs(s) + TINY          # (w itself is one rounded product: u more)
                        p = p - s
                        Ep = Ep + Es + u * np.abs(p)
                    else:
                        x = wd * p
                        Ex = wd * Ep + u * np.abs(x) + TINY
                        g = g + x
                        Eg = Eg + Ex + u * np.abs(g)
                a = b1 * m
                Ea = b1 * Em + u * np.abs(a) + TINY
                b = (1 - b1) * g
                Eb = (1 - b1) * Eg + 2 * u * np.abs(b) + TINY           # (1 - beta1 rounds once: u more)
                m = a + b
                Em = Ea + Eb + u * np.abs(m)
                a = b2 * v
                Ea = b2 * Ev + u * np.abs(a) + TINY
                q = g * g
                Eq = 2 * np.abs(g) * Eg + Eg * Eg + u * q + TINY
                b = (1 - b2) * q
                Eb = (1 - b2) * Eq + 2 * u * b + TINY
                v = a + b
                Ev = Ea + Eb + u * np.abs(v)
                mh = m / c1
                Emh = (Em + np.abs(mh) * Ec1) / (c1 - Ec1) + u * np.abs(mh) + TINY
                vh = v / c2
                Evh = (Ev + np.abs(vh) * Ec2) / (c2 - Ec2) + u * np.abs(vh) + TINY
                r = np.sqrt(vh)
                Er = np.minimum(np.sqrt(Evh), np.where(vh > 0, Evh / np.where(vh > 0, r, 1.0), np.inf)) + u * r
                dn = r + eps
                Edn = Er + u * dn
                x = mh / dn
                Ex = np.where(dn > Edn, (Emh + np.abs(x) * Edn) / np.where(dn > Edn, dn - Edn, 1.0), np.inf) + u * np.abs(x) + TINY
                x2 = lr * x
                Ex2 = lr * Ex + u * np.abs(x2) + TINY
                p = p - x2
                Ep = Ep + Ex2 + u * np.abs(p)
            t["p"], e["p"] = p, Ep
            if d.has_m:
                t["m"], e["m"] = m, Em
            if d.has_v:
                t["v"], e["v"] = v, Ev
    return ts, st, E


def bound_step(d, ts, gs, st, E=None, u=U):
    """[{p, m, v}] bounds of |step32 - step64| from the same state (E: the bounds the inputs carry), with the second-order factor"""
    _, _, E = step64(d, ts, gs, st, E, u)
    return [{k: a * (1 + 2.0 ** -10) for k, a in e.items()} for e in E]


# ---------------------------------------------------------------- the check the GPU tests use
def assert_same(got_ts, got_words, want_ts, want_st, d, what=""):
    """bit for bit: every parameter and moment the rule owns, and all eight state dwords.  Where both sides hold a NaN the element
    counts as equal: the header promises that a NaN propagates, not which sign and payload it carries (x86 and the device differ)"""
    for i, (a, b) in enumerate(zip(got_ts, want_ts)):
        for k in ("p",) + (("m",) if d.has_m else ()) + (("v",) if d.has_v else ()):
            bad = np.flatnonzero((bits(a[k]) != bits(b[k])) & ~(np.isnan(a[k]) & np.isnan(b[k])))      # (a NaN is a NaN: no payload is promised)
            assert not bad.size, f"{what} tensor {i} {k}: first of {bad.size} differing elements at {bad[0]}: got {a[k][bad[0]]!r}, want {b[k][bad[0]]!r}"
    want = state_words(want_st)
    got = np.asarray(got_words, np.int32)
    assert (got == want).all(), f"{what} state dwords: got {got.tolist()}, want {want.tolist()}"


def run32(d, sizes=SIZES, seed=0, steps=STEPS, lr=LR, mutant=None, nan_at=None):
    """`steps` steps of step32 on the shared data; nan_at = (step, tensor, element): a NaN planted in that step's gradient.
    Returns the list of (ts, st) after each step."""
    ts, st, out = tensor_list(sizes, seed, nan_m=d.kind == "sgd"), fresh_state(lr), []
    for k in range(steps):
        gs = grads(sizes, seed, k)
        if nan_at is not None and nan_at[0] == k:
            gs[nan_at[1]][nan_at[2]] = np.nan
        ts, st = step32(d, ts, gs, st, mutant)
        out.append((ts, st))
    return out
