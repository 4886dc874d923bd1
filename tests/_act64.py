"""float64 references of the elementwise math behind the layers (act_kernel's LeakyReLU / ELU / Tanh, the head's sigmoid) and the
error measure the per-element tests use: ulps of the float64 value rounded to fp32.  numpy only."""
from __future__ import annotations

import numpy as np

FLT_MIN = float(np.finfo(np.float32).tiny)
FLT_MAX = float(np.finfo(np.float32).max)


def ref64(act: str, v: np.ndarray, param: float = 0.0) -> np.ndarray:
    """act(v) in float64 from fp32 inputs; param is the fp32 slope / alpha the kernel receives"""
    v = np.asarray(v, np.float32).astype(np.float64)
    p = float(np.float32(param))
    with np.errstate(over="ignore", under="ignore"):
        if act == "leaky_relu":
            return np.where(v > 0, v, v * p)
        if act == "elu":
            return np.where(v > 0, v, p * np.expm1(np.minimum(v, 0.0)))
        if act == "tanh":
            return np.tanh(v)
        if act == "sigmoid":                                 # the form that neither overflows nor cancels on either side
            e = np.exp(-np.abs(v))
            return np.where(v >= 0, 1.0 / (1.0 + e), e / (1.0 + e))
    raise ValueError(act)


def ulps(got: np.ndarray, want64: np.ndarray) -> np.ndarray:
    """|got - want| in units of the spacing of fp32 at float32(want) (the subnormal spacing 2^-149 below FLT_MIN)"""
    want32 = np.asarray(want64, np.float64).astype(np.float32)
    with np.errstate(over="ignore"):
        sp = np.spacing(np.abs(want32)).astype(np.float64)
    sp = np.where(np.isfinite(sp), sp, np.spacing(np.float32(FLT_MAX) / 2).astype(np.float64) * 2)
    return np.abs(np.asarray(got, np.float64) - np.asarray(want64, np.float64)) / sp


def probe_values(n_random: int, seed: int, span: float) -> np.ndarray:
    """fp32 arguments: +-0, +-FLT_MIN, +-m 2^-k for k = 0 .. 60 and five mantissas (|v| <= 2^-10 well inside), the points where
    exp leaves fp32 on either side (+-87.3 .. +-104), +-1e3 .. +-FLT_MAX, and uniform draws on [-span, span], [-1, 1] and
    [-2^-10, 2^-10]"""
    rng = np.random.default_rng(seed)
    k = np.arange(0, 61, dtype=np.float64)
    mags = np.concatenate([m * 2.0 ** -k for m in (1.0, 1.25, 1.5, 1.75, 1.9999999)])
    edge = np.array([0.0, FLT_MIN, 2.0, 3.0, 5.0, 8.0, 9.0, 10.0, 16.0, 16.6, 17.0, 17.4, 20.0, 30.0, 50.0, 80.0, 87.0, 87.3, 87.34, 87.4, 88.0,
                     88.7, 88.73, 88.8, 89.0, 95.0, 100.0, 103.0, 103.9, 104.0, 110.0, 1e3, 1e10, 1e30, 1e38, FLT_MAX])
    det = np.concatenate([mags, edge])
    third = n_random // 3
    vals = np.concatenate([det, -det, rng.uniform(-span, span, n_random - 2 * third), rng.uniform(-1, 1, third),
                           rng.uniform(-2.0 ** -10, 2.0 ** -10, third)])
    return vals.astype(np.float32)
