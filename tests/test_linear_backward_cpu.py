"""s3r_linear_backward without a GPU: the two declarations and their bindings, host-side validation (every refusal happens before
anything is launched: a HIP call would have given S3R_ERR_HIP on a host without a device), the scratch query, and the numpy
restatements of tests/_linear64.py — against torch's own autograd in float64, which pins the DEFINITION to the true gradient
independently of the library, and the fp32 activation rules bit for bit against a scalar loop."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from tests import _linear64 as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID, WORKSPACE = -1, -3


@pytest.fixture(scope="module")
def lib(s3r):
    import __graft_entry__ as g
    if not os.path.exists(s3r.LIB_PATH):
        g.build()
    return s3r.load_library()


def _args(header, ret, name):
    m = re.search(r"\b%s\s+%s\s*\(([^)]*)\)\s*;" % (ret, name), re.sub(r"/\*.*?\*/", "", header, flags=re.S))
    assert m, f"{name} is not declared in include/s3r.h"
    return [" ".join(a.split()) for a in m.group(1).split(",")]


def test_header_prototypes_match_the_bindings(s3r, lib):
    header = open(os.path.join(ROOT, "include", "s3r.h")).read()
    assert "#define S3R_ABI_VERSION 8" in header                  # additive entry points: no version step
    assert _args(header, "int64_t", "s3r_linear_backward_scratch_elems") == ["int batch", "int cin", "int cout"]
    assert _args(header, "int", "s3r_linear_backward") == [
        "const float* x", "const float* w", "const float* y", "const float* grad_y", "float* grad_x", "float* grad_w",
        "float* grad_bias", "int batch", "int cin", "int cout", "int act", "float* scratch", "int64_t scratch_elems", "void* stream"]
    res, args = s3r._lib.SIGNATURES["s3r_linear_backward_scratch_elems"]
    assert res is C.c_int64 and args == [C.c_int] * 3
    res, args = s3r._lib.SIGNATURES["s3r_linear_backward"]
    assert res is C.c_int and args == [C.c_void_p] * 7 + [C.c_int] * 4 + [C.c_void_p, C.c_int64, C.c_void_p]
    assert lib.s3r_linear_backward.argtypes == args
    assert lib.s3r_abi_version() == 8
    names = {"linear", "linear_backward", "differentiable_linear"}
    assert names <= set(s3r.__all__) and all(callable(getattr(s3r, n)) for n in names)
    assert callable(s3r.PointHead.differentiable) and callable(s3r.Stereo2Point.latent)


# a non-NULL host address: validation rejects each case before anything could dereference it
_P = C.cast(C.create_string_buffer(64), C.c_void_p).value
_GOOD = dict(x=_P, w=_P, y=_P, gy=_P, gx=_P, gw=_P, gb=_P, batch=2, cin=16, cout=24, act=1, scratch=_P, elems=1 << 40)
_BAD = {
    "all-outputs-null": (dict(gx=None, gw=None, gb=None), INVALID),
    "y-null-relu": (dict(y=None, act=1), INVALID), "y-null-sigmoid": (dict(y=None, act=2), INVALID),
    "act-3": (dict(act=3), INVALID), "act-negative": (dict(act=-1), INVALID), "act-6": (dict(act=6), INVALID),
    "null-grad_y": (dict(gy=None), INVALID), "null-x-with-grad_w": (dict(x=None), INVALID), "null-w-with-grad_x": (dict(w=None), INVALID),
    "batch-zero": (dict(batch=0), INVALID), "batch-negative": (dict(batch=-1), INVALID), "cin-zero": (dict(cin=0), INVALID),
    "cin-negative": (dict(cin=-3), INVALID), "cout-zero": (dict(cout=0), INVALID), "cout-negative": (dict(cout=-1), INVALID),
    "4GiB-weight": (dict(cin=1 << 15, cout=1 << 15), INVALID), "4GiB-x": (dict(batch=1 << 15, cin=1 << 15), INVALID),
    "scratch-null": (dict(scratch=None), WORKSPACE), "scratch-zero": (dict(elems=0), WORKSPACE),
}


def _call(lib, x, w, y, gy, gx, gw, gb, batch, cin, cout, act, scratch, elems):
    return lib.s3r_linear_backward(x, w, y, gy, gx, gw, gb, batch, cin, cout, act, scratch, elems, None)


@pytest.mark.parametrize("case", list(_BAD), ids=list(_BAD))
def test_backward_rejects_bad_arguments_on_the_host(lib, case):
    change, code = _BAD[case]
    assert _call(lib, **dict(_GOOD, **change)) == code
    assert lib.s3r_last_error().decode()


def test_short_scratch_is_a_workspace_error(lib):
    for shape in ((2, 16, 24), (4, 64, 4096), (32, 1024, 6144)):
        need = lib.s3r_linear_backward_scratch_elems(*shape)
        b, ci, co = shape
        assert need > 0
        assert _call(lib, **dict(_GOOD, batch=b, cin=ci, cout=co, elems=need - 1)) == WORKSPACE
        assert b"s3r_linear_backward_scratch_elems" in lib.s3r_last_error()
    assert _call(lib, **dict(_GOOD, gx=None, gw=None, gb=None)) == INVALID and b"grad_x" in lib.s3r_last_error()
    assert _call(lib, **dict(_GOOD, y=None)) == INVALID and b"y is NULL" in lib.s3r_last_error()


def test_scratch_query(lib):
    q = lib.s3r_linear_backward_scratch_elems
    assert q(0, 4, 4) == INVALID and q(4, 0, 4) == INVALID and q(4, 4, -1) == INVALID
    for cin, cout in ((1, 1), (33, 31), (64, 4096), (1024, 1024), (1024, 6144), (32768, 1024)):
        sizes = [q(b, cin, cout) for b in range(1, 70)]
        assert sizes[0] > 0 and all(a <= b for a, b in zip(sizes, sizes[1:])), (cin, cout)      # positive, monotone in batch
        assert sizes[0] >= cout                                                                   # holds g at least


def test_python_layer_checks_before_the_device(s3r):
    x, w, b = torch.zeros(2, 5), torch.zeros(7, 5), torch.zeros(7)
    with pytest.raises(RuntimeError, match="HIP device"):                 # no CPU fallback
        s3r.linear(x, w, b)
    with pytest.raises(RuntimeError, match="HIP device"):
        s3r.linear_backward(x, w, None, torch.zeros(2, 7), "none")
    with pytest.raises(RuntimeError, match="HIP device"):
        s3r.differentiable_linear(x.requires_grad_(), w, b, "relu")
    with pytest.raises(RuntimeError, match="act must be"):
        s3r.linear(x, w, b, "tanh")
    with pytest.raises(RuntimeError, match="expects"):
        s3r.linear(x, torch.zeros(7, 6), b)


# ---------------------------------------------------------------- the restatements
def _case(B, cin, cout, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(B, cin, generator=g), torch.randn(cout, cin, generator=g) / cin ** 0.5, torch.randn(cout, generator=g),
            torch.randn(B, cout, generator=g))


def _rule64(y, gy, act):
    if act == "relu":
        return np.where(y > 0, gy, 0.0)
    if act == "sigmoid":
        return gy * (y * (1.0 - y))
    return gy.copy()


SHAPES = [(1, 1, 1), (3, 33, 31), (2, 40, 100), (33, 96, 160), (5, 256, 96)]


@pytest.mark.parametrize("act", R.ACTS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_fp64_restatement_is_the_true_gradient(shape, act):
    """backward64 and the rule against torch.autograd.grad of sum(grad_y * act(x W^T + bias)) in float64.  Both sides add the same K
    real terms per element in float64 in different orders: each is within gamma_{K+1} sum|term| of the real value (tests/_linear64.py,
    with 2^-53 for 2^-24), hence within twice that of each other."""
    B, cin, cout = shape
    x, w, bias, gy = (t.double() for t in _case(B, cin, cout, seed=cin * 1000 + cout))
    xd, wd, bd = x.clone().requires_grad_(), w.clone().requires_grad_(), bias.clone().requires_grad_()
    z = xd @ wd.T + bd
    y = {"none": z, "relu": torch.relu(z), "sigmoid": torch.sigmoid(z)}[act]
    want_x, want_w, want_b = torch.autograd.grad((gy * y).sum(), (xd, wd, bd))
    g = _rule64(y.detach().numpy(), gy.numpy(), act)
    (gw, kw, mw), (gx, kx, mx) = R.backward64(x.numpy(), w.numpy(), g)
    assert gw.dtype == np.float64 and kw == B and kx == cout
    gb, mb = g.sum(0), np.abs(g).sum(0)
    for got, want, k, mag, name in ((gw, want_w, kw, mw, "grad_w"), (gx, want_x, kx, mx, "grad_x"), (gb, want_b, B, mb, "grad_bias")):
        err = np.abs(got - want.numpy())
        lim = 2 * (k + 1) * R.EPS64 / (1 - (k + 1) * R.EPS64) * mag
        print(f"{shape} {act} {name}: max err {err.max():.3e}, max err / bound {(err / np.maximum(lim, 1e-300)).max():.3f}")
        assert (err <= lim).all()
    assert np.abs(gw).max() > 0 and np.abs(gx).max() > 0


@pytest.mark.parametrize("act", R.ACTS)
def test_fp32_rule_against_a_scalar_loop_bit_for_bit(act):
    g = torch.Generator().manual_seed(11)
    y = torch.rand(7, 13, generator=g).numpy() if act == "sigmoid" else torch.randn(7, 13, generator=g).numpy()
    gy = torch.randn(7, 13, generator=g).numpy()
    special = np.array([0.0, -0.0, np.nan, np.inf, -np.inf, 1.0, 2.0 ** -140, -1.5], np.float32)
    y[0, :8], gy[1, :8] = special, special
    y[1, :8] = special[::-1]
    got = R.g32(y, gy, act)
    want = np.empty_like(got)
    one, zero = np.float32(1), np.float32(0)
    with np.errstate(all="ignore"):
        for i in range(y.shape[0]):
            for j in range(y.shape[1]):
                yy, gg = np.float32(y[i, j]), np.float32(gy[i, j])
                if act == "relu":
                    want[i, j] = gg if yy > zero else zero
                elif act == "sigmoid":
                    t = np.float32(one - yy)
                    u = np.float32(yy * t)
                    want[i, j] = np.float32(gg * u)
                else:
                    want[i, j] = gg
    assert got.dtype == np.float32 and np.array_equal(R.bits(got), R.bits(want))
    if act == "relu":          # y = 0, -0, NaN, -inf give 0 whatever grad_y is, +inf passes grad_y
        assert R.bits(got[0, :5]).tolist() == [0, 0, 0, R.bits(gy[0, 3:4])[0], 0]


def test_fp32_rule_is_close_to_the_float64_rule():
    """three fp32 roundings: |g32 - g64| <= gamma_3 |g64| (+ one subnormal)"""
    g = torch.Generator().manual_seed(12)
    y, gy = torch.rand(50, 40, generator=g).numpy(), torch.randn(50, 40, generator=g).numpy()
    for act in R.ACTS:
        ref = _rule64(y.astype(np.float64), gy.astype(np.float64), act)
        assert (np.abs(R.g32(y, gy, act) - ref) <= R.gamma(3) * np.abs(ref) + 2.0 ** -149).all()


def test_grad_bias_order():
    """the sequential sum: equal to a scalar loop bit for bit, within the bound of float64, and observably an ORDER (the descending
    sum differs in fp32)"""
    g = torch.Generator().manual_seed(13)
    v = torch.randn(200, 9, generator=g).numpy()
    got = R.grad_bias32(v)
    for o in range(v.shape[1]):
        s = np.float32(v[0, o])
        for b in range(1, v.shape[0]):
            s = np.float32(s + v[b, o])
        assert R.bits(got[o:o + 1])[0] == R.bits(np.array([s]))[0]
    assert (np.abs(got - v.astype(np.float64).sum(0)) <= R.bound32(v.shape[0], np.abs(v).astype(np.float64).sum(0))).all()
    assert not np.array_equal(R.bits(got), R.bits(R.grad_bias32(v[::-1])))
    assert np.array_equal(R.bits(R.grad_bias32(v[:1])), R.bits(v[0]))            # B = 1: g itself
