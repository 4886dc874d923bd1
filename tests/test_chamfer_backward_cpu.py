"""s3r_chamfer_backward without a GPU: the declaration and its binding, host-side validation (every refusal is S3R_ERR_INVALID
with a message, before anything is launched: a HIP call would have given S3R_ERR_HIP on a host without a device), and the two
restatements of tests/_chamfer64.py — (b) against torch's own autograd through the oracle in float64, which pins the DEFINITION to
the true gradient independently of the library, and (a), the defined fp32 order, within the derived bound of (b)."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from tests import _chamfer64 as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = -1


@pytest.fixture(scope="module")
def lib(s3r):
    import __graft_entry__ as g
    if not os.path.exists(s3r.LIB_PATH):
        g.build()
    return s3r.load_library()


def test_header_prototype_matches_the_binding(s3r, lib):
    header = open(os.path.join(ROOT, "include", "s3r.h")).read()
    assert "#define S3R_ABI_VERSION 8" in header                  # an additive entry point: no version step
    m = re.search(r"\bint\s+s3r_chamfer_backward\s*\(([^)]*)\)\s*;", re.sub(r"/\*.*?\*/", "", header, flags=re.S))
    assert m, "s3r_chamfer_backward is not declared in include/s3r.h"
    assert [" ".join(a.split()) for a in m.group(1).split(",")] == [
        "const float* p", "const float* q", "const int32_t* idx1", "const int32_t* idx2", "const float* grad_dist1",
        "const float* grad_dist2", "float* grad_p", "float* grad_q", "int batch", "int n", "int m", "void* stream"]
    res, args = s3r._lib.SIGNATURES["s3r_chamfer_backward"]
    assert res is C.c_int and args == [C.c_void_p] * 8 + [C.c_int] * 3 + [C.c_void_p]
    assert lib.s3r_chamfer_backward.argtypes == args
    assert lib.s3r_abi_version() == 8
    assert callable(s3r.chamfer_distance_backward) and callable(s3r.differentiable_chamfer_distance)
    assert {"chamfer_distance_backward", "differentiable_chamfer_distance"} <= set(s3r.__all__)


# a non-NULL host address: validation rejects each case before anything could dereference it
_P = C.cast(C.create_string_buffer(64), C.c_void_p).value
_GOOD = dict(p=_P, q=_P, idx1=_P, idx2=_P, g1=_P, g2=_P, gp=_P, gq=_P, batch=2, n=16, m=24)
_BAD = {
    "null-p": dict(p=None), "null-q": dict(q=None), "null-idx1": dict(idx1=None), "null-idx2": dict(idx2=None),
    "both-grads-in-null": dict(g1=None, g2=None),
    "both-grads-out-null": dict(gp=None, gq=None),
    "batch-zero": dict(batch=0), "batch-negative": dict(batch=-1), "n-zero": dict(n=0), "n-negative": dict(n=-5),
    "m-zero": dict(m=0), "m-negative": dict(m=-1),
    "batch-65536": dict(batch=65536),
    "2^31-elements": dict(batch=1024, n=1 << 20, m=4),        # grad_p / p: 3 * 2^30 elements
    "2^31-elements-q": dict(batch=2, n=4, m=(1 << 30) // 3 + 1),
}


def _call(lib, p, q, idx1, idx2, g1, g2, gp, gq, batch, n, m):
    return lib.s3r_chamfer_backward(p, q, idx1, idx2, g1, g2, gp, gq, batch, n, m, None)


@pytest.mark.parametrize("case", list(_BAD), ids=list(_BAD))
def test_backward_rejects_bad_arguments_on_the_host(lib, case):
    assert _call(lib, **dict(_GOOD, **_BAD[case])) == INVALID
    assert lib.s3r_last_error().decode()


def test_backward_messages_name_the_rule(lib):
    assert _call(lib, **dict(_GOOD, batch=65536)) == INVALID and b"split the call" in lib.s3r_last_error()
    assert _call(lib, **dict(_GOOD, g1=None, g2=None)) == INVALID and b"grad_dist1" in lib.s3r_last_error()
    assert _call(lib, **dict(_GOOD, gp=None, gq=None)) == INVALID and b"grad_p" in lib.s3r_last_error()


def test_python_layer_checks_before_the_device(s3r):
    p, q = torch.zeros(2, 5, 3), torch.zeros(2, 7, 3)
    i1, i2 = torch.zeros(2, 5, dtype=torch.int32), torch.zeros(2, 7, dtype=torch.int32)
    with pytest.raises(RuntimeError, match="HIP device"):                 # no CPU fallback, as chamfer_distance
        s3r.chamfer_distance_backward(p, q, i1, i2, torch.zeros(2, 5), torch.zeros(2, 7))
    with pytest.raises(RuntimeError, match="expects"):
        s3r.chamfer_distance_backward(p[0], q, i1, i2, torch.zeros(2, 5), None)
    with pytest.raises(RuntimeError, match="HIP device"):
        s3r.ChamferDistance()(p.clone().requires_grad_(), q)


# ---------------------------------------------------------------- the restatements
def _case(B, N, M, seed):
    g = torch.Generator().manual_seed(seed)
    p, q = torch.rand(B, N, 3, generator=g), torch.rand(B, M, 3, generator=g)
    g1, g2 = torch.randn(B, N, generator=g), torch.randn(B, M, generator=g)
    return p, q, g1, g2


SHAPES = [(1, 1, 1), (1, 1, 9), (2, 7, 1), (2, 33, 65), (3, 130, 77), (1, 300, 300), (2, 64, 257)]


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_fp64_restatement_is_the_true_gradient(oracle, shape):
    """(b) against torch.autograd.grad of sum(g1 dist1) + sum(g2 dist2) through the oracle's chamfer_distance in float64 on tie-free
    random clouds.  Both sides evaluate the same k + 1 real terms per element in float64 with other roundings — autograd adds the two
    upstream gradients of a mutually-nearest pair BEFORE the product and sums the dense (N, M) gradient with its own reduction —
    so each is within (k + 3) 2^-53 sum|term| of the real value (the float64 form of the bound derived in tests/_chamfer64.py) and
    they are within twice that of each other."""
    B, N, M = shape
    p, q, g1, g2 = _case(B, N, M, seed=N * 1000 + M)
    pd, qd = p.double().requires_grad_(), q.double().requires_grad_()
    d1, d2, i1, i2 = oracle.chamfer_distance(pd, qd)
    dense = ((pd[:, :, None, :] - qd[:, None, :, :]) ** 2).sum(-1).detach()
    for b in range(B):                                             # tie-free: the minimum of every row and column is unique
        assert ((dense[b] == d1[b].detach()[:, None]).sum(1) == 1).all() and ((dense[b] == d2[b].detach()[None, :]).sum(0) == 1).all()
    want_p, want_q = torch.autograd.grad((g1.double() * d1).sum() + (g2.double() * d2).sum(), (pd, qd))
    (gp, kp, mp), (gq, kq, mq) = R.backward64(p.numpy(), q.numpy(), i1.numpy(), i2.numpy(), g1.numpy(), g2.numpy())
    assert gp.dtype == np.float64 and kp.sum() == B * M and kq.sum() == B * N      # every source scatters exactly one term
    for got, want, k, mag in ((gp, want_p, kp, mp), (gq, want_q, kq, mq)):
        err = np.abs(got - want.numpy())
        lim = 2 * (k[:, :, None] + 3) * R.EPS64 * mag
        print(f"{shape}: max err {err.max():.3e}, max err / bound {(err / np.maximum(lim, 1e-300)).max():.3f}, max k {k.max()}")
        assert (err <= lim).all()
        assert np.abs(got).max() > 0


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_fp32_order_stays_within_the_derived_bound_of_fp64(oracle, shape):
    B, N, M = shape
    p, q, g1, g2 = _case(B, N, M, seed=N * 1000 + M + 1)
    _, _, i1, i2 = oracle.chamfer_distance(p, q)
    a = R.backward32(p.numpy(), q.numpy(), i1.numpy(), i2.numpy(), g1.numpy(), g2.numpy())
    b = R.backward64(p.numpy(), q.numpy(), i1.numpy(), i2.numpy(), g1.numpy(), g2.numpy())
    for got, (ref, k, mag) in zip(a, b):
        assert got.dtype == np.float32
        err = np.abs(got.astype(np.float64) - ref)
        assert (err <= R.bound32(k, mag)).all(), (err / R.bound32(k, mag)).max()


def test_restatement_hand_computed_case():
    """one sample, p = {(0,0,0), (4,0,0)}, q = {(1,0,0)}: idx1 = [0, 0], idx2 = [0]; grad_dist1 = [1, 2], grad_dist2 = [3]:
    grad_p[0] = 2 (0 - 1) + 6 (0 - 1) = -8, grad_p[1] = 4 (4 - 1) = 12, grad_q[0] = 6 (1 - 0) + 2 (1 - 0) + 4 (1 - 4) = -4"""
    p = np.array([[[0, 0, 0], [4, 0, 0]]], np.float32)
    q = np.array([[[1, 0, 0]]], np.float32)
    i1, i2 = np.array([[0, 0]], np.int32), np.array([[0]], np.int32)
    g1, g2 = np.array([[1, 2]], np.float32), np.array([[3]], np.float32)
    gp, gq = R.backward32(p, q, i1, i2, g1, g2)
    assert gp[0, :, 0].tolist() == [-8.0, 12.0] and gq[0, 0, 0] == -4.0
    assert not gp[..., 1:].any() and not gq[..., 1:].any()
    (gp64, kp, mp), (gq64, kq, mq) = R.backward64(p, q, i1, i2, g1, g2)
    assert kp.tolist() == [[1, 0]] and kq.tolist() == [[2]] and mq[0, 0, 0] == 6 + 2 + 12 and gq64[0, 0, 0] == -4.0
    # None is a zero tensor; garbage indices: the own index is clamped, the scatter index matches nothing
    z = R.backward32(p, q, i1, i2, g1, None)
    assert np.array_equal(R.bits(z[0]), R.bits(R.backward32(p, q, i1, i2, g1, np.zeros((1, 1), np.float32))[0]))
    gp2, gq2 = R.backward32(p, q, np.array([[-1, 5]], np.int32), i2, g1, g2)
    assert gp2[0, :, 0].tolist() == [-8.0, 12.0] and gq2[0, 0, 0] == 6.0


def test_the_order_is_observable():
    """the defined order is a real constraint: on a heavy-collision target the ascending sum and the descending sum differ in fp32"""
    g = torch.Generator().manual_seed(5)
    p = (torch.rand(1, 500, 3, generator=g) * 0.1).numpy()
    q = np.concatenate([np.full((1, 1, 3), 0.05, np.float32), 100 + torch.rand(1, 7, 3, generator=g).numpy()], 1)
    i1 = np.zeros((1, 500), np.int32)
    i2 = np.zeros((1, 8), np.int32)
    g1 = torch.randn(1, 500, generator=g).numpy()
    asc = R.backward32(p, q, i1, i2, g1, None)[1]
    desc = R.backward32(p[:, ::-1], q, i1, i2, g1[:, ::-1], None)[1]
    assert not np.array_equal(R.bits(asc[0, 0]), R.bits(desc[0, 0]))
