"""Host-only checks of the train-mode BatchNorm entries: tests/_bn64.py's restatement against torch.nn.functional.batch_norm(training=True)
and its autograd in float64, the mutants of the header's order that the bit-for-bit comparison of tests/test_batchnorm_train_gpu.py must
catch, the cancellation pair (two-pass against the one-pass sum of squares), the scratch queries, the refusals (they return before anything
is enqueued, so they run without a device), and the prototypes against s3r._lib.SIGNATURES."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import __graft_entry__ as g
from tests import _bn64 as R
from tests import _stream_cases as SC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
EPS = 1e-5


@pytest.fixture(scope="module")
def lib(s3r):
    if not os.path.exists(s3r.LIB_PATH):
        g.build()
    return s3r.load_library()


def _data(shape, seed, act):
    rng = np.random.default_rng(seed)
    B, ch, S = shape
    z = (rng.standard_normal(shape) * 1.5 + 0.5).astype(F)
    gam = (1.0 + 0.5 * rng.standard_normal(ch)).astype(F)
    beta = (0.3 * rng.standard_normal(ch)).astype(F)
    gy = rng.standard_normal(shape).astype(F)
    return z, gam, beta, gy


def _torch64(z, gam, beta, gy, act):
    zt, gt, bt = (torch.from_numpy(np.asarray(a, np.float64)).requires_grad_() for a in (z, gam, beta))
    rm, rv = torch.zeros(z.shape[1], dtype=torch.float64), torch.ones(z.shape[1], dtype=torch.float64)
    u = torch.nn.functional.batch_norm(zt, rm, rv, gt, bt, training=True, momentum=1.0, eps=float(F(EPS)))
    y = {"none": u, "relu": torch.relu(u), "sigmoid": torch.sigmoid(u)}[act]
    y.backward(torch.from_numpy(gy.astype(np.float64)))
    return y.detach().numpy(), rm.numpy(), rv.numpy(), zt.grad.numpy(), gt.grad.numpy(), bt.grad.numpy()


@pytest.mark.parametrize("act", R.ACTS)
@pytest.mark.parametrize("shape", [(2, 3, 5), (3, 2, 513), (2, 2, 1029)], ids=lambda s: "x".join(map(str, s)))
def test_restatement_against_torch_float64(shape, act):
    """forward64 IS torch's training-mode batch_norm (to float64 rounding); the fp32 restatement is within the derived bounds of it; the
    fp32 backward is within backward64's bounds of the formula on its own statistics, and backward64 at float64 statistics is torch's
    autograd"""
    z, gam, beta, gy = _data(shape, 11 + sum(shape), act)
    B, ch, S = shape
    N = B * S
    y_t, mean_t, varu_t, gz_t, gg_t, gb_t = _torch64(z, gam, beta, gy, act)
    f = R.forward64(z, gam, beta, EPS, act)
    assert np.allclose(f["mean"], mean_t, rtol=1e-13, atol=1e-15) and np.allclose(f["var"] * N / (N - 1), varu_t, rtol=1e-12)
    assert np.allclose(f["y"], y_t, rtol=1e-12, atol=1e-14)
    mean, var, inv = R.stats32(z, EPS)
    for got, want, lim, name in ((mean, f["mean"], f["E_m"], "mean"), (var, f["var"], f["E_v"], "var"), (inv, f["invstd"], f["E_i"], "invstd")):
        err = np.abs(got.astype(np.float64) - want)
        assert (err <= lim).all(), (name, (err / lim).max())
        # (an any-order bound over N <= 2058 terms is about N u = 1.3e-4 of the magnitude sum, here O(1): a dropped chunk or sample,
        # a biased / unbiased mix-up (1 / N >= 5e-4 of var) or a missing eps stay visible)
        assert (lim <= 4e-4 * (np.abs(want) + 1.0)).all(), f"{name}: the bound is too loose to see a mistake"
    y = R.y32(z, mean, inv, gam, beta, act)
    err = np.abs(np.asarray(y, np.float64) - f["y"])
    assert (err <= f["E_y"]).all(), (err / f["E_y"]).max()
    # the backward: the restatement against float64 of the formula on the fp32 statistics, then that formula against torch's autograd
    y_in = None if act == "none" else np.asarray(y, F)
    gz, gg, gb = R.backward32(z, y_in, gy, gam, mean, inv, act)
    b = R.backward64(z, y_in, gy, gam, mean, inv, act)
    for got, want, lim, name in ((gz, b["grad_z"], b["E_z"], "grad_z"), (gg, b["grad_gamma"], b["E_c"], "grad_gamma"), (gb, b["grad_beta"], b["E_b"], "grad_beta")):
        err = np.abs(got.astype(np.float64) - want)
        assert (err <= lim).all(), (name, (err / lim).max())
    if act != "relu":             # (a ReLU gate at a rounded-to-zero y may differ from float64's: the gate window is the GPU tail test's business)
        scale = np.abs(gz_t).max()
        assert np.abs(b["grad_z"] - gz_t).max() <= 2e-5 * scale, "the formula is not torch's autograd"
        assert np.allclose(b["grad_gamma"], gg_t, rtol=1e-4, atol=1e-4) and np.allclose(b["grad_beta"], gb_t, rtol=1e-4, atol=1e-4)


def test_mutants_of_the_order_change_bits():
    """the data set: seeded N(0.5, 1.5) of (3, 8, 1029) — three chunks per row, three samples — and a row of -0.0"""
    z, gam, beta, gy = _data((3, 8, 1029), 5, "none")
    mean, var, inv = R.stats32(z, EPS)
    gz, gg, gb = R.backward32(z, None, gy, gam, mean, inv, "none")
    for m in ("descending-chunks", "descending-batch"):
        mm, mv, _ = R.stats32(z, EPS, mutant=m)
        _, mg, mb = R.backward32(z, None, gy, gam, mean, inv, "none", mutant=m)
        changed = [n for n, a, b in (("mean", mm, mean), ("var", mv, var), ("grad_gamma", mg, gg), ("grad_beta", mb, gb)) if (R.bits(a) != R.bits(b)).any()]
        print(m, "changes", changed)
        assert changed, m
    _, mv, _ = R.stats32(z, EPS, mutant="fma")
    assert (R.bits(mv) != R.bits(var)).any(), "a fused d * d + partial"
    _, mg, _ = R.backward32(z, None, gy, gam, mean, inv, "none", mutant="fma")
    assert (R.bits(mg) != R.bits(gg)).any(), "a fused g * xhat + partial"
    # the accumulator's start.  A lane partial that starts as +0.0 never holds -0.0, so no chunk sum is -0.0 and the finish's accumulators
    # (which start AS the first chunk's / sample's sum) cannot differ from ones that start at +0.0: the start matters in the lane partial,
    # where a row of -0.0 sums to +0.0 under the contract and to -0.0 when the partial starts as its first term
    neg = np.full((2, 1, 512), -0.0, F)                          # (a full chunk: a padding lane would add +0.0 in the tree)
    assert R.bits(R.total32(neg))[0] == 0
    assert R.bits(R.finish32(R.chunk_sums_mutant32(neg, None, "first-term")))[0] == np.int32(-2 ** 31)


@pytest.mark.parametrize("seed", [0, 1, 2])
@pytest.mark.parametrize("shape", R.CANCEL, ids=lambda s: "x".join(map(str, s)))
def test_cancellation_pair(shape, seed):
    """z = 100 + 0.1 randn: the two-pass variance is within 1e-5 relative of float64, the one-pass sum(z^2) / N - mean^2 misses by more
    than 1e-2"""
    z = R.cancel_data(shape, seed)
    z64 = z.astype(np.float64)
    var64 = z64.var(axis=(0, 2))
    _, var, _ = R.stats32(z, EPS)
    two = np.abs(var - var64) / var64
    one = np.abs(R.one_pass_var32(z) - var64) / var64
    print(f"{shape} seed {seed}: two-pass rel err {two.max():.3e}, one-pass rel err {one.min():.3e}")
    assert (two <= 1e-5).all()
    assert (one > 1e-2).all()


def test_scratch_queries_are_shape_only_and_monotone(lib):
    for q, want in ((lib.s3r_batchnorm_train_forward_scratch_elems, lambda B, ch, n: ch * B * n),
                    (lib.s3r_batchnorm_train_backward_scratch_elems, lambda B, ch, n: 2 * ch * B * n + 2 * ch)):
        for ch in (1, 3, 64):
            for S in (1, 5, 511, 512, 513, 1029, 32768):
                prev = 0
                for B in (0, 1, 2, 3, 65):
                    got = q(B, ch, S)
                    assert got == want(B, ch, (S + 511) // 512) and got >= prev
                    assert got == q(B, ch, S)
                    prev = got
        assert q(-1, 1, 1) == -1 and q(1, 0, 1) == -1 and q(1, 1, 0) == -1
        assert q(2, 2, 1 << 29) == -1 and b"4 GiB" in lib.s3r_last_error()      # 2^31 elements
        assert q(1, 1, (1 << 31)) == -1


def test_refusals_before_anything_is_enqueued(lib):
    p = C.c_void_p(1 << 20)                                       # never dereferenced: every call below is refused on the host
    fwd, bwd = lib.s3r_batchnorm_train_forward, lib.s3r_batchnorm_train_backward
    big = 1 << 20

    def f(act=1, B=2, ch=3, S=5, scratch=p, elems=big, y=p, z=p):
        return fwd(z, p, p, EPS, act, y, p, p, p, B, ch, S, scratch, elems, None)

    def b(act=1, B=2, ch=3, S=5, scratch=p, elems=big, outs=(p, p, p), y=p, z=p, gam=p):
        return bwd(z, y, p, gam, p, p, act, *outs, B, ch, S, scratch, elems, None)

    for call in (f, b):
        assert call(B=1, S=1) == -1 and b"more than one value" in lib.s3r_last_error()       # N < 2
        assert call(act=3) == -1 and b"none / relu / sigmoid" in lib.s3r_last_error()
        assert call(act=-1) == -1
        assert call(ch=0) == -1 and call(S=0) == -1 and call(B=-1) == -1
        assert call(B=4, ch=1 << 10, S=1 << 19) == -1 and b"4 GiB" in lib.s3r_last_error()   # 2^31 elements
        assert call(B=0) == 0                                                                # nothing launched
        assert call(scratch=None) == -3 and call(elems=0) == -3
        assert call(z=None) == -1
    need_f, need_b = lib.s3r_batchnorm_train_forward_scratch_elems(2, 3, 5), lib.s3r_batchnorm_train_backward_scratch_elems(2, 3, 5)
    assert f(elems=need_f - 1) == -3 and b(elems=need_b - 1) == -3
    assert f(y=None) == -1
    assert b(outs=(None, None, None)) == -1 and b"all NULL" in lib.s3r_last_error()
    assert b(act=1, y=None) == -1 and b"y is NULL" in lib.s3r_last_error()
    assert b(gam=None) == -1                                       # grad_z needs gamma
    assert b(B=0, outs=(None, None, None)) == -1                   # all NULL is refused before the batch is looked at


def test_prototypes_match_the_bindings(s3r):
    header = open(os.path.join(ROOT, "include", "s3r.h")).read()
    plain = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    want = {
        "s3r_batchnorm_train_forward": ["const float* z", "const float* gamma", "const float* beta", "float eps", "int act", "float* y",
                                        "float* save_mean", "float* save_var", "float* save_invstd", "int batch", "int channels",
                                        "int64_t positions", "float* scratch", "int64_t scratch_elems", "void* hip_stream"],
        "s3r_batchnorm_train_backward": ["const float* z", "const float* y", "const float* grad_y", "const float* gamma",
                                         "const float* save_mean", "const float* save_invstd", "int act", "float* grad_z",
                                         "float* grad_gamma", "float* grad_beta", "int batch", "int channels", "int64_t positions",
                                         "float* scratch", "int64_t scratch_elems", "void* hip_stream"],
        "s3r_batchnorm_train_forward_scratch_elems": ["int batch", "int channels", "int64_t positions"],
        "s3r_batchnorm_train_backward_scratch_elems": ["int batch", "int channels", "int64_t positions"],
    }
    ctype = {"int": C.c_int, "int64_t": C.c_int64, "float": C.c_float}
    for name, params in want.items():
        m = re.search(r"\b(int|int64_t)\s+%s\s*\(([^)]*)\)\s*;" % name, plain)
        assert m, f"{name} is not declared in include/s3r.h"
        assert [" ".join(a.split()) for a in m.group(2).split(",")] == params
        res, args = s3r._lib.SIGNATURES[name]
        assert res is ctype[m.group(1)]
        assert args == [C.c_void_p if "*" in a else ctype[a.split()[0]] for a in params]
    # `hip_stream`: the entries' stream contract has a file of its own (tests/test_batchnorm_train_streams_gpu.py)
    assert not {n for n in want if n in SC.stream_prototypes(header)}
    at = header.index("int s3r_batchnorm_train_backward(")
    comment = header[header[:at].rfind("/*"):at]
    for word in ("NaN", "hip_stream", "DOES depend on the batch", "ascending chunk order", "Launches", "not on the scratch's contents"):
        assert word in comment, word
    assert s3r.load_library().s3r_abi_version() == 8
