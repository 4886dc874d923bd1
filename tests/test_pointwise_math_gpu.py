"""The elementwise math behind the layers, per element against float64: act_kernel (LeakyReLU / ELU / Tanh behind a general layer,
csrc/s3r_general.hip) and the sigmoid of the occupancy head and of the linear finish (apply_act, csrc/s3r_pointwise.hip).

The whole-tensor norms of test_general_gpu.py and the tolerance tests of the head do not see an ELU written as expf(v) - 1 or a
sigmoid that loses its range (tests/mutants/table.py: elu_expf_minus_one, head_sigmoid_unsymmetric): both are wrong only where the
result is tiny or the argument large.  Here every element is its own check.

How the argument reaches the function unchanged: the layer is a linear layer whose weight is the identity (or a 1 x 1 x 1 head whose
weight is 1 on channel 0 and 0 elsewhere) with a zero bias and no BatchNorm, so its pre-activation is v * 1 + 0 + .. + 0 = v, exactly
(the same layer with act="none" returns the input bit for bit: asserted).

Bounds.
  LeakyReLU: v > 0 ? v : v * slope is one correctly rounded fp32 product: the result IS float32(v) * float32(slope), bit for bit.
  ELU, Tanh: alpha * expm1f(v) and tanhf(v) are the device library's functions; their ulp bounds are not in the headers this
      project builds against, so the bound is MEASURED: the stock kernel's largest error in ulps of the float64 value rounded to
      fp32, times two (docs/LAB_NOTES.md, "Kernel mutants", holds the measured values).
  sigmoid: the kernel computes 1.f / (1.f + __expf(-v)) and the compiler's HIP math header defines __expf(x) as
      exp2(float32(log2 e) * x): the argument's rounding (of the constant and of the product, 2^-23 relative together) moves the
      exponential by a relative |x| 2^-23, and d ln s / d ln e = -(1 - s).  So the error in ulps grows like 1 + (1 - s) |v|; the
      constant in front of that shape is measured as above (the hardware exp2's own error is not in the headers either).
      Where the float64 value is below FLT_MIN the hardware may return 0 or a subnormal: anything in [0, FLT_MIN] passes there.
"""
import numpy as np
import pytest
import torch

from tests import _act64 as A

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

# measured on the stock library (gfx950), in ulps of float32(float64 reference); the tests allow twice these
MEASURED_ELU_ULPS = 1.125          # alpha = 0.7 at v = -0.168 (alpha = 1: 0.754)
MEASURED_TANH_ULPS = 1.034         # at v = 0.672
MEASURED_SIGMOID_SHAPE = 1.973     # max of ulps / (1 + (1 - s) |v|), at v = -6.0e-4
FACTOR = 2.0

VALS = A.probe_values(3500, 20, 110.0)           # 4182 values: more than one 256-thread block, no multiple of one


def _through_linear(s3r, act, param, vals):
    """act(vals) through a 64 -> 64 linear layer with the identity as its weight"""
    L = s3r.arch_spec.Layer
    n = (len(vals) + 63) // 64
    x = np.zeros(n * 64, np.float32)
    x[:len(vals)] = vals
    ch = s3r.modules._HipChain([L("a", "linear", 64, 64, 1, 1, 0, False, act, 1, 0, param)], 1, precision="fp32")
    with torch.no_grad():
        ch.a.conv.weight.copy_(torch.eye(64))
        ch.a.conv.bias.zero_()
    ch.to(DEV)
    y = ch._run(torch.from_numpy(x).view(n, 64).to(DEV))
    torch.cuda.synchronize()
    return y.cpu().numpy().reshape(-1)[:len(vals)]


def _through_head(s3r, act, vals):
    """act(vals) through a Conv3d(16 -> 1, k1) head at 8^3 whose weight is 1 on channel 0"""
    L = s3r.arch_spec.Layer
    S = 512
    n = (len(vals) + S - 1) // S
    c0 = np.zeros(n * S, np.float32)
    c0[:len(vals)] = vals
    x = np.zeros((n, 16, S), np.float32)
    x[:, 0] = c0.reshape(n, S)
    ch = s3r.modules._HipChain([L("h", "conv3d", 16, 1, 1, 1, 0, False, act)], 8, precision="fp32")
    with torch.no_grad():
        ch.h.conv.weight.zero_()
        ch.h.conv.weight[0, 0] = 1.0
        ch.h.conv.bias.zero_()
    ch.to(DEV)
    y = ch._run(torch.from_numpy(x).view(n, 16, 8, 8, 8).to(DEV))
    torch.cuda.synchronize()
    return y.cpu().numpy().reshape(-1)[:len(vals)]


ROUTES = {"linear": lambda s3r, act, vals: _through_linear(s3r, act, None, vals), "head": _through_head}


@pytest.mark.parametrize("route", list(ROUTES))
def test_the_argument_arrives_unchanged(s3r, route):
    got = ROUTES[route](s3r, "none", VALS)
    assert np.array_equal(got.view(np.uint32) & 0x7fffffff, VALS.view(np.uint32) & 0x7fffffff), "the pre-activation is not the input"


@pytest.mark.parametrize("slope", [None, 0.3])
def test_leaky_relu_is_one_rounded_product(s3r, slope):
    got = _through_linear(s3r, "leaky_relu", slope, VALS)
    p = np.float32(0.01 if slope is None else slope)
    want = np.where(VALS > 0, VALS, (VALS * p).astype(np.float32))
    bad = got.view(np.uint32) != want.view(np.uint32)
    bad &= ~((got == 0) & (want == 0))                  # (the sign of a zero is the linear layer's, not the activation's)
    assert not bad.any(), (VALS[bad][:8], got[bad][:8], want[bad][:8])


def _worst(got, want, vals, weight=None):
    u = A.ulps(got, want)
    if weight is not None:
        u = u / weight
    i = int(np.argmax(u))
    return float(u[i]), float(vals[i])


@pytest.mark.parametrize("alpha", [None, 0.7])
def test_elu_per_element(s3r, alpha):
    got = _through_linear(s3r, "elu", alpha, VALS)
    want = A.ref64("elu", VALS, 1.0 if alpha is None else alpha)
    worst, at = _worst(got, want, VALS)
    print(f"elu alpha={alpha}: worst {worst:.3f} ulp at v = {at!r}")
    assert np.isfinite(got).all()
    assert worst <= FACTOR * MEASURED_ELU_ULPS, (worst, at)
    assert np.array_equal(got[VALS > 0], VALS[VALS > 0])


def test_tanh_per_element(s3r):
    got = _through_linear(s3r, "tanh", None, VALS)
    want = A.ref64("tanh", VALS)
    worst, at = _worst(got, want, VALS)
    print(f"tanh: worst {worst:.3f} ulp at v = {at!r}")
    assert np.isfinite(got).all() and (np.abs(got) <= 1).all()
    assert worst <= FACTOR * MEASURED_TANH_ULPS, (worst, at)


@pytest.mark.parametrize("route", list(ROUTES))
def test_sigmoid_per_element_over_the_whole_range(s3r, route):
    got = ROUTES[route](s3r, "sigmoid", VALS)
    want = A.ref64("sigmoid", VALS)
    assert np.isfinite(got).all() and (got >= 0).all() and (got <= 1).all(), VALS[~np.isfinite(got) | (got < 0) | (got > 1)][:8]
    tiny = want < A.FLT_MIN
    assert (got[tiny] <= A.FLT_MIN).all(), (VALS[tiny][got[tiny] > A.FLT_MIN][:8])
    shape = 1.0 + (1.0 - want) * np.abs(VALS.astype(np.float64))
    worst, at = _worst(got[~tiny], want[~tiny], VALS[~tiny], shape[~tiny])
    print(f"sigmoid ({route}): worst {worst:.3f} ulp / (1 + (1 - s) |v|) at v = {at!r}")
    assert worst <= FACTOR * MEASURED_SIGMOID_SHAPE, (worst, at)
