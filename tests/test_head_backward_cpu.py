"""s3r_head_backward without a GPU: the two declarations and their bindings, host-side validation (every refusal happens before
anything is launched: a HIP call would have given S3R_ERR_HIP on a host without a device), the scratch query, the numpy restatements
of tests/_head64.py against torch's own float64 autograd of conv3d + activation, the coverage condition on the device tests' shape
list, the mutants the cases must catch, and the Python surface's checks."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from tests import _head64 as R

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
    assert _args(header, "int64_t", "s3r_head_backward_scratch_elems") == ["int batch", "int channels", "int64_t voxels"]
    assert _args(header, "int", "s3r_head_backward") == [
        "const float* x", "const float* w", "const float* scale", "const float* y", "const float* grad_y", "float* grad_x",
        "float* grad_w", "float* grad_shift", "int batch", "int channels", "int64_t voxels", "int act", "float* scratch",
        "int64_t scratch_elems", "void* stream"]
    res, args = s3r._lib.SIGNATURES["s3r_head_backward_scratch_elems"]
    assert res is C.c_int64 and args == [C.c_int, C.c_int, C.c_int64]
    res, args = s3r._lib.SIGNATURES["s3r_head_backward"]
    assert res is C.c_int and args == [C.c_void_p] * 8 + [C.c_int, C.c_int, C.c_int64, C.c_int, C.c_void_p, C.c_int64, C.c_void_p]
    assert lib.s3r_head_backward.argtypes == args
    assert lib.s3r_abi_version() == 8
    names = {"head", "head_backward", "differentiable_head"}
    assert names <= set(s3r.__all__) and all(callable(getattr(s3r, n)) for n in names)
    assert all(callable(f) for f in (s3r.Decoder.features, s3r.Decoder.differentiable_head, s3r.Stereo2Voxel.head_features))
    flat = " ".join(header.replace("\n *", " ").split())
    linear = flat[flat.index("Backward of s3r_linear_forward's layer"):]
    rule = "none: g = grad_y; ReLU: g = (y > 0.f) ? grad_y : 0.f (a NaN y gives 0); sigmoid: t = 1 - y; u = y * t; g = grad_y * u, each operation rounded once, in this order."
    assert rule in linear and flat.count(rule) == 2               # the head backward copies the linear backward's rule word for word
    for sentence in ("chunks of 512 consecutive positions", "they are NOT fused", "in ascending b, starting from sample 0's",
                     "gs = g * scale, rounded once", "one multiplication (bit for bit)", "family 2, tag 1"):
        assert sentence in flat, sentence


# a non-NULL host address: validation rejects each case before anything could dereference it
_P = C.cast(C.create_string_buffer(64), C.c_void_p).value
_GOOD = dict(x=_P, w=_P, scale=_P, y=_P, gy=_P, gx=_P, gw=_P, gs=_P, batch=2, channels=16, voxels=24, act=2, scratch=_P, elems=1 << 40)
_BAD = {
    "all-outputs-null": (dict(gx=None, gw=None, gs=None), INVALID),
    "y-null-relu": (dict(y=None, act=1), INVALID), "y-null-sigmoid": (dict(y=None, act=2), INVALID),
    "act-3": (dict(act=3), INVALID), "act-negative": (dict(act=-1), INVALID), "act-6": (dict(act=6), INVALID),
    "null-grad_y": (dict(gy=None), INVALID), "null-x-with-grad_w": (dict(x=None), INVALID), "null-w-with-grad_x": (dict(w=None), INVALID),
    "batch-negative": (dict(batch=-1), INVALID), "channels-zero": (dict(channels=0), INVALID),
    "channels-negative": (dict(channels=-3), INVALID), "voxels-zero": (dict(voxels=0), INVALID), "voxels-negative": (dict(voxels=-1), INVALID),
    "4GiB-x": (dict(batch=32, channels=64, voxels=1 << 19), INVALID), "2^31-voxels": (dict(batch=1, channels=1, voxels=1 << 31), INVALID),
    "scratch-null": (dict(scratch=None), WORKSPACE), "scratch-zero": (dict(elems=0), WORKSPACE),
}
_FINE = {
    "x-null-without-grad_w": dict(x=None, gw=None), "w-null-without-grad_x": dict(w=None, gx=None), "y-null-act-none": dict(y=None, act=0),
    "scale-null": dict(scale=None),
}


def _call(lib, x, w, scale, y, gy, gx, gw, gs, batch, channels, voxels, act, scratch, elems):
    return lib.s3r_head_backward(x, w, scale, y, gy, gx, gw, gs, batch, channels, voxels, act, scratch, elems, None)


@pytest.mark.parametrize("case", list(_BAD), ids=list(_BAD))
def test_backward_rejects_bad_arguments_on_the_host(lib, case):
    change, code = _BAD[case]
    assert _call(lib, **dict(_GOOD, **change)) == code
    assert lib.s3r_last_error().decode()


@pytest.mark.parametrize("case", list(_FINE), ids=list(_FINE))
def test_allowed_null_forms_pass_validation(lib, case):
    """the allowed NULL forms get past every host check: with a short scratch they end in S3R_ERR_WORKSPACE, the LAST check, not in
    S3R_ERR_INVALID (nothing is launched either way)"""
    assert _call(lib, **dict(_GOOD, **_FINE[case], elems=1)) == WORKSPACE


def test_batch_zero_launches_nothing(lib):
    assert _call(lib, **dict(_GOOD, batch=0, scratch=None, elems=0)) == 0          # S3R_OK with no device: nothing was enqueued
    assert lib.s3r_head_backward_scratch_elems(0, 16, 24) == 0
    assert _call(lib, **dict(_GOOD, batch=0, gx=None, gw=None, gs=None)) == INVALID


def test_short_scratch_is_a_workspace_error(lib):
    for shape in ((2, 16, 24), (4, 64, 4096), (32, 64, 32768)):
        need = lib.s3r_head_backward_scratch_elems(*shape)
        b, c, s = shape
        assert need == (c + 1) * b * ((s + 511) // 512)            # the header's formula
        assert _call(lib, **dict(_GOOD, batch=b, channels=c, voxels=s, elems=need - 1)) == WORKSPACE
        assert b"s3r_head_backward_scratch_elems" in lib.s3r_last_error()
    assert _call(lib, **dict(_GOOD, gx=None, gw=None, gs=None)) == INVALID and b"grad_x" in lib.s3r_last_error()
    assert _call(lib, **dict(_GOOD, y=None)) == INVALID and b"y is NULL" in lib.s3r_last_error()


def test_scratch_query(lib):
    q = lib.s3r_head_backward_scratch_elems
    assert q(-1, 4, 4) == INVALID and q(4, 0, 4) == INVALID and q(4, 4, 0) == INVALID and q(32, 64, 1 << 19) == INVALID
    for c, s in ((1, 1), (3, 5), (64, 511), (64, 512), (64, 513), (64, 32768), (5, 65537)):
        sizes = [q(b, c, s) for b in range(0, 70)]
        assert sizes[0] == 0 and sizes[1] > 0 and all(a <= b for a, b in zip(sizes, sizes[1:])), (c, s)      # monotone in batch
        assert sizes[1] >= c + 1                                  # one chunk sum per channel and one for grad_shift at least


def test_python_layer_checks_before_the_device(s3r):
    x, w, b = torch.zeros(2, 5, 4, 4, 4), torch.zeros(1, 5, 1, 1, 1), torch.zeros(1)
    with pytest.raises(RuntimeError, match="HIP device"):         # no CPU fallback
        s3r.head(x, w, b)
    with pytest.raises(RuntimeError, match="HIP device"):
        s3r.head_backward(x, w, None, torch.zeros(2, 4, 4, 4), "none")
    with pytest.raises(RuntimeError, match="HIP device"):
        s3r.differentiable_head(x, w.requires_grad_(), b, "sigmoid")
    with pytest.raises(RuntimeError, match="act must be"):
        s3r.head(x, w, b, "tanh")
    with pytest.raises(RuntimeError, match="weight of 5 elements"):
        s3r.head(x, torch.zeros(6), b)


# ---------------------------------------------------------------- the restatements
def _case(B, C, n, seed, act):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, C, n, n, n, generator=g)
    w = torch.randn(C, generator=g) / C ** 0.5
    bias = torch.randn(1, generator=g)
    gy = torch.randn(B, n, n, n, generator=g)
    return x, w, bias, gy


def _rule64(y, gy, act):
    if act == "relu":
        return np.where(y > 0, gy, 0.0)
    if act == "sigmoid":
        return gy * (y * (1.0 - y))
    return gy.copy()


@pytest.mark.parametrize("scale", [None, 0.75], ids=["scale-null", "scale-0.75"])
@pytest.mark.parametrize("act", R.ACTS)
@pytest.mark.parametrize("shape", [(1, 1, 1), (2, 3, 5), (3, 17, 4), (2, 64, 9)], ids=lambda s: "x".join(map(str, s)))
def test_fp64_restatement_is_the_true_gradient(shape, act, scale):
    """backward64, the rule and gs * w against torch.autograd.grad of sum(grad_y * act(conv3d(x, w) * scale + bias)) in float64.  Both
    sides add the same K real terms per element in float64 in different orders: each within gamma_{K+1} sum|term| of the real value
    (2^-53 for 2^-24), hence within twice that of each other."""
    B, C, n = shape
    x, w, bias, gy = (t.double() for t in _case(B, C, n, seed=C * 100 + n, act=act))
    xd, wd, bd = x.clone().requires_grad_(), w.clone().requires_grad_(), bias.clone().requires_grad_()
    z = torch.nn.functional.conv3d(xd, wd.view(1, C, 1, 1, 1)).squeeze(1) * (1.0 if scale is None else scale) + bd
    y = {"none": z, "relu": torch.relu(z), "sigmoid": torch.sigmoid(z)}[act]
    want_x, want_w, want_b = torch.autograd.grad((gy * y).sum(), (xd, wd, bd))
    g = _rule64(y.detach().numpy(), gy.numpy(), act).reshape(B, -1)
    gs = g if scale is None else g * scale
    xf = x.numpy().reshape(B, C, -1)
    gw, gw_mag = np.einsum("bs,bcs->c", gs, xf), np.einsum("bs,bcs->c", np.abs(gs), np.abs(xf))
    K = g.size
    lim = lambda k, mag: 2 * (k + 1) * R.EPS64 / (1 - (k + 1) * R.EPS64) * mag
    assert (np.abs(gw - want_w.numpy()) <= lim(K, gw_mag)).all()
    assert abs(g.sum() - want_b.item()) <= lim(K, np.abs(g).sum())
    gx = gs[:, None, :] * w.numpy()[None, :, None]
    assert (np.abs(gx - want_x.numpy().reshape(B, C, -1)) <= lim(1, np.abs(gx))).all()
    # ... and backward64 is that computation on fp32 inputs
    (gw2, k2, m2), (gb2, k3, m3) = R.backward64(xf.astype(np.float32), gs.astype(np.float32), g.astype(np.float32))
    assert k2 == K and k3 == K and gw2.shape == (C,) and np.allclose(gw2, gw, rtol=1e-5, atol=1e-5 * max(gw_mag.max(), 1e-30))


@pytest.mark.parametrize("shape", [(2, 3, 5), (3, 5, 255), (2, 7, 511), (2, 5, 512), (3, 4, 513), (5, 3, 1025)], ids=lambda s: "x".join(map(str, s)))
def test_fp32_order_against_a_scalar_loop_and_float64(shape):
    """grad_w32 / grad_shift32 against a scalar restatement of the header's sentences (bit for bit) and within bound32 of float64"""
    B, C, S = shape
    g = torch.Generator().manual_seed(sum(shape))
    x, gsv = torch.randn(B, C, S, generator=g).numpy(), torch.randn(B, S, generator=g).numpy()
    f = np.float32

    def scalar(terms):                                            # terms (B, S)
        acc = None
        for b in range(B):
            part = None
            for k in range((S + 511) // 512):
                lanes = []
                for lane in range(64):
                    p = f(0)
                    for j in range(2):
                        for i in range(4):
                            s = 512 * k + 256 * j + 4 * lane + i
                            if s < S:
                                p = f(p + terms[b, s])
                    lanes.append(p)
                o = 32
                while o:
                    lanes = [f(lanes[l] + lanes[l + o]) for l in range(o)]
                    o //= 2
                part = lanes[0] if part is None else f(part + lanes[0])
            acc = part if acc is None else f(acc + part)
        return acc

    got_w, got_s = R.grad_w32(gsv, x), R.grad_shift32(gsv)
    c = C - 1
    assert R.bits(got_w[c:c + 1])[0] == R.bits(scalar((gsv * x[:, c, :]).astype(f)))[()]
    assert R.bits(got_s)[()] == R.bits(scalar(gsv))[()]
    (gw, K, mw), (gb, _, mb) = R.backward64(x, gsv, gsv)
    assert (np.abs(got_w - gw) <= R.bound32(K, mw)).all() and abs(float(got_s) - gb) <= R.bound32(K, mb)


# ---------------------------------------------------------------- coverage conditions and mutants
def test_shape_list_contains_every_boundary_of_the_order():
    sizes = {s for _, _, s in R.SHAPES}
    assert set(R.boundaries()) <= sizes, sorted(set(R.boundaries()) - sizes)
    issue = [(1, 1, 1), (1, 1, 4), (2, 3, 5), (1, 64, 256), (2, 64, 257), (3, 17, 1023), (2, 64, 4096), (33, 2, 64), (1, 5, 65537), (2, 64, 32768)]
    assert R.SHAPES[:len(issue)] == issue
    assert any(b == 1 for b, _, _ in R.SHAPES) and any(b > 64 for b, _, _ in R.SHAPES)      # B = 1, and more samples than one wave's lanes
    assert any(b > 1 and s % 4 for b, _, s in R.SHAPES)           # rows that start only 4-byte aligned


def test_mutants_are_caught_by_the_cases():
    """another batch order, or a forgotten scale, gives other bits on the random data of the listed shapes"""
    seen = {"descending": False, "pairwise": False}
    for B, C, S in R.SHAPES:
        if B < 3 or B * C * S > 1 << 18:
            continue
        g = torch.Generator().manual_seed(B + C + S)
        x, gv = torch.randn(B, C, S, generator=g).numpy(), torch.randn(B, S, generator=g).numpy()
        want = R.grad_w32(gv, x)
        for m in seen:
            seen[m] |= bool((R.bits(R.grad_w32(gv, x, batch_order=m)) != R.bits(want)).any())
            seen[m] |= bool(R.bits(R.grad_shift32(gv, batch_order=m)) != R.bits(R.grad_shift32(gv)))
    assert all(seen.values()), seen
    gv = torch.randn(2, 40, generator=torch.Generator().manual_seed(1)).numpy()
    w = np.array([1.5, -0.3], np.float32)
    assert (R.bits(R.grad_x32(R.gs32(gv, 0.75), w)) != R.bits(R.grad_x32(R.gs32(gv, None), w))).any()       # a missing scale
    # gs is rounded BEFORE the multiplication by w: (g * scale) * w, not g * (scale * w)
    other = (gv[:, None, :] * (np.float32(0.75) * w).astype(np.float32)[None, :, None]).astype(np.float32)
    assert (R.bits(R.grad_x32(R.gs32(gv, 0.75), w)) != R.bits(other)).any()
    # grad_shift sums g, not gs
    assert R.bits(R.grad_shift32(gv)) != R.bits(R.grad_shift32(R.gs32(gv, 0.75)))
