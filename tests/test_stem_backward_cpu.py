"""s3r_stem_backward without a device: tests/_stem64.py's restatement against torch's float64 autograd of conv2d + affine + ReLU, the
8-bit scaling against float32(u) / float32(255), the scratch query, every refusal of the header (all are host-side: nothing is enqueued,
so they run without a GPU), the prototypes against s3r._lib.SIGNATURES, and the order mutants on the device table's data."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from tests import _convbwd64 as R
from tests import _stem64 as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID, WORKSPACE = -1, -3


@pytest.fixture(scope="module")
def lib(s3r):
    return s3r.load_library()


def test_prototypes_match_the_ctypes_table(s3r):
    header = open(os.path.join(ROOT, "include", "s3r.h")).read()
    proto = re.search(r"int s3r_stem_backward\((.*?)\);", header, re.S).group(1)
    args = [a.strip() for a in proto.split(",")]
    assert len(args) == 15 and args[-1] == "void* hip_stream"
    res, argtypes = s3r._lib.SIGNATURES["s3r_stem_backward"]
    assert res is C.c_int and len(argtypes) == 15
    q = re.search(r"int64_t s3r_stem_backward_scratch_elems\((.*?)\);", header, re.S).group(1)
    assert [a.strip() for a in q.split(",")] == ["int n_images", "int in_size"]
    assert s3r._lib.SIGNATURES["s3r_stem_backward_scratch_elems"] == (C.c_int64, [C.c_int, C.c_int])
    assert "stem_backward" in s3r.__all__ and callable(s3r.stem_backward)


@pytest.mark.parametrize("case", [c for c in S.CASES if c[1] <= 64], ids=S.case_id)
@pytest.mark.parametrize("act", S.ACTS)
def test_restatement_against_torch_float64_autograd(case, act):
    """grad_w64 and the float64 sum of g against torch's autograd of sum(grad_y * act(conv2d(X, w) * scale + shift)) with respect to w and
    shift, X = the host conversion of the 8-bit renders; the gates are taken from float64's own y"""
    n, s = case
    g = torch.Generator().manual_seed(3 + s)
    x, scale, _, gy = S.make(n, s, seed=9, act=act, u8=True)
    x64 = torch.from_numpy(S.render32(x)).double()
    w = (torch.randn((32, 3, 3, 3), generator=g) / 27 ** 0.5).double().requires_grad_()
    sh = (0.1 * torch.randn(32, generator=g)).double().requires_grad_()
    z = torch.nn.functional.conv2d(x64, w, None, 2, 1) * torch.from_numpy(scale).double().view(1, -1, 1, 1) + sh.view(1, -1, 1, 1)
    y = torch.relu(z) if act == "relu" else z
    want_w, want_b = torch.autograd.grad((torch.from_numpy(gy).double() * y).sum(), (w, sh))
    g32 = S.g32(None if act == "none" else y.detach().float().numpy(), gy, act)
    gs = g32.astype(np.float64) * scale.astype(np.float64).reshape(1, -1, 1, 1)      # (unrounded: the identity is about the formula)
    ref, K, mag = R.grad_w64(S.conv_case(n, s), S.render32(x), gs)
    assert np.allclose(ref, want_w.numpy(), rtol=1e-10, atol=1e-12)
    assert np.allclose(g32.astype(np.float64).sum(axis=(0, 2, 3)), want_b.numpy(), rtol=1e-10, atol=1e-12)
    ref32, K32, _ = S.grad_w64(S.render32(x), S.gs32(g32, scale))
    assert K32 == n * S.out_edge(s) ** 2 and ref32.shape == (32, 3, 3, 3)


def test_u8_scaling_is_the_correctly_rounded_quotient():
    from fractions import Fraction
    u = np.arange(256, dtype=np.uint8)
    got = S.render32(u)
    for v, q in zip(u.tolist(), got.tolist()):
        exact = Fraction(v, 255)
        lo, hi = np.nextafter(np.float32(q), np.float32(-1)), np.nextafter(np.float32(q), np.float32(2))
        assert abs(Fraction(float(q)) - exact) <= min(abs(Fraction(float(lo)) - exact), abs(Fraction(float(hi)) - exact))
    assert got.dtype == np.float32 and got[0] == 0 and got[255] == 1


def test_scratch_query_is_device_free_monotone_and_zero_for_no_image(lib):
    for s in sorted({c[1] for c in S.CASES} | {3, 63, 65, 127, 129}):
        assert lib.s3r_stem_backward_scratch_elems(0, s) == 0
        last = 0
        for n in (1, 2, 3, 64, 65, 70):
            got = lib.s3r_stem_backward_scratch_elems(n, s)
            assert got == S.scratch_elems(n, s) and got >= last
            last = got
    assert S.slices(112) == (4, 28) and S.slices(65) == (3, 22) and S.slices(1) == (1, 1)
    assert lib.s3r_stem_backward_scratch_elems(1, 0) == INVALID and lib.s3r_stem_backward_scratch_elems(-1, 8) == INVALID
    assert lib.s3r_stem_backward_scratch_elems(2 ** 20, 224) == INVALID      # y of 2^31 elements or more


def _call(lib, **kv):
    """a call on FAKE but aligned addresses: every refusal comes before anything is enqueued or dereferenced"""
    a = dict(left=0x10000, right=0x20000, n_left=2, u8=0, y=0x30000, gy=0x40000, scale=0x50000, gw=0x60000, gb=0x70000, n=3, in_size=7,
             act=1, scr=0x80000, elems=1 << 40)
    a.update(kv)
    return lib.s3r_stem_backward(a["left"], a["right"], a["n_left"], a["u8"], a["y"], a["gy"], a["scale"], a["gw"], a["gb"], a["n"],
                                 a["in_size"], a["act"], a["scr"], a["elems"], None)


REFUSALS = [
    (dict(gw=None, gb=None), INVALID, "both NULL"), (dict(gy=None), INVALID, "null"), (dict(left=None), INVALID, "null"),
    (dict(y=None), INVALID, "y is NULL"), (dict(act=2), INVALID, "none / relu"), (dict(act=-1), INVALID, "none / relu"),
    (dict(n_left=0), INVALID, "n_left"), (dict(n_left=4), INVALID, "n_left"), (dict(right=None), INVALID, "n_left"),
    (dict(right=None, n_left=2, n=3), INVALID, "n_left"), (dict(in_size=0), INVALID, "in_size"), (dict(n=-1), INVALID, "n_images"),
    (dict(left=0x10004), INVALID, "16-byte aligned"), (dict(right=0x20008), INVALID, "16-byte aligned"),
    (dict(left=0x10001, u8=1), INVALID, "16-byte aligned"),
    (dict(n=2 ** 20, n_left=1, in_size=224), INVALID, "2^31"),                      # y of 2^31 elements or more
    (dict(n=700, n_left=1, in_size=1024, u8=0), INVALID, "2^31"),                   # 699 fp32 renders of 1024^2: 2.2e9 elements
    (dict(scr=None), WORKSPACE, "scratch"), (dict(elems=S.scratch_elems(3, 7) - 1), WORKSPACE, "scratch"),
]


@pytest.mark.parametrize("i", range(len(REFUSALS)))
def test_refusals_are_host_side(lib, i):
    kv, code, word = REFUSALS[i]
    assert _call(lib, **kv) == code
    assert word in lib.s3r_last_error().decode(), lib.s3r_last_error()


def test_what_is_allowed_is_not_refused(lib):
    """n_images == 0 returns S3R_OK before any pointer matters; the same fake call with act none and y NULL passes every check up to the
    scratch (refused only there, with a short one)"""
    assert _call(lib, n=0, n_left=0, left=None, right=None, gy=None, scr=None, elems=0) == 0
    assert _call(lib, act=0, y=None, scale=None, elems=0) == WORKSPACE
    assert _call(lib, right=None, n_left=3, gb=None, elems=0) == WORKSPACE
    assert _call(lib, n_left=3, elems=0) == WORKSPACE                               # (two tensors, the second one empty)


@pytest.mark.parametrize("case", [(5, 20), (3, 64), (70, 4)], ids=S.case_id)
def test_order_mutants_move_the_result_on_the_device_tables_data(case):
    """the device test's data tell the orders apart: the image order reversed changes bits of grad_shift and of the slice-ordered
    grad_w; the slice order reversed changes bits of grad_w (where an image has more than two slices)"""
    n, s = case
    x, scale, y, gy = S.make(n, s, seed=17 * s + n + 2, act="relu", u8=True)
    g = S.g32(y, gy, "relu")
    assert (S.bits(S.grad_shift32(g)) != S.bits(S.grad_shift32(g, "descending"))).any()
    if n > 2:
        assert (S.bits(S.grad_shift32(g)) != S.bits(S.grad_shift32(g, "pairwise"))).any()
    gs, x32 = S.gs32(g, scale), S.render32(x)
    base = S.grad_w_ordered32(x32, gs)
    ref, K, mag = S.grad_w64(x32, gs)
    assert (np.abs(base.astype(np.float64) - ref) <= S.bound32(K, mag)).all()
    assert (S.bits(base) != S.bits(S.grad_w_ordered32(x32, gs, image_order="descending"))).any()
    if S.slices(S.out_edge(s))[1] > 2:
        assert (S.bits(base) != S.bits(S.grad_w_ordered32(x32, gs, slice_order="descending"))).any()
