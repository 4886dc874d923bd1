"""Disparity supervision without a GPU: the three C-ABI declarations and bindings, every refusal on the host with a message (a HIP call
would have given S3R_ERR_HIP on a host without a device), batch 0, and the restatements the GPU tests measure against
(tests/_dispbwd64.py): the float64 one against torch's float64 autograd of a plain formulation, the fp32 one within the derived bound
of it, the mutants of the order on the equal-cost case, and the loss on hand-computed cases."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from tests import _disp64 as D64
from tests import _dispbwd64 as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = -1
F32, BF16 = 0, 1
ENTRIES = ("s3r_disparity_soft_backward", "s3r_disparity_loss_forward", "s3r_disparity_loss_backward")


@pytest.fixture(scope="module")
def lib(s3r):
    import __graft_entry__ as g
    if not os.path.exists(s3r.LIB_PATH):
        g.build()
    return s3r.load_library()


def _prototype(name):
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "s3r.h")).read(), flags=re.S)
    m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", header)
    assert m, f"{name} is not declared in include/s3r.h"
    return [" ".join(a.split()) for a in m.group(1).split(",")]


def test_header_declares_the_three_entries():
    assert _prototype("s3r_disparity_soft_backward") == [
        "const void* feat_l", "const void* feat_r", "int feat_dtype", "const float* grad_disp_l", "const float* grad_disp_r",
        "float* grad_left", "float* grad_right", "int batch", "int channels", "int height", "int width", "int max_disp",
        "float temperature", "int out_height", "int out_width", "float disp_scale", "void* hip_stream"]
    assert _prototype("s3r_disparity_loss_forward") == [
        "const float* pred", "const float* gt", "float beta", "float* loss_sum", "int32_t* count", "float* loss_elem", "int batch",
        "int64_t pixels", "void* hip_stream"]
    assert _prototype("s3r_disparity_loss_backward") == [
        "const float* pred", "const float* gt", "const float* grad_scale", "float beta", "float* grad_pred", "int batch",
        "int64_t pixels", "void* hip_stream"]
    header = open(os.path.join(ROOT, "include", "s3r.h")).read()
    assert "#define S3R_ABI_VERSION 8" in header                  # additive entry points: no version step
    for name in ENTRIES:                                          # each has a header comment that states order, NaN rule and stream
        at = header.index(f"int {name}(")
        comment = header[header[:at].rfind("/*"):at]
        for word in ("hip_stream", "hipStream_t", "propagates through", "Profiler", "family 9", "NULL", "Nothing is enqueued"):
            assert word in comment, (name, word)


def test_lib_binds_the_three_entries(s3r, lib):
    sig = s3r._lib.SIGNATURES
    res, args = sig["s3r_disparity_soft_backward"]
    assert res is C.c_int and len(args) == 17 and args[2] is C.c_int and args[12] is C.c_float and args[15] is C.c_float
    assert [a is C.c_int for a in args[7:12]] == [True] * 5 and args[13] is C.c_int and args[14] is C.c_int
    res, args = sig["s3r_disparity_loss_forward"]
    assert res is C.c_int and len(args) == 9 and args[2] is C.c_float and args[6] is C.c_int and args[7] is C.c_int64
    res, args = sig["s3r_disparity_loss_backward"]
    assert res is C.c_int and len(args) == 8 and args[3] is C.c_float and args[5] is C.c_int and args[6] is C.c_int64
    for name in ENTRIES:
        assert getattr(lib, name).argtypes == sig[name][1]
    assert lib.s3r_abi_version() == 8


# a non-NULL host address: validation rejects each case before anything could dereference it
_P = C.cast(C.create_string_buffer(64), C.c_void_p).value
_GOOD = dict(dtype=F32, batch=2, c=32, h=28, w=28, d=28, tau=1.0, oh=224, ow=224, scale=8.0)
_SOFT_BAD = {          # tests/test_disparity_soft_cpu.py's table: what the forward refuses, the backward refuses
    "temperature-zero": dict(tau=0.0),
    "temperature-negative": dict(tau=-1.0),
    "temperature-nan": dict(tau=float("nan")),
    "temperature-inf": dict(tau=float("inf")),
    "max-disp-zero": dict(d=0),
    "channels-zero": dict(c=0),
    "height-negative": dict(h=-1),
    "width-zero": dict(w=0),
    "out-height-zero": dict(oh=0),
    "out-width-negative": dict(ow=-3),
    "batch-negative": dict(batch=-1),
    "unknown-dtype": dict(dtype=7),
    "bf16-channels-not-multiple-of-8": dict(dtype=BF16, c=12),
    "lds-too-large": dict(c=64, w=200, d=4),
    "features-2^31-elements": dict(batch=4096, c=32, h=128, w=128, d=4),
    "output-2^31-elements": dict(batch=2, oh=32768, ow=32768),
    # ... and what only the backward refuses
    "bf16": dict(dtype=BF16),
    "batch-x-height-2^24": dict(batch=1 << 14, c=1, h=1 << 10, w=2, d=1, oh=1, ow=1),
}


def _bwd(lib, dtype, batch, c, h, w, d, tau, oh, ow, scale, grads=(_P, _P), outs=(_P, _P), feats=(_P, _P)):
    return lib.s3r_disparity_soft_backward(*feats, dtype, *grads, *outs, batch, c, h, w, d, tau, oh, ow, scale, None)


@pytest.mark.parametrize("case", list(_SOFT_BAD), ids=list(_SOFT_BAD))
def test_backward_rejects_bad_arguments_on_the_host(lib, case):
    assert _bwd(lib, **dict(_GOOD, **_SOFT_BAD[case])) == INVALID
    msg = lib.s3r_last_error().decode()
    assert msg
    if case == "bf16":
        assert "bf16" in msg
    if case in ("lds-too-large", "temperature-nan", "output-2^31-elements"):      # the forward's own words
        lib.s3r_disparity_soft(_P, _P, F32, _P, _P, None, None, *[dict(_GOOD, **_SOFT_BAD[case])[k] for k in
                                                                 ("batch", "c", "h", "w", "d", "tau", "oh", "ow", "scale")], None)
        assert lib.s3r_last_error().decode() == msg


def test_backward_null_forms_on_the_host(lib):
    assert _bwd(lib, **_GOOD, grads=(None, None)) == INVALID and "grad_disp" in lib.s3r_last_error().decode()
    assert _bwd(lib, **_GOOD, outs=(None, None)) == INVALID and "grad_left" in lib.s3r_last_error().decode()
    assert _bwd(lib, **_GOOD, feats=(None, _P)) == INVALID and lib.s3r_last_error().decode()
    # batch 0 launches nothing: OK with either NULL form that is allowed, and without features
    zero = dict(_GOOD, batch=0)
    assert _bwd(lib, **zero) == 0
    assert _bwd(lib, **zero, grads=(None, _P), outs=(_P, None), feats=(None, None)) == 0
    assert _bwd(lib, **zero, grads=(None, None)) == INVALID       # (the NULL rule does not depend on the batch)


def test_backward_lds_rule_is_the_forwards(lib):
    def need(c, w, d):
        return 4 * (2 * c * w + 2 * w * min(d, w) + 12 * w)
    ok, bad = (258, 28, 28), (259, 28, 28)
    assert need(*ok) <= 65536 < need(*bad)
    assert _bwd(lib, F32, 0, ok[0], 4, ok[1], ok[2], 1.0, 8, 8, 1.0) == 0
    assert _bwd(lib, F32, 0, bad[0], 4, bad[1], bad[2], 1.0, 8, 8, 1.0) == INVALID
    assert "64 KiB" in lib.s3r_last_error().decode()


_LOSS_BAD = {
    "beta-negative": dict(beta=-0.5), "beta-nan": dict(beta=float("nan")), "beta-inf": dict(beta=float("inf")),
    "batch-negative": dict(batch=-1), "pixels-zero": dict(pixels=0), "pixels-negative": dict(pixels=-4),
    "sample-2^31-elements": dict(batch=1, pixels=1 << 31), "tensor-2^31-elements": dict(batch=4, pixels=1 << 29),
    "null-pred": dict(pred=None), "null-gt": dict(gt=None),
}


@pytest.mark.parametrize("case", list(_LOSS_BAD) + ["null-loss_sum", "null-count"])
def test_loss_forward_rejects_bad_arguments_on_the_host(lib, case):
    a = dict(pred=_P, gt=_P, beta=1.0, loss_sum=_P, count=_P, batch=2, pixels=64)
    a.update(_LOSS_BAD.get(case, {}))
    if case.startswith("null-l") or case == "null-count":
        a[case[5:]] = None
    assert lib.s3r_disparity_loss_forward(a["pred"], a["gt"], a["beta"], a["loss_sum"], a["count"], None, a["batch"], a["pixels"],
                                          None) == INVALID
    assert lib.s3r_last_error().decode()


@pytest.mark.parametrize("case", list(_LOSS_BAD) + ["null-grad_scale", "null-grad_pred"])
def test_loss_backward_rejects_bad_arguments_on_the_host(lib, case):
    a = dict(pred=_P, gt=_P, beta=1.0, grad_scale=_P, grad_pred=_P, batch=2, pixels=64)
    a.update(_LOSS_BAD.get(case, {}))
    if case.startswith("null-grad"):
        a[case[5:]] = None
    assert lib.s3r_disparity_loss_backward(a["pred"], a["gt"], a["grad_scale"], a["beta"], a["grad_pred"], a["batch"], a["pixels"],
                                           None) == INVALID
    assert lib.s3r_last_error().decode()


def test_loss_batch_zero_returns_ok(lib):
    assert lib.s3r_disparity_loss_forward(None, None, 1.0, None, None, None, 0, 16, None) == 0
    assert lib.s3r_disparity_loss_backward(None, None, None, 0.0, None, 0, 16, None) == 0
    assert lib.s3r_disparity_loss_forward(None, None, -1.0, None, None, None, 0, 16, None) == INVALID


def test_python_layer_refusals_before_the_device(s3r):
    f32, bf = torch.zeros(1, 8, 4, 4), torch.zeros(1, 8, 4, 4, dtype=torch.bfloat16)
    with pytest.raises(RuntimeError, match="float32"):
        s3r.differentiable_disparity_soft(bf, bf, 4, 1.0)
    with pytest.raises(RuntimeError, match="one shape"):
        s3r.differentiable_disparity_soft(f32, f32[:, :4], 4, 1.0)
    with pytest.raises(RuntimeError, match="need_left or need_right"):
        s3r.disparity_soft_backward(f32, f32, f32[:, 0], None, 4, 1.0, need_left=False, need_right=False)
    with pytest.raises(RuntimeError, match="grad_disp_l or grad_disp_r"):
        s3r.disparity_soft_backward(f32, f32, None, None, 4, 1.0)
    with pytest.raises(ValueError, match="beta"):
        s3r.DisparityLoss(beta=-1.0)
    with pytest.raises(ValueError, match="beta"):
        s3r.DisparityLoss(beta=float("nan"))
    with pytest.raises(RuntimeError, match="one shape"):
        s3r.disparity_loss(torch.zeros(2, 4), torch.zeros(2, 5))
    with pytest.raises(RuntimeError, match="forward/inference path only"):
        s3r.Stereo2Voxel().train()                                 # .train() stays refused
    assert s3r.DisparityLoss().beta == 1.0


# ---------------------------------------------------------------- the restatements
def _torch64(fl, fr, gdl, gdr, D, tau, out_size, scale):
    """torch's float64 autograd of the plain formulation: costs via abs, a min-shifted softmax, the bilinear blend as an explicit matrix
    built from tests/_disp64's fp32 index rule (F.interpolate on float64 forms its indices in float64 and may pick another neighbour)"""
    L = torch.tensor(np.asarray(fl, np.float64), requires_grad=True)
    Rt = torch.tensor(np.asarray(fr, np.float64), requires_grad=True)
    B, Cc, H, W = L.shape
    tau = float(np.float32(tau))
    loss = 0.0
    for right, g in ((False, gdl), (True, gdr)):
        disp = torch.zeros(B, H, W, dtype=torch.float64)
        cols = []
        for w in range(W):
            n = min(D, (W - w) if right else (w + 1))
            a = (Rt if right else L)[:, :, :, w]
            c = torch.stack([(a - (L[:, :, :, w + d] if right else Rt[:, :, :, w - d])).abs().sum(1) for d in range(n)], -1)
            p = torch.softmax((c.min(-1, keepdim=True).values.detach() - c) / tau, -1)
            cols.append((p * torch.arange(n, dtype=torch.float64)).sum(-1))
        disp = torch.stack(cols, -1)
        if out_size is not None:
            wy, wx = torch.tensor(R.weights64(H, out_size[0])), torch.tensor(R.weights64(W, out_size[1]))
            disp = torch.einsum("oh,bhw,pw->bop", wy, disp, wx)
        loss = loss + (disp * float(np.float32(scale)) * torch.tensor(np.asarray(g, np.float64))).sum()
    loss.backward()
    return L.grad.numpy(), Rt.grad.numpy()


@pytest.mark.parametrize("sizes", [(28, 28, 224, 224), (7, 13, 37, 100), (12, 40, 5, 17), (3, 5, 7, 12)], ids=lambda s: "x".join(map(str, s)))
def test_weight_matrix_is_disp64s_bilinear(sizes):
    h, w, oh, ow = sizes
    x = np.random.default_rng(h * w).random((2, h, w))
    want = D64.bilinear(x, oh, ow)
    got = np.einsum("oh,bhw,pw->bop", R.weights64(h, oh), x, R.weights64(w, ow))
    assert np.abs(got - want).max() <= 1e-15
    assert np.abs(R.weights32(h, oh) - R.weights64(h, oh)).max() <= 2.0 ** -23


@pytest.mark.parametrize("case", R.CASES, ids=R.case_id)
def test_float64_restatement_is_torch_float64_autograd(case):
    B, Cc, H, W, D, OH, OW = case
    fl, fr, gdl, gdr = R.random_case(case)
    tau, scale = 0.7, 2.5
    (gl, gr), _ = R.backward64(fl, fr, gdl, gdr, D, tau, R.out_size(case), scale)
    wl, wr = _torch64(fl, fr, gdl, gdr, D, tau, R.out_size(case), scale)
    for got, want in ((gl, wl), (gr, wr)):
        assert np.abs(got - want).max() <= 1e-12 * max(np.abs(want).max(), 1.0)
    if W == 1:
        assert not gl.any() and not gr.any()                       # one disparity: the read-out is the constant 0
    else:
        assert np.abs(wl).max() > 0 and np.abs(wr).max() > 0


@pytest.mark.parametrize("tau", [0.7, 0.05])
@pytest.mark.parametrize("case", R.CASES, ids=R.case_id)
def test_fp32_restatement_is_within_the_derived_bound(case, tau):
    B, Cc, H, W, D, OH, OW = case
    fl, fr, gdl, gdr = R.random_case(case)
    (gl64, gr64), (bl, br) = R.backward64(fl, fr, gdl, gdr, D, tau, R.out_size(case), 8.0)
    gl, gr = R.backward32(fl, fr, gdl, gdr, D, tau, R.out_size(case), 8.0)
    worst = max((np.abs(gl - gl64) / bl).max(), (np.abs(gr - gr64) / br).max())
    print(f"{R.case_id(case)} tau {tau}: largest error / bound {worst:.3e}")
    assert worst <= 1.0
    # the bound is a rounding bound, not a tolerance: small against the gradients it guards
    assert bl.max() <= 1e-2 * max(np.abs(gl64).max(), 1e-30) or not gl64.any()
    # a NULL gradient is a tensor of zeros
    for a, b in zip(R.backward32(fl, fr, None, gdr, D, tau, R.out_size(case), 8.0),
                    R.backward32(fl, fr, np.zeros_like(gdl), gdr, D, tau, R.out_size(case), 8.0)):
        assert np.array_equal(a, b)


@pytest.mark.parametrize("case", [R.CASES[0], R.CASES[1], R.UPSAMPLED], ids=R.case_id)
def test_equal_costs_are_exact_and_the_mutants_fail(case):
    """the equal-cost case: every weight is exp(0) = 1, so the fp32 restatement is defined bit for bit; it agrees with float64 within the
    bound, the channel with equal features gets exactly 0, and each mutant of the order changes values"""
    B, Cc, H, W, D, OH, OW = case
    fl, fr, gdl, gdr = R.equal_cost_case(case)
    for right in (False, True):
        c = D64.costs(fl, fr, D, right)
        fin = np.isfinite(c)
        assert all(np.unique(c[b][fin[b]]).size == 1 for b in range(B))
    args = (fl, fr, gdl, gdr, D, 0.3, R.out_size(case), 8.0)
    want = R.backward32(*args)
    (gl64, gr64), (bl, br) = R.backward64(*args)
    assert (np.abs(want[0] - gl64) <= bl).all() and (np.abs(want[1] - gr64) <= br).all()
    assert not want[0][:, Cc // 2].any() and not want[1][:, Cc // 2].any() and np.abs(want[0]).max() > 0
    for mutant in ("descending", "from-zero-subtracting", "q-separately"):
        got = R.backward32(*args, order=mutant)
        assert not (np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])), mutant


# ---------------------------------------------------------------- the loss
def test_loss_hand_computed_case():
    inf, nan = float("inf"), float("nan")
    gt = np.array([[10, 10, 10, 10, 0, inf, nan, -1, 4, 4]], np.float32)
    pred = np.array([[10.5, 9.5, 12, 7, 1, 3, 3, nan, nan, 6]], np.float32)
    # beta = 2: e = .5, -.5 (quadratic: .0625), 2 (|e| == beta: linear, 1), -3 (2), 1 (.25); inf, NaN, -1 invalid; NaN pred at a valid pixel
    l, ok = R.loss32(pred, gt, 2.0)
    assert ok.tolist() == [[True, True, True, True, True, False, False, False, True, True]]
    assert l[0, :8].tolist() == [0.0625, 0.0625, 1.0, 2.0, 0.25, 0.0, 0.0, 0.0] and np.isnan(l[0, 8]) and l[0, 9] == 1.0
    assert not np.signbit(l[0, 5:8]).any()
    g = R.loss_grad32(pred, gt, [2.0], 2.0)
    assert g[0, :8].tolist() == [0.5, -0.5, 2.0, -2.0, 1.0, 0.0, 0.0, 0.0] and np.isnan(g[0, 8]) and g[0, 9] == 2.0
    # beta = 0: plain L1 and sgn
    l0, _ = R.loss32(pred, gt, 0.0)
    assert l0[0, :8].tolist() == [0.5, 0.5, 2.0, 3.0, 1.0, 0.0, 0.0, 0.0] and np.isnan(l0[0, 8])
    g0 = R.loss_grad32(np.array([[10.5, 9.5, 10, 7]], np.float32), gt[:, :4], [3.0], 0.0)
    assert g0.tolist() == [[3.0, -3.0, 0.0, -3.0]]
    # the branches meet at |e| == beta: the quadratic branch would give the same value there
    assert R.loss32(np.float32([[3]]), np.float32([[1]]), 2.0)[0][0, 0] == 0.5 * 2 * 2 / 2 == 2 - 0.5 * 2
    # against torch's smooth_l1_loss on the valid pixels (fp32, elementwise)
    rng = np.random.default_rng(0)
    p, t = rng.standard_normal((3, 50)).astype(np.float32) * 3, np.abs(rng.standard_normal((3, 50))).astype(np.float32)
    for beta in (0.0, 0.5, 1.0):
        want = torch.nn.functional.smooth_l1_loss(torch.from_numpy(p), torch.from_numpy(t), beta=beta, reduction="none").numpy()
        assert np.abs(R.loss32(p, t, beta)[0] - want).max() <= 4e-7 * np.abs(want).max()


def test_loss_sum_order_restatement():
    rng = np.random.default_rng(1)
    for P in (1, 1023, 1024, 1025, 5000):
        x = rng.random((2, P)).astype(np.float32)
        s = R.loss_sum32(x)
        assert np.abs(s - x.astype(np.float64).sum(1)).max() <= P * 2.0 ** -24 * x.astype(np.float64).sum(1).max()
    x = np.ones((1, 2048 + 7), np.float32)
    assert R.loss_sum32(x)[0] == 2055.0
    from tests import _bce64                                      # the same order as the BCE restatement's
    y = rng.random((2, 3001)).astype(np.float32)
    assert np.array_equal(R.loss_sum32(y), np.array([_bce64.sum_order32(y[b]) for b in range(2)], np.float32))
