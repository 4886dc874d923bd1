"""s3r_voxel_bce_forward / s3r_voxel_bce_backward without a GPU: the declarations and their bindings, host-side validation (every
refusal happens before anything is launched: a HIP call would have given S3R_ERR_HIP on a host without a device), the numpy
restatements of tests/_bce64.py against torch's own float64 BCELoss and its autograd (the -100 and 1e-12 clamps included), the coverage
condition on the device tests' shape list, the mutants the planted cases must catch, and the module surface's refusals."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from tests import _bce64 as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = -1


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
    assert _args(header, "int", "s3r_voxel_bce_forward") == [
        "const float* pred", "const float* target", "float* loss_sum", "float* loss_elem", "int batch", "int64_t voxels", "void* stream"]
    assert _args(header, "int", "s3r_voxel_bce_backward") == [
        "const float* pred", "const float* target", "const float* grad_scale", "float* grad_pred", "int batch", "int64_t voxels",
        "void* stream"]
    for name in ("s3r_voxel_bce_forward", "s3r_voxel_bce_backward"):
        res, args = s3r._lib.SIGNATURES[name]
        assert res is C.c_int and args == [C.c_void_p] * 4 + [C.c_int, C.c_int64, C.c_void_p]
        assert getattr(lib, name).argtypes == args
    assert lib.s3r_abi_version() == 8
    names = {"VoxelBCELoss", "voxel_bce", "voxel_bce_backward", "differentiable_voxel_bce"}
    assert names <= set(s3r.__all__) and all(callable(getattr(s3r, n)) for n in names)
    # the header pins the rules the device tests quote
    flat = " ".join(header.replace("\n *", " ").split())
    for sentence in ("clamp(v) = (v < -100.f) ? -100.f : v", "The clamp comes BEFORE the multiplication", "a NaN passes through it",
                     "chunks of 1024 consecutive elements", "o = 32, 16, 8, 4, 2, 1", "torch.nn.BCELoss raises",
                     "d = max((1.f - p) * p, 1e-12f)", "family 6, tag 1", "family 6, tag 2"):
        assert sentence in flat, sentence


# a non-NULL host address: validation rejects each case before anything could dereference it
_P = C.cast(C.create_string_buffer(64), C.c_void_p).value
_FWD = dict(pred=_P, target=_P, loss_sum=_P, loss_elem=_P, batch=2, voxels=8)
_FWD_BAD = {
    "both-outputs-null": dict(loss_sum=None, loss_elem=None), "null-pred": dict(pred=None), "null-target": dict(target=None),
    "batch-negative": dict(batch=-1), "voxels-zero": dict(voxels=0), "voxels-negative": dict(voxels=-4),
    "2^31-elements": dict(batch=2, voxels=1 << 30), "4GiB": dict(batch=1, voxels=1 << 30), "voxels-2^31": dict(batch=1, voxels=1 << 31),
}
_BWD = dict(pred=_P, target=_P, grad_scale=_P, grad_pred=_P, batch=2, voxels=8)
_BWD_BAD = {
    "null-pred": dict(pred=None), "null-target": dict(target=None), "null-grad_scale": dict(grad_scale=None),
    "null-grad_pred": dict(grad_pred=None), "batch-negative": dict(batch=-1), "voxels-zero": dict(voxels=0),
    "4GiB": dict(batch=4, voxels=1 << 28),
}


@pytest.mark.parametrize("case", list(_FWD_BAD), ids=list(_FWD_BAD))
def test_forward_rejects_bad_arguments_on_the_host(lib, case):
    a = dict(_FWD, **_FWD_BAD[case])
    assert lib.s3r_voxel_bce_forward(a["pred"], a["target"], a["loss_sum"], a["loss_elem"], a["batch"], a["voxels"], None) == INVALID
    assert lib.s3r_last_error().decode()


@pytest.mark.parametrize("case", list(_BWD_BAD), ids=list(_BWD_BAD))
def test_backward_rejects_bad_arguments_on_the_host(lib, case):
    a = dict(_BWD, **_BWD_BAD[case])
    assert lib.s3r_voxel_bce_backward(a["pred"], a["target"], a["grad_scale"], a["grad_pred"], a["batch"], a["voxels"], None) == INVALID
    assert lib.s3r_last_error().decode()


def test_batch_zero_launches_nothing(lib):
    """S3R_OK on a host with no device: nothing was enqueued (a launch would have been S3R_ERR_HIP); pointers are not even looked at"""
    assert lib.s3r_voxel_bce_forward(None, None, _P, None, 0, 8, None) == 0
    assert lib.s3r_voxel_bce_backward(None, None, None, None, 0, 8, None) == 0
    assert lib.s3r_voxel_bce_forward(None, None, None, None, 0, 8, None) == INVALID      # both outputs NULL is a malformed call at any batch


# ---------------------------------------------------------------- the restatements against torch in float64
def _random(B, V, seed):
    g = torch.Generator().manual_seed(seed)
    p = torch.rand(B, V, generator=g).numpy()
    t = (torch.rand(B, V, generator=g) < 0.3).float().numpy()
    t[:, ::3] = torch.rand(B, len(range(0, V, 3)), generator=g).numpy()         # soft targets among the hard ones
    return p, t


def _with_planted(B, V, seed):
    p, t = _random(B, V, seed)
    pp, pt = R.planted()
    n = min(V, pp.size)
    p[0, :n], t[0, :n] = pp[:n], pt[:n]
    return p, t


def test_fp64_restatement_is_torch_bceloss_and_its_gradient():
    """loss_elem64 / grad64 against torch.nn.BCELoss in float64, the planted corners included: torch clamps log at -100 and divides
    by max((1 - p) p, 1e-12) exactly as the header says.  Two float64 evaluations: 1e-12 relative, plus 2^-52 absolute for log(1 - p)
    of a p below 2^-53 (torch rounds 1 - p to 1; the restatement uses log1p)."""
    B, V = 3, 40
    p, t = _with_planted(B, V, 1)
    pd = torch.from_numpy(p).double().requires_grad_()
    td = torch.from_numpy(t).double()
    elem = torch.nn.BCELoss(reduction="none")(pd, td)
    mean = torch.nn.BCELoss()(pd, td)
    (grad,) = torch.autograd.grad(mean, pd)
    got = R.loss_elem64(p, t)
    assert (np.abs(got - elem.detach().numpy()) <= 1e-12 * np.abs(got) + 2.0 ** -52).all()
    assert got[0, 1] == 50.0 and got[0, 2] == 100.0 and got[0, 15] == 100.0 and got[0, 0] == 0.0 and got[0, 17] == 0.0
    g64 = R.grad64(p, t, np.full(B, 1.0 / (B * V)))
    assert (np.abs(g64 - grad.numpy()) <= 1e-12 * np.abs(g64)).all()
    assert np.abs(g64).max() > 1e9                                 # the 1e-12 epsilon is in play: (0 - 1) / 1e-12 / 120


def test_fp32_restatement_is_within_the_derived_bounds():
    p, t = _with_planted(2, 3000, 2)
    l32, l64, lim = R.loss_elem32(p, t), R.loss_elem64(p, t), R.elem_bound(p, t)
    err = np.abs(l32.astype(np.float64) - l64)
    print(f"loss_elem32 (numpy's float32 log): max err / bound {(err / lim).max():.3f}")
    assert (err <= lim).all()
    s = np.array([R.sum_order32(l32[b]) for b in range(2)])
    for b in range(2):
        assert abs(float(s[b]) - l32[b].astype(np.float64).sum()) <= R.sum_bound(l32[b])
    scale = np.array([0.25, -3.0], np.float32)
    g32, g64 = R.grad32(p, t, scale), R.grad64(p, t, scale)
    # four roundings (p - t, the product, 1 - p, (1 - p) p) and one division: gamma_5; a subnormal ulp where the numerator underflows
    # (0.25 * 2^-149 rounds to 0), divided by d like the numerator itself, and one where the quotient does
    d64 = np.maximum((1.0 - p.astype(np.float64)) * p.astype(np.float64), 1e-12)
    assert (np.abs(g32 - g64) <= R.gamma(5) * np.abs(g64) + 2.0 ** -149 / d64 + 2.0 ** -149).all()


def test_exact_values_at_the_clamps():
    p, t = R.planted()
    l = R.loss_elem32(p, t).reshape(len(R.PLANTED_P), len(R.PLANTED_T))
    assert l[0].tolist() == [0.0, 50.0, 100.0]                    # p == 0: t = 0 gives 0 (not 0 * -inf), t = 1 exactly 100
    assert l[5].tolist() == [100.0, 50.0, 0.0]                    # p == 1: t = 0 exactly 100, t = 1 gives 0
    assert l[1].tolist() == [0.0, 50.0, 100.0]                    # p = 2^-149: log p = -103.3 is clamped, 1 - p rounds to 1
    assert np.isfinite(l).all()
    bad = R.loss_elem32(np.array([np.nan, -0.5, 1.5, 0.5], np.float32), np.array([0.0, 1.0, 0.5, 0.5], np.float32))
    assert np.isnan(bad[:3]).all() and np.isfinite(bad[3])        # NaN and out-of-range pred: NaN, that element only
    g = R.grad32(p.reshape(1, -1), t.reshape(1, -1), [1.0]).reshape(l.shape)
    assert g[0].tolist() == [0.0, np.float32(-0.5) / np.float32(1e-12), np.float32(-1) / np.float32(1e-12)]       # the epsilon
    assert g[3].tolist() == [2.0, 0.0, -2.0]                      # p = 0.5: (p - t) / 0.25


# ---------------------------------------------------------------- coverage conditions and mutants
def test_shape_list_contains_every_boundary_of_the_order():
    sizes = {v for _, v in R.SHAPES}
    assert set(R.boundaries()) <= sizes, sorted(set(R.boundaries()) - sizes)
    issue = [(1, 1), (1, 3), (2, 4), (1, 255), (1, 256), (1, 257), (3, 1023), (2, 1024), (2, 1025), (2, 4099), (2, 32768), (1, 2 ** 20 + 5)]
    assert R.SHAPES[:len(issue)] == issue
    assert any(b > 1 and v % 4 for b, v in R.SHAPES)              # a sample row that starts only 4-byte aligned


def test_mutants_of_the_element_rule_are_caught_by_the_planted_cases():
    p, t = R.planted()
    rule = R.loss_elem32(p, t)
    after = R.loss_elem32(p, t, mutant="clamp-after-multiply")
    assert np.isnan(after).any() and not np.isnan(rule).any()     # 0 * -inf at p = 0, t = 0
    nan_p, nan_t = np.array([np.nan, 2.0], np.float32), np.array([0.5, 0.5], np.float32)
    assert np.isnan(R.loss_elem32(nan_p, nan_t)).all()
    assert np.isfinite(R.loss_elem32(nan_p, nan_t, mutant="fmax-clamp")).all()      # fmaxf swallows the NaN: the NaN case sees it


def test_mutants_of_the_summation_order_are_caught_by_the_shapes():
    """another order gives other bits on the random data of at least one listed shape of each kind"""
    def sequential(l):
        s = np.float32(0)
        for v in l:
            s = np.float32(s + v)
        return s

    def no_chunks(l):                                              # one tree over lane partials of the whole sample
        x = np.zeros((l.size + 255) // 256 * 256, np.float32)
        x[:l.size] = l
        v = x.reshape(-1, 64, 4).transpose(1, 0, 2).reshape(64, -1)
        acc = np.zeros(64, np.float32)
        for k in range(v.shape[1]):
            acc = (acc + v[:, k]).astype(np.float32)
        for o in (32, 16, 8, 4, 2, 1):
            acc = (acc[:o] + acc[o:2 * o]).astype(np.float32)
        return acc[0]

    seen = {"sequential": False, "no_chunks": False}
    for B, V in R.SHAPES:
        if V > 40000:
            continue
        p, t = _random(1, V, V)
        l = R.loss_elem32(p, t)[0]
        want = R.sum_order32(l)
        seen["sequential"] |= R.bits(sequential(l)) != R.bits(want)
        seen["no_chunks"] |= R.bits(no_chunks(l)) != R.bits(want)
        if V <= 1024:                                              # one chunk: the two tree orders coincide by construction
            assert R.bits(no_chunks(l)) == R.bits(want)
    assert all(seen.values()), seen


# ---------------------------------------------------------------- the module surface
def test_python_layer_checks_before_the_device(s3r):
    p, t = torch.rand(2, 4, 4, 4), torch.rand(2, 4, 4, 4)
    with pytest.raises(RuntimeError, match="HIP device"):         # no CPU fallback
        s3r.voxel_bce(p, t)
    with pytest.raises(RuntimeError, match="HIP device"):
        s3r.VoxelBCELoss()(p.requires_grad_(), t)
    with pytest.raises(RuntimeError, match="one shape"):
        s3r.voxel_bce(p, t[:, :2])
    with pytest.raises(RuntimeError, match="one shape"):
        s3r.voxel_bce_backward(p, t[:1], torch.ones(2))


def test_the_voxel_models_refuse_bf16_and_train(s3r):
    img = torch.zeros(1, 3, 224, 224)
    for make in (lambda: s3r.Stereo2Voxel("bf16").head_features(img, img),
                 lambda: s3r.Decoder("bf16").features(torch.zeros(1, 64, 28, 28, 28)),
                 lambda: s3r.Decoder("bf16").differentiable_head(torch.zeros(1, 64, 32, 32, 32))):
        with pytest.raises(RuntimeError, match="fp32 models only"):
            make()
    model = s3r.Stereo2Voxel()
    for m in (model, model.decoder):
        with pytest.raises(RuntimeError):
            m.train()
        assert not m.training
    with pytest.raises(RuntimeError, match="HIP device"):         # fp32: accepted, and then there is no CPU path
        model.decoder.differentiable_head(torch.zeros(1, 64, 32, 32, 32))
