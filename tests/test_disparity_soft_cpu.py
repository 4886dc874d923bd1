"""The sub-pixel disparity read-out and the stereo metrics without a GPU: the C-ABI declarations and bindings, host-side
validation (every bad argument is S3R_ERR_INVALID with a message: a HIP call would have given S3R_ERR_HIP on a host without a
device), the Python layer's argument checks, and the fp64 restatement (tests/_disp64.py) the GPU tests measure against."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest
import torch

from tests import _disp64 as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = -1
F32, BF16 = 0, 1


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


def test_header_declares_both_entries():
    assert _prototype("s3r_disparity_soft") == [
        "const void* feat_l", "const void* feat_r", "int feat_dtype", "float* disp_l", "float* disp_r", "float* conf_l",
        "float* conf_r", "int batch", "int channels", "int height", "int width", "int max_disp", "float temperature",
        "int out_height", "int out_width", "float disp_scale", "void* stream"]
    assert _prototype("s3r_disparity_metrics") == [
        "const float* pred", "const float* gt", "float* epe", "int32_t* counts", "int batch", "int64_t pixels", "void* stream"]
    header = open(os.path.join(ROOT, "include", "s3r.h")).read()
    assert "#define S3R_ABI_VERSION 8" in header                  # additive entry points: no version step


def test_lib_binds_both_entries(s3r, lib):
    res, args = s3r._lib.SIGNATURES["s3r_disparity_soft"]
    assert res is C.c_int and len(args) == 17
    assert args[2] is C.c_int and args[12] is C.c_float and args[15] is C.c_float
    assert [a is C.c_int for a in args[7:12]] == [True] * 5 and args[13] is C.c_int and args[14] is C.c_int
    res, args = s3r._lib.SIGNATURES["s3r_disparity_metrics"]
    assert res is C.c_int and len(args) == 7 and args[4] is C.c_int and args[5] is C.c_int64
    assert lib.s3r_disparity_soft.argtypes == s3r._lib.SIGNATURES["s3r_disparity_soft"][1]
    assert lib.s3r_disparity_metrics.argtypes == s3r._lib.SIGNATURES["s3r_disparity_metrics"][1]


# a non-NULL host address: validation rejects each case before anything could dereference it
_P = C.cast(C.create_string_buffer(64), C.c_void_p).value
_GOOD = dict(dtype=F32, batch=2, c=32, h=28, w=28, d=28, tau=1.0, oh=224, ow=224, scale=8.0)
_SOFT_BAD = {
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
}


def _soft(lib, dtype, batch, c, h, w, d, tau, oh, ow, scale, ptr=_P):
    return lib.s3r_disparity_soft(ptr, ptr, dtype, ptr, ptr, None, None, batch, c, h, w, d, tau, oh, ow, scale, None)


@pytest.mark.parametrize("case", list(_SOFT_BAD), ids=list(_SOFT_BAD))
def test_soft_readout_rejects_bad_arguments_on_the_host(s3r, lib, case):
    args = dict(_GOOD, **_SOFT_BAD[case])
    assert _soft(lib, **args) == INVALID
    assert lib.s3r_last_error().decode()


def test_soft_readout_lds_rule_is_the_stated_one(lib):
    """4 (2 C W + 2 W min(D, W) + 12 W) bytes <= 64 KiB, as include/s3r.h states it; batch 0 gets past validation and launches
    nothing (no device needed)"""
    def need(c, w, d):
        return 4 * (2 * c * w + 2 * w * min(d, w) + 12 * w)
    ok, bad = (258, 28, 28), (259, 28, 28)
    assert need(*ok) <= 65536 < need(*bad)
    assert _soft(lib, F32, 0, ok[0], 4, ok[1], ok[2], 1.0, 8, 8, 1.0) == 0
    assert _soft(lib, F32, 0, bad[0], 4, bad[1], bad[2], 1.0, 8, 8, 1.0) == INVALID


def test_soft_readout_batch_zero_and_null_features(lib):
    assert lib.s3r_disparity_soft(None, None, F32, None, None, None, None, 0, 32, 28, 28, 28, 1.0, 224, 224, 8.0, None) == 0
    assert lib.s3r_disparity_soft(None, None, F32, _P, _P, None, None, 1, 32, 28, 28, 28, 1.0, 28, 28, 1.0, None) == INVALID


@pytest.mark.parametrize("case", ["pixels-negative", "batch-negative", "2^31-elements", "null-pointer"])
def test_metrics_reject_bad_arguments_on_the_host(lib, case):
    args = {"pixels-negative": (_P, _P, _P, _P, 2, -1), "batch-negative": (_P, _P, _P, _P, -2, 16),
            "2^31-elements": (_P, _P, _P, _P, 2, 1 << 30), "null-pointer": (None, _P, _P, _P, 2, 16)}[case]
    assert lib.s3r_disparity_metrics(*args, None) == INVALID
    assert lib.s3r_last_error().decode()
    assert lib.s3r_disparity_metrics(None, None, None, None, 0, 16, None) == 0


def test_python_layer_rejects_a_bad_readout_before_the_device(s3r):
    model = s3r.Stereo2Voxel()
    x = torch.zeros(1, 3, 224, 224)
    with pytest.raises(ValueError):
        model.disparity(x, x, readout="bogus")
    with pytest.raises(ValueError):
        model.disparity(x, x, full_resolution=True)                 # WTA is feature-resolution only
    with pytest.raises(ValueError):
        model.disparity(x, x, readout="wta", full_resolution=True)
    with pytest.raises(ValueError):
        s3r.evaluate.test_disparity(model, x, x, torch.zeros(1, 28, 28), torch.zeros(1, 28, 28), device="cpu", readout="x")
    assert s3r.Stereo2Point().disparity_temperature == s3r.DISPARITY_TEMPERATURE > 0


def test_restatement_hand_computed_case():
    """C = 1, W = 3, D = 3, tau = 1: L = [0, 1, 3], R = [1, 3, 0]."""
    fl = np.array([0, 1, 3], np.float32).reshape(1, 1, 1, 3)
    fr = np.array([1, 3, 0], np.float32).reshape(1, 1, 1, 3)
    cl = R.costs(fl, fr, 3, right=False)[0, 0]
    cr = R.costs(fl, fr, 3, right=True)[0, 0]
    inf = np.inf
    assert np.array_equal(cl, [[1, inf, inf], [2, 0, inf], [3, 0, 2]])
    assert np.array_equal(cr, [[1, 0, 2], [2, 0, inf], [3, inf, inf]])
    (dl, dr), (ql, qr) = R.soft(fl, fr, 3, 1.0)
    e = math.exp
    want_dl = [0.0, 1 / (1 + e(-2)), (1 + 2 * e(-2)) / (1 + e(-2) + e(-3))]
    want_ql = [1.0, 1 / (1 + e(-2)), 1 / (1 + e(-2) + e(-3))]
    want_dr = [(1 + 2 * e(-2)) / (1 + e(-1) + e(-2)), 1 / (1 + e(-2)), 0.0]
    want_qr = [1 / (1 + e(-1) + e(-2)), 1 / (1 + e(-2)), 1.0]
    for got, want in ((dl, want_dl), (ql, want_ql), (dr, want_dr), (qr, want_qr)):
        assert np.allclose(got[0, 0], want, rtol=1e-15, atol=0)
    (d1, _), (q1, _) = R.soft(fl, fr, 1, 0.05)                      # one disparity: exactly 0 and 1
    assert np.array_equal(d1, np.zeros((1, 1, 3))) and np.array_equal(q1, np.ones((1, 1, 3)))


@pytest.mark.parametrize("sizes", [(28, 28, 224, 224), (7, 13, 37, 100), (12, 40, 5, 17), (9, 9, 9, 9)],
                         ids=lambda s: "x".join(map(str, s)))
def test_restatement_bilinear_is_torch_align_corners_false(sizes):
    h, w, oh, ow = sizes
    x = torch.rand(2, h, w, generator=torch.Generator().manual_seed(h * w))
    # torch forms the fp32 input's source indices in fp32, as the restatement and the kernel do; its blend is fp32 as well
    want = torch.nn.functional.interpolate(x[:, None], size=(oh, ow), mode="bilinear", align_corners=False)[:, 0]
    assert np.abs(R.bilinear(x.numpy(), oh, ow) - want.double().numpy()).max() <= 4e-7


def test_restatement_metrics_hand_computed_case():
    inf, nan = float("inf"), float("nan")
    gt = np.array([[10, 10, 10, 100, 100, 60, inf, nan, -1, 0],
                   [inf, nan, -2, inf, inf, -1, nan, inf, inf, -0.5]], np.float32)
    pred = np.array([[10, 11, 13, 105, 106, 64, 0, 0, 0, 4],
                     [1, 2, 3, 4, 5, 6, 7, 8, 9, 10]], np.float32)
    epe, counts = R.metrics(pred, gt)
    # valid errors of sample 0: 0, 1 (not > 1), 3 (not > 3), 5 (= 0.05 gt: not D1), 6, 4 and 4 (gt = 0)
    assert counts.tolist() == [[7, 5, 4, 3], [0, 0, 0, 0]]
    assert epe[0] == (0 + 1 + 3 + 5 + 6 + 4 + 4) / 7 and epe[1] == 0
