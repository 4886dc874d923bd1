"""The sub-pixel disparity read-out (s3r_disparity_soft) and the stereo metrics (s3r_disparity_metrics) on the device: values
against the fp64 restatement (tests/_disp64.py), the WTA and uniform limits, torch's bilinear upsampling, the bf16 channels-last
input, determinism, guarded buffers, the model-level read-out and the evaluation drivers."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import _abi_bodies as AB
from tests import _disp64 as R
from tests import _guard as G

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32, BF16 = 0, 1

SHAPES = [(2, 32, 28, 28, 28), (3, 5, 7, 13, 4), (1, 16, 12, 40, 40), (2, 8, 9, 9, 1)]
SID = ["x".join(map(str, s)) for s in SHAPES]


@pytest.fixture(scope="module")
def lib(s3r):
    return s3r.load_library()


def _feats(shape, seed, integer=False):
    B, Cc, H, W, _ = shape
    g = torch.Generator().manual_seed(seed)
    if integer:
        return (torch.randint(-3, 4, (B, Cc, H, W), generator=g).float(),
                torch.randint(-3, 4, (B, Cc, H, W), generator=g).float())
    return torch.randn(B, Cc, H, W, generator=g), torch.randn(B, Cc, H, W, generator=g)


def _cl_bf16(x):
    """fp32 (B,C,H,W) -> logical (B,C,H,W) bf16 in channels-last memory, as the bf16 encoder emits it"""
    return x.to(torch.bfloat16).contiguous(memory_format=torch.channels_last)


# ---------------------------------------------------------------- 1. feature resolution vs the fp64 restatement
@pytest.mark.parametrize("tau", [0.05, 1.0, 100.0])
@pytest.mark.parametrize("shape", SHAPES, ids=SID)
def test_feature_resolution_matches_fp64(s3r, shape, tau):
    D = shape[4]
    fl, fr = _feats(shape, sum(shape))
    dl, dr, cl, cr = (t.cpu().double().numpy() for t in s3r.disparity_soft(fl.to(DEV), fr.to(DEV), D, tau, confidence=True))
    (wl, wr), (ql, qr) = R.soft(fl.numpy(), fr.numpy(), D, tau)
    for got, want in ((dl, wl), (dr, wr)):
        assert np.abs(got - want).max() <= 2e-5 * D
    for got, want in ((cl, ql), (cr, qr)):
        assert (np.abs(got - want) / want).max() <= 1e-5
    if D == 1:
        assert (dl == 0).all() and (dr == 0).all() and (cl == 1).all() and (cr == 1).all()


# ---------------------------------------------------------------- 2. limits
@pytest.mark.parametrize("shape", SHAPES[:3], ids=SID[:3])
def test_cold_limit_is_the_wta_bit_for_bit(s3r, shape):
    """integer features give integer costs; tau = 0.01 and a unique minimum by >= 1 leave one weight (the others underflow)"""
    D = shape[4]
    fl, fr = _feats(shape, 7 + sum(shape), integer=True)
    sl, sr = s3r.disparity_soft(fl.to(DEV), fr.to(DEV), D, 0.01)
    wl, wr = s3r.disparity_wta(fl.to(DEV), fr.to(DEV), D)
    checked = 0
    for right, got, want in ((False, sl, wl), (True, sr, wr)):
        c = np.sort(R.costs(fl.numpy(), fr.numpy(), D, right), -1)
        unique = (c[..., 1] - c[..., 0] >= 1) | np.isinf(c[..., 1])
        m = torch.from_numpy(unique)
        assert torch.equal(got.cpu()[m], want.cpu()[m])
        checked += int(unique.sum())
    assert checked >= 0.2 * 2 * fl[:, 0].numel()


@pytest.mark.parametrize("shape", SHAPES, ids=SID)
def test_hot_limit_is_the_middle_of_the_range(s3r, shape):
    B, _, H, W, D = shape
    fl, fr = _feats(shape, 3 + sum(shape))
    dl, dr = s3r.disparity_soft(fl.to(DEV), fr.to(DEV), D, 1e6)
    w = torch.arange(W, dtype=torch.float32)
    nl = torch.clamp(w, max=D - 1) + 1
    nr = torch.clamp(W - 1 - w, max=D - 1) + 1
    assert ((dl.cpu() - (nl - 1) / 2).abs() <= 1e-3).all()
    assert ((dr.cpu() - (nr - 1) / 2).abs() <= 1e-3).all()


GAPS = [87.0, 87.5, 95.0, 103.0, 103.5, 104.0]      # exp(-gap): 1.6e-38 (kept), 9.9e-39 .. 1.4e-45 (subnormal), 0 in fp32


@pytest.mark.parametrize("size", [None, (11, 9)], ids=["feature", "11x9"])
def test_a_weight_below_flt_min_counts_as_zero(s3r, size):
    """The kernel's rule `e < FLT_MIN -> 0` (csrc/s3r_disparity.hip): row h has features g_h w in both views and tau = 1, so every
    pixel's best disparity is 0 with cost 0 and disparity d costs exactly g_h d.  Where exp(-g_h) is below FLT_MIN the float64
    soft-argmin WITH the rule is exactly 0 and the confidence exactly 1 — a kernel without the rule leaves the subnormal residue
    sum_d d e_d there; where it is above (g = 87) the far weight stays, within the float64 value's 1e-5."""
    H, W, D = len(GAPS), 6, 6
    g = np.array(GAPS, np.float32)[:, None] * np.arange(W, dtype=np.float32)[None, :]          # exact products
    fl = torch.from_numpy(np.broadcast_to(g, (2, 1, H, W)).copy())
    kw = {} if size is None else {"out_size": size}
    dl, dr, cl, cr = (t.cpu().double().numpy() for t in s3r.disparity_soft(fl.to(DEV), fl.clone().to(DEV), D, 1.0, confidence=True, **kw))
    want_d, want_c = [], []
    for right in (False, True):
        c = R.costs(fl.numpy(), fl.numpy(), D, right).astype(np.float64)
        e = np.exp(c.min(-1, keepdims=True) - c)
        e[e < np.finfo(np.float32).tiny] = 0.0                                                 # the rule
        want_d.append((e * np.arange(D)).sum(-1) / e.sum(-1))
        want_c.append(1.0 / e.sum(-1))
    assert (want_d[0][:, 1:, 1:] == 0).all() and (want_d[0][:, 0, 1:] > 0).all()                # rows 1.. are the flushed ones
    if size is None:
        for got, want in ((dl, want_d[0]), (dr, want_d[1])):
            assert (got[:, 1:] == 0).all(), got[0, 1:]
            assert (np.abs(got[:, 0] - want[:, 0]) <= 1e-5 * want[:, 0]).all(), (got[0, 0], want[0, 0])
        for got, want in ((cl, want_c[0]), (cr, want_c[1])):
            assert (got == 1).all() and (want == 1).all()
    else:
        # output rows that interpolate between flushed feature rows only (source row >= 1 on both sides): exact zeros again
        src = (np.arange(size[0], dtype=np.float32) + np.float32(0.5)) * (np.float32(H) / np.float32(size[0])) - np.float32(0.5)
        rows = np.floor(np.maximum(src, 0)) >= 1
        assert rows.sum() >= size[0] // 2
        assert (dl[:, rows] == 0).all() and (dr[:, rows] == 0).all() and (cl == 1).all() and (cr == 1).all()


# ---------------------------------------------------------------- 3. upsampling
UPS =[((2, 32, 28, 28, 28), (224, 224), 8.0), ((3, 5, 7, 13, 4), (37, 100), 2.5), ((2, 8, 9, 9, 5), (9, 9), 8.0),
       ((1, 16, 12, 40, 40), (5, 17), 1.0)]


@pytest.mark.parametrize("case", UPS, ids=["28to224", "7x13to37x100", "identity", "12x40to5x17"])
def test_upsampling_is_torch_bilinear_of_the_feature_maps(s3r, case):
    shape, size, scale = case
    D = shape[4]
    fl, fr = _feats(shape, 11 + sum(shape))
    fl, fr = fl.to(DEV), fr.to(DEV)
    feat = s3r.disparity_soft(fl, fr, D, 1.0, confidence=True)
    up = s3r.disparity_soft(fl, fr, D, 1.0, out_size=size, scale=scale, confidence=True)
    for k, (f, u) in enumerate(zip(feat, up)):
        assert u.shape == (shape[0],) + size
        want = F.interpolate(f.cpu()[:, None], size=size, mode="bilinear", align_corners=False)[:, 0]
        if k < 2:
            want = want * scale
        assert (u.cpu() - want).abs().max().item() <= 1e-5 * want.abs().max().item()
    if size == tuple(shape[2:4]):
        same = s3r.disparity_soft(fl, fr, D, 1.0, out_size=size, confidence=True)
        for f, u in zip(feat, same):
            assert torch.equal(f, u)


# ---------------------------------------------------------------- 4. bf16 channels-last input
@pytest.mark.parametrize("size", [None, (224, 224)], ids=["feature", "224"])
@pytest.mark.parametrize("shape", [SHAPES[0], (3, 8, 7, 13, 4), SHAPES[2]], ids=[SID[0], "3x8x7x13x4", SID[2]])
def test_bf16_channels_last_equals_fp32_on_the_converted_features(s3r, shape, size):
    D = shape[4]
    fl, fr = _feats(shape, 5 + sum(shape))
    bl, br = _cl_bf16(fl.to(DEV)), _cl_bf16(fr.to(DEV))
    got = s3r.disparity_soft(bl, br, D, 0.5, out_size=size, scale=8.0, confidence=True)
    want = s3r.disparity_soft(s3r.modules.channels_last_to_f32(bl), s3r.modules.channels_last_to_f32(br), D, 0.5,
                              out_size=size, scale=8.0, confidence=True)
    for g, w in zip(got, want):
        assert torch.equal(g, w)


# ---------------------------------------------------------------- 5. determinism and batch invariance
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_deterministic_and_batch_invariant(s3r, dtype):
    shape = (4, 32, 28, 28, 28)
    fl, fr = (t.to(DEV) for t in _feats(shape, 17))
    if dtype == "bf16":
        fl, fr = _cl_bf16(fl), _cl_bf16(fr)
    a = s3r.disparity_soft(fl, fr, 28, 1.0, out_size=(224, 224), scale=8.0, confidence=True)
    b = s3r.disparity_soft(fl, fr, 28, 1.0, out_size=(224, 224), scale=8.0, confidence=True)
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    for i in range(shape[0]):
        one = s3r.disparity_soft(fl[i:i + 1], fr[i:i + 1], 28, 1.0, out_size=(224, 224), scale=8.0, confidence=True)
        for x, y in zip(a, one):
            assert torch.equal(x[i], y[0])


# ---------------------------------------------------------------- 6. guarded buffers
GUARDED = [("fp32-upsample", F32, (2, 32, 28, 28, 28), (224, 224), True), ("fp32-feature", F32, (3, 5, 7, 13, 4), (7, 13), True),
           ("bf16-upsample", BF16, (2, 16, 9, 11, 6), (23, 40), True), ("fp32-no-confidence", F32, (2, 8, 12, 40, 40), (60, 80), False),
           ("bf16-no-confidence", BF16, (1, 32, 28, 28, 28), (224, 224), False)]


@pytest.mark.parametrize("case", GUARDED, ids=[c[0] for c in GUARDED])
def test_guarded_buffers(s3r, lib, case):
    AB.disparity_soft(s3r, lib, case)


def test_batch_zero_launches_nothing(s3r, lib):
    fl = G.Guarded("left", (1, 8, 4, 4), torch.float32, DEV, "in", data=torch.ones(1, 8, 4, 4, device=DEV))
    out = G.Guarded("disp", (1, 8, 8), torch.float32, DEV, "in", data=torch.full((1, 8, 8), 3.0, device=DEV))
    s3r.profile_enable(64)
    try:
        s3r.profile_reset()
        assert lib.s3r_disparity_soft(fl.ptr, fl.ptr, F32, out.ptr, out.ptr, out.ptr, out.ptr, 0, 8, 4, 4, 4, 1.0, 8, 8, 8.0,
                                      None) == 0
        assert lib.s3r_disparity_metrics(fl.ptr, fl.ptr, out.ptr, out.ptr, 0, 128, None) == 0
        torch.cuda.synchronize()
        assert s3r.profile_read() == []
        s3r.disparity_soft(fl.t, fl.t, 4, 1.0, out_size=(8, 8))        # one record, one launch, the stated bytes
        recs = s3r.profile_read()
        assert len(recs) == 1 and recs[0]["family"] == "disparity" and recs[0]["launches"] == 1
        assert recs[0]["bytes"] == 4.0 * 2 * 8 * 16 + 4.0 * 2 * 64
    finally:
        s3r.profile_enable(0)
    G.check_all(fl, out)


# ---------------------------------------------------------------- 7. metrics vs numpy fp64
def _metric_case():
    g = torch.Generator().manual_seed(31)
    B, P = 5, 1000
    gt = torch.rand(B, P, generator=g) * 120
    pred = gt + (torch.rand(B, P, generator=g) - 0.5) * 16
    gt[0, ::7] = float("inf")
    gt[1, ::5] = float("nan")
    gt[2, 1::3] = -1.0
    gt[3] = float("inf")                                          # an all-invalid sample
    gt[3, ::2] = -2.0
    gt[4, :3] = torch.tensor([10.0, 10.0, 100.0])                 # errors of exactly 1, 3 and 0.05 gt: not counted
    pred[4, :3] = torch.tensor([11.0, 13.0, 105.0])
    return pred, gt


def test_metrics_match_numpy(s3r, lib):
    pred, gt = _metric_case()
    pb = G.Guarded("pred", pred.shape, torch.float32, DEV, "in", data=pred.to(DEV))
    gb = G.Guarded("gt", gt.shape, torch.float32, DEV, "in", data=gt.to(DEV))
    e = G.Guarded("epe", pred.shape[0], torch.float32, DEV, "out")
    c = G.Guarded("counts", (pred.shape[0], 4), torch.int32, DEV, "out")
    assert lib.s3r_disparity_metrics(pb.ptr, gb.ptr, e.ptr, c.ptr, pred.shape[0], pred.shape[1], None) == 0
    torch.cuda.synchronize()
    G.check_all(pb, gb, e, c)
    want_e, want_c = R.metrics(pred.numpy(), gt.numpy())
    assert np.array_equal(c.t.cpu().numpy(), want_c)
    assert (np.abs(e.t.cpu().double().numpy() - want_e) <= 1e-6 * want_e.max()).all()
    assert e.t[3].item() == 0 and c.t[3].tolist() == [0, 0, 0, 0]
    head = R.metrics(pred[4:5, :3].numpy(), gt[4:5, :3].numpy())[1]
    assert head.tolist() == [[3, 2, 1, 0]]                         # err 1: none; err 3: > 1 only; err 5 = 0.05 gt: > 1, > 3, not D1
    epe, cnt = s3r.disparity_epe(pred.to(DEV), gt.to(DEV))
    assert torch.equal(e.t, epe) and torch.equal(c.t[:, 0], cnt)  # the EPE kernel's bits


def test_metrics_on_the_exr_fixture(s3r, golden_dir):
    gt = s3r.exr.disparity_channel(s3r.exr.read_exr(os.path.join(golden_dir, "disp_zip_half.exr")))
    gt = torch.from_numpy(np.ascontiguousarray(gt, np.float32))[None]
    g = torch.Generator().manual_seed(3)
    pred = torch.where(torch.isfinite(gt), gt, torch.zeros_like(gt)) + (torch.rand(gt.shape, generator=g) - 0.5) * 12
    epe, counts = s3r.disparity_metrics(pred.to(DEV), gt.to(DEV))
    want_e, want_c = R.metrics(pred.numpy(), gt.numpy())
    assert np.array_equal(counts.cpu().numpy(), want_c) and want_c[0, 0] > 0
    assert abs(epe.item() - want_e[0]) <= 1e-6 * want_e[0]
    assert torch.equal(epe, s3r.disparity_epe(pred.to(DEV), gt.to(DEV))[0])


# ---------------------------------------------------------------- 8. model level
@pytest.fixture(scope="module")
def nets(s3r):
    out = {}
    for name, cls in (("voxel", s3r.Stereo2Voxel), ("point", s3r.Stereo2Point)):
        for prec in ("fp32", "bf16"):
            m = cls(precision=prec)
            s3r.seed_module(m, 2)
            out[f"{name}-{prec}"] = m.to(DEV)
    return out


@pytest.mark.parametrize("net", ["voxel-fp32", "voxel-bf16", "point-fp32", "point-bf16"])
def test_model_readouts(s3r, nets, net):
    model = nets[net]
    left, right = s3r.synthetic_pairs(3, seed=6)
    left, right = left.to(DEV), right.to(DEV)
    dl, dr = model.disparity(left, right, readout="soft", full_resolution=True)
    assert dl.shape == (3, 224, 224) and dr.shape == (3, 224, 224)
    assert torch.isfinite(dl).all() and torch.isfinite(dr).all()
    feats = model.encoder.forward_pair(left, right)
    want = s3r.disparity_soft(feats[:3], feats[3:], s3r.arch_spec.MAX_DISP, model.disparity_temperature, (224, 224), 8.0)
    assert torch.equal(dl, want[0]) and torch.equal(dr, want[1])
    sl, sr, cl, cr = model.disparity(left, right, readout="soft", confidence=True)
    assert sl.shape == (3, 28, 28) and cl.shape == (3, 28, 28) and bool(((cl > 0) & (cl <= 1)).all())
    f32 = feats if feats.dtype == torch.float32 else s3r.modules.channels_last_to_f32(feats)
    wl, wr = s3r.disparity_wta(f32[:3], f32[3:], s3r.arch_spec.MAX_DISP)
    gl, gr = model.disparity(left, right)                          # the default: today's WTA output
    assert torch.equal(gl, wl * 8) and torch.equal(gr, wr * 8)


# ---------------------------------------------------------------- 9. evaluation
def test_eval_driver_pools_soft_rates(s3r, nets):
    model = nets["voxel-fp32"]
    left, right, _ = s3r.evaluate.synthetic_eval_set(5, 4)
    g = torch.Generator().manual_seed(12)
    gl, gr = torch.rand(5, 224, 224, generator=g) * 40, torch.rand(5, 224, 224, generator=g) * 40
    gl[0, :50] = float("inf")
    gr[1] = -1.0                                                  # one sample without a valid right pixel
    res = s3r.evaluate.test_disparity(model, left, right, gl, gr, batch=2, device=DEV, readout="soft")
    parts = [model.disparity(left[i:i + 2].to(DEV), right[i:i + 2].to(DEV), readout="soft", full_resolution=True)
             for i in range(0, 5, 2)]                             # the driver's batches
    dl, dr = (torch.cat(p, 0) for p in zip(*parts))
    for side, pred, gt in (("left", dl, gl), ("right", dr, gr)):
        e, c = R.metrics(pred.cpu().numpy(), gt.numpy())
        n = c[:, 0].sum()
        assert res[f"valid_{side}"] == n
        for k, name in enumerate(("bad1", "bad3", "d1")):
            assert res[f"{name}_{side}"] == 100.0 * c[:, k + 1].sum() / n
        assert abs(res[f"epe_{side}"] - (e * c[:, 0]).sum() / n) <= 1e-6 * res[f"epe_{side}"]


@pytest.mark.timeout(300)
def test_runner_reports_soft_rates_and_keeps_the_default_keys(s3r, tmp_path):
    left, right, gt = s3r.evaluate.synthetic_eval_set(3, 5)
    g = torch.Generator().manual_seed(2)
    full = [torch.rand(3, 224, 224, generator=g) * 60 for _ in range(2)]
    feat = [torch.rand(3, 28, 28, generator=g) * 60 for _ in range(2)]
    runs = {}
    for name, disp, extra in (("soft", full, ["--disparity-readout", "soft", "--disparity-temperature", "2.0"]),
                              ("default", feat, [])):
        data = tmp_path / f"{name}.npz"
        np.savez(data, left=left.numpy(), right=right.numpy(), volume=gt.numpy(), disp_left=disp[0].numpy(),
                 disp_right=disp[1].numpy())
        runs[name] = subprocess.Popen([sys.executable, os.path.join(ROOT, "runner.py"), "--test", "--data", str(data),
                                       "--batch", "2"] + extra, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True,
                                      cwd=ROOT)
    out = {}
    for name, p in runs.items():
        try:
            so, se = p.communicate(timeout=240)
        except subprocess.TimeoutExpired:
            for q in runs.values():
                q.kill()
            raise
        assert p.returncode == 0, se[-2000:]
        out[name] = json.loads(so.strip().splitlines()[-1])
    rates = {f"disparity_{k}_{s}_pct" for k in ("bad1", "bad3", "d1") for s in ("left", "right")}
    assert out["soft"]["disparity_readout"] == "soft" and rates <= set(out["soft"])
    assert all(0 <= out["soft"][k] <= 100 for k in rates)
    assert set(out["default"]) == {"samples", "n_gpus", "thresholds", "mean_iou", "precision", "eval_pairs_per_s", "renders",
                                   "weights", "data", "disparity_epe_left_px", "disparity_epe_right_px"}
