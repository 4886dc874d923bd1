"""The training entry: s3r.train.fit, checkpoint.save_checkpoint and `runner.py --train`, all at B = 2 on 6 synthetic samples.

fit twice gives identical per-step losses and parameters; a run stopped after step 2 and resumed in a fresh model and optimizer takes
step 3 with the bits of the uninterrupted run; the per-step loss equals a hand-written loop over the same public ops; both variants
run, disparity supervision runs once; `runner.py --train` writes a checkpoint that `runner.py --test --weights` loads; what is not
implemented is refused."""
import hashlib
import json
import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
N, B = 6, 2
_CACHE = {}


def _sets(s3r, variant="voxel", disparity=False):
    key = (variant, disparity)
    if key not in _CACHE:
        left, right, gt = s3r.evaluate.synthetic_eval_set(N, 3, "uint8")
        if variant == "point":
            gt = torch.rand(N, 2048, 3, generator=torch.Generator().manual_seed(5)) - 0.5
        fields = [left, right, gt]
        if disparity:
            g = torch.Generator().manual_seed(6)
            for _ in range(2):
                d = torch.rand(N, 224, 224, generator=g) * 24
                d[torch.rand(N, 224, 224, generator=g) < 0.3] = float("inf")      # background: the loaders' invalid marker
                fields.append(d)
        _CACHE[key] = torch.utils.data.TensorDataset(*fields)
    return _CACHE[key]


def _model(s3r, variant="voxel"):
    model = s3r.Stereo2Point() if variant == "point" else s3r.Stereo2Voxel()
    s3r.seed_module(model, seed=0)
    return model.to(DEV)


def _augment(s3r):
    return s3r.AugmentConfig.default(seed=9)


def _cfg(s3r, **kw):
    base = dict(variant="voxel", epochs=1, batch=B, lr=1e-3, optimizer="adam", clip_grad_norm=1.0, augment=_augment(s3r), seed=4,
                val_every=0, save_every=0)
    base.update(kw)
    return s3r.TrainConfig(**base)


def _digest(model):
    h = hashlib.sha256()
    for n, p in sorted(model.state_dict().items()):
        h.update(n.encode())
        h.update(p.detach().cpu().contiguous().reshape(-1).numpy().tobytes())
    return h.hexdigest()


def _reference_run(s3r):
    """the uninterrupted voxel run of three steps, computed once: (losses, digest)"""
    if "ref" not in _CACHE:
        model = _model(s3r)
        res = s3r.fit(model, _sets(s3r), None, _cfg(s3r))
        torch.cuda.synchronize()
        _CACHE["ref"] = (res["losses"], _digest(model), res)
    return _CACHE["ref"]


def test_fit_twice_is_bit_identical(s3r):
    losses, digest, res = _reference_run(s3r)
    assert len(losses) == 3 and res["step"] == 3 and res["epoch"] == 1 and all(l == l and abs(l) < float("inf") for l in losses)
    model = _model(s3r)
    start = _digest(model)
    again = s3r.fit(model, _sets(s3r), None, _cfg(s3r))
    assert again["losses"] == losses
    assert _digest(model) == digest != start
    assert isinstance(again["optimizer"], s3r.Adam)


def test_stop_save_resume_continues_with_the_same_bits(s3r, tmp_path):
    losses, digest, _ = _reference_run(s3r)
    first = s3r.fit(_model(s3r), _sets(s3r), None, _cfg(s3r, max_steps=2, out_dir=str(tmp_path)))
    assert first["losses"] == losses[:2] and first["step"] == 2 and first["epoch"] == 0
    path = first["checkpoint"]
    assert path == str(tmp_path / "last.pth") and os.path.exists(path)
    ck = s3r.checkpoint.load_training_checkpoint(path)
    assert set(ck) == {"model", "optimizer", "epoch", "step", "best", "config"} and (ck["epoch"], ck["step"]) == (0, 2)
    assert ck["config"]["batch"] == B and ck["config"]["augment"]["max_shift"] == 8 and "s3r_device_state" in ck["optimizer"]
    fresh = s3r.Stereo2Voxel()
    s3r.seed_module(fresh, seed=123)                                   # another initial state: everything comes from the file
    fresh.to(DEV)
    second = s3r.fit(fresh, _sets(s3r), None, _cfg(s3r, resume=path))
    assert second["losses"] == losses[2:] and second["step"] == 3 and second["epoch"] == 1
    assert _digest(fresh) == digest
    # the file is a checkpoint the inference path loads as it is
    other = s3r.Stereo2Voxel()
    s3r.checkpoint.load_checkpoint(other, path)
    assert all(torch.equal(v, ck["model"][k]) for k, v in other.state_dict().items())


def test_loss_equals_a_hand_written_loop_over_the_public_ops(s3r):
    losses, digest, _ = _reference_run(s3r)
    cfg, ds = _cfg(s3r), _sets(s3r)
    model = _model(s3r)
    opt = s3r.Adam([p for p in model.parameters() if p.requires_grad], lr=cfg.lr, clip_grad_norm=cfg.clip_grad_norm)
    bce = s3r.VoxelBCELoss()
    order = torch.randperm(N, generator=torch.Generator().manual_seed(cfg.seed + 0)).tolist()
    assert order == s3r.train.epoch_order(N, cfg.seed, 0)
    left, right, gt = ds.tensors
    got = []
    for i in range(0, N, B):
        idx = order[i:i + B]
        ids = torch.tensor(idx, dtype=torch.int64, device=DEV) + 0 * N
        l, r = s3r.ops.augment_pair(left[idx].to(DEV), right[idx].to(DEV), ids, cfg.augment)
        opt.zero_grad()
        loss = bce(model.differentiable(l, r), gt[idx].to(DEV))
        loss.backward()
        opt.step()
        got.append(loss.item())
    assert got == losses
    assert _digest(model) == digest


def test_point_variant_runs_and_validates(s3r, tmp_path):
    ds = _sets(s3r, "point")
    model = _model(s3r, "point")
    lines = []
    res = s3r.fit(model, ds, ds.tensors, _cfg(s3r, variant="point", optimizer="sgd", lr=1e-2, val_every=1, save_every=1,
                                              out_dir=str(tmp_path)), log=lines.append)
    assert len(res["losses"]) == 3 and all(abs(l) < float("inf") for l in res["losses"])
    assert len(lines) == 1 and lines[0]["epoch"] == 0 and lines[0]["step"] == 3 and lines[0]["val"]["samples"] == N and lines[0]["best"]
    assert res["best"] == -lines[0]["val"]["mean_chamfer"] and isinstance(res["optimizer"], s3r.SGD)
    assert os.path.exists(tmp_path / "best.pth") and os.path.exists(tmp_path / "last.pth")
    json.dumps(lines[0])


def test_disparity_supervision_and_the_schedule(s3r):
    ds = _sets(s3r, "voxel", disparity=True)
    plain = _reference_run(s3r)[0]
    cfg = _cfg(s3r, disparity_weight=0.5, epochs=2, milestones=(1,), gamma=0.5, optimizer="adamw", max_steps=4)
    res = s3r.fit(_model(s3r), ds, None, cfg)
    assert len(res["losses"]) == 4 and all(abs(l) < float("inf") for l in res["losses"])
    assert res["losses"][0] > plain[0]                                 # the same first batch and augmentation, plus the disparity terms
    assert s3r.train.learning_rate(cfg, 0) == 1e-3 and s3r.train.learning_rate(cfg, 1) == 5e-4
    assert res["optimizer"].param_groups[0]["lr"] == 5e-4
    assert float(res["optimizer"].device_state().view(torch.float32)[3]) == pytest.approx(5e-4, rel=1e-6)


# ---------------------------------------------------------------- runner.py
def _runner(*args, timeout=400):
    return subprocess.run([sys.executable, os.path.join(ROOT, "runner.py"), *args], capture_output=True, text=True, timeout=timeout, cwd=ROOT)


def test_runner_trains_and_its_checkpoint_evaluates(tmp_path):
    out = tmp_path / "run"
    r = _runner("--train", "--epochs", "1", "--samples", "4", "--batch", "2", "--out", str(out))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    lines = [json.loads(l) for l in r.stdout.strip().splitlines() if l.startswith("{")]
    assert lines[0]["epoch"] == 0 and lines[0]["step"] == 1 and "loss" in lines[0] and "mean_iou" in lines[0]["val"]
    assert lines[-1]["done"] and lines[-1]["steps"] == 1 and lines[-1]["train_samples"] == 2 and lines[-1]["val_samples"] == 2
    last = out / "last.pth"
    assert os.path.exists(last) and os.path.exists(out / "best.pth")
    r = _runner("--test", "--weights", str(last), "--samples", "2", "--batch", "2")
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    res = json.loads(r.stdout.strip().splitlines()[-1])
    assert res["samples"] == 2 and res["weights"] == str(last) and len(res["mean_iou"]) > 0


def test_runner_refuses_what_training_does_not_implement():
    r = _runner("--train", "--gpus", "2", timeout=120)
    assert r.returncode != 0 and "one GPU" in r.stderr and "all-reduce" in r.stderr
    r = _runner("--train", "--precision", "bf16", timeout=120)
    assert r.returncode != 0 and "bf16" in r.stderr
    r = _runner(timeout=120)
    assert r.returncode != 0 and "only --test is implemented" in (r.stderr + r.stdout) and "--train" in (r.stderr + r.stdout)


def test_fit_refuses_what_it_cannot_train(s3r):
    with pytest.raises(RuntimeError, match="bf16"):
        s3r.fit(s3r.Stereo2Voxel("bf16").to(DEV), _sets(s3r), None, _cfg(s3r))
    with pytest.raises(RuntimeError, match="forward/inference path only"):
        s3r.Stereo2Voxel().train()                                     # the modules' mode flag stays refused
    with pytest.raises(ValueError):
        s3r.TrainConfig(optimizer="lion")
