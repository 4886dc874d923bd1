"""`fit`: the training loop of `python3 runner.py --train` on the library's own pieces — `StereoAugment` on the device, the whole
network under autograd (`model.differentiable`), the HIP losses, the HIP optimizer step, `evaluate` for validation and
`checkpoint.save_checkpoint` for checkpoints that carry the optimizer.

What a run is a function of: the model's initial state, the data set, `TrainConfig`.  The index order of epoch e is
`torch.randperm(len(train_set), generator=torch.Generator().manual_seed(seed + e))`; the augmentation of a sample depends on (the
augmentation's seed, id = e * len(train_set) + index) only, and so does the ground-truth cloud that variant "point" draws from a
sample's occupancy grid (`SurfacePoints`, seed `cloud_seed`, the same id: a fresh cloud of each shape every epoch); every kernel
of the step sums in a fixed order.  Two runs give the same per-step losses and parameters bit for bit, and a run resumed from a checkpoint continues with the bits of the uninterrupted one.
Nothing is read back from the device inside an epoch: the per-step losses stay on the device until the epoch ends.

The step runs eagerly.  Single GPU, fp32 models only: there is no gradient all-reduce and no bf16 backward.
"""
from __future__ import annotations

import dataclasses
import json
import os
import time
from typing import Callable, List, Optional, Sequence, Tuple

import torch

from . import checkpoint, evaluate
from . import optim as _optim
from .augment import AugmentConfig, StereoAugment
from .graph import PrefetchingLoader
from .ops import ChamferDistance, DisparityLoss, SurfacePoints, VoxelBCELoss

__all__ = ["TrainConfig", "fit", "loss_of_batch", "learning_rate", "epoch_order"]

OPTIMIZERS = ("adam", "adamw", "sgd")


@dataclasses.dataclass
class TrainConfig:
    variant: str = "voxel"                       # "voxel": Stereo2Voxel + VoxelBCELoss; "point": Stereo2Point + ChamferDistance
    epochs: int = 1
    batch: int = 32
    lr: float = 1e-3
    optimizer: str = "adam"                      # adam | adamw | sgd (momentum 0.9)
    weight_decay: float = 0.0
    clip_grad_norm: Optional[float] = None
    milestones: Tuple[int, ...] = ()             # epochs at which the learning rate is multiplied by gamma
    gamma: float = 0.1
    augment: Optional[AugmentConfig] = None      # None: AugmentConfig.identity()
    batch_stats: bool = False                    # BatchNorm on batch statistics (trains bn.weight) instead of folded
    disparity_weight: float = 0.0                # > 0 and a set with disparity maps: + weight * (DisparityLoss left + right)
    val_every: int = 1                           # validate every N epochs (0: never)
    save_every: int = 1                          # write last.pth every N epochs (0: only at the end)
    out_dir: Optional[str] = None                # where last.pth / best.pth go (None: nothing is written)
    resume: Optional[str] = None                 # a checkpoint of save_checkpoint to continue from
    seed: int = 0
    workers: int = 0
    max_steps: Optional[int] = None              # stop (and save) once this many steps have run in total
    cloud_points: int = 2048                     # variant "point" on (D,H,W) grids: points per ground-truth cloud ...
    cloud_seed: int = 0                          # ... and the seed of ops.voxel_surface_points

    def __post_init__(self):
        if self.variant not in ("voxel", "point"):
            raise ValueError(f"variant must be 'voxel' or 'point', got {self.variant!r}")
        if self.optimizer not in OPTIMIZERS:
            raise ValueError(f"optimizer must be one of {OPTIMIZERS}, got {self.optimizer!r}")
        if self.epochs < 0 or self.batch < 1:
            raise ValueError("epochs must be >= 0 and batch >= 1")
        self.milestones = tuple(sorted(int(m) for m in self.milestones))

    def as_dict(self) -> dict:
        d = dataclasses.asdict(self)
        d["milestones"] = list(self.milestones)
        if self.augment is not None:
            d["augment"] = {k: (list(v) if isinstance(v, tuple) else v) for k, v in dataclasses.asdict(self.augment).items()}
        return d


def learning_rate(cfg: TrainConfig, epoch: int) -> float:
    """the multi-step schedule: lr * gamma ^ (milestones that are <= epoch)"""
    return float(cfg.lr) * float(cfg.gamma) ** sum(1 for m in cfg.milestones if m <= epoch)


def epoch_order(n: int, seed: int, epoch: int) -> List[int]:
    return torch.randperm(n, generator=torch.Generator().manual_seed(seed + epoch)).tolist()


def make_optimizer(cfg: TrainConfig, params):
    kw = dict(lr=cfg.lr, weight_decay=cfg.weight_decay, clip_grad_norm=cfg.clip_grad_norm)
    if cfg.optimizer == "sgd":
        return _optim.SGD(params, momentum=0.9, **kw)
    return (_optim.AdamW if cfg.optimizer == "adamw" else _optim.Adam)(params, **kw)


def loss_of_batch(model, cfg: TrainConfig, left, right, target, disp_left=None, disp_right=None, losses=None):
    """the step's loss from augmented fp32 renders: the variant's loss of `model.differentiable`, plus `disparity_weight` times the
    two `DisparityLoss` terms of `model.differentiable_disparity(full_resolution=True)` when maps are given"""
    main, disp = losses or (VoxelBCELoss() if cfg.variant == "voxel" else ChamferDistance(), DisparityLoss())
    loss = main(model.differentiable(left, right, batch_stats=cfg.batch_stats), target)
    if disp_left is not None and cfg.disparity_weight > 0:
        dl, dr = model.differentiable_disparity(left, right, full_resolution=True, batch_stats=cfg.batch_stats)
        loss = loss + cfg.disparity_weight * (disp(dl, disp_left) + disp(dr, disp_right))
    return loss


def _host_batches(ds, order: Sequence[int], batch: int, base_id: int, workers: int):
    """(fields..., ids) host batches over `order`: ids = base_id + index, int64"""
    groups = [list(order[i:i + batch]) for i in range(0, len(order), batch)]
    loader = torch.utils.data.DataLoader(ds, batch_sampler=groups, num_workers=workers, pin_memory=False)
    for idx, fields in zip(groups, loader):
        yield tuple(fields) + (torch.tensor(idx, dtype=torch.int64) + base_id,)


def _tensors_of(ds, limit=None):
    """a map-style set as stacked host tensors (validation lists are small)"""
    if isinstance(ds, (tuple, list)) and all(isinstance(t, torch.Tensor) for t in ds):
        return tuple(ds)
    if isinstance(ds, torch.utils.data.TensorDataset):
        return tuple(ds.tensors)
    n = len(ds) if limit is None else min(len(ds), limit)
    items = [ds[i] for i in range(n)]
    return tuple(torch.stack([it[k] for it in items]) for k in range(len(items[0])))


def validate(model, val_set, cfg: TrainConfig, device) -> dict:
    """`evaluate.test_net` (voxel: score = the best mean IoU over the thresholds) or `evaluate.test_point_net` (point: score =
    minus the mean Chamfer distance) on the inference path; a higher score is better"""
    t = _tensors_of(val_set)
    left, right, target = t[0], t[1], t[2]
    if left.shape[1] == 4:                       # RGBA lists validate composited over white, as the inference path reads them
        from .ops import augment_pair
        ids = torch.zeros(left.shape[0], dtype=torch.int64, device=device)
        out = [augment_pair(left[i:i + cfg.batch].to(device), right[i:i + cfg.batch].to(device), ids[i:i + cfg.batch], AugmentConfig.identity())
               for i in range(0, left.shape[0], cfg.batch)]
        left, right = torch.cat([o[0] for o in out]).cpu(), torch.cat([o[1] for o in out]).cpu()
    if cfg.variant == "point":
        res = evaluate.test_point_net(model, left, right, target, batch=cfg.batch, device=device, cloud_points=cfg.cloud_points,
                                      cloud_seed=cfg.cloud_seed)
        return {"samples": res["samples"], "mean_chamfer": res["mean_chamfer"], "score": -res["mean_chamfer"]}
    res = evaluate.test_net(model, left, right, target, batch=cfg.batch, device=device)
    return {"samples": res["samples"], "thresholds": res["thresholds"], "mean_iou": res["mean_iou"], "score": max(res["mean_iou"])}


def fit(model, train_set, val_set, cfg: TrainConfig, log: Optional[Callable[[dict], None]] = None) -> dict:
    """Train `model` (a Stereo2Voxel or Stereo2Point on the GPU, fp32) on `train_set`, a map-style data set whose items are
    (left, right, target[, disp_left, disp_right]): uint8 renders (3 or 4, H, W), target the (32,32,32) occupancy or the (M,3) cloud
    (variant "point" also takes the occupancy grid and draws `cloud_points` points on its surface on the device, every step).
    `val_set` is such a set, a tuple of stacked tensors, or None.  Returns {"losses": the per-step losses of THIS call as floats,
    "epochs": one record per finished epoch (what `log` received), "step", "epoch", "best", "optimizer", "checkpoint"}."""
    if getattr(model, "precision", "fp32") != "fp32":
        raise RuntimeError("fit trains fp32 models only: there is no bf16 backward")
    device = next(model.parameters()).device
    if device.type != "cuda":
        raise RuntimeError("fit needs the model on the GPU: this path has no CPU fallback")
    n = len(train_set)
    if n == 0:
        raise RuntimeError("fit needs a non-empty training set")
    params = [p for p in model.parameters() if p.requires_grad]
    opt = make_optimizer(cfg, params)
    epoch, step, best = 0, 0, None
    if cfg.resume:
        ck = checkpoint.load_training_checkpoint(cfg.resume)
        model.load_state_dict(ck["model"])
        opt.load_state_dict(ck["optimizer"])
        epoch, step, best = ck["epoch"], ck["step"], ck["best"]
    aug = StereoAugment(cfg.augment or AugmentConfig.identity())
    clouds = SurfacePoints(cfg.cloud_points, cfg.cloud_seed)
    losses_fn = (VoxelBCELoss() if cfg.variant == "voxel" else ChamferDistance(), DisparityLoss())
    per_epoch = -(-n // cfg.batch)
    losses, records, last_path = [], [], None

    def save(name):
        if cfg.out_dir is None:
            return None
        return checkpoint.save_checkpoint(os.path.join(cfg.out_dir, name), model, opt, epoch, step, best, cfg.as_dict())

    stop = False
    while epoch < cfg.epochs and not stop:
        lr = learning_rate(cfg, epoch)
        if any(float(g["lr"]) != lr for g in opt.param_groups):
            opt.set_lr(lr)
        order = epoch_order(n, cfg.seed, epoch)
        done = step - epoch * per_epoch                  # batches of this epoch a resumed run has behind it
        t0 = time.perf_counter()
        pending = []
        host = _host_batches(train_set, order[done * cfg.batch:], cfg.batch, epoch * n, cfg.workers)
        for fields in PrefetchingLoader(host, device):
            if cfg.max_steps is not None and step >= cfg.max_steps:
                stop = True
                break
            ids = fields[-1]
            with_disp = len(fields) >= 6
            out = aug(fields[0], fields[1], ids, *(fields[3:5] if with_disp else ()))
            target = fields[2].float()
            if cfg.variant == "point" and target.dim() == 4:
                target = clouds(target, ids)
            opt.zero_grad(set_to_none=True)
            loss = loss_of_batch(model, cfg, out[0], out[1], target, *(out[2:4] if with_disp else ()), losses=losses_fn)
            loss.backward()
            opt.step()
            pending.append(loss.detach())
            step += 1
        if pending:
            losses += torch.stack(pending).cpu().tolist()                # the epoch's one read-back
        if cfg.max_steps is not None and step >= cfg.max_steps:
            stop = True
        if step < (epoch + 1) * per_epoch:               # stopped inside the epoch: the checkpoint resumes there
            break
        rec = {"epoch": epoch, "step": step, "lr": lr, "loss": sum(losses[-len(pending):]) / max(len(pending), 1),
               "seconds": round(time.perf_counter() - t0, 3)}
        epoch += 1
        if val_set is not None and cfg.val_every and epoch % cfg.val_every == 0:
            val = validate(model, val_set, cfg, device)
            rec["val"] = {k: v for k, v in val.items() if k != "score"}
            if best is None or val["score"] > best:
                best = val["score"]
                rec["best"] = True
                save("best.pth")
        if cfg.save_every and epoch % cfg.save_every == 0:
            last_path = save("last.pth")
        records.append(rec)
        if log is not None:
            log(rec)
    last_path = save("last.pth") or last_path
    return {"losses": losses, "epochs": records, "step": step, "epoch": epoch, "best": best, "optimizer": opt, "checkpoint": last_path}


def json_line(rec: dict) -> None:
    print(json.dumps(rec), flush=True)
