"""Eval driver of the path: what `runner.py --test` does after building the model
(/root/reference/README.md:88-92) — forward over an eval list, thresholded IoU per sample, mean per
threshold — with the forward on the HIP modules and the IoU reduced on the device, so that multi-GPU
collation gathers a few scalars per sample instead of 32^3 grids.

The reference's threshold list and IoU formula are not in the mount; this build evaluates
IoU = |pred>t & gt| / |pred>t | gt| (binary ground truth) at t in THRESHOLDS (build-specified) and labels it so.
"""
from __future__ import annotations

from typing import Dict, Iterable, Optional, Sequence, Tuple

import torch

from . import arch_spec as spec
from . import collate
from .modules import READOUTS
from .ops import chamfer_distance, disparity_metrics, voxel_iou, voxel_surface_points

THRESHOLDS = (0.2, 0.3, 0.4, 0.5)


def _device_batches(tensors: Sequence[torch.Tensor], b0: int, e0: int, batch: int, device):
    """[b0, e0) of a host-resident eval list as device batches.  Each batch's slices are page-locked IN PLACE
    (hipHostRegister, no copy), so they are DMA-able at PCIe rate (~55 GB/s here against 4.6 GB/s from pageable memory)
    and the next batch crosses on a side stream while the current one runs (graph.PrefetchingLoader).  A plain
    `.to(device)` per batch made this loop 10x slower than the forward.  Page-locking costs ~0.04 ms per MB — 0.12 s for a
    4 GB list of fp32 renders when done for the whole list before the first kernel starts (r02) — so it is done PER BATCH,
    one registration per slice (a copy must lie inside ONE registration: tools/reg_debug.py), by the loader's look-ahead:
    the pages of batch i+1 are locked while batch i-1 runs on the GPU.  (Measured, bf16 path, 3072 pairs at batch 256:
    31.9 k pairs/s with 8-bit renders, 14.1 k with fp32 renders — 13 ms of page-locking per batch against a 6.5 ms
    forward; a helper thread locking ahead of the loop made both worse, 21.0 k / 9.9 k.)"""
    from .graph import PrefetchingLoader
    if torch.device(device).type != "cuda" or any(t.is_cuda for t in tensors):
        for s in range(b0, e0, batch):
            yield tuple(t[s:min(e0, s + batch)].to(device) for t in tensors)
        return
    rt = torch.cuda.cudart()
    locked = []                                               # addresses registered so far
    lockable = [bool(t.numel()) and t.is_contiguous() and not t.is_pinned() for t in tensors]

    def host():
        for s in range(b0, e0, batch):
            e = min(e0, s + batch)
            out = []
            for i, t in enumerate(tensors):
                sl = t[s:e]
                if lockable[i] and sl.numel():
                    if int(rt.cudaHostRegister(sl.data_ptr(), sl.numel() * sl.element_size(), 0)) == 0:
                        locked.append(sl.data_ptr())
                    else:                                     # not lockable: the loader stages this tensor through its ring
                        lockable[i] = False
                        _clear_hip_error()
                out.append(sl)
            yield tuple(out)

    try:
        yield from PrefetchingLoader(host(), device)
    finally:
        torch.cuda.synchronize(device)
        for ptr in locked:
            rt.cudaHostUnregister(ptr)


def _clear_hip_error():
    """A failed hipHostRegister leaves its code in the runtime's sticky last-error slot, where the next unrelated torch
    call would find (and raise) it: read it out."""
    try:
        import ctypes
        ctypes.CDLL("libamdhip64.so").hipGetLastError()
    except OSError:                                           # pragma: no cover
        pass


def synthetic_eval_set(n: int, seed: int = 0, render_dtype: str = "float32") -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """n synthetic (left, right, ground-truth 32^3 occupancy) triples: there is no dataset in this
    container (README.md:29 is a download link).  GT is a random axis-aligned box per sample.
    render_dtype="uint8": 8-bit renders (uniform 0..255), what a decoded PNG list looks like."""
    g = torch.Generator().manual_seed(seed)
    if render_dtype == "uint8":
        left = torch.randint(0, 256, (n, 3, 224, 224), generator=g, dtype=torch.uint8)
        right = torch.randint(0, 256, (n, 3, 224, 224), generator=g, dtype=torch.uint8)
    else:
        left, right = torch.rand(n, 3, 224, 224, generator=g), torch.rand(n, 3, 224, 224, generator=g)
    gt = torch.zeros(n, 32, 32, 32)
    lo = torch.randint(0, 12, (n, 3), generator=g)
    hi = lo + torch.randint(8, 20, (n, 3), generator=g)
    for i in range(n):
        gt[i, lo[i, 0]:hi[i, 0], lo[i, 1]:hi[i, 1], lo[i, 2]:hi[i, 2]] = 1.0
    return left, right, gt


# per-sample disparity rows (float64: integer counts stay exact): epe_l, n_l, epe_r, n_r, then >1 px, >3 px, D1 counts left, right
_DISP_COLS = 10


def _disparity_rows(model, l, r, gl, gr, readout: str, temperature) -> torch.Tensor:
    """the model's (left, right) read-out against ground truth gl / gr of one device batch -> (n, _DISP_COLS) float64 rows.
    readout="soft" reads out at the ground truth's resolution: (n,224,224) render-resolution maps or (n,28,28) feature-resolution
    ones; "wta" predicts at feature resolution only."""
    if readout not in READOUTS:
        raise ValueError(f"readout must be one of {READOUTS}, got {readout!r}")
    if readout == "soft":
        full = tuple(gl.shape[-2:]) == (spec.IMG_HW, spec.IMG_HW)
        if not full and tuple(gl.shape[-2:]) != (spec.FEAT_HW, spec.FEAT_HW):
            raise ValueError(f"soft read-out: ground truth must be (N,{spec.IMG_HW},{spec.IMG_HW}) or (N,{spec.FEAT_HW},{spec.FEAT_HW}), "
                             f"got {tuple(gl.shape)}")
        dl, dr = model.disparity(l, r, readout="soft", temperature=temperature, full_resolution=full)
    else:
        dl, dr = model.disparity(l, r)
    el, cl = disparity_metrics(dl, gl)
    er, cr = disparity_metrics(dr, gr)
    cl, cr = cl.double(), cr.double()
    return torch.cat([torch.stack([el.double(), cl[:, 0], er.double(), cr[:, 0]], 1), cl[:, 1:], cr[:, 1:]], 1)


def _disparity_pooled(rows: torch.Tensor) -> Dict[str, object]:
    """EPE pooled over every valid pixel of the list and the bad-pixel rates (percent of valid pixels) from the integer counts"""
    out: Dict[str, object] = {}
    for side, e, n, c0 in (("left", 0, 1, 4), ("right", 2, 3, 7)):
        nv = rows[:, n].sum().item()
        out[f"epe_{side}"] = (rows[:, e] * rows[:, n]).sum().item() / nv if nv else float("nan")
        out[f"valid_{side}"] = int(nv)
        for k, name in enumerate(("bad1", "bad3", "d1")):
            out[f"{name}_{side}"] = 100.0 * rows[:, c0 + k].sum().item() / nv if nv else float("nan")
    return out


@torch.no_grad()
def test_dataset(model, ds, batch: int = 32, thresholds: Sequence[float] = THRESHOLDS, device="cuda", group=None,
                 workers: int = 0, disparity_readout: str = "wta", disparity_temperature: Optional[float] = None) -> Dict[str, object]:
    """test_net over a data.StereoShapeNet: each rank decodes and evaluates only its shard_bounds slice of the item
    list, host batches cross PCIe on a copy stream while the previous batch runs (graph.PrefetchingLoader), and the
    per-sample IoUs are all-gathered in list order.  A dataset built with_disparity=True also yields the end-point error
    and bad-pixel rates of the model's disparity read-out against the EXR ground truth, pooled over valid pixels (see
    test_disparity): disparity_readout="wta" against the maps block-averaged to 28x28 (downsample_disparity), "soft" against
    the 224x224 maps as they are."""
    import torch.distributed as dist
    from . import data as _data
    from .graph import PrefetchingLoader
    dist_on = dist.is_available() and dist.is_initialized()
    world = dist.get_world_size(group) if dist_on else 1
    rank = dist.get_rank(group) if dist_on else 0
    total = len(ds)
    b0, e0 = collate.shard_bounds(total, world, rank)
    ious = torch.empty((e0 - b0, len(thresholds)), dtype=torch.float32, device=device)
    with_disp = bool(getattr(ds, "with_disparity", False))
    if with_disp and disparity_readout not in READOUTS:
        raise ValueError(f"disparity_readout must be one of {READOUTS}, got {disparity_readout!r}")
    rows = torch.zeros((e0 - b0, _DISP_COLS), dtype=torch.float64, device=device)
    host = _data.batches(ds, batch, range(b0, e0), workers)
    done = 0
    for item in PrefetchingLoader(host, device):
        l, r, g = item[:3]
        pred = model(l, r)
        for j, t in enumerate(thresholds):
            ious[done:done + l.shape[0], j] = voxel_iou(pred, g, t)
        if with_disp:
            gl, gr = item[3], item[4]
            if disparity_readout == "wta":
                gl, gr = _data.downsample_disparity(gl, spec.FEAT_HW), _data.downsample_disparity(gr, spec.FEAT_HW)
            rows[done:done + l.shape[0]] = _disparity_rows(model, l, r, gl, gr, disparity_readout, disparity_temperature)
        done += l.shape[0]
    if dist_on:
        ious = collate.all_gather_ragged(ious, total, group)
        if with_disp:
            rows = collate.all_gather_ragged(rows, total, group)
    mean = ious.mean(0).cpu().tolist() if total else [float("nan")] * len(thresholds)
    out = {"samples": total, "thresholds": list(thresholds), "mean_iou": mean, "per_sample": ious.cpu()}
    # per-taxonomy breakdown (what a ShapeNet test log lists): mean IoU per threshold and sample count per category
    per_tax: Dict[str, Dict[str, object]] = {}
    cpu = out["per_sample"]
    for tax in sorted({it[0] for it in getattr(ds, "items", [])}):
        idx = [i for i, it in enumerate(ds.items) if it[0] == tax]
        per_tax[tax] = {"samples": len(idx), "mean_iou": cpu[idx].mean(0).tolist()}
    out["per_taxonomy"] = per_tax
    if with_disp:
        pooled = _disparity_pooled(rows.cpu())
        out.update({k: v for k, v in pooled.items() if not k.startswith("valid_")})
        out["disparity_readout"] = disparity_readout
    return out


def _chamfer_rows(model, l, r, g, first_id: int, cloud_points: int, cloud_seed: int) -> torch.Tensor:
    """per-sample Chamfer distance of one device batch; (n,D,H,W) ground-truth grids become clouds first, sample i with id first_id + i"""
    if g.dim() == 4:
        ids = torch.arange(first_id, first_id + g.shape[0], dtype=torch.int64, device=g.device)
        g = voxel_surface_points(g.float(), ids, cloud_points, cloud_seed)
    d1, d2, _, _ = chamfer_distance(model(l, r), g)
    return d1.mean(1) + d2.mean(1)


@torch.no_grad()
def test_point_net(model, left: torch.Tensor, right: torch.Tensor, gt_clouds: torch.Tensor, batch: int = 32, device="cuda",
                   group=None, cloud_points: int = 2048, cloud_seed: int = 0) -> Dict[str, object]:
    """Stereo2Point's metric (the reference's one native op, extensions/chamfer_dist, README.md:59-66): per-sample
    Chamfer distance mean_i min_j |p_i - q_j|^2 + mean_j min_i |p_i - q_j|^2 between the predicted (N,2048,3) cloud and
    the ground-truth (N,M,3) cloud, on the device; with torch.distributed initialised the per-sample scalars of every
    rank's shard are all-gathered in list order.  (Squared / mean is this build's stated choice — SURVEY.md §8a row 5.)
    gt_clouds may also be (N,D,H,W) occupancy grids: each batch's clouds are then drawn on the device (ops.voxel_surface_points,
    cloud_points points, seed cloud_seed, id = the sample's index in the list), so a validation list's clouds are fixed."""
    import torch.distributed as dist
    dist_on = dist.is_available() and dist.is_initialized()
    world = dist.get_world_size(group) if dist_on else 1
    rank = dist.get_rank(group) if dist_on else 0
    total = left.shape[0]
    b0, e0 = collate.shard_bounds(total, world, rank)
    cd = torch.empty((e0 - b0,), dtype=torch.float32, device=device)
    done = 0
    for l, r, g in _device_batches((left, right, gt_clouds), b0, e0, batch, device):
        cd[done:done + l.shape[0]] = _chamfer_rows(model, l, r, g, b0 + done, cloud_points, cloud_seed)
        done += l.shape[0]
    if dist_on:
        cd = collate.all_gather_ragged(cd, total, group)
    return {"samples": total, "mean_chamfer": cd.mean().item() if total else float("nan"), "per_sample": cd.cpu()}


@torch.no_grad()
def test_point_dataset(model, ds, batch: int = 32, device="cuda", group=None, workers: int = 0, cloud_points: int = 2048,
                       cloud_seed: int = 0) -> Dict[str, object]:
    """test_point_net over a data.StereoShapeNet, as test_dataset is test_net over one: each rank decodes and evaluates its
    shard_bounds slice, host batches cross PCIe on a copy stream (graph.PrefetchingLoader), the ground-truth clouds are drawn on the
    device from the tree's occupancy grids (id = the item's index in the list) and the per-sample Chamfer distances are all-gathered in
    list order; per_taxonomy lists the mean Chamfer distance and sample count per category."""
    import torch.distributed as dist
    from . import data as _data
    from .graph import PrefetchingLoader
    dist_on = dist.is_available() and dist.is_initialized()
    world = dist.get_world_size(group) if dist_on else 1
    rank = dist.get_rank(group) if dist_on else 0
    total = len(ds)
    b0, e0 = collate.shard_bounds(total, world, rank)
    cd = torch.empty((e0 - b0,), dtype=torch.float32, device=device)
    done = 0
    for item in PrefetchingLoader(_data.batches(ds, batch, range(b0, e0), workers), device):
        l, r, g = item[:3]
        cd[done:done + l.shape[0]] = _chamfer_rows(model, l, r, g, b0 + done, cloud_points, cloud_seed)
        done += l.shape[0]
    if dist_on:
        cd = collate.all_gather_ragged(cd, total, group)
    cpu = cd.cpu()
    per_tax: Dict[str, Dict[str, object]] = {}
    for tax in sorted({it[0] for it in getattr(ds, "items", [])}):
        idx = [i for i, it in enumerate(ds.items) if it[0] == tax]
        per_tax[tax] = {"samples": len(idx), "mean_chamfer": cpu[idx].mean().item()}
    return {"samples": total, "mean_chamfer": cpu.mean().item() if total else float("nan"), "per_sample": cpu, "per_taxonomy": per_tax}


@torch.no_grad()
def test_disparity(model, left: torch.Tensor, right: torch.Tensor, disp_l_gt: torch.Tensor, disp_r_gt: torch.Tensor,
                   batch: int = 32, device="cuda", group=None, readout: str = "wta",
                   temperature: Optional[float] = None) -> Dict[str, object]:
    """End-point error and bad-pixel rates of the model's predicted left / right disparity (Stereo2Voxel.disparity, render
    pixels) against ground-truth maps in render pixels (the dataset's disp_%02d_{l,r}.exr,
    /root/reference/README.md:75-76; invalid pixels: inf / negative).  readout="wta": (N,28,28) ground truth at feature
    resolution (downsampled by the caller).  readout="soft": the sub-pixel read-out at `temperature` (default: the model's
    disparity_temperature) compared at the ground truth's own resolution, (N,224,224) render resolution or (N,28,28).
    EPE is pooled over all valid pixels of the list, and bad1 / bad3 / d1 (percent of valid pixels with |err| > 1 px, > 3 px,
    > 3 px and > 5 % of the ground truth) from integer counts: per-sample rows are reduced on the device and, with
    torch.distributed initialised, all-gathered (rank order = list order)."""
    import torch.distributed as dist
    dist_on = dist.is_available() and dist.is_initialized()
    world = dist.get_world_size(group) if dist_on else 1
    rank = dist.get_rank(group) if dist_on else 0
    total = left.shape[0]
    b0, e0 = collate.shard_bounds(total, world, rank)
    if readout not in READOUTS:
        raise ValueError(f"readout must be one of {READOUTS}, got {readout!r}")
    rows = torch.zeros((e0 - b0, _DISP_COLS), dtype=torch.float64, device=device)
    done = 0
    for l, r, gl, gr in _device_batches((left, right, disp_l_gt, disp_r_gt), b0, e0, batch, device):
        rows[done:done + l.shape[0]] = _disparity_rows(model, l, r, gl, gr, readout, temperature)
        done += l.shape[0]
    if dist_on:
        rows = collate.all_gather_ragged(rows, total, group)
    rows = rows.cpu()
    out = {"samples": total, "readout": readout}
    out.update(_disparity_pooled(rows))
    out["per_sample"] = rows[:, :4]                                        # epe_l, n_l, epe_r, n_r
    out["counts"] = torch.stack([rows[:, [1, 4, 5, 6]], rows[:, [3, 7, 8, 9]]], 1).long()   # (N, left/right, 4)
    return out


@torch.no_grad()
def test_net(model, left: torch.Tensor, right: torch.Tensor, gt: torch.Tensor, batch: int = 32,
             thresholds: Sequence[float] = THRESHOLDS, device="cuda", group=None) -> Dict[str, object]:
    """Mean IoU per threshold over the eval list.  With torch.distributed initialised every rank
    evaluates its shard_bounds slice and the per-sample IoUs are all-gathered (rank order = list order)."""
    import torch.distributed as dist
    dist_on = dist.is_available() and dist.is_initialized()
    world = dist.get_world_size(group) if dist_on else 1
    rank = dist.get_rank(group) if dist_on else 0
    total = left.shape[0]
    b0, e0 = collate.shard_bounds(total, world, rank)
    ious = torch.empty((e0 - b0, len(thresholds)), dtype=torch.float32, device=device)
    done = 0
    for l, r, g in _device_batches((left, right, gt), b0, e0, batch, device):
        pred = model(l, r)
        for j, t in enumerate(thresholds):
            # the device kernel thresholds both operands at t; GT is binary {0,1}, so gt > t == (gt == 1)
            ious[done:done + l.shape[0], j] = voxel_iou(pred, g, t)
        done += l.shape[0]
    if dist_on:
        ious = collate.all_gather_ragged(ious, total, group)
    mean = ious.mean(0).cpu().tolist() if total else [float("nan")] * len(thresholds)
    return {"samples": total, "thresholds": list(thresholds), "mean_iou": mean, "per_sample": ious.cpu()}
