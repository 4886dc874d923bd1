#!/usr/bin/env python3
"""runner.py — the reference's entry point for this path, on the MI355X-native modules.

    python3 runner.py --test --weights=/path/to/Stereo2Voxel.pth          (/root/reference/README.md:91)
    python3 runner.py --test --gpus 8 ...             (starts its own 8 ranks, one process per GPU, as a child)
    python -m torch.distributed.run --nproc-per-node 8 runner.py --test ...   (or under an external launcher)

    python3 runner.py --train --out runs/a [--dataset-root ... | --data x.npz] [--resume runs/a/last.pth]
    python3 runner.py --train|--test --variant point --dataset-root ...   (ground-truth clouds drawn from the tree's 32^3 grids)

`--test` evaluates and `--train` trains (s3r.train.fit: one GPU, fp32; deterministic on-device augmentation, the HIP losses and
optimizer step, validation through the --test path, checkpoints that carry the optimizer; one JSON line per epoch).  `python3
runner.py` with neither says so and exits non-zero.  Without --weights the model
is seeded random-init (BASELINE.json configs[0]); with it the checkpoint goes through
s3r.checkpoint.load_checkpoint (container unwrapping + keymap.json).  There is no dataset in this
environment (README.md:29 is a download link), so the eval list is synthetic unless --data names an
.npz with arrays left, right (N,3,224,224) and volume (N,32,32,32).
"""
import argparse
import json
import os
import socket
import subprocess
import sys

# the host driver of this pool only supports dmabuf IPC: without this RCCL's buffer exchange between the per-GPU
# processes fails with `hipIpcGetMemHandle: invalid argument` (must be set before the HIP runtime starts)
os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser(description="Stereo2Voxel / Stereo2Point evaluation on MI355X")
    ap.add_argument("--test", action="store_true", help="evaluate")
    ap.add_argument("--train", action="store_true", help="train (one GPU, fp32): prints one JSON line per epoch")
    ap.add_argument("--epochs", type=int, default=1, help="--train: epochs to run in total (a resumed run counts from its checkpoint)")
    ap.add_argument("--lr", type=float, default=1e-3, help="--train: learning rate")
    ap.add_argument("--milestones", default="", help="--train: comma-separated epochs at which the learning rate is multiplied by --gamma")
    ap.add_argument("--gamma", type=float, default=0.1, help="--train: the multi-step schedule's factor")
    ap.add_argument("--optimizer", default="adam", choices=["adam", "adamw", "sgd"], help="--train: s3r.Adam, s3r.AdamW or s3r.SGD (momentum 0.9)")
    ap.add_argument("--augment", default="default", choices=["none", "default"],
                    help="--train: none (the renders as they are) or default (s3r.AugmentConfig.default(): shift, channel permutation, "
                         "brightness / contrast / saturation jitter, noise — a transform set this build invented)")
    ap.add_argument("--out", default=None, help="--train: directory for last.pth / best.pth")
    ap.add_argument("--resume", default=None, help="--train: a checkpoint written by an earlier --train run to continue from")
    ap.add_argument("--val-samples", type=int, default=None, help="--train: length of the validation list (default: a tenth, at least 2)")
    ap.add_argument("--weights", default=None, help="checkpoint (.pth) to load")
    ap.add_argument("--keymap", default=None, help="JSON: reference state_dict key -> this build's key")
    ap.add_argument("--suggest-keymap", action="store_true",
                    help="print the key map derived from --weights by tensor order and shape (JSON) and exit; needs no GPU")
    ap.add_argument("--data", default=None, help=".npz with left, right, volume [, disp_left, disp_right]; default: synthetic")
    ap.add_argument("--dataset-root", default=None,
                    help="StereoShapeNet root (ShapeNetStereoRendering/ + ShapeNetVox32/, README.md:73-77)")
    ap.add_argument("--disparity", action="store_true",
                    help="with --dataset-root: also read disp_%%02d_{l,r}.exr and report the disparity end-point error")
    ap.add_argument("--disparity-readout", default="wta", choices=["wta", "soft"],
                    help="disparity read-out the disparity metrics use: wta (default: integer, at feature resolution, against "
                         "28x28 ground truth) or soft (sub-pixel soft-argmin, compared at the ground truth's resolution: the "
                         "224x224 EXR maps as they are, or (N,224,224) / (N,28,28) .npz maps); soft adds the bad-pixel rates")
    ap.add_argument("--disparity-temperature", type=float, default=None,
                    help="temperature of the soft read-out (default: s3r.DISPARITY_TEMPERATURE)")
    ap.add_argument("--variant", default="voxel", choices=["voxel", "point"],
                    help="voxel: Stereo2Voxel + IoU (default); point: Stereo2Point + Chamfer distance (.npz key `points`, "
                         "(N,M,3), or clouds drawn on the device from `volume` / the tree's grids; synthetic clouds otherwise)")
    ap.add_argument("--cloud-points", type=int, default=2048,
                    help="--variant point on occupancy grids: points per ground-truth cloud (s3r.voxel_surface_points)")
    ap.add_argument("--cloud-seed", type=int, default=0, help="--variant point on occupancy grids: the seed of the clouds")
    ap.add_argument("--precision", default="fp32", choices=["fp32", "bf16"], help="fp32 (exact-fp32 MFMA) or the bf16 MFMA path")
    ap.add_argument("--samples", type=int, default=64, help="synthetic eval list length")
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--workers", type=int, default=0, help="with --dataset-root: DataLoader decode workers (PNG / MAT / EXR "
                                                           "decoding is host work: ~300 pairs/s per worker)")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--renders", default="u8", choices=["u8", "f32"],
                    help="dtype of the renders handed to the model: u8 (default: 8-bit, as the PNG decode yields them; the "
                         "first kernel scales by 1/255) or f32 (converted on the host: 4x the bytes across PCIe, same result)")
    ap.add_argument("--force-dist", action="store_true",
                    help="take the multi-rank code path (init_process_group, metric all-gather) even with one rank: a "
                         "world-size-1 RCCL rehearsal on a 1-GPU box")
    ap.add_argument("--backend", default="nccl", choices=["nccl", "gloo"], help="torch.distributed backend (nccl = RCCL)")
    ap.add_argument("--same-device", action="store_true",
                    help="testing only: every rank uses cuda:0 (with --backend gloo) so the N>1 path — at the real world size of "
                         "BASELINE configs[4] — runs on a 1-GPU box")
    ap.add_argument("--gpus", type=int, default=1,
                    help="evaluate on N GPUs of this node: the eval list is sharded over one process per GPU (RCCL "
                         "all-gather of the per-sample metrics); runner.py starts the ranks itself")
    args = ap.parse_args()
    if args.disparity_temperature is not None and args.disparity_readout != "soft":
        sys.exit("--disparity-temperature needs --disparity-readout soft")
    if args.disparity_temperature is not None and not (0 < args.disparity_temperature < float("inf")):
        sys.exit("--disparity-temperature must be finite and > 0")
    if args.same_device and args.backend == "nccl" and max(args.gpus, int(os.environ.get("WORLD_SIZE", "1"))) > 1:
        sys.exit("--same-device puts every rank on cuda:0, which RCCL refuses (one communicator rank per device): "
                 "use --backend gloo with it")
    if args.test and (args.gpus > 1 or args.force_dist) and "WORLD_SIZE" not in os.environ:
        # single-process entry point (README.md:85,91) kept: the ranks are a CHILD process started before anything
        # here touches the GPU (never exec from a process that has); rank 0's JSON line reaches our stdout
        with socket.socket() as sk:
            sk.bind(("127.0.0.1", 0))
            port = sk.getsockname()[1]
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={max(1, args.gpus)}",
               "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
        # (one process per GPU shares the host: a few intra-op threads each, as bench.py's launcher sets)
        env = dict(os.environ, MASTER_ADDR="127.0.0.1", OMP_NUM_THREADS=os.environ.get("OMP_NUM_THREADS", "4"))
        sys.exit(subprocess.run(cmd, env=env).returncode)
    if args.suggest_keymap:
        import torch
        import s3r
        if not args.weights:
            sys.exit("--suggest-keymap needs --weights")
        m = s3r.Stereo2Voxel(args.precision) if args.variant == "voxel" else s3r.Stereo2Point(args.precision)
        print(json.dumps(s3r.checkpoint.suggest_keymap(torch.load(args.weights, map_location="cpu", weights_only=True), m),
                         indent=1))
        return
    if args.train:
        if args.test:
            sys.exit("runner.py: --train and --test are two runs: name one")
        if args.gpus > 1 or int(os.environ.get("WORLD_SIZE", "1")) > 1 or args.force_dist:
            sys.exit("runner.py --train runs on one GPU: there is no gradient all-reduce (--gpus > 1 is for --test)")
        if args.precision != "fp32":
            sys.exit("runner.py --train trains fp32 models only: there is no bf16 backward")
        return train_main(args)
    if not args.test:
        sys.exit("runner.py: only --test is implemented for evaluation, and --train for training: name one of them")

    import numpy as np
    import torch
    import s3r

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = 0 if args.same_device else int(os.environ.get("LOCAL_RANK", "0"))
    if not torch.cuda.is_available():
        sys.exit("runner.py --test needs an MI355X: this path has no CPU fallback")
    if (world > 1 and not args.same_device) or local_rank != 0 or args.force_dist:
        # (not in a plain single-process run: with the current device set explicitly the look-ahead page-locking of the eval
        #  loop no longer overlaps the GPU work on this runtime — bf16, 3072 pairs at batch 256: 22.0-24.5 k pairs/s with
        #  the call, 32.6 k without; same box, alternating runs)
        torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)
    dist_on = world > 1 or args.force_dist
    if dist_on:
        import torch.distributed as dist
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if args.backend == "nccl":
            dist.init_process_group("nccl", rank=rank, world_size=world, device_id=dev)
        else:
            dist.init_process_group("gloo", rank=rank, world_size=world)

    model = s3r.Stereo2Voxel(args.precision) if args.variant == "voxel" else s3r.Stereo2Point(args.precision)
    if args.weights:
        keymap = json.load(open(args.keymap)) if args.keymap else None
        s3r.checkpoint.load_checkpoint(model, args.weights, keymap)
    else:
        s3r.seed_module(model, args.seed)
    model.to(dev)

    import time
    with torch.no_grad():          # one-time work (weight packing, the batch-size layout of the activation arena,
        wb = max(1, min(args.batch, 256))                          # library init) stays out of the rate
        if args.renders == "u8":
            model(torch.randint(0, 256, (wb, 3, 224, 224), dtype=torch.uint8, device=dev),
                  torch.randint(0, 256, (wb, 3, 224, 224), dtype=torch.uint8, device=dev))
        else:
            model(torch.rand(wb, 3, 224, 224, device=dev), torch.rand(wb, 3, 224, 224, device=dev))
        # ... and so does the metric path's (copy stream, pinned staging, the IoU / Chamfer / read-out kernels' first
        # launches): one tiny untimed pass of the same driver
        # (two samples PER RANK: the eval drivers shard the list over the ranks, and a rank with an empty shard would
        # meet its first metric launches inside the timed region)
        nw = 2 * max(1, int(os.environ.get("WORLD_SIZE", "1")))
        ws = s3r.evaluate.synthetic_eval_set(nw, 1, "uint8" if args.renders == "u8" else "float32")
        if args.variant == "point":
            s3r.evaluate.test_point_net(model, ws[0], ws[1], torch.rand(nw, 2048, 3) - 0.5, batch=2, device=dev)
        else:
            s3r.evaluate.test_net(model, ws[0], ws[1], ws[2], batch=2, device=dev)
            if args.disparity_readout == "soft":                # (the soft read-out's first launch as well)
                model.disparity(ws[0][:2].to(dev), ws[1][:2].to(dev), readout="soft", full_resolution=True)
        zeros = torch.zeros(wb, 3, 224, 224, dtype=ws[0].dtype, device=dev)
        model(zeros, zeros)                                     # back to the eval batch's arena layout
        del zeros
    torch.cuda.synchronize()
    clock = {"t": 0.0}

    def timed(fn, *a, **kw):       # the eval loop alone: host batches -> device, forward, metric, collation
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn(*a, **kw)
        torch.cuda.synchronize()
        clock["t"] += time.perf_counter() - t0
        return out

    def rate(n):
        return round(n / max(clock["t"], 1e-9), 1)

    rdt = "uint8" if args.renders == "u8" else "float32"

    def renders(a):                 # an .npz array of renders in the requested dtype (uint8 arrays are 8-bit renders)
        t = torch.from_numpy(a)
        if t.dtype == torch.uint8:
            return t if args.renders == "u8" else s3r.data.renders_to_float(t)
        return t.float()            # already scaled to [0,1]: stays fp32 whatever --renders says

    def dist_info():
        if not dist_on:
            return {}
        rccl = None
        if args.backend == "nccl":
            try:
                rccl = ".".join(str(v) for v in torch.cuda.nccl.version())
            except Exception:
                rccl = None
        one = torch.ones(1, dtype=torch.int64, device=dev)
        dist.all_reduce(one)
        return {"collective_backend": args.backend, "rccl_version": rccl, "n_ranks_seen": int(one.item())}

    if args.variant == "point":
        cloud_kw = dict(cloud_points=args.cloud_points, cloud_seed=args.cloud_seed)
        if args.dataset_root:
            ds = s3r.data.StereoShapeNet(args.dataset_root, render_dtype=rdt)
            res = timed(s3r.evaluate.test_point_dataset, model, ds, batch=args.batch, device=dev, workers=args.workers, **cloud_kw)
            left = None
        else:
            if args.data:
                z = np.load(args.data)
                left, right = renders(z["left"]), renders(z["right"])
                clouds = torch.from_numpy(z["points" if "points" in z.files else "volume"]).float()
            else:
                left, right, _ = s3r.evaluate.synthetic_eval_set(args.samples, args.seed, rdt)
                clouds = torch.rand(args.samples, 2048, 3, generator=torch.Generator().manual_seed(args.seed)) - 0.5
            res = timed(s3r.evaluate.test_point_net, model, left, right, clouds, batch=args.batch, device=dev, **cloud_kw)
        info = dist_info()
        if rank == 0:
            print(json.dumps(dict({"samples": res["samples"], "n_gpus": world, "mean_chamfer": round(res["mean_chamfer"], 8),
                                   "precision": args.precision, "eval_pairs_per_s": rate(res["samples"]),
                                   "renders": rdt if left is None else str(left.dtype).replace("torch.", ""),
                                   "weights": args.weights or f"seeded random init (seed {args.seed})",
                                   "data": args.dataset_root or args.data or "synthetic"},
                                  **({"per_taxonomy": {k: {"samples": v["samples"], "mean_chamfer": round(v["mean_chamfer"], 8)}
                                                       for k, v in res["per_taxonomy"].items()}} if "per_taxonomy" in res else {}),
                                  **info)))
        if dist_on:
            dist.destroy_process_group()
        return

    disp = None
    if args.dataset_root:
        ds = s3r.data.StereoShapeNet(args.dataset_root, with_disparity=args.disparity, render_dtype=rdt)
        res = timed(s3r.evaluate.test_dataset, model, ds, batch=args.batch, device=dev, workers=args.workers,
                    disparity_readout=args.disparity_readout, disparity_temperature=args.disparity_temperature)
        left = None
        if args.disparity:
            disp = res
    elif args.data:
        z = np.load(args.data)
        left, right, gt = renders(z["left"]), renders(z["right"]), torch.from_numpy(z["volume"]).float()
    else:
        left, right, gt = s3r.evaluate.synthetic_eval_set(args.samples, args.seed, rdt)
    if left is not None:
        res = timed(s3r.evaluate.test_net, model, left, right, gt, batch=args.batch, device=dev)
        if args.data and "disp_left" in z.files and "disp_right" in z.files:
            # ground-truth disparity in render pixels, (N,28,28) at feature resolution (soft: or (N,224,224)); inf / negative =
            # invalid
            disp = s3r.evaluate.test_disparity(model, left, right, torch.from_numpy(z["disp_left"]).float(),
                                               torch.from_numpy(z["disp_right"]).float(), batch=args.batch, device=dev,
                                               readout=args.disparity_readout, temperature=args.disparity_temperature)
    info = dist_info()
    if rank == 0:
        out = {"samples": res["samples"], "n_gpus": world, "thresholds": res["thresholds"],
               "mean_iou": [round(x, 6) for x in res["mean_iou"]],
               "precision": args.precision, "eval_pairs_per_s": rate(res["samples"]),
               "renders": rdt if left is None else str(left.dtype).replace("torch.", ""),
               "weights": args.weights or f"seeded random init (seed {args.seed})",
               "data": args.dataset_root or args.data or "synthetic"}
        if "per_taxonomy" in res:
            out["per_taxonomy"] = {k: {"samples": v["samples"], "mean_iou": [round(x, 6) for x in v["mean_iou"]]}
                                   for k, v in res["per_taxonomy"].items()}
        if disp is not None:
            out.update({"disparity_epe_left_px": round(disp["epe_left"], 4), "disparity_epe_right_px": round(disp["epe_right"], 4)})
            if args.disparity_readout == "soft":
                out["disparity_readout"] = "soft"
                out.update({f"disparity_{k}_{side}_pct": round(disp[f"{k}_{side}"], 4)
                            for k in ("bad1", "bad3", "d1") for side in ("left", "right")})
        out.update(info)
        print(json.dumps(out))
    if dist_on:
        dist.destroy_process_group()


def train_main(args):
    import numpy as np
    import torch
    import s3r
    from s3r import train as T

    if not torch.cuda.is_available():
        sys.exit("runner.py --train needs an MI355X: this path has no CPU fallback")
    dev = torch.device("cuda", 0)
    model = s3r.Stereo2Voxel("fp32") if args.variant == "voxel" else s3r.Stereo2Point("fp32")
    if args.weights:
        s3r.checkpoint.load_checkpoint(model, args.weights, json.load(open(args.keymap)) if args.keymap else None)
    else:
        s3r.seed_module(model, args.seed)
    model.to(dev)

    if args.dataset_root:
        full = s3r.data.StereoShapeNet(args.dataset_root, with_disparity=args.disparity, render_channels=4 if args.augment == "default" else 3)
        n = len(full)
    else:
        if args.data:
            z = np.load(args.data)
            fields = [torch.from_numpy(z["left"]), torch.from_numpy(z["right"]),
                      torch.from_numpy(z["points" if args.variant == "point" and "points" in z.files else "volume"]).float()]
            if fields[0].dtype != torch.uint8:
                sys.exit("runner.py --train reads 8-bit renders: the .npz arrays left / right must be uint8")
            if "disp_left" in z.files and "disp_right" in z.files and tuple(z["disp_left"].shape[1:]) == tuple(fields[0].shape[2:]):
                fields += [torch.from_numpy(z["disp_left"]).float(), torch.from_numpy(z["disp_right"]).float()]
        else:
            left, right, gt = s3r.evaluate.synthetic_eval_set(args.samples, args.seed, "uint8")
            if args.variant == "point":
                gt = torch.rand(args.samples, 2048, 3, generator=torch.Generator().manual_seed(args.seed)) - 0.5
            fields = [left, right, gt]
        full = torch.utils.data.TensorDataset(*fields)
        n = fields[0].shape[0]
    n_val = min(n - 1, args.val_samples if args.val_samples is not None else max(2, n // 10))
    if n_val > 0:                                        # the LAST n_val items of the list validate, the rest train
        train_set = torch.utils.data.Subset(full, range(n - n_val))
        val_set = torch.utils.data.Subset(full, range(n - n_val, n))
    else:
        train_set, val_set = full, None
    with_disp = len(full[0]) >= 5
    cfg = T.TrainConfig(variant=args.variant, epochs=args.epochs, batch=args.batch, lr=args.lr, optimizer=args.optimizer,
                        milestones=tuple(int(m) for m in args.milestones.split(",") if m.strip()), gamma=args.gamma,
                        augment=s3r.AugmentConfig.default(args.seed) if args.augment == "default" else s3r.AugmentConfig.identity(args.seed),
                        disparity_weight=1.0 if with_disp else 0.0, out_dir=args.out, resume=args.resume, seed=args.seed, workers=args.workers,
                        cloud_points=args.cloud_points, cloud_seed=args.cloud_seed)
    res = T.fit(model, train_set, val_set, cfg, log=T.json_line)
    print(json.dumps({"done": True, "epochs": res["epoch"], "steps": res["step"], "best": res["best"], "checkpoint": res["checkpoint"],
                      "train_samples": len(train_set), "val_samples": 0 if val_set is None else len(val_set)}))


if __name__ == "__main__":
    main()
