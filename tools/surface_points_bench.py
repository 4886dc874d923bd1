#!/usr/bin/env python3
"""Micro-benchmark of the ground-truth clouds (s3r_voxel_surface_points) at --batch grids of 32^3 and --points points, from cold caches
(256 MB streamed between rounds), HIP events around the call, median and min..max of --rounds, in us; for a radius-12 ball (2688
exposed faces) and for the checkerboard, the most faces a grid can have (98304).

  1. the call (three launches) against its byte model over --hbm TB/s: the grids read once (B x V x 4 bytes), the mask bytes and chunk
     counts written once and read once (2 x B x (V + 4 V / 64) bytes), the clouds written once (B x points x 12 bytes).  At these sizes
     the model is a few microseconds: the call is three launches' latency, and the ratio says so;
  2. the same rule composed from torch eager ops on the device (exposure by shifted comparisons, a cumulative sum over the 6 V face
     bits, searchsorted for the k-th exposed face; draws from torch's generator: the values differ, the work is the same);
  3. the numpy restatement of tests/_surface64.py on ONE host core, per sample: what a loader worker would spend per grid;
  4. with --step: one eager training step of Stereo2Point.differentiable + ChamferDistance at the same batch, and the call's share.

    python tools/surface_points_bench.py [--batch 32] [--points 2048] [--rounds 20] [--hbm 6.29] [--step]
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402
import s3r  # noqa: E402
from tests import _surface64 as R  # noqa: E402

EDGE = 32


def _timed(fn, big, rounds):
    ts = []
    for r in range(rounds + 2):
        big.add_(1.0)                                                          # 256 MB through the caches
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        if r >= 2:
            ts.append(e0.elapsed_time(e1) * 1e3)
    ts.sort()
    return ts[len(ts) // 2], ts[0], ts[-1]


def torch_eager(vol, n_points, gen, threshold=0.5):
    """the rule from torch ops: (B, n_points, 3)"""
    B, D, H, W = vol.shape
    dev = vol.device
    occ = vol > threshold
    pad = torch.nn.functional.pad(occ, (1, 1, 1, 1, 1, 1))
    nb = [pad[:, :-2, 1:-1, 1:-1], pad[:, 2:, 1:-1, 1:-1], pad[:, 1:-1, :-2, 1:-1], pad[:, 1:-1, 2:, 1:-1], pad[:, 1:-1, 1:-1, :-2],
          pad[:, 1:-1, 1:-1, 2:]]
    exposed = torch.stack([occ & ~n for n in nb], -1).view(B, -1)                # (B, 6 V): bit e = 6 v + f
    csum = exposed.to(torch.int32).cumsum(1)
    N = csum[:, -1:]
    w = torch.rand(B, n_points, 3, generator=gen, device=dev)
    k = (w[..., 0] * N).to(torch.int32).clamp_(max=(N - 1).clamp_(min=0))
    e = torch.searchsorted(csum, k + 1).clamp_(max=exposed.shape[1] - 1)
    v, f = e // 6, e % 6
    idx = torch.stack([v // (H * W), (v // W) % H, v % W], -1).float()
    a, side = f // 2, (f % 2).float()
    size = torch.tensor([D, H, W], device=dev).float()
    axes = torch.arange(3, device=dev).view(1, 1, 3)
    normal = axes == a.unsqueeze(-1)
    first = torch.where(a == 0, 1, 0).unsqueeze(-1)
    u = torch.where(axes == first, w[..., 1:2], w[..., 2:3])
    t = torch.where(normal, idx + side.unsqueeze(-1), idx + u)
    p = t / size - 0.5
    return torch.where(N.unsqueeze(-1) > 0, p, torch.zeros_like(p))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--points", type=int, default=2048)
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--hbm", type=float, default=6.29, help="HBM rate of the byte model's bound, TB/s (MI355X measured float4 copy)")
    ap.add_argument("--host-samples", type=int, default=8, help="grids the numpy restatement runs")
    ap.add_argument("--step", action="store_true", help="also time one eager training step at --batch and print the call's share")
    args = ap.parse_args()
    torch.set_num_threads(1)
    dev = torch.device("cuda:0")
    B, P, V = args.batch, args.points, EDGE ** 3
    ids = torch.arange(B, dtype=torch.int64, device=dev)
    big = torch.empty(64 << 20, device=dev)
    model_bytes = B * V * 4 + 2 * B * (V + 4 * V // 64) + B * P * 12
    bound = model_bytes / args.hbm / 1e6
    print(f"{B} grids of {EDGE}^3, {P} points each; {args.rounds} rounds from cold caches, us: median [min .. max]")
    print(f"  byte model {model_bytes / 1e6:.2f} MB (grids {B * V * 4 / 1e6:.2f} + masks and counts twice {2 * B * (V + 4 * V // 64) / 1e6:.2f} "
          f"+ clouds {B * P * 12 / 1e6:.2f}): {bound:.2f} us at {args.hbm} TB/s")
    call_us = {}
    for kind in ("ball", "checkerboard"):
        grid = R.grid(kind, (EDGE,) * 3)
        vol = torch.from_numpy(np.broadcast_to(grid, (B,) + grid.shape).copy()).to(dev)
        mod = s3r.SurfacePoints(P, seed=1)
        mod(vol, ids)
        torch.cuda.synchronize()
        med, lo, hi = _timed(lambda: mod(vol, ids), big, args.rounds)
        call_us[kind] = med
        faces = int(R.faces(grid).size)
        print(f"  {kind + f' ({faces} faces): s3r_voxel_surface_points':60s} {med:9.1f} [{lo:9.1f} .. {hi:9.1f}]   {med / bound:6.1f} x the byte model")
        gen = torch.Generator(device=dev).manual_seed(0)
        torch_eager(vol, P, gen)
        torch.cuda.synchronize()
        med, lo, hi = _timed(lambda: torch_eager(vol, P, gen), big, max(3, args.rounds // 2))
        print(f"  {kind + ': torch eager ops on the device':60s} {med:9.1f} [{lo:9.1f} .. {hi:9.1f}]   {med / call_us[kind]:6.1f} x the call")
        R.surface32(grid[None], [0], P)
        t0 = time.perf_counter()
        for i in range(args.host_samples):
            R.surface32(grid[None], [i], P, seed=1)
        secs = (time.perf_counter() - t0) / args.host_samples
        print(f"  {kind + ': numpy restatement on one host core':60s} {secs * 1e6:9.1f} per sample ({B * secs * 1e6 / call_us[kind]:.0f} x the call per batch)")
    if args.step:
        net = s3r.Stereo2Point()
        net.load_state_dict(s3r.seeded_state_dict(net, seed=4))
        net.to(dev)
        opt = s3r.Adam([p for p in net.parameters() if p.requires_grad], lr=1e-5)
        chamfer = s3r.ChamferDistance()
        g = torch.Generator().manual_seed(0)
        left = torch.randint(0, 256, (B, 3, 224, 224), generator=g, dtype=torch.uint8).to(dev)
        right = torch.randint(0, 256, (B, 3, 224, 224), generator=g, dtype=torch.uint8).to(dev)
        aug = s3r.StereoAugment(s3r.AugmentConfig.default(1))
        grid = R.grid("ball", (EDGE,) * 3)
        vol = torch.from_numpy(np.broadcast_to(grid, (B,) + grid.shape).copy()).to(dev)
        mod = s3r.SurfacePoints(P, seed=1)

        def step():
            l, r = aug(left, right, ids)
            target = mod(vol, ids)
            opt.zero_grad(set_to_none=True)
            loss = chamfer(net.differentiable(l, r), target)
            loss.backward()
            opt.step()

        step()
        torch.cuda.synchronize()
        med, lo, hi = _timed(step, big, max(3, args.rounds // 4))
        print(f"  one eager Stereo2Point training step at {B} pairs, clouds included: {med:9.1f} [{lo:9.1f} .. {hi:9.1f}]; "
              f"the call (ball) is {100 * call_us['ball'] / med:.3f} % of it")


if __name__ == "__main__":
    main()
