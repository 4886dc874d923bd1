#!/usr/bin/env python3
"""Micro-benchmark of the stereo augmentation (s3r_augment_pair) at --batch pairs of 224 x 224 RGBA renders, every op on, from cold
caches (256 MB streamed between rounds), HIP events around the call, median and min..max of --rounds, in us.

  1. the call (three launches with contrast) against its byte model over --hbm TB/s: the 8-bit source read twice (the luma pass and
     the apply pass: 2 x B x 2 x 4 x S bytes) and the fp32 output written once (B x 2 x 3 x S x 4 bytes);
  2. the same transform set composed from torch eager ops on the device (per-sample parameters drawn with torch's generator: the
     values differ, the work is the same);
  3. a numpy version on ONE host core, in pairs/s: what a loader worker would spend per pair in front of the PCIe copy;
  4. with --step: one eager training step of Stereo2Voxel.differentiable at the same batch, and the call's share of it.

    python tools/augment_bench.py [--batch 32] [--rounds 20] [--hbm 6.29] [--step]
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

H = W = 224
LUMA = (0.299, 0.587, 0.114)


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


def torch_eager(left, right, cfg, gen):
    """the transform set from torch ops, both views sharing the per-pair parameters"""
    B = left.shape[0]
    dev = left.device
    k = cfg.max_shift
    dy = torch.randint(-k, k + 1, (B, 1, 1), generator=gen, device=dev)
    dx = torch.randint(-k, k + 1, (B, 1, 1), generator=gen, device=dev)
    ys = torch.arange(H, device=dev).view(1, H, 1) - dy
    xs = torch.arange(W, device=dev).view(1, 1, W) - dx
    inside = ((ys >= 0) & (ys < H) & (xs >= 0) & (xs < W)).unsqueeze(1)
    flat = (ys.clamp(0, H - 1) * W + xs.clamp(0, W - 1)).view(B, 1, H * W)
    bg = torch.randint(cfg.background[0], cfg.background[1] + 1, (B, 3, 1, 1), generator=gen, device=dev).float()
    jit = [lo + (hi - lo) * torch.rand(B, 1, 1, 1, generator=gen, device=dev) for lo, hi in (cfg.brightness, cfg.contrast, cfg.saturation)]
    perm = torch.stack([torch.randperm(3, generator=gen, device=dev) for _ in range(B)])
    luma = torch.tensor(LUMA, device=dev).view(1, 3, 1, 1)
    views = []
    for x in (left, right):
        x = torch.gather(x.view(B, 4, H * W), 2, flat.expand(B, 4, H * W)).view(B, 4, H, W).float()
        a = x[:, 3:4]
        code = torch.floor((x[:, :3] * a + bg * (255 - a) + 127) / 255)
        v = torch.where(inside, code, bg.expand(B, 3, H, W)) / 255
        views.append((v * jit[0]).clamp(0, 1))
    m = torch.stack([(v * luma).sum(1, keepdim=True).mean((2, 3), keepdim=True) for v in views]).mean(0)
    out = []
    for v in views:
        v = (jit[1] * v + (1 - jit[1]) * m).clamp(0, 1)
        v = (jit[2] * v + (1 - jit[2]) * (v * luma).sum(1, keepdim=True)).clamp(0, 1)
        n = (torch.rand((4,) + v.shape, generator=gen, device=dev).sum(0) - 2) * 1.7320508
        v = (v + cfg.noise_sigma * n).clamp(0, 1)
        out.append(torch.gather(v, 1, perm.view(B, 3, 1, 1).expand(B, 3, H, W)))
    return out


def numpy_pair(left, right, cfg, rng):
    """one pair on the host in fp32 numpy"""
    k = cfg.max_shift
    dy, dx = (int(v) for v in rng.integers(-k, k + 1, 2))
    bg = rng.integers(cfg.background[0], cfg.background[1] + 1, 3).astype(np.uint32)
    br, ct, st = (np.float32(lo + (hi - lo) * rng.random()) for lo, hi in (cfg.brightness, cfg.contrast, cfg.saturation))
    perm = rng.permutation(3)
    luma = np.array(LUMA, np.float32).reshape(3, 1, 1)
    views = []
    for x in (left, right):
        c, a = x[:3].astype(np.uint32), x[3:4].astype(np.uint32)
        code = (c * a + bg.reshape(3, 1, 1) * (255 - a) + 127) // 255
        sh = np.empty_like(code)
        sh[:] = bg.reshape(3, 1, 1)
        y0, y1, x0, x1 = max(dy, 0), H + min(dy, 0), max(dx, 0), W + min(dx, 0)
        sh[:, y0:y1, x0:x1] = code[:, y0 - dy:y1 - dy, x0 - dx:x1 - dx]
        views.append(np.clip(sh.astype(np.float32) / np.float32(255) * br, 0, 1))
    m = np.float32(np.mean([(v * luma).sum(0).mean() for v in views]))
    out = []
    for v in views:
        v = np.clip(ct * v + (1 - ct) * m, 0, 1)
        v = np.clip(st * v + (1 - st) * (v * luma).sum(0, keepdims=True), 0, 1)
        n = (rng.random((4,) + v.shape, dtype=np.float32).sum(0) - 2) * np.float32(1.7320508)
        out.append(np.clip(v + np.float32(cfg.noise_sigma) * n, 0, 1)[perm])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--hbm", type=float, default=6.29, help="HBM rate of the byte model's bound, TB/s (MI355X measured float4 copy)")
    ap.add_argument("--host-pairs", type=int, default=32, help="pairs the numpy version runs")
    ap.add_argument("--step", action="store_true", help="also time one eager training step at --batch and print the call's share")
    args = ap.parse_args()
    torch.set_num_threads(1)
    dev = torch.device("cuda:0")
    B = args.batch
    cfg = s3r.AugmentConfig(seed=1, max_shift=8, permute_rgb=True, background=(0, 255), brightness=(0.8, 1.2), contrast=(0.8, 1.2),
                            saturation=(0.8, 1.2), noise_sigma=0.02)
    g = torch.Generator().manual_seed(0)
    left = torch.randint(0, 256, (B, 4, H, W), generator=g, dtype=torch.uint8)
    right = torch.randint(0, 256, (B, 4, H, W), generator=g, dtype=torch.uint8)
    dl, dr = left.to(dev), right.to(dev)
    ids = torch.arange(B, dtype=torch.int64, device=dev)
    big = torch.empty(64 << 20, device=dev)
    aug = s3r.StereoAugment(cfg)
    aug(dl, dr, ids)
    torch.cuda.synchronize()
    src, out = 2 * B * 2 * 4 * H * W, B * 2 * 3 * H * W * 4
    print(f"{B} pairs of {H} x {W} RGBA, every op on; {args.rounds} rounds from cold caches, us: median [min .. max]")
    med, lo, hi = _timed(lambda: aug(dl, dr, ids), big, args.rounds)
    bound = (src + out) / args.hbm / 1e6
    print(f"  {'s3r_augment_pair (3 launches)':44s} {med:9.1f} [{lo:9.1f} .. {hi:9.1f}]   byte model {(src + out) / 1e6:.1f} MB "
          f"(source twice {src / 1e6:.1f} + output {out / 1e6:.1f}): {bound:.1f} us   {(src + out) / med / 1e3:7.1f} GB/s")
    call_us = med
    quiet = s3r.StereoAugment(s3r.AugmentConfig(seed=1, max_shift=8, permute_rgb=True, background=(0, 255), brightness=(0.8, 1.2),
                                                saturation=(0.8, 1.2)))
    quiet(dl, dr, ids)
    med, lo, hi = _timed(lambda: quiet(dl, dr, ids), big, args.rounds)
    print(f"  {'... without contrast and noise (1 launch)':44s} {med:9.1f} [{lo:9.1f} .. {hi:9.1f}]   {(src // 2 + out) / med / 1e3:7.1f} GB/s")
    gen = torch.Generator(device=dev).manual_seed(0)
    torch_eager(dl, dr, cfg, gen)
    torch.cuda.synchronize()
    med, lo, hi = _timed(lambda: torch_eager(dl, dr, cfg, gen), big, max(3, args.rounds // 2))
    print(f"  {'torch eager ops on the device':44s} {med:9.1f} [{lo:9.1f} .. {hi:9.1f}]")
    rng = np.random.default_rng(0)
    ln, rn = left.numpy(), right.numpy()
    numpy_pair(ln[0], rn[0], cfg, rng)
    n = args.host_pairs
    t0 = time.perf_counter()
    for i in range(n):
        numpy_pair(ln[i % B], rn[i % B], cfg, rng)
    secs = time.perf_counter() - t0
    print(f"  numpy on one host core: {n / secs:8.1f} pairs/s ({secs / n * 1e3:.2f} ms per pair)")
    if args.step:
        model = s3r.Stereo2Voxel()
        model.load_state_dict(s3r.seeded_state_dict(model, seed=4))
        model.to(dev)
        opt = s3r.Adam([p for p in model.parameters() if p.requires_grad], lr=1e-5)
        bce = s3r.VoxelBCELoss()
        gt = (torch.rand(B, 32, 32, 32, generator=torch.Generator().manual_seed(2)) < 0.3).float().to(dev)

        def step():
            l, r = aug(dl, dr, ids)
            opt.zero_grad(set_to_none=True)
            loss = bce(model.differentiable(l, r), gt)
            loss.backward()
            opt.step()

        step()
        torch.cuda.synchronize()
        med, lo, hi = _timed(step, big, max(3, args.rounds // 4))
        print(f"  one eager training step at {B} pairs, augmentation included: {med:9.1f} [{lo:9.1f} .. {hi:9.1f}]; "
              f"the call is {100 * call_us / med:.2f} % of it")


if __name__ == "__main__":
    main()
