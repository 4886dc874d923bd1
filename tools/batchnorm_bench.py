#!/usr/bin/env python3
"""Micro-benchmark of train-mode BatchNorm + ReLU (s3r_batchnorm_train_forward / s3r_batchnorm_train_backward) at d3's output geometry
(B, 64, 32^3) and at v1's (B, 64, 28^3).  Timed by the library's profiler (HIP events around each call's launches) from cold caches,
median and min..max of --rounds.

Each is set against
  - its byte model over --hbm TB/s: forward 3 reads + 1 write of z (two statistics passes and the normalise pass), backward 6 reads +
    1 write (z, y and grad_y in the sums pass and again in the grad_z pass), 4 B each — the profiler record's `bytes` adds the (C) vectors;
  - torch on the same device, HIP-event timed around the call alone: relu(torch.nn.functional.batch_norm(training=True)) for the forward
    and torch.autograd.grad of it with respect to (z, weight, bias) for the backward.

    python tools/batchnorm_bench.py [--batch 32] [--rounds 20] [--hbm 6.29]
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
import s3r  # noqa: E402
from tools.voxel_loss_bench import _evented, _profiled  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--hbm", type=float, default=6.29, help="HBM rate of the byte model's bound, TB/s (MI355X measured float4 copy)")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    F = torch.nn.functional
    B, ch, eps = args.batch, 64, s3r.arch_spec.BN_EPS
    big = torch.empty(64 << 20, device=dev)
    print(f"batch {B}, C {ch}; {args.rounds} rounds from cold caches, us: median [min .. max]; bound = model bytes / {args.hbm} TB/s")
    for name, n in (("d3", s3r.arch_spec.VOX), ("v1", s3r.arch_spec.MAX_DISP)):
        g = torch.Generator().manual_seed(0)
        z = torch.randn(B, ch, n, n, n, generator=g).to(dev)
        gy = torch.randn(B, ch, n, n, n, generator=g).to(dev)
        gam, beta = (torch.rand(ch, generator=g) + 0.5).to(dev), torch.randn(ch, generator=g).to(dev)
        y, mean, var, inv = s3r.batchnorm_train_forward(z, gam, beta, eps, "relu")
        T = 4.0 * z.numel()
        rows = [
            ("forward", 4 * T, _profiled(lambda: s3r.batchnorm_train_forward(z, gam, beta, eps, "relu"), big, args.rounds)),
            ("backward, all gradients", 7 * T, _profiled(lambda: s3r.batchnorm_train_backward(z, y, gy, gam, mean, inv, "relu"), big, args.rounds)),
            ("backward, no grad_z", 3 * T, _profiled(lambda: s3r.batchnorm_train_backward(z, y, gy, gam, mean, inv, "relu", need_z=False), big, args.rounds)),
        ]
        hip = {}
        for what, model, ((med, lo, hi), by) in rows:
            hip[what] = med
            assert abs(by - model) <= 4.0 * 8 * ch, (by, model)       # the record's bytes are the model's plus the (C) vectors
            print(f"{name} ({n}^3) HIP {what:24s} {med:8.1f} [{lo:8.1f} .. {hi:8.1f}]   bound {model / args.hbm / 1e6:6.1f}   "
                  f"{model / med / 1e3:7.1f} GB/s of the model's bytes   {model / args.hbm / 1e6 / med:.3f} of the byte model's rate")
        zt, wt, bt = z.clone().requires_grad_(), gam.clone().requires_grad_(), beta.clone().requires_grad_()

        def torch_forward():
            return lambda: torch.relu(F.batch_norm(zt.detach(), None, None, wt.detach(), bt.detach(), True, 0.1, eps))

        def torch_backward(inputs):
            out = torch.relu(F.batch_norm(zt, None, None, wt, bt, True, 0.1, eps))
            return lambda: torch.autograd.grad(out, inputs, gy)

        for what, t, ours in (("forward", _evented(torch_forward, big, args.rounds), hip["forward"]),
                              ("backward to (z, w, b)", _evented(lambda: torch_backward((zt, wt, bt)), big, args.rounds), hip["backward, all gradients"]),
                              ("backward to (w, b)", _evented(lambda: torch_backward((wt, bt)), big, args.rounds), hip["backward, no grad_z"])):
            med, lo, hi = t
            print(f"{name} ({n}^3) torch {what:22s} {med:10.1f} [{lo:10.1f} .. {hi:10.1f}]   the HIP kernels for the same work: {ours:8.1f} us, "
                  f"{ours / med:.4f} x torch's time")
        del z, gy, y, zt


if __name__ == "__main__":
    main()
