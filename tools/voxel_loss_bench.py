#!/usr/bin/env python3
"""Micro-benchmark of the voxel branch's training kernels at the headline shape (B = 32, C = 64, V = 32^3): s3r_voxel_bce_forward,
s3r_voxel_bce_backward, s3r_head_backward with all three outputs and without grad_x (the fine-tune case behind a frozen trunk).
Timed by the library's profiler (HIP events around each call's launches) from cold caches, median and min..max of --rounds.

Each is set against
  - its byte-model time: the bytes the call must read and write (the profiler record's `bytes`) over --hbm TB/s;
  - torch on the same device, HIP-event timed around the call alone: BCELoss's forward for the BCE forward, and torch.autograd.grad of
    BCELoss(sigmoid(conv3d(x, w, b))) with respect to (x, w, b) and to (w, b) — which runs binary_cross_entropy, sigmoid and conv3d
    backward — for "BCE backward + head backward" with and without grad_x; and the same graph with the 1x1x1 convolution written as
    an einsum over the channels, which takes torch's matrix-product path instead of its convolution library's.

    python tools/voxel_loss_bench.py [--batch 32] [--rounds 20] [--hbm 6.29]
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
import s3r  # noqa: E402


def _stats(ts):
    ts = sorted(ts)
    return ts[len(ts) // 2], ts[0], ts[-1]


def _profiled(fn, big, rounds):
    """(median, min, max) in us and the byte model of ONE library call, from cold caches"""
    ts, by = [], 0.0
    for r in range(rounds + 2):
        big.add_(1.0)                                         # 256 MB through the caches: evicts the tensors from L2 and the Infinity Cache
        s3r.profile_enable(16)
        fn()
        torch.cuda.synchronize()
        rec = s3r.profile_read(16)
        s3r.profile_enable(0)
        assert len(rec) == 1, rec
        by = rec[0]["bytes"]
        if r >= 2:
            ts.append(rec[0]["ms"] * 1e3)
    return _stats(ts), by


def _evented(make, big, rounds):
    """(median, min, max) in us of `make()()`; `make` runs outside the timed window (torch: it builds the graph whose backward is timed)"""
    ts = []
    for r in range(rounds + 2):
        fn = make()
        big.add_(1.0)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        if r >= 2:
            ts.append(e0.elapsed_time(e1) * 1e3)
    return _stats(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--hbm", type=float, default=6.29, help="HBM rate of the byte model's bound, TB/s (MI355X measured float4 copy)")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    B, ch, n = args.batch, 64, s3r.arch_spec.VOX
    g = torch.Generator().manual_seed(0)
    x = torch.randn(B, ch, n, n, n, generator=g).to(dev)
    w = (torch.randn(1, ch, 1, 1, 1, generator=g) / 8).to(dev)
    b = torch.randn(1, generator=g).to(dev)
    gt = (torch.rand(B, n, n, n, generator=g) < 0.3).float().to(dev)
    big = torch.empty(64 << 20, device=dev)
    y = s3r.head(x, w, b, "sigmoid")
    scale = torch.full((B,), 1.0 / y.numel(), device=dev)
    gy = s3r.voxel_bce_backward(y, gt, scale)
    F = torch.nn.functional
    xt, wt, bt = x.clone().requires_grad_(), w.clone().requires_grad_(), b.clone().requires_grad_()

    def torch_backward(inputs):
        loss = F.binary_cross_entropy(torch.sigmoid(F.conv3d(xt, wt, bt)).squeeze(1), gt)
        return lambda: torch.autograd.grad(loss, inputs)

    def torch_backward_matmul(inputs):                        # the same layer written as a contraction over C: rocBLAS instead of MIOpen
        z = torch.einsum("bcs,c->bs", xt.view(B, ch, -1), wt.view(ch)) + bt
        loss = F.binary_cross_entropy(torch.sigmoid(z), gt.view(B, -1))
        return lambda: torch.autograd.grad(loss, inputs)

    rows = [
        ("HIP BCE forward (loss_sum)", *_profiled(lambda: s3r.voxel_bce(y, gt), big, args.rounds)),
        ("HIP BCE backward", *_profiled(lambda: s3r.voxel_bce_backward(y, gt, scale), big, args.rounds)),
        ("HIP head backward, all gradients", *_profiled(lambda: s3r.head_backward(x, w, y, gy, "sigmoid"), big, args.rounds)),
        ("HIP head backward, no grad_x", *_profiled(lambda: s3r.head_backward(x, w, y, gy, "sigmoid", need_x=False), big, args.rounds)),
    ]
    print(f"batch {B}, C {ch}, V {n ** 3}; {args.rounds} rounds from cold caches, us: median [min .. max]; bound = model bytes / {args.hbm} TB/s")
    hip = {}
    for name, (med, lo, hi), by in rows:
        hip[name] = med
        print(f"{name:36s} {med:8.1f} [{lo:8.1f} .. {hi:8.1f}]   bound {by / args.hbm / 1e6:6.1f}   {by / med / 1e3:7.1f} GB/s of the model's bytes")
    torch_rows = [
        ("torch BCELoss forward (mean)", _evented(lambda: lambda: F.binary_cross_entropy(y, gt), big, args.rounds), hip["HIP BCE forward (loss_sum)"]),
        ("torch backward to (x, w, b)", _evented(lambda: torch_backward((xt, wt, bt)), big, args.rounds),
         hip["HIP BCE backward"] + hip["HIP head backward, all gradients"]),
        ("torch backward to (w, b)", _evented(lambda: torch_backward((wt, bt)), big, args.rounds),
         hip["HIP BCE backward"] + hip["HIP head backward, no grad_x"]),
        ("torch backward to (x, w, b), einsum", _evented(lambda: torch_backward_matmul((xt, wt, bt)), big, args.rounds),
         hip["HIP BCE backward"] + hip["HIP head backward, all gradients"]),
        ("torch backward to (w, b), einsum", _evented(lambda: torch_backward_matmul((wt, bt)), big, args.rounds),
         hip["HIP BCE backward"] + hip["HIP head backward, no grad_x"]),
    ]
    for name, (med, lo, hi), ours in torch_rows:
        print(f"{name:36s} {med:10.1f} [{lo:10.1f} .. {hi:10.1f}]   the HIP kernels for the same work: {ours:8.1f} us, {ours / med:.4f} x torch's time")


if __name__ == "__main__":
    main()
