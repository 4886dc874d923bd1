#!/usr/bin/env python3
"""Micro-benchmark of s3r_cost_volume_backward at the network's shape (C = 32, D = H = W = 28) at B = 1, 8, 32: both gradients, and
grad_left alone.  Timed by the library's profiler (HIP events around the call's launch) from cold caches, median and min..max of
--rounds.  The plain forward (s3r_cost_volume_forward, halo 0: what the differentiable path runs) is timed beside it.

Each is set against
  - its byte-model time: one read of grad_volume and one write of the gradients, 4 B (2 C D H W + 2 C H W) bytes (the profiler record's
    `bytes`), over --hbm TB/s;
  - torch on the same device, HIP-event timed around the call alone: torch.autograd.grad of the stock formulation of the forward — a
    Python loop over D of slice assignments of differences, as the oracle states it — with respect to both feature maps.

    python tools/cost_volume_backward_bench.py [--batches 1,8,32] [--rounds 20] [--hbm 6.29]
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
    """(median, min, max) in us of `make()()`; `make` runs outside the timed window (it builds the graph whose backward is timed)"""
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


def stock_cost_volume(fl, fr, D):
    """the stock-PyTorch formulation (a Python loop over D), under autograd"""
    B, C, H, W = fl.shape
    vol = fl.new_zeros(B, 2 * C, D, H, W)
    for d in range(min(D, W)):
        vol[:, :C, d, :, d:] = fl[:, :, :, d:] - fr[:, :, :, :W - d]
        vol[:, C:, d, :, :W - d] = fr[:, :, :, :W - d] - fl[:, :, :, d:]
    return vol


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="1,8,32")
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--hbm", type=float, default=6.29, help="HBM rate of the byte model's bound, TB/s (MI355X measured float4 copy)")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    C, D, n = s3r.arch_spec.FEAT_C, s3r.arch_spec.MAX_DISP, s3r.arch_spec.FEAT_HW
    big = torch.empty(64 << 20, device=dev)
    cv = s3r.CostVolume(max_disp=D)
    print(f"C {C}, D {D}, H = W {n}; {args.rounds} rounds from cold caches, us: median [min .. max]; bound = model bytes / {args.hbm} TB/s")
    for B in (int(b) for b in args.batches.split(",")):
        g = torch.Generator().manual_seed(B)
        gv = torch.randn(B, 2 * C, D, n, n, generator=g).to(dev)
        fl, fr = torch.randn(B, C, n, n, generator=g).to(dev), torch.randn(B, C, n, n, generator=g).to(dev)
        rows = [
            ("HIP backward, both gradients", *_profiled(lambda: s3r.cost_volume_backward(gv), big, args.rounds)),
            ("HIP backward, grad_left alone", *_profiled(lambda: s3r.cost_volume_backward(gv, need_right=False), big, args.rounds)),
            ("HIP forward (plain volume)", *_profiled(lambda: cv(fl, fr), big, args.rounds)),
        ]
        print(f"batch {B}")
        for name, (med, lo, hi), by in rows:
            bound = by / args.hbm / 1e6
            print(f"  {name:32s} {med:8.1f} [{lo:8.1f} .. {hi:8.1f}]   bound {bound:6.1f}   {by / med / 1e3:7.1f} GB/s of the model's bytes, "
                  f"{bound / med:.3f} of the byte model")
        a, b = fl.clone().requires_grad_(), fr.clone().requires_grad_()

        def torch_backward():
            vol = stock_cost_volume(a, b, D)
            return lambda: torch.autograd.grad(vol, (a, b), gv)

        med, lo, hi = _evented(torch_backward, big, args.rounds)
        ours = rows[0][1][0]
        print(f"  {'torch autograd of the stock loop':32s} {med:8.1f} [{lo:8.1f} .. {hi:8.1f}]   the HIP kernel: {ours:8.1f} us, {ours / med:.4f} x torch's time")


if __name__ == "__main__":
    main()
