#!/usr/bin/env python3
"""Micro-benchmark of the disparity supervision kernels: s3r_disparity_soft_backward at the network's shape (B = 32, C = 32, 28 x 28
features, max_disp 28) for the 224 x 224 render-size maps and for the feature-size maps, both gradients and grad_left alone, with the
forward read-out beside it; s3r_disparity_loss_forward (with and without loss_elem) and s3r_disparity_loss_backward at 64 x 224 x 224.
Timed by the library's profiler (HIP events around the call's launch) from cold caches, median and min..max of --rounds.

Each is set against
  - its byte-model time: the profiler record's `bytes` (features read once, each gradient given read once, each output asked for
    written once; the loss: pred, gt, the outputs) over --hbm TB/s;
  - torch on the same device, HIP-event timed around the call alone: torch.autograd.grad of the stock formulation — the per-disparity
    |L - R| sums, softmax, sum_d d p_d, F.interpolate(mode="bilinear") — with respect to both feature maps, and smooth_l1_loss on the
    valid pixels with its autograd backward.

    python tools/disparity_backward_bench.py [--batch 32] [--loss-batch 64] [--rounds 20] [--hbm 6.29]
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


def stock_readout(fl, fr, D, tau, size, scale):
    """the stock-PyTorch formulation of the soft read-out, under autograd: (disp_l, disp_r)"""
    B, C, H, W = fl.shape
    dm = min(D, W)
    d = torch.arange(dm, dtype=fl.dtype, device=fl.device)
    out = []
    for right in (False, True):
        cols = []
        for k in range(dm):
            c = (fr[..., :W - k] - fl[..., k:]).abs().sum(1) if right else (fl[..., k:] - fr[..., :W - k]).abs().sum(1)
            pad = c.new_full(c.shape[:-1] + (k,), float("inf"))
            cols.append(torch.cat([c, pad], -1) if right else torch.cat([pad, c], -1))
        c = torch.stack(cols, -1)
        disp = (torch.softmax(-c / tau, -1) * d).sum(-1)
        if size is not None:
            disp = torch.nn.functional.interpolate(disp[:, None], size=size, mode="bilinear", align_corners=False)[:, 0]
        out.append(disp * scale)
    return out


def _row(name, stat, by, hbm):
    med, lo, hi = stat
    bound = by / hbm / 1e6
    print(f"  {name:44s} {med:8.1f} [{lo:8.1f} .. {hi:8.1f}]   bound {bound:6.1f}   {by / med / 1e3:7.1f} GB/s of the model's bytes, "
          f"{bound / med:.3f} of the byte model")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--loss-batch", type=int, default=64)
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--hbm", type=float, default=6.29, help="HBM rate of the byte model's bound, TB/s (MI355X measured float4 copy)")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    C, D, n, full = s3r.arch_spec.FEAT_C, s3r.arch_spec.MAX_DISP, s3r.arch_spec.FEAT_HW, s3r.arch_spec.IMG_HW
    tau, B = s3r.DISPARITY_TEMPERATURE, args.batch
    big = torch.empty(64 << 20, device=dev)
    print(f"B {B}, C {C}, D {D}, H = W {n}, temperature {tau}; {args.rounds} rounds from cold caches, us: median [min .. max]; "
          f"bound = model bytes / {args.hbm} TB/s")
    g = torch.Generator().manual_seed(B)
    fl, fr = torch.randn(B, C, n, n, generator=g).relu().to(dev), torch.randn(B, C, n, n, generator=g).relu().to(dev)
    for size, scale in (((full, full), float(full // n)), (None, 1.0)):
        oh, ow = size or (n, n)
        gl, gr = torch.randn(B, oh, ow, generator=g).to(dev), torch.randn(B, oh, ow, generator=g).to(dev)
        print(f"soft read-out, maps {oh} x {ow}")
        bwd = lambda **kw: s3r.disparity_soft_backward(fl, fr, gl, gr, D, tau, size, scale, **kw)
        ours, by = _profiled(bwd, big, args.rounds)
        _row("HIP backward, both gradients", ours, by, args.hbm)
        _row("HIP backward, grad_left alone", *_profiled(lambda: bwd(need_right=False), big, args.rounds), args.hbm)
        _row("HIP forward (both disparity maps)", *_profiled(lambda: s3r.disparity_soft(fl, fr, D, tau, size, scale), big, args.rounds), args.hbm)
        a, b = fl.clone().requires_grad_(), fr.clone().requires_grad_()

        def torch_backward():
            dl, dr = stock_readout(a, b, D, tau, size, scale)
            return lambda: torch.autograd.grad((dl, dr), (a, b), (gl, gr))

        med, lo, hi = _evented(torch_backward, big, args.rounds)
        print(f"  {'torch autograd of the stock formulation':44s} {med:8.1f} [{lo:8.1f} .. {hi:8.1f}]   the HIP kernel: {ours[0]:8.1f} us, "
              f"{ours[0] / med:.4f} x torch's time")
    LB = args.loss_batch
    gt = (torch.rand(LB, full, full, generator=g) * 100)
    gt[torch.rand(LB, full, full, generator=g) < 0.3] = float("inf")
    gt = gt.to(dev)
    pred = (gt.nan_to_num(posinf=0.0) + torch.randn(LB, full, full, generator=g).to(dev) * 2).contiguous()
    gs = torch.full((LB,), 1.0 / (LB * full * full), device=dev)
    print(f"disparity loss, {LB} x {full} x {full}, beta 1")
    fwd, by = _profiled(lambda: s3r.disparity_loss(pred, gt, 1.0), big, args.rounds)
    _row("HIP loss forward (sums and counts)", fwd, by, args.hbm)
    _row("HIP loss forward (+ loss_elem)", *_profiled(lambda: s3r.disparity_loss(pred, gt, 1.0, elements=True), big, args.rounds), args.hbm)
    bwd, by = _profiled(lambda: s3r.disparity_loss_backward(pred, gt, gs, 1.0), big, args.rounds)
    _row("HIP loss backward", bwd, by, args.hbm)
    ok = torch.isfinite(gt) & (gt >= 0)
    p = pred.clone().requires_grad_()
    stock = lambda: torch.nn.functional.smooth_l1_loss(p[ok], gt[ok], beta=1.0)
    med, lo, hi = _evented(lambda: stock, big, args.rounds)
    print(f"  {'torch smooth_l1_loss on the valid pixels':44s} {med:8.1f} [{lo:8.1f} .. {hi:8.1f}]   the HIP kernel: {fwd[0]:8.1f} us, "
          f"{fwd[0] / med:.4f} x torch's time")

    def torch_loss_backward():
        loss = stock()
        return lambda: torch.autograd.grad(loss, p)

    med, lo, hi = _evented(torch_loss_backward, big, args.rounds)
    print(f"  {'torch autograd of it':44s} {med:8.1f} [{lo:8.1f} .. {hi:8.1f}]   the HIP kernel: {bwd[0]:8.1f} us, {bwd[0] / med:.4f} x torch's time")


if __name__ == "__main__":
    main()
