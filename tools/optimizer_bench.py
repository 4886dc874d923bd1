#!/usr/bin/env python3
"""Micro-benchmark of the optimizer step (s3r_optim_step) on the parameter list of Stereo2Voxel and at ONE tensor of 16 M elements, from
cold caches (256 MB streamed between rounds), HIP events around the call, median and min..max of --rounds, in us.

  1. s3r.Adam with clip_grad_norm (the three-launch step: chunk sums of g * g, the one-wave advance, the update) and without (the
     advance and the update launch: the update kernel and one wave in front of it), s3r.SGD(momentum=0.9) — each against its byte
     model over --hbm TB/s: Adam 28 B per element (p, g, m, v read; p, m, v written), + 4 B for the norm's pass over g; SGD with
     momentum 20 B.
  2. torch on the same device and tensors: Adam(fused=True), Adam(capturable=True, foreach=True), SGD(momentum=0.9, foreach=True),
     and torch.nn.utils.clip_grad_norm_ in front of the fused Adam.
  3. One whole training step of Stereo2Voxel.differentiable under VoxelBCELoss at --batch pairs (zero_grad, forward, loss, backward,
     step) with torch's fused Adam and with s3r.Adam (--no-step skips it).  Every eager step bumps each parameter's `_version`, so the next
     forward re-packs each layer's weight image: both rows carry that cost alike.

    python tools/optimizer_bench.py [--rounds 20] [--hbm 6.29] [--batch 8] [--no-step]
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
    return _stats(ts)


def _params(shapes, dev):
    g = torch.Generator().manual_seed(0)
    ps = [torch.nn.Parameter((0.1 * torch.randn(s, generator=g)).to(dev)) for s in shapes]
    for p in ps:
        p.grad = (1e-3 * torch.randn(p.shape, generator=g)).to(dev)
    return ps


def optimizer_rows(name, shapes, dev, big, args):
    n = sum(int(torch.Size(s).numel()) for s in shapes)
    print(f"\n{name}: {len(shapes)} tensors, {n} elements; {args.rounds} rounds from cold caches, us: median [min .. max]")
    rows = [
        ("s3r.Adam, clip_grad_norm (3 launches / 64 tensors)", lambda ps: s3r.Adam(ps, lr=1e-3, clip_grad_norm=1.0), 32.0),
        ("s3r.Adam (advance + update)", lambda ps: s3r.Adam(ps, lr=1e-3), 28.0),
        ("s3r.AdamW (advance + update)", lambda ps: s3r.AdamW(ps, lr=1e-3), 28.0),
        ("s3r.SGD momentum 0.9 (advance + update)", lambda ps: s3r.SGD(ps, lr=1e-3, momentum=0.9), 20.0),
        ("torch Adam(fused=True)", lambda ps: torch.optim.Adam(ps, lr=1e-3, fused=True), 28.0),
        ("torch Adam(capturable=True, foreach=True)", lambda ps: torch.optim.Adam(ps, lr=1e-3, capturable=True, foreach=True), 28.0),
        ("torch SGD(momentum=0.9, foreach=True)", lambda ps: torch.optim.SGD(ps, lr=1e-3, momentum=0.9, foreach=True), 20.0),
    ]
    out = {}
    for label, make, bpe in rows:
        ps = _params(shapes, dev)
        opt = make(ps)
        opt.step()                                                             # state allocated, kernels loaded
        torch.cuda.synchronize()
        med, lo, hi = _timed(opt.step, big, args.rounds)
        bound = bpe * n / args.hbm / 1e6
        out[label] = med
        print(f"  {label:52s} {med:9.1f} [{lo:9.1f} .. {hi:9.1f}]   byte model {bpe:.0f} B/elem: {bound:8.1f} us   {bpe * n / med / 1e3:7.1f} GB/s")
        del opt, ps
    ps = _params(shapes, dev)
    med, lo, hi = _timed(lambda: torch.nn.utils.clip_grad_norm_(ps, 1.0), big, args.rounds)
    print(f"  {'torch clip_grad_norm_ alone':52s} {med:9.1f} [{lo:9.1f} .. {hi:9.1f}]")
    return out


def training_step(dev, big, args):
    B = args.batch
    left, right = s3r.synthetic_pairs(B, seed=0, device=dev)
    gt = (torch.rand(B, 32, 32, 32, generator=torch.Generator().manual_seed(2)) < 0.3).float().to(dev)
    bce = s3r.VoxelBCELoss()
    print(f"\none training step of Stereo2Voxel.differentiable under VoxelBCELoss, {B} pairs, us: median [min .. max]")
    for label, make in (("torch Adam(fused=True)", lambda ps: torch.optim.Adam(ps, lr=1e-5, fused=True)),
                        ("s3r.Adam", lambda ps: s3r.Adam(ps, lr=1e-5))):
        model = s3r.Stereo2Voxel()
        model.load_state_dict(s3r.seeded_state_dict(model, seed=4))
        model.to(dev)
        opt = make([p for p in model.parameters() if p.requires_grad])

        def step():
            opt.zero_grad(set_to_none=True)
            loss = bce(model.differentiable(left, right), gt)
            loss.backward()
            opt.step()

        step()
        torch.cuda.synchronize()
        med, lo, hi = _timed(step, big, max(3, args.rounds // 4))
        print(f"  {label:52s} {med:9.1f} [{lo:9.1f} .. {hi:9.1f}]")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--hbm", type=float, default=6.29, help="HBM rate of the byte model's bound, TB/s (MI355X measured float4 copy)")
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--no-step", action="store_true")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    big = torch.empty(64 << 20, device=dev)
    shapes = [tuple(p.shape) for p in s3r.Stereo2Voxel().parameters() if p.requires_grad]
    optimizer_rows("Stereo2Voxel's parameters", shapes, dev, big, args)
    optimizer_rows("one tensor", [(16 << 20,)], dev, big, args)
    if not args.no_step:
        training_step(dev, big, args)


if __name__ == "__main__":
    main()
