#!/usr/bin/env python3
"""Micro-benchmark of the Stereo2Point-only kernels at BASELINE.json configs[3] size (B = 32): the three point-head
linear layers (weight streaming: GB/s of weights) and the Chamfer kernel (pairs/s, "TFLOP/s" at 8 flops per pair),
HIP-event timed by the library's profiler, median of --rounds.  --backward also times s3r_chamfer_backward (both directions, the
indices of the forward, random gradients) at the same shape in the same rounds: the forward is its yardstick.

--linear-backward times s3r_linear_backward instead: per point-head layer (p1, p2, p3 at --batch) from cold caches, HIP-event timed
around each call, median and min..max spread of --rounds: all three gradients; grad_w + grad_bias only (p1's case behind a frozen
trunk); the same layer's s3r_linear_forward; and the backward of torch.nn.functional.linear (+ activation) on the same device for
the same shapes (torch.autograd.grad of x, weight and bias).  Next to them the byte model's lower bound: the bytes the call must
read and write (the library's profiler model) over --hbm TB/s.

    python tools/point_bench.py [--batch 32] [--rounds 20] [--backward | --linear-backward]
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
import s3r  # noqa: E402


def _timed(make, big, rounds):
    """median, min, max in us of `make()()` from cold caches (a 256 MB sweep before every call), device events around the call alone;
    `make` runs outside the timed window (torch: it builds the graph whose backward is timed)"""
    ts = []
    for r in range(rounds + 2):
        fn = make()
        big.add_(1.0)                                         # evict weights / gradients from L2 and the Infinity Cache
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        if r >= 2:
            ts.append(e0.elapsed_time(e1) * 1e3)
    ts.sort()
    return ts[len(ts) // 2], ts[0], ts[-1]


def linear_backward_bench(args, dev):
    B, F = args.batch, torch.nn.functional
    big = torch.empty(64 << 20, device=dev)
    g = torch.Generator().manual_seed(0)
    acts = {"none": lambda z: z, "relu": torch.relu, "sigmoid": torch.sigmoid}
    print(f"batch {B}, {args.rounds} rounds from cold caches, us: median [min .. max]; bound = model bytes / {args.hbm} TB/s")
    for l in s3r.arch_spec.POINT_HEAD:
        x = torch.randn(B, l.cin, generator=g).to(dev)
        w = (torch.randn(l.cout, l.cin, generator=g) / l.cin ** 0.5).to(dev)
        b = torch.randn(l.cout, generator=g).to(dev)
        gy = torch.randn(B, l.cout, generator=g).to(dev)
        y = s3r.linear(x, w, b, l.act)
        xt, wt, bt = x.clone().requires_grad_(), w.clone().requires_grad_(), b.clone().requires_grad_()

        def torch_backward(inputs):
            yt = acts[l.act](F.linear(xt, wt, bt))            # (the graph is rebuilt outside the timed window)
            return lambda: torch.autograd.grad(yt, inputs, gy)

        act_bytes = 4.0 * B * l.cout * (2 if l.act != "none" else 1)
        gemm_w = 4.0 * (B * l.cin + l.cin * l.cout)           # read x, write grad_w  |  read w, write grad_x
        rows = [
            ("HIP backward, all gradients", _timed(lambda: lambda: s3r.linear_backward(x, w, y, gy, l.act), big, args.rounds),
             act_bytes + 2 * gemm_w + 4.0 * l.cout),
            ("HIP grad_w + grad_bias", _timed(lambda: lambda: s3r.linear_backward(x, w, y, gy, l.act, need_x=False), big, args.rounds),
             act_bytes + gemm_w + 4.0 * l.cout),
            ("HIP forward", _timed(lambda: lambda: s3r.linear(x, w, b, l.act), big, args.rounds), 4.0 * (l.cin * l.cout + B * (l.cin + l.cout) + l.cout)),
            ("torch backward, all gradients", _timed(lambda: torch_backward((xt, wt, bt)), big, args.rounds), act_bytes + 2 * gemm_w + 4.0 * l.cout),
            ("torch grad_w + grad_bias", _timed(lambda: torch_backward((wt, bt)), big, args.rounds), act_bytes + gemm_w + 4.0 * l.cout),
        ]
        for name, (med, lo, hi), by in rows:
            print(f"{l.name} ({l.cin} -> {l.cout}, {l.act:7s}) {name:30s} {med:8.1f} [{lo:8.1f} .. {hi:8.1f}]   bound {by / args.hbm / 1e6:6.1f}   "
                  f"{by / med / 1e3:7.1f} GB/s of the model's bytes")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--points", type=int, default=2048)
    ap.add_argument("--backward", action="store_true", help="time the Chamfer backward as well (profiler family chamfer, tag 1)")
    ap.add_argument("--linear-backward", action="store_true", help="time s3r_linear_backward per layer against torch's backward")
    ap.add_argument("--hbm", type=float, default=6.29, help="HBM rate of the byte model's bound, TB/s (MI355X measured float4 copy)")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    if args.linear_backward:
        return linear_backward_bench(args, dev)
    spec = s3r.arch_spec
    B = args.batch
    head = s3r.PointHead()
    s3r.seed_module(head, 0)
    head.to(dev)
    x = torch.randn(B, spec.LATENT_C, 4, 4, 4, device=dev)
    g = torch.Generator().manual_seed(0)
    p = torch.rand(B, args.points, 3, generator=g).to(dev)
    q = torch.rand(B, args.points, 3, generator=g).to(dev)
    g1 = torch.randn(B, args.points, generator=g).to(dev)
    g2 = torch.randn(B, args.points, generator=g).to(dev)
    big = torch.empty(64 << 20, device=dev)                   # 256 MB: flushed through the caches between rounds
    res = {}
    for r in range(args.rounds + 2):
        big.add_(1.0)                                         # evict weights / clouds from L2 and the Infinity Cache
        s3r.profile_enable(64)
        head(x)
        _, _, i1, i2 = s3r.chamfer_distance(p, q)
        if args.backward:
            s3r.chamfer_distance_backward(p, q, i1, i2, g1, g2)
        rec = s3r.profile_read(64)
        s3r.profile_enable(0)
        if r < 2:
            continue
        for e in rec:
            key = (e["family"], e["tag"])
            res.setdefault(key, []).append((e["ms"], e["bytes"], e["flops"]))
    names = {300 + i: l.name for i, l in enumerate(spec.POINT_HEAD)}
    for (fam, tag), v in sorted(res.items()):
        ms = sorted(t for t, _, _ in v)[len(v) // 2]
        by, fl = v[0][1], v[0][2]
        label = names.get(tag, fam)
        if fam == "linear":
            print(f"{label:8s} {ms * 1e3:8.1f} us   {by / ms / 1e6:8.1f} GB/s algorithmic (weights + activations, incl. the split-K finish)")
        elif fam == "chamfer" and tag == 1:
            print(f"chamfer backward {ms * 1e3:8.1f} us   {by / ms / 1e6:8.1f} GB/s algorithmic, {2.0 * B * args.points ** 2 / ms / 1e9:.2f} T (target, source) "
                  f"compares/s, {ms / fwd_ms:.2f} x the forward's time")
        elif fam == "chamfer":
            fwd_ms = ms
            print(f"chamfer  {ms * 1e3:8.1f} us   {fl / ms / 1e9:8.2f} TFLOP/s at 8 flops per pair ({2.0 * B * args.points ** 2 / ms / 1e9:.2f} T pairs/s)")


if __name__ == "__main__":
    main()
