#!/usr/bin/env python3
"""Micro-benchmark of the encoder's backward at the network's own shape: the stem's weight / shift gradient over 64 renders of 224^2
(B = 32 pairs), and one whole training step.  From cold caches (256 MB streamed between rounds), median and min..max of --rounds, the
whole table --runs times.

  1. s3r_stem_backward, 8-bit renders in two tensors and fp32 renders in one: the call's profiler record split into its launches at
     detail level 1 (the shift pass and its finish, the per-image and the batch finish as family-10 records; the weight-gradient GEMM is
     the rest), and the whole Python call between HIP events — against the byte model: grad_y and y once for grad_w, once more for
     grad_shift (it is a pass of its own), the renders once, over --hbm TB/s.
  2. The route without the entry, for the same job from the same 8-bit renders: `.float() / 255` of both tensors, `torch.cat`,
     `conv_backward(..., need_x=False)` on e1 — between HIP events, and conv_backward alone on the already converted tensor.
  3. torch's own autograd backward of the layer (conv2d + scale / shift + ReLU) to (w, shift) on the same device.
  4. One training step at --batch pairs: forward + backward of `Stereo2Voxel.differentiable` under `VoxelBCELoss` (--no-step skips it).

    python tools/encoder_backward_bench.py [--batch 32] [--rounds 20] [--runs 2] [--hbm 8.0] [--no-step]
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


def _fmt(st):
    return f"{st[0]:9.1f} [{st[1]:9.1f} .. {st[2]:9.1f}]"


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


def one_run(args, dev, big):
    B = args.batch
    layer = s3r.arch_spec.ENCODER[0]
    g = torch.Generator().manual_seed(0)
    left = torch.randint(0, 256, (B, 3, 224, 224), generator=g).to(torch.uint8).to(dev)
    right = torch.randint(0, 256, (B, 3, 224, 224), generator=g).to(torch.uint8).to(dev)
    w = (torch.randn(32, 3, 3, 3, generator=g) / 27 ** 0.5).to(dev)
    scale = (0.5 + torch.rand(32, generator=g)).to(dev)
    shift = (0.1 * torch.randn(32, generator=g)).to(dev)
    gy = torch.randn(2 * B, 32, 112, 112, generator=g).to(dev)
    x32 = torch.cat([left.float() / 255, right.float() / 255])
    y = s3r.conv_forward(x32 - 0.5, w, scale, shift, layer)                    # (centred: about half of the gates are open)
    Y = 4.0 * gy.numel()
    print(f"e1 backward to (w, shift), {2 * B} renders of 224^2; {args.rounds} rounds from cold caches, us: median [min .. max]")
    med = {}
    for name, lr, rbytes in (("8-bit renders, two tensors", (left, right), 1.0), ("fp32 renders, one tensor", (x32, None), 4.0)):
        rows = {k: [] for k in ("record", "shift pass", "shift finish", "grad_w GEMM", "image finish", "batch finish")}
        for r in range(args.rounds + 2):
            big.add_(1.0)
            s3r.profile_enable(64)
            s3r.profile_detail(1)
            s3r.stem_backward(lr[0], lr[1], y, gy, scale, "relu")
            torch.cuda.synchronize()
            rec = s3r.profile_read(64)
            s3r.profile_detail(0)
            s3r.profile_enable(0)
            call = [q for q in rec if q["family"] == "stem"]
            aux = [q for q in rec if q["family"] == "aux"]
            assert len(call) == 1 and len(aux) == 4, rec
            if r >= 2:
                us = lambda q: q["ms"] * 1e3
                rows["record"].append(us(call[0]))
                for k, q in zip(("shift pass", "shift finish", "image finish", "batch finish"), aux):
                    rows[k].append(us(q))
                rows["grad_w GEMM"].append(us(call[0]) - sum(us(q) for q in aux))
        whole = _timed(lambda: s3r.stem_backward(lr[0], lr[1], y, gy, scale, "relu"), big, args.rounds)
        print(f"s3r_stem_backward, {name}")
        for k, ts in rows.items():
            print(f"    {k:24s} {_fmt(_stats(ts))}")
        print(f"    {'whole call (events)':24s} {_fmt(whole)}")
        model_w = 2 * Y + rbytes * 2 * B * 3 * 224 * 224
        gemm, shp = _stats(rows["grad_w GEMM"])[0], _stats(rows["shift pass"])[0]
        print(f"    byte model: grad_w {model_w / 1e6:.1f} MB = {model_w / args.hbm / 1e6:.1f} us at {args.hbm} TB/s (the GEMM moves "
              f"{model_w / gemm / 1e6:.2f} TB/s); grad_shift {2 * Y / 1e6:.1f} MB more (its pass moves {2 * Y / shp / 1e6:.2f} TB/s)")
        med[name] = whole[0]

    def parent():
        x = torch.cat([left.float() / 255, right.float() / 255])
        return s3r.conv_backward(x, w, y, gy, layer, scale=scale, need_x=False)

    parent()
    st = _timed(parent, big, args.rounds)
    st2 = _timed(lambda: s3r.conv_backward(x32, w, y, gy, layer, scale=scale, need_x=False), big, args.rounds)
    print(f"{'convert + cat + conv_backward':34s} {_fmt(st)}   s3r_stem_backward on the 8-bit renders: "
          f"{med['8-bit renders, two tensors'] / st[0]:.3f} x its time")
    print(f"{'conv_backward alone (fp32, one)':34s} {_fmt(st2)}   s3r_stem_backward on the same tensor: "
          f"{med['fp32 renders, one tensor'] / st2[0]:.3f} x its time")

    F = torch.nn.functional
    wt, sht = w.clone().requires_grad_(), shift.clone().requires_grad_()

    def torch_backward():
        out = torch.relu(F.conv2d(x32, wt, None, 2, 1) * scale.view(1, -1, 1, 1) + sht.view(1, -1, 1, 1))
        return lambda: torch.autograd.grad(out, (wt, sht), gy)

    ts = []
    for r in range(args.rounds + 2):
        fn = torch_backward()
        big.add_(1.0)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        if r >= 2:
            ts.append(e0.elapsed_time(e1) * 1e3)
    print(f"{'torch backward to (w, shift)':34s} {_fmt(_stats(ts))}")
    del gy, y, x32

    if not args.no_step:
        model = s3r.Stereo2Voxel().to(dev)
        s3r.seed_module(model, seed=0)
        loss_fn = s3r.VoxelBCELoss()
        gt = (torch.rand(B, 32, 32, 32, generator=g) < 0.3).float().to(dev)
        params = [p for p in model.parameters() if p.requires_grad]

        def step():
            for p in params:
                p.grad = None
            loss_fn(model.differentiable(left, right), gt).backward()

        step()
        st = _timed(step, big, max(3, args.rounds // 4))
        print(f"{'training step, B = %d (fwd + bwd)' % B:34s} {_fmt(st)}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--runs", type=int, default=2)
    ap.add_argument("--hbm", type=float, default=8.0, help="HBM rate of the byte model, TB/s (MI355X: 8 spec)")
    ap.add_argument("--no-step", action="store_true")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    big = torch.empty(64 << 20, device=dev)
    for run in range(args.runs):
        print(f"--- run {run + 1} of {args.runs}")
        one_run(args, dev, big)


if __name__ == "__main__":
    main()
