#!/usr/bin/env python3
"""Micro-benchmark of the convolution backward at d3's geometry (ConvTranspose3d 128 -> 64, k4 s2 p1, 16^3 -> 32^3, folded BatchNorm +
ReLU) at B = 32: s3r_conv_backward split into its passes by the library's profiler at detail level 1 (the prep pass, the grad_shift
finish, the slab finish as family-10 records nested in the call's record; the weight-gradient GEMM is the rest of the record), and
grad_x as the adjoint layer's forward (one s3r_chain_forward call, its pack excluded: the packed weight is cached per weight version).
From cold caches, median and min..max of --rounds.

Set against
  - torch's own autograd backward of the same ConvTranspose3d + scale / shift + ReLU on the same device, HIP-event timed around
    torch.autograd.grad alone, to (x, w, shift) and to (w, shift);
  - the matrix model of grad_w: 2 B Q Ca Cf 64 FLOPs over --peak TFLOP/s (the fp32 matrix peak of MI355X_MICROARCH.md: 157.3 spec).

    python tools/conv_backward_bench.py [--batch 32] [--rounds 20] [--peak 157.3]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--peak", type=float, default=157.3, help="fp32 matrix peak, TFLOP/s")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    layer = s3r.arch_spec.DECODER[-2]
    B, n = args.batch, 16
    g = torch.Generator().manual_seed(0)
    x = torch.randn(B, layer.cin, n, n, n, generator=g).to(dev)
    w = (torch.randn(layer.cin, layer.cout, 4, 4, 4, generator=g) / (layer.cin * 8) ** 0.5).to(dev)
    scale = (0.5 + torch.rand(layer.cout, generator=g)).to(dev)
    shift = (0.1 * torch.randn(layer.cout, generator=g)).to(dev)
    gy = torch.randn(B, layer.cout, 32, 32, 32, generator=g).to(dev)
    y = s3r.conv_forward(x, w, scale, shift, layer)
    big = torch.empty(64 << 20, device=dev)
    tag = s3r._lib.CONV_BACKWARD_TAG
    rows = {k: [] for k in ("call (no grad_x)", "prep: g, gs, chunk sums", "grad_shift finish", "grad_w GEMM", "grad_w slab finish",
                            "grad_x: adjoint forward")}
    flops = 0.0
    s3r.conv_backward(x, w, y, gy, layer, scale=scale)                        # packs the adjoint weight once
    for r in range(args.rounds + 2):
        big.add_(1.0)                                                          # 256 MB through the caches
        s3r.profile_enable(64)
        s3r.profile_detail(1)
        s3r.conv_backward(x, w, y, gy, layer, scale=scale)
        torch.cuda.synchronize()
        rec = s3r.profile_read(64)
        s3r.profile_detail(0)
        s3r.profile_enable(0)
        call = [q for q in rec if q["family"] == "conv_mfma" and q["tag"] == tag]
        aux = [q for q in rec if q["family"] == "aux" and q["tag"] == tag]
        fwd = [q for q in rec if q["family"] in ("conv_mfma", "pad_copy") and q["tag"] != tag]      # the adjoint layer (+ its padded copy)
        assert len(call) == 1 and len(aux) == 3 and len(fwd) >= 1, rec
        flops = call[0]["flops"]
        if r >= 2:
            us = lambda q: q["ms"] * 1e3
            rows["call (no grad_x)"].append(us(call[0]))
            rows["prep: g, gs, chunk sums"].append(us(aux[0]))
            rows["grad_shift finish"].append(us(aux[1]))
            rows["grad_w slab finish"].append(us(aux[2]))
            rows["grad_w GEMM"].append(us(call[0]) - sum(us(q) for q in aux))
            rows["grad_x: adjoint forward"].append(sum(us(q) for q in fwd))
    print(f"d3 geometry, batch {B}; {args.rounds} rounds from cold caches, us: median [min .. max]")
    med = {}
    for name, ts in rows.items():
        st = _stats(ts)
        med[name] = st[0]
        print(f"{name:28s} {_fmt(st)}")
    model = flops / (args.peak * 1e12) * 1e6
    print(f"grad_w matrix model: {flops / 1e9:.1f} GFLOP / {args.peak} TFLOP/s = {model:.1f} us; the GEMM runs at "
          f"{flops / med['grad_w GEMM'] / 1e6:.1f} TFLOP/s = {100 * model / med['grad_w GEMM']:.1f} % of the peak")

    F = torch.nn.functional
    xt, wt, st_ = x.clone().requires_grad_(), w.clone().requires_grad_(), shift.clone().requires_grad_()

    def torch_backward(inputs):
        out = torch.relu(F.conv_transpose3d(xt, wt, None, 2, 1) * scale.view(1, -1, 1, 1, 1) + st_.view(1, -1, 1, 1, 1))
        return lambda: torch.autograd.grad(out, inputs, gy)

    for name, inputs, ours in (("torch backward to (x, w, shift)", (xt, wt, st_), med["call (no grad_x)"] + med["grad_x: adjoint forward"]),
                               ("torch backward to (w, shift)", (wt, st_), med["call (no grad_x)"])):
        ts = []
        for r in range(args.rounds + 2):
            fn = torch_backward(inputs)
            big.add_(1.0)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            if r >= 2:
                ts.append(e0.elapsed_time(e1) * 1e3)
        st = _stats(ts)
        print(f"{name:32s} {_fmt(st)}   the HIP kernels for the same work: {ours:9.1f} us, {ours / st[0]:.3f} x torch's time")


if __name__ == "__main__":
    main()
