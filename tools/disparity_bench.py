#!/usr/bin/env python3
"""Micro-benchmark of the sub-pixel disparity read-out (s3r_disparity_soft, both directions, no confidence maps) at B = 1, 32
and 256, fp32 NCHW and bf16 channels-last features (28 x 28 x 32, max_disp 28), written at feature resolution (28^2) and at render
resolution (224^2); and of the stereo metrics at 224^2.  HIP-event timed by the library's profiler (one record per call), median
of --rounds, caches flushed between rounds.  Prints one line per case with the algorithmic bytes (features read + maps written)
over time, against the 6.3 TB/s and 8 TB/s HBM roofs.

    python tools/disparity_bench.py [--rounds 20] [--batches 1,32,256] [--json rows.json]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
import s3r  # noqa: E402


def _median_record(fn, rounds, big):
    ms = []
    by = 0.0
    for r in range(rounds + 2):
        big.add_(1.0)                                         # evict the features from L2 and the Infinity Cache
        s3r.profile_enable(8)
        fn()
        rec = s3r.profile_read(8)
        s3r.profile_enable(0)
        assert len(rec) == 1 and rec[0]["family"] == "disparity", rec
        if r >= 2:
            ms.append(rec[0]["ms"])
            by = rec[0]["bytes"]
    ms.sort()
    return ms[len(ms) // 2], by


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--batches", default="1,32,256")
    ap.add_argument("--json", default=None, help="also write the rows to this file")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    spec = s3r.arch_spec
    C, H, D = spec.ENCODER[-1].cout, spec.FEAT_HW, spec.MAX_DISP
    big = torch.empty(64 << 20, device=dev)                   # 256 MB
    rows = []
    for B in (int(b) for b in args.batches.split(",")):
        g = torch.Generator().manual_seed(B)
        fl = torch.randn(B, C, H, H, generator=g).to(dev)
        fr = torch.randn(B, C, H, H, generator=g).to(dev)
        for dtype in ("fp32", "bf16"):
            a, b = (fl, fr) if dtype == "fp32" else (x.to(torch.bfloat16).contiguous(memory_format=torch.channels_last)
                                                      for x in (fl, fr))
            for size in (None, (spec.IMG_HW, spec.IMG_HW)):
                ms, by = _median_record(lambda: s3r.disparity_soft(a, b, D, 1.0, size, 8.0), args.rounds, big)
                rows.append(dict(op="soft", batch=B, dtype=dtype, out=(size or (H, H))[0], us=round(ms * 1e3, 2), bytes=by,
                                 tb_s=round(by / ms / 1e9, 3), roof_6_3=round(by / ms / 1e9 / 6.3, 4),
                                 roof_8=round(by / ms / 1e9 / 8.0, 4)))
        gt = torch.rand(B, spec.IMG_HW, spec.IMG_HW, generator=g).to(dev) * 200
        pred = torch.rand(B, spec.IMG_HW, spec.IMG_HW, generator=g).to(dev) * 200
        ms, by = _median_record(lambda: s3r.disparity_metrics(pred, gt), args.rounds, big)
        rows.append(dict(op="metrics", batch=B, dtype="fp32", out=spec.IMG_HW, us=round(ms * 1e3, 2), bytes=by,
                         tb_s=round(by / ms / 1e9, 3), roof_6_3=round(by / ms / 1e9 / 6.3, 4), roof_8=round(by / ms / 1e9 / 8.0, 4)))
    for r in rows:
        print(f"{r['op']:8s} B={r['batch']:<4d} {r['dtype']:5s} out {r['out']:3d}^2  {r['us']:9.2f} us  {r['bytes'] / 1e6:8.2f} MB  "
              f"{r['tb_s']:6.3f} TB/s  ({100 * r['roof_6_3']:5.1f} % of 6.3, {100 * r['roof_8']:5.1f} % of 8 TB/s)")
    if args.json:
        with open(args.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
