"""Call plumbing shared by the GPU files that drive the C-ABI directly (tests/test_buffers_gpu.py, tests/test_exact_gpu.py):
halo-padded buffers in both physical layouts, their interiors, return-code checks and guarded weight packing."""
import ctypes as C

import torch

from tests import _guard as G

DEV = "cuda:0"


def sync():
    torch.cuda.synchronize()


def rc_ok(lib, rc, what):
    assert rc == 0, f"{what}: {lib.s3r_last_error().decode()} ({rc})"


def pad(x, h, cl=False):
    """zero-halo buffer of logical x (B, C, *sp); channels-last (B, *sp, C) when cl"""
    if cl:
        x = x.permute(0, *range(2, x.dim()), 1)
        sp = tuple(range(1, x.dim() - 1))
    else:
        sp = tuple(range(2, x.dim()))
    shape = list(x.shape)
    for d in sp:
        shape[d] += 2 * h
    out = torch.zeros(shape, dtype=x.dtype, device=x.device)
    idx = [slice(None)] * x.dim()
    for d in sp:
        idx[d] = slice(h, h + x.shape[d])
    out[tuple(idx)] = x
    return out, sp


def interior(y, h, sp, cl):
    idx = [slice(None)] * y.dim()
    for d in sp:
        idx[d] = slice(h, y.shape[d] - h)
    t = y[tuple(idx)]
    return t.permute(0, t.dim() - 1, *range(1, t.dim() - 1)) if cl else t


def pack(lib, s3r, desc, w, name="packed"):
    n = C.c_int64(0)
    rc_ok(lib, lib.s3r_conv_packed_elems(C.byref(desc), C.byref(n)), "packed_elems")
    wb = G.Guarded("w", w.shape, torch.float32, DEV, "in", data=w)
    pk = G.Guarded(name, n.value, torch.float32, DEV, "out")
    rc_ok(lib, lib.s3r_conv_pack_weights(C.byref(desc), wb.ptr, pk.ptr, None), "pack_weights")
    sync()
    G.check_all(wb, pk)
    return pk, wb
