"""The tensor contracts of the C-ABI (include/s3r.h, Conventions) that the networks (modules.py) and the stand-alone ops (ops.py) share:
what a tensor must be before its address goes to the library — device, dtype, shape, contiguity, alignment — and the two memory
layouts, plain (B,C,...) fp32 and physical channels-last (B,...,C) bf16 behind a logical (B,C,...) view."""
from __future__ import annotations

from typing import Sequence

import torch

from . import _lib
from . import arch_spec as spec


def _aligned16(x: torch.Tensor) -> torch.Tensor:
    """The library's alignment contract (include/s3r.h, Conventions) for the tensors that need more than their element size: a
    bf16 tensor and a render must start 16-byte aligned.  A torch view at a storage offset that breaks it (a slice of a larger
    buffer) is copied once, so that no view is ever refused; fp32 / int32 tensors need 4 bytes and never come here."""
    return x.clone() if x.data_ptr() % 16 else x


def _to_logical(x: torch.Tensor) -> torch.Tensor:
    """physical channels-last (B,...,C) -> logical (B,C,...) view (torch's channels_last convention)."""
    nd = x.dim()
    return x.permute(0, nd - 1, *range(1, nd - 1))


def _stream_ptr(device) -> int:
    return torch.cuda.current_stream(device).cuda_stream


def _check_input(x: torch.Tensor, name: str, shape_tail: Sequence[int], dtype=torch.float32):
    if not isinstance(x, torch.Tensor):
        raise TypeError(f"{name} must be a torch.Tensor")
    if not x.is_cuda:
        raise RuntimeError(f"{name} must live on a HIP device (got {x.device}); this path has no CPU fallback")
    if x.dtype != dtype:
        raise RuntimeError(f"{name} must be {dtype} (got {x.dtype})")
    if tuple(x.shape[1:]) != tuple(shape_tail):
        raise RuntimeError(f"{name} must have shape (B, {', '.join(map(str, shape_tail))}), got {tuple(x.shape)}")
    x = x.contiguous()
    return _aligned16(x) if dtype == torch.bfloat16 else x      # (fp32 / 8-bit: the storage offset is kept; renders: _check_render)


def _check_input_cl(x: torch.Tensor, name: str, shape_tail: Sequence[int], dtype=torch.bfloat16) -> torch.Tensor:
    """bf16 hand-off: validate a LOGICAL (B,C,...) tensor and return its PHYSICAL channels-last (B,...,C) form.  A
    tensor that already is channels-last in memory (what the bf16 modules hand each other: `_to_logical` views, also
    sliced along the batch) passes through as a view — no kernel runs; anything else is copied once."""
    if not isinstance(x, torch.Tensor):
        raise TypeError(f"{name} must be a torch.Tensor")
    if not x.is_cuda:
        raise RuntimeError(f"{name} must live on a HIP device (got {x.device}); this path has no CPU fallback")
    if x.dtype != dtype:
        raise RuntimeError(f"{name} must be {dtype} (got {x.dtype})")
    if tuple(x.shape[1:]) != tuple(shape_tail):
        raise RuntimeError(f"{name} must have shape (B, {', '.join(map(str, shape_tail))}), got {tuple(x.shape)}")
    nd = x.dim()
    phys = x.permute(0, *range(2, nd), 1)
    return _aligned16(phys if phys.is_contiguous() else phys.contiguous())


def _check_render(x: torch.Tensor, name: str) -> torch.Tensor:
    """A batch of renders, (B,3,224,224): float32 in [0,1], or uint8 as a PNG decode yields them (the stem scales by
    1/255 as it reads, bit-identical to `x.float() / 255` on the host: `s3r_encoder_forward_u8`)."""
    dt = x.dtype if isinstance(x, torch.Tensor) and x.dtype == torch.uint8 else torch.float32
    # the stems fetch whole rows by 16-byte LDS-DMA: a view at an odd storage offset is copied once
    return _aligned16(_check_input(x, name, (3, spec.IMG_HW, spec.IMG_HW), dt))


def _check_channel_vector(v, cout, device, who, name):
    if v is None:
        return None
    v = v.detach()
    if tuple(v.shape) != (cout,) or v.device != device or v.dtype != torch.float32:
        raise RuntimeError(f"{who}: {name} must be a fp32 tensor of shape ({cout},) on {device}")
    return v.contiguous()


@torch.no_grad()
def channels_last_to_f32(x: torch.Tensor) -> torch.Tensor:
    """Hand-off from the bf16 path to an fp32 consumer: a logical (B,C,...) bfloat16 tensor in channels-last memory (what
    the bf16 modules return) -> contiguous fp32 (B,C,...), exact, by `s3r_channels_last_to_f32` (no torch kernel)."""
    phys = _check_input_cl(x, "x", x.shape[1:])
    B, Cc = x.shape[0], x.shape[1]
    y = torch.empty(tuple(x.shape), dtype=torch.float32, device=x.device)
    if B and y.numel():
        _lib.check(_lib.load().s3r_channels_last_to_f32(phys.data_ptr(), y.data_ptr(), B, Cc, y[0, 0].numel(),
                                                        _stream_ptr(x.device)), "channels_last_to_f32")
    return y
