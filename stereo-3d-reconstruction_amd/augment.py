"""Training-time augmentation of stereo batches on the device (`s3r_augment_pair`, include/s3r.h): 8-bit renders in, fp32 network inputs
out, the ground-truth disparity maps shifted by the same call.

The reference's own transforms are on unmounted branches (`data.py`'s docstring).  INVENTED by this build (each a field
of `AugmentConfig.default()`, to be overwritten from the reference the day it is mounted): the transform set itself — an integer shift
of up to 8 pixels shared by the two views, a random permutation of the colour channels, brightness / contrast / saturation factors
drawn from [0.8, 1.2], additive noise of sigma 0.02 and a white background behind what the shift uncovers — and its order.

A sample's augmentation depends on (seed, sample id) only: not on the batch it is in, its position there or the launch shape.  Nothing
is drawn on the host: the ids live in a device buffer, so a captured training step replays with fresh augmentation.
"""
from __future__ import annotations

import ctypes as C
import dataclasses
import math
from typing import Optional, Tuple

import torch

from . import _lib
from ._tensors import _stream_ptr

__all__ = ["AugmentConfig", "StereoAugment", "augment_pair"]


@dataclasses.dataclass(frozen=True)
class AugmentConfig:
    """The fields of `s3r_augment_desc` but `channels`, which follows the renders.  A range (lo, hi) equal to (1, 1) switches its op
    off, as max_shift = 0, permute_rgb = False and noise_sigma = 0 do; the draws of the other ops do not change."""
    seed: int = 0
    max_shift: int = 0
    permute_rgb: bool = False
    background: Tuple[int, int] = (255, 255)
    brightness: Tuple[float, float] = (1.0, 1.0)
    contrast: Tuple[float, float] = (1.0, 1.0)
    saturation: Tuple[float, float] = (1.0, 1.0)
    noise_sigma: float = 0.0

    def __post_init__(self):
        if not 0 <= int(self.seed) < 2 ** 64:
            raise ValueError(f"seed must be in [0, 2^64), got {self.seed!r}")
        if not 0 <= int(self.max_shift) <= _lib.AUG_MAX_SHIFT:
            raise ValueError(f"max_shift must be in [0, {_lib.AUG_MAX_SHIFT}], got {self.max_shift!r}")
        lo, hi = self.background
        if not 0 <= int(lo) <= int(hi) <= 255:
            raise ValueError(f"background codes must satisfy 0 <= lo <= hi <= 255, got {self.background!r}")
        for name in ("brightness", "contrast", "saturation"):
            lo, hi = getattr(self, name)
            if not (math.isfinite(lo) and math.isfinite(hi) and 0.0 <= lo <= hi):
                raise ValueError(f"{name} must be a finite range with 0 <= lo <= hi, got {(lo, hi)!r}")
        if not (math.isfinite(self.noise_sigma) and self.noise_sigma >= 0.0):
            raise ValueError(f"noise_sigma must be finite and >= 0, got {self.noise_sigma!r}")

    @classmethod
    def identity(cls, seed: int = 0) -> "AugmentConfig":
        """every op off: the call is `data.renders_to_float` (of `data.composite_over_white_u8` for RGBA renders)"""
        return cls(seed=seed)

    @classmethod
    def default(cls, seed: int = 0) -> "AugmentConfig":
        """the transform set of `runner.py --train --augment default` (INVENTED by this build: the module docstring)"""
        return cls(seed=seed, max_shift=8, permute_rgb=True, background=(255, 255), brightness=(0.8, 1.2), contrast=(0.8, 1.2),
                   saturation=(0.8, 1.2), noise_sigma=0.02)

    @property
    def needs_scratch(self) -> bool:
        return tuple(self.contrast) != (1.0, 1.0)

    def desc(self, channels: int) -> "_lib.AugmentDesc":
        return _lib.AugmentDesc(int(self.seed), int(channels), int(self.max_shift), _lib.AUG_PERMUTE_RGB if self.permute_rgb else 0,
                                int(self.background[0]), int(self.background[1]), *self.brightness, *self.contrast, *self.saturation,
                                self.noise_sigma)


def _check_render(x, name):
    if not isinstance(x, torch.Tensor):
        raise TypeError(f"{name} must be a torch.Tensor")
    if not x.is_cuda:
        raise RuntimeError(f"{name} must live on a HIP device (got {x.device}); this path has no CPU fallback")
    if x.dtype != torch.uint8 or x.dim() != 4 or x.shape[1] not in (3, 4) or not x.is_contiguous():
        raise RuntimeError(f"{name} must be a contiguous (B, 3 or 4, H, W) uint8 tensor, got {tuple(x.shape)} {x.dtype}")
    return x


def _check_map(t, name, shape, device):
    if not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or tuple(t.shape) != tuple(shape) or t.device != device \
            or not t.is_contiguous():
        raise RuntimeError(f"{name} must be a contiguous fp32 tensor of shape {tuple(shape)} on {device}")
    return t


@torch.no_grad()
def augment_pair(left: torch.Tensor, right: torch.Tensor, sample_ids: torch.Tensor, config: AugmentConfig,
                 disp_left: Optional[torch.Tensor] = None, disp_right: Optional[torch.Tensor] = None, out=None, scratch=None):
    """(out_left, out_right) — with disparity maps (out_left, out_right, out_disp_left, out_disp_right) — of `s3r_augment_pair`:
    left, right (B, 3 or 4, H, W) uint8 renders, sample_ids (B,) int64 ON THE DEVICE, disp_* (B, H, W) fp32 ground-truth maps in render
    pixels (both or neither).  The outputs are (B, 3, H, W) fp32 in [0, 1] and the maps shifted with the renders (+inf where the shift
    uncovers the border).  `out` is a tuple of tensors to write into (as many as are returned); `scratch` a float buffer of at least
    `s3r_augment_scratch_elems` floats.  No autograd: renders are data."""
    if not isinstance(config, AugmentConfig):
        raise TypeError("config must be an AugmentConfig")
    left, right = _check_render(left, "left"), _check_render(right, "right")
    if right.shape != left.shape or right.device != left.device:
        raise RuntimeError(f"left and right must have one shape and device, got {tuple(left.shape)} and {tuple(right.shape)}")
    B, ch, H, W = left.shape
    dev = left.device
    if not isinstance(sample_ids, torch.Tensor) or sample_ids.dtype != torch.int64 or tuple(sample_ids.shape) != (B,) \
            or sample_ids.device != dev or not sample_ids.is_contiguous():
        raise RuntimeError(f"sample_ids must be a contiguous ({B},) int64 tensor on {dev}")
    if (disp_left is None) != (disp_right is None):
        raise RuntimeError("disp_left and disp_right must be given together")
    with_disp = disp_left is not None
    if with_disp:
        disp_left, disp_right = _check_map(disp_left, "disp_left", (B, H, W), dev), _check_map(disp_right, "disp_right", (B, H, W), dev)
    shapes = [(B, 3, H, W)] * 2 + [(B, H, W)] * (2 if with_disp else 0)
    if out is None:
        out = tuple(torch.empty(s, dtype=torch.float32, device=dev) for s in shapes)
    else:
        out = tuple(out)
        if len(out) != len(shapes):
            raise RuntimeError(f"out must hold {len(shapes)} tensors, got {len(out)}")
        for i, (t, s) in enumerate(zip(out, shapes)):
            _check_map(t, f"out[{i}]", s, dev)
    if B == 0:
        return out
    lib = _lib.load()
    desc = config.desc(ch)
    need = _lib.check(lib.s3r_augment_scratch_elems(C.byref(desc), B, H, W), "augment_pair")
    if need and scratch is None:
        scratch = torch.empty(need, dtype=torch.float32, device=dev)
    if scratch is not None:
        if scratch.dtype != torch.float32 or scratch.device != dev or not scratch.is_contiguous():
            raise RuntimeError(f"scratch must be a contiguous fp32 tensor on {dev}")
    dl, dr = (disp_left.data_ptr(), disp_right.data_ptr()) if with_disp else (None, None)
    odl, odr = (out[2].data_ptr(), out[3].data_ptr()) if with_disp else (None, None)
    with torch.cuda.device(dev):
        _lib.check(lib.s3r_augment_pair(C.byref(desc), left.data_ptr(), right.data_ptr(), sample_ids.data_ptr(), dl, dr, out[0].data_ptr(),
                                        out[1].data_ptr(), odl, odr, B, H, W, None if scratch is None else scratch.data_ptr(),
                                        0 if scratch is None else scratch.numel(), _stream_ptr(dev)), "augment_pair")
    return out


class StereoAugment:
    """`augment_pair` with its output and scratch buffers kept between calls, keyed on the batch's shape: the same addresses at every
    call, so it can sit inside a captured training step (the renders, the ids and the maps are then copied into fixed buffers by the
    caller and the graph replays with fresh augmentation from the new ids).  `__call__` returns the kept tensors: copy what must
    outlive the next call."""

    def __init__(self, config: AugmentConfig):
        if not isinstance(config, AugmentConfig):
            raise TypeError("config must be an AugmentConfig")
        self.config = config
        self._key = None
        self._out = None
        self._scratch = None

    def buffers(self, left: torch.Tensor, with_disparity: bool):
        """allocate (not under stream capture) and return the kept (outputs, scratch) for batches shaped like `left`"""
        key = (tuple(left.shape), left.device, bool(with_disparity))
        if self._key != key:
            if torch.cuda.is_current_stream_capturing():
                raise RuntimeError("StereoAugment met a new batch shape under stream capture: run one batch of this shape before capturing")
            B, ch, H, W = left.shape
            shapes = [(B, 3, H, W)] * 2 + [(B, H, W)] * (2 if with_disparity else 0)
            need = 0
            if B:
                need = _lib.check(_lib.load().s3r_augment_scratch_elems(C.byref(self.config.desc(ch)), B, H, W), "StereoAugment")
            self._out = tuple(torch.empty(s, dtype=torch.float32, device=left.device) for s in shapes)
            self._scratch = torch.empty(need, dtype=torch.float32, device=left.device) if need else None
            self._key = key
        return self._out, self._scratch

    def __call__(self, left, right, sample_ids, disp_left=None, disp_right=None):
        left = _check_render(left, "left")
        out, scratch = self.buffers(left, disp_left is not None)
        return augment_pair(left, right, sample_ids, self.config, disp_left, disp_right, out=out, scratch=scratch)
