"""Host-side mirror of the reference's plugin surface for this path: ordinary `torch.nn.Module`s
named `encoder`, `cost_volume`, `decoder` (BASELINE.json north_star; the reference's own class
names live on unmounted branches, /root/reference/README.md:5) whose parameters are plain
nn.Conv/BatchNorm parameters — so `state_dict()` / `load_state_dict()` behave exactly like a stock
PyTorch model — but whose `forward` enqueues the hand-written HIP kernels of libs3r_hip.so through
its C-ABI.  PyTorch is plumbing here (device memory, streams); no torch conv / BN op runs in any
forward below, and nothing falls back to the CPU: without the HIP library every forward raises.

Inference modules (eval-mode BatchNorm): their forwards carry no autograd graph; the `differentiable_*` functions and methods below
record one, with the library's own deterministic backward kernels behind it.
"""
from __future__ import annotations

import collections
import ctypes as C
import dataclasses
import os
import weakref
from typing import Dict, List, Optional, Sequence

import torch
import torch.nn as nn

from . import _lib
from . import arch_spec as spec

MAX_CHUNK = 256      # pairs per C-ABI call: keeps every activation < 2^31 elements / 4 GiB

# Per-layer descriptor overrides of tuning / diagnosis runs: layer name -> value, for every module of the process, while a
# `debug_overrides(...)` context is open.  The release path consults nothing else: no environment variable reaches a descriptor
# (r05 read S3R_TILE_<layer> / S3R_KSPLIT_<layer> / S3R_ALGO_<layer> on every forward).
_DEBUG = {"tile": {}, "ksplit": {}, "algo": {}}


class debug_overrides:
    """`with s3r.debug_overrides(tile={"v2": 2}, ksplit={"v4": 2}, algo={"e6": s3r.ALGO_DIRECT}): ...`

    Forces descriptor fields of named layers — the direct kernel's tile code, the split-K factor, the algorithm — for every
    forward enqueued inside the context.  These CHANGE RESULT BITS (another summation order / another algorithm): a tuning and
    diagnosis facility (tools/layer_bench.py, tools/ab_*.py), never set on a deployment path.  Nesting merges; leaving restores.
    A module captured in a HIP graph keeps the plan it was captured with."""

    def __init__(self, tile=None, ksplit=None, algo=None):
        self._new = {"tile": dict(tile or {}), "ksplit": dict(ksplit or {}), "algo": dict(algo or {})}
        for kind, d in self._new.items():
            for name, v in d.items():
                if not isinstance(name, str) or not isinstance(v, int):
                    raise TypeError(f"debug_overrides({kind}=...): layer name -> int, got {name!r}: {v!r}")

    def __enter__(self):
        self._saved = {k: dict(v) for k, v in _DEBUG.items()}
        for k, d in self._new.items():
            _DEBUG[k].update(d)
        return self

    def __exit__(self, *exc):
        for k in _DEBUG:
            _DEBUG[k].clear()
            _DEBUG[k].update(self._saved[k])
        return False

    @staticmethod
    def active() -> dict:
        """what is in force now ({} x 3 on a release path; bench.py marks a run under any of it as not the plain configuration)"""
        return {k: dict(v) for k, v in _DEBUG.items() if v}


def _aligned16(x: torch.Tensor) -> torch.Tensor:
    """The library's alignment contract (include/s3r.h, Conventions) for the tensors that need more than their element size: a
    bf16 tensor and a render must start 16-byte aligned.  A torch view at a storage offset that breaks it (a slice of a larger
    buffer) is copied once, so that no view is ever refused; fp32 / int32 tensors need 4 bytes and never come here."""
    return x.clone() if x.data_ptr() % 16 else x


def _to_channels_last_physical(x: torch.Tensor) -> torch.Tensor:
    """logical (B,C,...) tensor -> contiguous physical (B,...,C) tensor (no copy if already channels-last)."""
    nd = x.dim()
    return x.permute(0, *range(2, nd), 1).contiguous()


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


def _check_render(x: torch.Tensor, name: str) -> torch.Tensor:
    """A batch of renders, (B,3,224,224): float32 in [0,1], or uint8 as a PNG decode yields them (the stem scales by
    1/255 as it reads, bit-identical to `x.float() / 255` on the host: `s3r_encoder_forward_u8`)."""
    dt = x.dtype if isinstance(x, torch.Tensor) and x.dtype == torch.uint8 else torch.float32
    # the stems fetch whole rows by 16-byte LDS-DMA: a view at an odd storage offset is copied once
    return _aligned16(_check_input(x, name, (3, spec.IMG_HW, spec.IMG_HW), dt))


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


class _Workspace:
    """A chain's activation arena.  Every intermediate of the chain has its own region in it, stored with
    the zero halo the next layer's gather reads; the kernels write interiors only, so the
    arena is zeroed ONCE per (layout = batch size) — `fresh` tells the C-ABI call to do that — and then
    stays resident: nothing is re-allocated or re-zeroed on the steady-state path."""

    def __init__(self):
        self.buf: Optional[torch.Tensor] = None
        self.layout = None
        self.pinned = False      # a captured HIP graph holds this buffer's address and layout

    def get(self, device, elems: int, layout):
        fresh = 0
        if self.buf is None or self.buf.device != device or self.buf.numel() < elems or self.layout != layout:
            if self.pinned:
                raise RuntimeError("this module's activation arena is captured in a HIP graph (GraphedForward) for "
                                   f"layout {self.layout}; run other batch shapes on another module instance")
        if self.buf is None or self.buf.device != device or self.buf.numel() < elems:
            self.buf = torch.empty(max(elems, 1), dtype=torch.float32, device=device)
            fresh = 1
        if self.layout != layout:
            self.layout, fresh = layout, 1
        return self.buf, fresh


class _Block(nn.Module):
    """Parameter holder for one arch_spec.Layer (conv [+ bn]); never called."""

    def __init__(self, layer: spec.Layer):
        super().__init__()
        self.layer = layer
        if layer.op == "conv2d":
            self.conv = nn.Conv2d(layer.cin, layer.cout, layer.k, layer.s, layer.p, dilation=layer.dil, bias=True)
            self.bn = nn.BatchNorm2d(layer.cout, eps=spec.BN_EPS) if layer.bn else None
        elif layer.op == "conv3d":
            self.conv = nn.Conv3d(layer.cin, layer.cout, layer.k, layer.s, layer.p, dilation=layer.dil, bias=True)
            self.bn = nn.BatchNorm3d(layer.cout, eps=spec.BN_EPS) if layer.bn else None
        elif layer.op == "deconv3d":
            self.conv = nn.ConvTranspose3d(layer.cin, layer.cout, layer.k, layer.s, layer.p, output_padding=layer.opad,
                                           dilation=layer.dil, bias=True)
            self.bn = nn.BatchNorm3d(layer.cout, eps=spec.BN_EPS) if layer.bn else None
        elif layer.op == "deconv2d":
            self.conv = nn.ConvTranspose2d(layer.cin, layer.cout, layer.k, layer.s, layer.p, output_padding=layer.opad,
                                           dilation=layer.dil, bias=True)
            self.bn = nn.BatchNorm2d(layer.cout, eps=spec.BN_EPS) if layer.bn else None
        elif layer.op == "linear":
            self.conv = nn.Linear(layer.cin, layer.cout, bias=True)
            self.bn = None
        else:
            raise ValueError(layer.op)

    def forward(self, *a, **k):
        raise RuntimeError("parameter holder: the enclosing HIP module runs the kernel")

    @torch.no_grad()
    def folded(self):
        """(scale, shift) of the fused epilogue y = conv_nobias(x) * scale + shift."""
        bias = self.conv.bias.detach().float()
        if self.bn is None:
            return None, bias.contiguous()
        bn = self.bn
        scale = bn.weight.detach().float() * torch.rsqrt(bn.running_var.detach().float() + bn.eps)
        shift = bn.bias.detach().float() + (bias - bn.running_mean.detach().float()) * scale
        return scale.contiguous(), shift.contiguous()


class _HipChain(nn.Module):
    """A sequence of arch_spec layers executed by one C-ABI stage call."""

    _entry = "s3r_chain_forward"

    def __init__(self, layers: Sequence[spec.Layer], in_size: int, tag_base: int = 0, precision: str = "fp32",
                 winograd=None):
        super().__init__()
        if precision not in _lib.DTYPE:
            raise ValueError(f"precision must be one of {list(_lib.DTYPE)}")
        if winograd not in (None, True, False):
            raise ValueError("winograd must be None (the library's geometry-only policy), True or False")
        self.precision = precision
        # fp32 convolution algorithm of every layer that has both kernels (include/s3r.h, s3r_algo): None = the library's
        # policy; False = the direct kernels only (what a latency-bound deployment at batches < 8 may prefer: DESIGN.md);
        # True = the Winograd kernel wherever the layer has one.  The two agree to fp32 rounding, not bit for bit, so the
        # choice belongs to the model, never to the batch.
        self.winograd = winograd
        self.algo_override: Dict[str, int] = {}      # layer name -> _lib.ALGO_*                    (tuning / tests)
        self._dtype = _lib.DTYPE[precision]
        self._layers = tuple(layers)
        self._in_size = in_size
        self._tag_base = tag_base
        self.names = [l.name for l in layers]
        for l in layers:
            self.add_module(l.name, _Block(l))
        self._packed = None          # (key, [(packed_w, scale, shift)])
        self._ws = _Workspace()
        self.tile_override: Dict[str, int] = {}      # layer name -> tile cfg + 16*gather width  (tuning)
        self.ksplit_override: Dict[str, int] = {}    # layer name -> split-K factor               (tuning)
        if self.training:
            self.eval()              # inference path: eval-mode BatchNorm is the only mode implemented

    def train(self, mode: bool = True):
        if mode:
            raise RuntimeError("this build implements the forward/inference path only (eval-mode BatchNorm)")
        return super().train(False)

    # -- weight packing cache ------------------------------------------------------------------
    def _cache_key(self, device):
        # (the bf16 weight image depends on the matrix instruction the library packs for: S3R_BF16_MFMA, an A/B switch)
        items = [str(device), self.precision, os.environ.get("S3R_BF16_MFMA", "")]
        for t in list(self.parameters()) + list(self.buffers()):
            items.append((id(t), t._version, t.device.type))
        return tuple(items)

    def _sizes(self):
        rows, n = [], self._in_size
        for l in self._layers:
            m = spec.out_size(l, n)
            rows.append((n, m))
            n = m
        return rows

    @torch.no_grad()
    def _ensure_packed(self, device):
        key = self._cache_key(device)
        if self._packed is not None and self._packed[0] == key:
            return self._packed[1]
        if self._ws.pinned:
            raise RuntimeError("parameters changed after this module was captured in a HIP graph (GraphedForward): "
                               "re-capture (build a new GraphedForward) after load_state_dict / .to()")
        lib = _lib.load()
        packed = []
        stream = _stream_ptr(device)
        for l, (n_in, _) in zip(self._layers, self._sizes()):
            blk: _Block = getattr(self, l.name)
            w = blk.conv.weight.detach()
            if w.device != device:
                raise RuntimeError(f"{l.name}: parameters are on {w.device}, input on {device}; call .to(device) first")
            w = w.float().contiguous()
            desc = _lib.make_desc(l, 1, n_in, dtype=self._dtype)
            n = C.c_int64(0)
            _lib.check(lib.s3r_conv_packed_elems(C.byref(desc), C.byref(n)), f"{l.name}: packed_elems")
            pw = torch.empty(n.value, dtype=torch.float32, device=device)
            _lib.check(lib.s3r_conv_pack_weights(C.byref(desc), w.data_ptr(), pw.data_ptr(), stream),
                       f"{l.name}: pack_weights")
            scale, shift = blk.folded()
            packed.append((pw, scale, shift, w))   # keep w alive until the pack kernel has run
        self._packed = (key, packed)
        return packed

    def _layer_array(self, batch: int, device, upto: Optional[str] = None, in_halo: int = 0, in_layout: int = 0):
        packed = self._ensure_packed(device)
        n_layers = len(self._layers) if upto is None else self.names.index(upto) + 1
        arr = (_lib.Layer * n_layers)()
        for i, (l, (n_in, _)) in enumerate(zip(self._layers[:n_layers], self._sizes())):
            pw, scale, shift, _ = packed[i]
            tile, ksplit = self._tile_ksplit_of(l)
            algo = self._algo_of(l)
            # only the chain's own input / output halos are the caller's to state (the output is always
            # a plain contiguous tensor); the library plans the intermediates
            arr[i].desc = _lib.make_desc(l, batch, n_in, tag=self._tag_base + i, tile=tile,
                                         in_halo=in_halo if i == 0 else 0, ksplit=ksplit,
                                         dtype=self._dtype, in_layout=in_layout if i == 0 else 0, algo=algo)
            arr[i].packed_w = pw.data_ptr()
            arr[i].scale = scale.data_ptr() if scale is not None else None
            arr[i].shift = shift.data_ptr() if shift is not None else None
        return arr, n_layers

    def _has_winograd_form(self, l: spec.Layer) -> bool:
        """Whether the LIBRARY has a Winograd form for this layer at the size it has in this chain (edge >= 4, a transposed
        layer's edge % 4 == 0, no sigmoid, ...: the rules live in s3r_plan.hip's resolve_algo, so the question is put to the scratch query of a
        descriptor with algo = WINOGRAD instead of being mirrored here)."""
        if self.precision != "fp32" or l.op not in ("conv2d", "conv3d", "deconv3d"):
            return False
        n_in = self._sizes()[self.names.index(l.name)][0]
        desc = _lib.make_desc(l, 1, n_in, in_halo=1 if l.op == "deconv3d" else l.p, dtype=self._dtype, algo=_lib.ALGO_WINOGRAD)
        return _lib.load().s3r_conv_scratch_elems(C.byref(desc)) >= 0

    def _tile_ksplit_of(self, l: spec.Layer):
        """(tile, ksplit) of a layer's descriptor: an open `debug_overrides` context, else this module's tuning tables
        (`autotune`), else the library's own choice (-1, 0)."""
        return (int(_DEBUG["tile"].get(l.name, self.tile_override.get(l.name, -1))),
                int(_DEBUG["ksplit"].get(l.name, self.ksplit_override.get(l.name, 0))))

    def _algo_of(self, l: spec.Layer) -> int:
        """s3r_algo of a layer's descriptor: a per-layer override, else the model's `winograd` switch (only layers that
        have the Winograd form can be asked for it), else AUTO."""
        if l.name in _DEBUG["algo"]:
            return int(_DEBUG["algo"][l.name])
        if l.name in self.algo_override:
            return int(self.algo_override[l.name])
        if self.winograd is None:
            return _lib.ALGO_AUTO
        if self.winograd and self._has_winograd_form(l):
            return _lib.ALGO_WINOGRAD
        return _lib.ALGO_DIRECT

    def wino_input_layout(self, batch: int) -> int:
        """The transformed layout the chain's first layer would read from its producer for a halo-1 input of this batch —
        `_lib.LAYOUT_WINO_H` (one-axis Winograd kernel), `_lib.LAYOUT_WINO_DH` (two-axis kernel) — or `_lib.LAYOUT_PLAIN` when
        it runs the direct kernel or the batch does not fit one transformed call (CostVolume.forward_wino / forward_wino2)."""
        if self.precision != "fp32" or batch <= 0:
            return _lib.LAYOUT_PLAIN
        l, (n_in, _) = self._layers[0], self._sizes()[0]
        tile, ksplit = self._tile_ksplit_of(l)
        desc = _lib.make_desc(l, batch, n_in, tile=tile, in_halo=1, ksplit=ksplit, dtype=self._dtype, algo=self._algo_of(l))
        return _lib.check(_lib.load().s3r_conv_wino_input_layout(C.byref(desc)), "wino_input_layout")

    def takes_wino_input(self, batch: int) -> bool:
        return self.wino_input_layout(batch) != _lib.LAYOUT_PLAIN

    def _out_shape(self, batch: int, n_layers: int):
        l = self._layers[n_layers - 1]
        m = self._sizes()[n_layers - 1][1]
        nd = spec.ndim(l)
        return (batch, l.cout) + (m,) * nd

    def _out_is_bf16(self, n_layers: int) -> bool:
        l = self._layers[n_layers - 1]
        return self.precision == "bf16" and not (l.cout == 1 and l.k == 1)      # the occupancy head writes fp32

    @torch.no_grad()
    def _run(self, x: torch.Tensor, upto: Optional[str] = None, in_halo: int = 0,
             x2: Optional[torch.Tensor] = None, in_layout: int = 0) -> torch.Tensor:
        """x: the chain input; with in_halo > 0 it is a halo-padded buffer (B, C, n+2h, ...) whose border
        is zero (internal hand-off from the cost-volume kernel), otherwise a plain contiguous tensor.
        x2 (encoder only): a second tensor of as many images — the chain runs over x's images, then x2's."""
        lib = _lib.load()
        device, batch = x.device, x.shape[0] + (x2.shape[0] if x2 is not None else 0)
        if in_layout in (_lib.LAYOUT_WINO_H, _lib.LAYOUT_WINO_DH):      # (6 | 36, B, C, ...): the transformed plane sets of the padded input
            batch = x.shape[1]
        if batch == 0:                 # same dtype / layout contract as a non-empty batch
            n0 = len(self._layers) if upto is None else self.names.index(upto) + 1
            shape = self._out_shape(0, n0)
            if self._out_is_bf16(n0):
                return _to_logical(torch.empty((0,) + shape[2:] + (shape[1],), dtype=torch.bfloat16, device=device))
            return torch.empty(shape, dtype=torch.float32, device=device)
        arr, n = self._layer_array(batch, device, upto, in_halo, in_layout)
        shape = self._out_shape(batch, n)
        if self._out_is_bf16(n):    # physical channels-last (B,...,C) bf16; handed back as a logical (B,C,...) view
            y = torch.empty((shape[0],) + shape[2:] + (shape[1],), dtype=torch.bfloat16, device=device)
        else:
            y = torch.empty(shape, dtype=torch.float32, device=device)
        need = _lib.check(lib.s3r_chain_workspace_elems(arr, n), "workspace query")
        # the arena's layout is the library's PLAN for this chain: batch, depth, input halo and every layer's
        # requested (tile, split-K) — those decide head fusion and where the split-K scratch starts.  Any change
        # re-zeroes the arena (fresh), so no region is ever read with another plan's bytes in its halo.
        cfg = tuple((arr[i].desc.tile, arr[i].desc.ksplit, arr[i].desc.algo) for i in range(n)) + (in_layout,)
        ws, fresh = self._ws.get(device, need, (batch, n, in_halo, need, cfg))
        u8 = x.dtype == torch.uint8
        if (u8 or x2 is not None) and self._entry != "s3r_encoder_forward":
            raise RuntimeError("8-bit renders / a (left, right) tensor pair are inputs of the encoder only")
        if x2 is not None and x2.dtype != x.dtype:
            raise RuntimeError("left and right renders must share one dtype")
        if x2 is not None or u8:                 # (any prefix of the tower: the entry takes a chain that starts with the stem)
            enc = lib.s3r_encoder_forward_u8 if u8 else lib.s3r_encoder_forward
            _lib.check(enc(arr, n, x.data_ptr(), x2.data_ptr() if x2 is not None else None, y.data_ptr(), ws.data_ptr(),
                           ws.numel(), fresh, _stream_ptr(device)), type(self).__name__)
        elif upto is None and self._entry == "s3r_encoder_forward":
            _lib.check(lib.s3r_encoder_forward(arr, n, x.data_ptr(), None, y.data_ptr(), ws.data_ptr(), ws.numel(), fresh,
                                               _stream_ptr(device)), type(self).__name__)
        else:
            entry = getattr(lib, self._entry if upto is None else "s3r_chain_forward")
            _lib.check(entry(arr, n, x.data_ptr(), y.data_ptr(), ws.data_ptr(), ws.numel(), fresh, _stream_ptr(device)),
                       type(self).__name__)
        return _to_logical(y) if self._out_is_bf16(n) else y


    # -- measured per-layer configuration ----------------------------------------------------------
    _TUNE_TILES = (1, 2, 3, 7, 0)               # fp32 tile configurations (s3r_conv_glds.hip)
    _TUNE_TILES_BF16 = (1, 3, 9, 17, 22, 23)    # bf16: per-tap (128 / 128x128 / 32-ch K), row-reuse, plane-reuse.  (30 / 31,
                                                # plane-reuse over a parity-split input, are not candidates: forcing them
                                                # also switches the PRODUCER's output layout, a cost these per-layer
                                                # timings would not count; the hand-off measured slower)
    _TUNE_KSPLITS = (1, 2, 4, 8)

    def _differentiable_layers(self, x: torch.Tensor, first: int, stop: int, batch_stats: bool = False) -> torch.Tensor:
        """Layers first .. stop - 1 of this chain, one `differentiable_conv` each, on this module's OWN parameters.  A block's BatchNorm
        stays in eval mode and folded: `scale` is `_Block.folded()`'s scale (detached: `bn.weight` is FROZEN on this path, and so are the
        running statistics); `shift` is folded()'s expression evaluated with torch operations under grad, so grad_shift reaches
        `bn.bias` and `conv.bias` through torch.
        batch_stats=True: a layer WITH a BatchNorm runs as torch runs the block in training mode, in two calls —
        `differentiable_conv(x, conv.weight, None, conv.bias, <the layer with act "none">)`, then
        `differentiable_batchnorm(z, blk.bn, layer.act)`: batch statistics, gradients to `bn.weight` and `bn.bias`, the running
        statistics updated.  Layers without a BatchNorm are unchanged."""
        n_in = self._sizes()[first][0]
        x = _check_input(x, "x", (self._layers[first].cin,) + (n_in,) * spec.ndim(self._layers[first]))
        for l in self._layers[first:stop]:
            blk: _Block = getattr(self, l.name)
            if batch_stats and blk.bn is not None:
                z = differentiable_conv(x, blk.conv.weight, None, blk.conv.bias, dataclasses.replace(l, act="none"))
                x = differentiable_batchnorm(z, blk.bn, l.act)
                continue
            scale, _ = blk.folded()
            if scale is None:
                shift = blk.conv.bias
            else:
                shift = blk.bn.bias + (blk.conv.bias - blk.bn.running_mean.detach()) * scale
            x = differentiable_conv(x, blk.conv.weight, scale, shift, l)
        return x

    def _mfma_layers(self):
        return [l for l in self._layers
                if l.op in ("conv2d", "conv3d", "deconv3d") and l.cin % 16 == 0 and not (l.cout == 1 and l.k == 1)]

    @torch.no_grad()
    def autotune(self, x: torch.Tensor, in_halo: int = 0, rounds: int = 3, log=None):
        """Pick every MFMA layer's (tile, split-K) by timing the candidates on `x` (HIP events around the
        layer's own launches, median of `rounds` runs of the whole chain) and keep the winners in
        tile_override / ksplit_override.  Split-K changes a sample's summation order, so an autotuned
        module is deterministic for a given batch size but no longer bit-identical ACROSS batch sizes."""
        chosen = {}
        for l in self._mfma_layers():
            tag = self._tag_base + self.names.index(l.name)
            bf16 = self.precision == "bf16"
            chunks = l.cin // (32 if bf16 else 16)
            best = None
            for ks in self._TUNE_KSPLITS:
                if chunks % ks:
                    continue
                for t in (self._TUNE_TILES_BF16 if bf16 else self._TUNE_TILES):
                    self.tile_override[l.name], self.ksplit_override[l.name] = t, ks
                    ms = []
                    try:
                        for r in range(rounds + 1):
                            _lib.profile_enable(8 * len(self._layers) + 8)
                            self._run(x, None, in_halo)
                            rec = _lib.profile_read(8 * len(self._layers) + 8)
                            _lib.profile_enable(0)
                            if r:
                                ms.append(sum(q["ms"] for q in rec if q["tag"] == tag and q["family"] == "conv_mfma"))
                    except _lib.S3RError:
                        _lib.profile_enable(0)
                        continue
                    ms.sort()
                    if best is None or ms[len(ms) // 2] < best[0]:
                        best = (ms[len(ms) // 2], t, ks)
            if best is None:
                self.tile_override.pop(l.name, None), self.ksplit_override.pop(l.name, None)
                continue
            self.tile_override[l.name], self.ksplit_override[l.name] = best[1], best[2]
            chosen[l.name] = {"tile": best[1], "ksplit": best[2], "ms": round(best[0], 4)}
            if log:
                log(f"autotune {l.name}: tile {best[1]} ksplit {best[2]} -> {best[0]:.4f} ms")
        return chosen


class Encoder(_HipChain):
    """Shared-weight 2D conv tower: (N,3,224,224) renders -> (N,32,28,28) features.

    The same weights serve both views: `forward_pair(left, right)` runs the tower once over both tensors (what
    Stereo2Voxel / Stereo2Point call); `forward(images)` takes any single batch of renders.
    """
    _entry = "s3r_encoder_forward"

    def __init__(self, precision: str = "fp32", winograd=None):
        super().__init__(spec.ENCODER, spec.IMG_HW, tag_base=100, precision=precision, winograd=winograd)

    def forward(self, images: torch.Tensor, upto: Optional[str] = None) -> torch.Tensor:
        """fp32: (N,32,28,28) contiguous.  bf16: (N,32,28,28) bfloat16 in channels_last memory format.
        `images`: float32 in [0,1] or uint8 (`_check_render`).
        `upto`: stop after the named layer (stage-by-stage checks), as on Decoder.forward."""
        x = _check_render(images, "images")
        return self._run(x, upto)

    def forward_pair(self, left: torch.Tensor, right: torch.Tensor) -> torch.Tensor:
        """The tower over the B left and the B right renders in ONE pass, read from their two tensors (the first
        kernel picks its source by image index): features (2B,32,28,28), left batch first.  Equal, bit for bit, to
        `forward(torch.cat([left, right]))` — without the concatenation copy."""
        left = _check_render(left, "left")
        right = _check_render(right, "right")
        if left.shape[0] != right.shape[0] or left.device != right.device or left.dtype != right.dtype:
            raise RuntimeError("left and right must be two batches of one size and dtype on one device")
        if left.shape[0] == 0:
            return self._run(left)
        return self._run(left, None, 0, right)

    # -- the trainable tower (fp32 models) --------------------------------------------------------------
    def _differentiable(self, left: torch.Tensor, right: Optional[torch.Tensor], batch_stats: bool, who: str) -> torch.Tensor:
        if self.precision != "fp32":
            raise RuntimeError(f"{who} is implemented for fp32 models only (this one is {self.precision}): the backward kernels read "
                               "fp32 activations")
        n = left.shape[0] + (right.shape[0] if right is not None else 0)
        if n == 0 or n > 2 * MAX_CHUNK:
            raise RuntimeError(f"{who} takes 1 .. {MAX_CHUNK} pairs ({2 * MAX_CHUNK} images) per call, got {n} images: split the batch")
        l = self._layers[0]
        blk: _Block = getattr(self, l.name)
        if batch_stats:
            z = _StemFunction.apply(blk.conv.weight, blk.conv.bias, None, self, left, right, "none")
            x = differentiable_batchnorm(z, blk.bn, l.act)
        else:
            scale, _ = blk.folded()
            shift = blk.bn.bias + (blk.conv.bias - blk.bn.running_mean.detach()) * scale
            x = _StemFunction.apply(blk.conv.weight, shift, scale, self, left, right, l.act)
        return self._differentiable_layers(x, 1, len(self._layers), batch_stats)

    def differentiable_pair(self, left: torch.Tensor, right: torch.Tensor, batch_stats: bool = False) -> torch.Tensor:
        """`forward_pair` recorded for autograd on this module's OWN parameters: features (2B,32,28,28), left batch first; B <= MAX_CHUNK
        pairs, fp32 models only.  e1 runs as `_StemFunction`: the stem kernel's forward on the renders as given (8-bit or fp32, in their
        two tensors: the one-layer chain `_run(left, "e1", 0, right)`), and `stem_backward` (`s3r_stem_backward`) behind it — no input
        gradient: nothing upstream of a render is trained.  e2 .. e8 run as `differentiable_conv`, one call each
        (`_differentiable_layers`).  By default every BatchNorm stays in eval mode and folded: `bn.weight` and the running statistics
        are frozen, the shift expression bn.bias + (conv.bias - running_mean) * scale is evaluated under grad, as on the decoder's path.
        batch_stats=True runs every block as torch runs it in training mode: the convolution without scale and activation, then
        `differentiable_batchnorm` with the statistics of all 2B images (what the reference's `encoder(torch.cat([left, right]))` does in
        training mode); `bn.weight` and `bn.bias` get gradients and the running statistics are updated.  The stem's forward kernel has
        no form without its activation, so e1's forward then goes through `conv_forward` (the general route) on the fp32 conversion of
        the concatenated renders, while its backward still is `s3r_stem_backward` (act none) on the renders as given."""
        left = _check_render(left, "left")
        right = _check_render(right, "right")
        if left.shape[0] != right.shape[0] or left.device != right.device or left.dtype != right.dtype:
            raise RuntimeError("left and right must be two batches of one size and dtype on one device")
        return self._differentiable(left, right, batch_stats, "Encoder.differentiable_pair")

    def differentiable(self, images: torch.Tensor, batch_stats: bool = False) -> torch.Tensor:
        """`forward` recorded for autograd on one tensor of renders (N <= 2 MAX_CHUNK images): see `differentiable_pair`."""
        return self._differentiable(_check_render(images, "images"), None, batch_stats, "Encoder.differentiable")


class CostVolume(nn.Module):
    """Bidirectional shift-and-diff disparity cost volume, (B,C,H,W) x2 -> (B,2C,D,H,W)."""

    def __init__(self, max_disp: int = spec.MAX_DISP, precision: str = "fp32"):
        super().__init__()
        self.max_disp = max_disp
        self.precision = precision
        self._padded: Optional[torch.Tensor] = None      # resident halo-padded volume (internal hand-off)
        self._planes: Optional[torch.Tensor] = None      # ... or its Winograd-transformed planes (forward_wino / forward_wino2)

    def _bf16(self, feat_left, feat_right, halo, resident):
        """bf16 path: logical (B,C,H,W) channels_last features -> physical (B,D+2h,H+2h,W+2h,2C) volume."""
        if feat_left.shape != feat_right.shape or feat_left.dim() != 4:
            raise RuntimeError("feature maps must both be (B,C,H,W)")
        fl = _check_input_cl(feat_left, "feat_left", feat_left.shape[1:])
        fr = _check_input_cl(feat_right, "feat_right", feat_left.shape[1:])
        B, H, W, Cc = fl.shape
        shape = (B, self.max_disp + 2 * halo, H + 2 * halo, W + 2 * halo, 2 * Cc)
        if resident:
            if self._padded is None or tuple(self._padded.shape) != shape or self._padded.device != fl.device \
                    or self._padded.dtype != torch.bfloat16:
                if getattr(self, "_pinned", False):
                    raise RuntimeError("the padded cost volume of this module is captured in a HIP graph for another shape")
                self._padded = torch.zeros(shape, dtype=torch.bfloat16, device=fl.device)
            vol = self._padded
        else:
            vol = torch.empty(shape, dtype=torch.bfloat16, device=fl.device)
        if B:
            _lib.check(_lib.load().s3r_cost_volume_forward_bf16(fl.data_ptr(), fr.data_ptr(), vol.data_ptr(), B, Cc,
                                                                self.max_disp, H, W, halo, _stream_ptr(fl.device)),
                       "cost_volume (bf16)")
        return vol

    @torch.no_grad()
    def forward_padded(self, feat_left: torch.Tensor, feat_right: torch.Tensor, halo: int = 1) -> torch.Tensor:
        """Internal hand-off to the decoder: the volume written straight into a resident
        (B,2C,D+2h,H+2h,W+2h) buffer whose zero halo the decoder's first 3D conv reads as its padding.
        The buffer is zeroed when (re)allocated; the kernel writes the interior only."""
        if self.precision == "bf16":
            return self._bf16(feat_left, feat_right, halo, resident=True)
        fl = _check_input(feat_left, "feat_left", feat_left.shape[1:])
        fr = _check_input(feat_right, "feat_right", feat_left.shape[1:])
        B, Cc, H, W = fl.shape
        shape = (B, 2 * Cc, self.max_disp + 2 * halo, H + 2 * halo, W + 2 * halo)
        if self._padded is None or tuple(self._padded.shape) != shape or self._padded.device != fl.device:
            if getattr(self, "_pinned", False):
                raise RuntimeError("the padded cost volume of this module is captured in a HIP graph for another shape")
            self._padded = torch.zeros(shape, dtype=torch.float32, device=fl.device)
        if B == 0:
            return self._padded
        _lib.check(_lib.load().s3r_cost_volume_forward(fl.data_ptr(), fr.data_ptr(), self._padded.data_ptr(), B, Cc,
                                                       self.max_disp, H, W, halo, _stream_ptr(fl.device)),
                   "cost_volume")
        return self._padded

    @torch.no_grad()
    def forward_wino(self, feat_left: torch.Tensor, feat_right: torch.Tensor) -> torch.Tensor:
        """fp32 internal hand-off to a decoder whose first 3D conv runs the Winograd kernel (`takes_wino_input`): the volume
        written directly as the six F(4,3)-along-H plane sets of its halo-1 padded form, (6,B,2C,D+2,H/4,W+2) — bit-identical
        to the consumer's own input transform, without the volume's round trip through HBM."""
        fl = _check_input(feat_left, "feat_left", feat_left.shape[1:])
        fr = _check_input(feat_right, "feat_right", feat_left.shape[1:])
        B, Cc, H, W = fl.shape
        shape = (6, B, 2 * Cc, self.max_disp + 2, H // 4, W + 2)      # F(4,3) along H: six plane sets, one row per four outputs
        if self._planes is None or tuple(self._planes.shape) != shape or self._planes.device != fl.device:
            if getattr(self, "_pinned", False):
                raise RuntimeError("the padded cost volume of this module is captured in a HIP graph for another shape")
            self._planes = torch.zeros(shape, dtype=torch.float32, device=fl.device)
        _lib.check(_lib.load().s3r_cost_volume_forward_wino(fl.data_ptr(), fr.data_ptr(), self._planes.data_ptr(), B, Cc,
                                                            self.max_disp, H, W, _stream_ptr(fl.device)), "cost_volume (wino)")
        return self._planes

    @torch.no_grad()
    def forward_wino2(self, feat_left: torch.Tensor, feat_right: torch.Tensor) -> torch.Tensor:
        """The same hand-off for a decoder whose first 3D conv runs the TWO-AXIS Winograd kernel: the 36 F(4,3) x F(4,3) plane
        sets of the halo-1 padded volume, (36,B,2C,D/4,H/4,W+2), bit-identical to the consumer's own input transform."""
        fl = _check_input(feat_left, "feat_left", feat_left.shape[1:])
        fr = _check_input(feat_right, "feat_right", feat_left.shape[1:])
        B, Cc, H, W = fl.shape
        shape = (36, B, 2 * Cc, self.max_disp // 4, H // 4, W + 2)
        if self._planes is None or tuple(self._planes.shape) != shape or self._planes.device != fl.device:
            if getattr(self, "_pinned", False):
                raise RuntimeError("the padded cost volume of this module is captured in a HIP graph for another shape")
            self._planes = torch.zeros(shape, dtype=torch.float32, device=fl.device)
        _lib.check(_lib.load().s3r_cost_volume_forward_wino2(fl.data_ptr(), fr.data_ptr(), self._planes.data_ptr(), B, Cc,
                                                             self.max_disp, H, W, _stream_ptr(fl.device)), "cost_volume (wino2)")
        return self._planes

    def forward_for(self, consumer, feat_left: torch.Tensor, feat_right: torch.Tensor):
        """(volume, in_layout) in whatever form `consumer` (a Decoder / VolumeEncoder) reads fastest for this batch."""
        layout = consumer.wino_input_layout(feat_left.shape[0])
        if layout == _lib.LAYOUT_WINO_H:
            return self.forward_wino(feat_left, feat_right), layout
        if layout == _lib.LAYOUT_WINO_DH:
            return self.forward_wino2(feat_left, feat_right), layout
        return self.forward_padded(feat_left, feat_right), _lib.LAYOUT_PLAIN

    @torch.no_grad()
    def forward(self, feat_left: torch.Tensor, feat_right: torch.Tensor) -> torch.Tensor:
        if self.precision == "bf16":      # logical (B,2C,D,H,W) view of the channels-last volume
            return _to_logical(self._bf16(feat_left, feat_right, 0, resident=False))
        if feat_left.shape != feat_right.shape or feat_left.dim() != 4:
            raise RuntimeError(f"feature maps must both be (B,C,H,W), got {tuple(feat_left.shape)} and "
                               f"{tuple(feat_right.shape)}")
        fl = _check_input(feat_left, "feat_left", feat_left.shape[1:])
        fr = _check_input(feat_right, "feat_right", feat_left.shape[1:])
        B, Cc, H, W = fl.shape
        vol = torch.empty((B, 2 * Cc, self.max_disp, H, W), dtype=torch.float32, device=fl.device)
        if B == 0:
            return vol
        _lib.check(_lib.load().s3r_cost_volume_forward(fl.data_ptr(), fr.data_ptr(), vol.data_ptr(), B, Cc,
                                                       self.max_disp, H, W, 0, _stream_ptr(fl.device)), "cost_volume")
        return vol

    def differentiable(self, feat_left: torch.Tensor, feat_right: torch.Tensor) -> torch.Tensor:
        """`forward` recorded for autograd on the two feature maps: the plain (B,2C,D,H,W) volume with the bits of `forward`, and the
        deterministic `cost_volume_backward` behind it (`differentiable_cost_volume`).  fp32 modules only.  The first step of a
        decoder fine-tune from the features:
        `model.decoder.differentiable_tail(model.cost_volume.differentiable(fl, fr), start="v1")`."""
        if self.precision != "fp32":
            raise RuntimeError(f"CostVolume.differentiable is implemented for fp32 models only (this one is {self.precision}): the "
                               "cost-volume backward kernel reads fp32 tensors")
        return differentiable_cost_volume(feat_left, feat_right, self.max_disp)


def _check_wino_planes(v: torch.Tensor, layout: int = _lib.LAYOUT_WINO_H) -> torch.Tensor:
    if layout == _lib.LAYOUT_WINO_DH:
        ncls, want = 36, (2 * spec.FEAT_C, spec.MAX_DISP // 4, spec.FEAT_HW // 4, spec.FEAT_HW + 2)
    else:
        ncls, want = 6, (2 * spec.FEAT_C, spec.MAX_DISP + 2, spec.FEAT_HW // 4, spec.FEAT_HW + 2)
    if not isinstance(v, torch.Tensor) or not v.is_cuda or v.dtype != torch.float32 or v.dim() != 6 or v.shape[0] != ncls or \
            tuple(v.shape[2:]) != want or not v.is_contiguous():
        raise RuntimeError(f"transformed volume must be a contiguous float32 HIP tensor ({ncls}, B, {', '.join(map(str, want))})")
    return v


class Decoder(_HipChain):
    """3D conv hourglass: cost volume (B,64,28,28,28) -> occupancy probabilities (B,32,32,32)."""
    _entry = "s3r_decoder_forward"

    def __init__(self, precision: str = "fp32", winograd=None):
        super().__init__(spec.DECODER, spec.MAX_DISP, tag_base=200, precision=precision, winograd=winograd)

    def forward(self, volume: torch.Tensor, upto: Optional[str] = None) -> torch.Tensor:
        tail = (2 * spec.FEAT_C, spec.MAX_DISP, spec.FEAT_HW, spec.FEAT_HW)
        if self.precision == "bf16":
            x = _check_input_cl(volume, "volume", tail)
        else:
            x = _check_input(volume, "volume", tail)
        y = self._run(x, upto)
        return y.squeeze(1) if upto is None or upto == self.names[-1] else y

    def forward_padded(self, volume_padded: torch.Tensor, halo: int = 1, in_layout: int = 0, upto: Optional[str] = None) -> torch.Tensor:
        """Decoder on the halo-padded volume CostVolume.forward_padded produced (no pad copy), or (in_layout =
        LAYOUT_WINO_H) on the transformed planes CostVolume.forward_wino produced."""
        last = upto is None or upto == self.names[-1]
        if in_layout in (_lib.LAYOUT_WINO_H, _lib.LAYOUT_WINO_DH):
            y = self._run(_check_wino_planes(volume_padded, in_layout), upto, in_halo=1, in_layout=in_layout)
            return y.squeeze(1) if last else y
        n = (spec.MAX_DISP + 2 * halo, spec.FEAT_HW + 2 * halo, spec.FEAT_HW + 2 * halo)
        if self.precision == "bf16":
            x = _check_input(volume_padded, "volume_padded", n + (2 * spec.FEAT_C,), torch.bfloat16)
        else:
            x = _check_input(volume_padded, "volume_padded", (2 * spec.FEAT_C,) + n)
        y = self._run(x, upto, in_halo=halo)
        return y.squeeze(1) if last else y

    # -- the trainable occupancy head (fp32 models) ---------------------------------------------------
    FEATURES = "d3"          # the layer whose output the occupancy head reads

    def _fp32_only(self, what: str):
        if self.precision != "fp32":
            raise RuntimeError(f"{what} is implemented for fp32 models only (this one is {self.precision}): the head backward and the "
                               "BCE kernels read fp32 tensors")

    def features(self, volume: torch.Tensor) -> torch.Tensor:
        """`forward(volume, upto="d3")`: the (B,64,32,32,32) activation the occupancy head reads, without a graph.  `forward`
        fuses d4 into d3's finish kernel, so this tensor exists only here."""
        self._fp32_only("Decoder.features")
        return self.forward(volume, upto=self.FEATURES)

    def differentiable_head(self, features: torch.Tensor) -> torch.Tensor:
        """The occupancy head d4 alone, recorded for autograd on d4's own nn.Conv3d parameters (the weight viewed as (64), gradients
        returned in the parameters' shapes): (B,64,32,32,32) -> (B,32,32,32).  The value is the STANDALONE head kernel's
        (`differentiable_head` below); `forward` computes d4 inside d3's finish pass, which agrees to fp32 rounding, not by contract
        bit for bit.  The head of a fine-tune step on a frozen trunk:
        `VoxelBCELoss()(model.decoder.differentiable_head(model.head_features(l, r)), gt).backward()`."""
        self._fp32_only("Decoder.differentiable_head")
        l = self._layers[-1]
        x = _check_input(features, "features", (l.cin,) + (spec.VOX,) * 3)
        blk: _Block = getattr(self, l.name)
        return differentiable_head(x, blk.conv.weight, blk.conv.bias, l.act)

    def differentiable_features(self, x: torch.Tensor, start: str = "d3", batch_stats: bool = False) -> torch.Tensor:
        """Layers `start` .. d3 recorded for autograd on this module's OWN parameters: x is `start`'s input (for "d3" the
        (B,128,16,16,16) activation `Stereo2Voxel.trunk_features(l, r, upto="d2")` returns), the result d3's (B,64,32,32,32) output —
        what `features()` returns, with a graph.  Every layer runs as `differentiable_conv`: its kernel's forward under the AUTO
        algorithm, `s3r_conv_backward` and the adjoint layer's forward behind it.  A block's BatchNorm stays in eval mode and folded:
        `scale` is `_Block.folded()`'s scale (detached: `bn.weight` is FROZEN on this path, its gradient stays None, and so are the
        running statistics); `shift` is folded()'s expression, bn.bias + (conv.bias - running_mean) * scale, evaluated with torch
        operations under grad, so grad_shift reaches `bn.bias` and `conv.bias` through torch.
        With start = "d3" the value HAS the bits of `features()` (the chain up to d3): measured bit-identical at B = 1, 2 and 5 on an
        MI355X (LAB_NOTES, "Conv backward") and pinned by
        tests/test_conv_backward_gpu.py::test_standalone_d3_forward_has_the_bits_of_the_chain on THIS method's output — both run d3's
        three-axis Winograd form on the same input, and its launch forms agree bit for bit.
        batch_stats=True trains the blocks as torch trains `nn.ConvTranspose3d + nn.BatchNorm3d + ReLU` in training mode: each BatchNorm
        layer runs `differentiable_conv` without scale and activation and then `differentiable_batchnorm` (batch statistics;
        `bn.weight.grad` and `bn.bias.grad` from the HIP backward; running statistics updated).  The value then depends on the batch."""
        self._fp32_only("Decoder.differentiable_features")
        if start not in self.names[:-1]:
            raise RuntimeError(f"start must be one of {self.names[:-1]}, got {start!r}")
        return self._differentiable_layers(x, self.names.index(start), len(self._layers) - 1, batch_stats)

    def differentiable_tail(self, x: torch.Tensor, start: str = "d3", batch_stats: bool = False) -> torch.Tensor:
        """`differentiable_head(differentiable_features(x, start))`: layers `start` .. d4 under autograd, (B,32,32,32) occupancy out.
        d4's standalone kernel agrees with the fused d3 + d4 pass of `forward` to fp32 rounding (`differentiable_head`).  `bn.weight`
        is frozen unless batch_stats=True (see `differentiable_features`).  The fine-tune step on a frozen trunk:
        `VoxelBCELoss()(model.decoder.differentiable_tail(model.trunk_features(l, r, upto="d2")), gt).backward()`."""
        self._fp32_only("Decoder.differentiable_tail")
        return self.differentiable_head(self.differentiable_features(x, start, batch_stats))


class VolumeEncoder(_HipChain):
    """The down half of the hourglass alone (Stereo2Point): cost volume -> (B,512,4,4,4) latent."""
    _entry = "s3r_decoder_forward"

    def __init__(self, precision: str = "fp32", winograd=None):
        super().__init__(spec.DECODER_DOWN, spec.MAX_DISP, tag_base=200, precision=precision, winograd=winograd)

    def forward(self, volume: torch.Tensor) -> torch.Tensor:
        tail = (2 * spec.FEAT_C, spec.MAX_DISP, spec.FEAT_HW, spec.FEAT_HW)
        if self.precision == "bf16":
            return self._run(_check_input_cl(volume, "volume", tail))
        return self._run(_check_input(volume, "volume", tail))

    def forward_padded(self, volume_padded: torch.Tensor, halo: int = 1, in_layout: int = 0) -> torch.Tensor:
        if in_layout in (_lib.LAYOUT_WINO_H, _lib.LAYOUT_WINO_DH):
            return self._run(_check_wino_planes(volume_padded, in_layout), None, in_halo=1, in_layout=in_layout)
        n = (spec.MAX_DISP + 2 * halo, spec.FEAT_HW + 2 * halo, spec.FEAT_HW + 2 * halo)
        if self.precision == "bf16":            # physical (B,D+2h,H+2h,W+2h,2C) bf16 -> logical (B,512,4,4,4) bf16
            x = _check_input(volume_padded, "volume_padded", n + (2 * spec.FEAT_C,), torch.bfloat16)
        else:
            x = _check_input(volume_padded, "volume_padded", (2 * spec.FEAT_C,) + n)
        return self._run(x, None, in_halo=halo)

    def differentiable_features(self, x: torch.Tensor, start: str = "v1", batch_stats: bool = False) -> torch.Tensor:
        """Layers `start` .. v6 recorded for autograd on this module's own parameters, by the loop of `Decoder.differentiable_features`
        (`bn.weight` frozen, `bn.bias` and `conv.bias` reached through the folded shift): x is `start`'s input — for "v1" the plain
        (B,64,28,28,28) volume `CostVolume.differentiable` returns —, the result the (B,512,4,4,4) latent
        `PointHead.differentiable` reads.  fp32 models only.  batch_stats=True: every BatchNorm layer in training form, as
        `Decoder.differentiable_features` describes."""
        if self.precision != "fp32":
            raise RuntimeError(f"VolumeEncoder.differentiable_features is implemented for fp32 models only (this one is "
                               f"{self.precision}): the conv backward kernels read fp32 tensors")
        if start not in self.names:
            raise RuntimeError(f"start must be one of {self.names}, got {start!r}")
        return self._differentiable_layers(x, self.names.index(start), len(self._layers), batch_stats)


class PointHead(_HipChain):
    """MLP on the flattened latent: (B,512,4,4,4) -> (B,2048,3)."""

    def __init__(self):
        super().__init__(spec.POINT_HEAD, 1, tag_base=300)

    def forward(self, latent: torch.Tensor) -> torch.Tensor:
        x = _check_input(latent, "latent", (spec.LATENT_C, 4, 4, 4))
        return self._run(x.view(x.shape[0], spec.LATENT_C * 64)).view(x.shape[0], spec.N_POINTS, 3)   # (B may be 0)

    def differentiable(self, latent: torch.Tensor) -> torch.Tensor:
        """`forward` recorded for autograd: the three layers run one by one through `differentiable_linear` on this module's own
        nn.Linear parameters — the kernel the chain launches for a linear layer, with the same arguments, so the value has the bits
        of `forward` — and carry the deterministic backward `linear_backward`.  The head of a fine-tune step on a frozen trunk:
        `ChamferDistance()(head.differentiable(model.latent(l, r)), target).backward()`.  An optimizer's in-place step bumps the
        parameters' `_version`, which invalidates `forward`'s packed-weight cache."""
        x = _check_input(latent, "latent", (spec.LATENT_C, 4, 4, 4))
        h = x.view(x.shape[0], spec.LATENT_C * 64)
        for l in self._layers:
            blk: _Block = getattr(self, l.name)
            h = differentiable_linear(h, blk.conv.weight, blk.conv.bias, l.act)
        return h.view(x.shape[0], spec.N_POINTS, 3)


# Default temperature of the soft read-out (`disparity_soft`, `disparity(readout="soft")`), in units of the matching cost (a sum of
# C = 32 absolute feature differences).  BUILD-SPECIFIED: no learned disparity head exists to fix it.
DISPARITY_TEMPERATURE = 1.0

READOUTS = ("wta", "soft")


class _DisparityMixin:
    """`disparity()` and `stereo_features()` for the networks that hold an `encoder` and a `cost_volume`."""

    disparity_temperature = DISPARITY_TEMPERATURE      # what disparity(readout="soft") uses when temperature is None

    @torch.no_grad()
    def disparity(self, left: torch.Tensor, right: torch.Tensor, in_pixels: bool = True, readout: str = "wta",
                  temperature: Optional[float] = None, full_resolution: bool = False, confidence: bool = False):
        """Predicted (left, right) disparity maps from this model's encoder features.

        readout="wta" (default): the winner-take-all read-out of the cost volume's shift-and-diff costs (`disparity_wta`), (B,28,28)
        each, integer feature pixels.  readout="soft": the sub-pixel soft-argmin over the same costs (`disparity_soft`) at
        `temperature` (default: the `disparity_temperature` attribute), (B,28,28), or (B,224,224) upsampled bilinearly when
        full_resolution; confidence=True also returns the two confidence maps (dl, dr, cl, cr).  Both are stand-in read-outs, not
        a learned head.  in_pixels scales disparities to 224x224 render pixels (x8), the unit of the dataset's EXR ground truth."""
        if readout not in READOUTS:
            raise ValueError(f"readout must be one of {READOUTS}, got {readout!r}")
        if readout == "wta" and (full_resolution or confidence or temperature is not None):
            raise ValueError("full_resolution / confidence / temperature need readout='soft' (the WTA read-out is integer, "
                             "at feature resolution)")
        if readout == "soft":
            return self._disparity_soft(left, right, in_pixels, temperature, full_resolution, confidence)
        left = _check_render(left, "left")
        right = _check_render(right, "right")
        if left.shape[0] != right.shape[0]:
            raise RuntimeError("left and right batch sizes differ")
        dls, drs = [], []
        for s in range(0, max(left.shape[0], 1), MAX_CHUNK):
            l, r = left[s:s + MAX_CHUNK], right[s:s + MAX_CHUNK]
            b = l.shape[0]
            feats = self.encoder.forward_pair(l, r)
            if feats.dtype != torch.float32:                     # bf16 path: channels-last bf16 -> fp32 NCHW (HIP kernel)
                feats = channels_last_to_f32(feats)
            dl, dr = disparity_wta(feats[:b], feats[b:], self.cost_volume.max_disp)
            dls.append(dl), drs.append(dr)
        dl = dls[0] if len(dls) == 1 else torch.cat(dls, 0)
        dr = drs[0] if len(drs) == 1 else torch.cat(drs, 0)
        scale = float(spec.IMG_HW // spec.FEAT_HW) if in_pixels else 1.0
        return dl * scale, dr * scale

    def _disparity_soft(self, left, right, in_pixels, temperature, full_resolution, confidence):
        tau = float(self.disparity_temperature if temperature is None else temperature)
        left = _check_render(left, "left")
        right = _check_render(right, "right")
        if left.shape[0] != right.shape[0]:
            raise RuntimeError("left and right batch sizes differ")
        scale = float(spec.IMG_HW // spec.FEAT_HW) if in_pixels else 1.0
        size = (spec.IMG_HW, spec.IMG_HW) if full_resolution else None
        parts = []
        for s in range(0, max(left.shape[0], 1), MAX_CHUNK):
            l, r = left[s:s + MAX_CHUNK], right[s:s + MAX_CHUNK]
            b = l.shape[0]
            feats = self.encoder.forward_pair(l, r)            # fp32 NCHW, or the bf16 channels-last features as they are
            parts.append(disparity_soft(feats[:b], feats[b:], self.cost_volume.max_disp, tau, size, scale, confidence))
        return tuple(p[0] if len(parts) == 1 else torch.cat(p, 0) for p in zip(*parts))

    def differentiable_disparity(self, left: torch.Tensor, right: torch.Tensor, in_pixels: bool = True,
                                 temperature: Optional[float] = None, full_resolution: bool = False, batch_stats: bool = False):
        """`disparity(readout="soft")`'s (left, right) disparity maps recorded for autograd on the encoder's parameters: the encoder
        through `encoder.differentiable_pair` (B <= MAX_CHUNK pairs, fp32 models only; batch_stats as there), then
        `differentiable_disparity_soft` with the scaling rules of `disparity`: (B,28,28), or (B,224,224) upsampled bilinearly when
        full_resolution; in_pixels scales to 224x224 render pixels (x8), the unit of the dataset's EXR ground truth; temperature
        defaults to the `disparity_temperature` attribute.  A training step on the disparity ground truth:
        `dl, dr = model.differentiable_disparity(l, r, full_resolution=True); (DisparityLoss()(dl, gt_l) + DisparityLoss()(dr, gt_r)).backward()`."""
        tau = float(self.disparity_temperature if temperature is None else temperature)
        feats = self.encoder.differentiable_pair(left, right, batch_stats)
        b = feats.shape[0] // 2
        scale = float(spec.IMG_HW // spec.FEAT_HW) if in_pixels else 1.0
        size = (spec.IMG_HW, spec.IMG_HW) if full_resolution else None
        return differentiable_disparity_soft(feats[:b], feats[b:], self.cost_volume.max_disp, tau, size, scale)

    @torch.no_grad()
    def stereo_features(self, left: torch.Tensor, right: torch.Tensor):
        """(feat_left, feat_right), (B,32,28,28) fp32 each: the FROZEN encoder without a graph — the two maps `forward` feeds the cost
        volume, through the same `encoder.forward_pair` per chunk of MAX_CHUNK pairs.  Leaves for a decoder fine-tune that wants gradients
        with respect to the features: `fl.requires_grad_()`, then `cost_volume.differentiable(fl, fr)`.  fp32 models only."""
        if self.precision != "fp32":
            raise RuntimeError(f"stereo_features is implemented for fp32 models only (this one is {self.precision}): the cost-volume "
                               "backward kernel reads fp32 tensors")
        left = _check_render(left, "left")
        right = _check_render(right, "right")
        if left.shape[0] != right.shape[0]:
            raise RuntimeError("left and right batch sizes differ")
        fls, frs = [], []
        for s in range(0, max(left.shape[0], 1), MAX_CHUNK):
            l, r = left[s:s + MAX_CHUNK], right[s:s + MAX_CHUNK]
            b = l.shape[0]
            feats = self.encoder.forward_pair(l, r)              # (2b,32,28,28): left batch, then right batch
            fls.append(feats[:b]), frs.append(feats[b:])
        if len(fls) == 1:
            return fls[0].clone(), frs[0].clone()                # (own tensors: the chain's output buffer is not the caller's)
        return torch.cat(fls, 0), torch.cat(frs, 0)


class Stereo2Voxel(_DisparityMixin, nn.Module):
    """left,right (B,3,224,224) -> (B,32,32,32) occupancy.  state_dict keys: encoder.*, decoder.*

    precision="fp32": exact-fp32 MFMA path, NCHW (BASELINE configs[1]).  precision="bf16": bf16 MFMA path,
    channels-last bf16 activations with fp32 accumulation (BASELINE configs[2]); parameters stay fp32
    nn.Parameters either way (same state_dict), the bf16 images of the weights are made at pack time."""

    def __init__(self, precision: str = "fp32", winograd=None):
        """winograd: None = the library's policy (S3R_ALGO_AUTO: every layer that has a Winograd form runs it — one-axis F(4,3) on
        e2 / e4, two-axis F(4,3)^2 / F(2,4)^2 on the stride-1 layers with an edge <= 28, F(2,2)^2 inside the parity classes of the
        transposed layers; each measured faster than the direct kernel at B = 1, 4, 8 and 32); False = the direct
        kernels only; True = ask for the Winograd kernel on every layer the library has one for (direct elsewhere).
        Results differ between the settings at fp32 rounding level (never with the batch)."""
        super().__init__()
        self.precision = precision
        self.winograd = winograd
        self.encoder = Encoder(precision, winograd)
        self.cost_volume = CostVolume(precision=precision)
        self.decoder = Decoder(precision, winograd)
        self.eval()

    def train(self, mode: bool = True):
        if mode:
            raise RuntimeError("forward/inference path only")
        return super().train(False)

    def _decoded(self, left: torch.Tensor, right: torch.Tensor, upto: Optional[str] = None):
        """Encoder, cost volume and the decoder up to `upto` (None: all of it) per chunk of MAX_CHUNK pairs.  `forward` and
        `head_features` both run THIS, so the two cannot drift apart."""
        left = _check_render(left, "left")
        right = _check_render(right, "right")
        if left.shape[0] != right.shape[0]:
            raise RuntimeError("left and right batch sizes differ")
        for s in range(0, max(left.shape[0], 1), MAX_CHUNK):
            l, r = left[s:s + MAX_CHUNK], right[s:s + MAX_CHUNK]
            b = l.shape[0]
            feats = self.encoder.forward_pair(l, r)          # (2b,32,28,28): left batch, then right batch
            # (v1 on a Winograd kernel: the volume goes over in the transformed layout that kernel reads)
            vol, layout = self.cost_volume.forward_for(self.decoder, feats[:b], feats[b:])
            yield self.decoder.forward_padded(vol, in_layout=layout, upto=upto)

    @torch.no_grad()
    def forward(self, left: torch.Tensor, right: torch.Tensor) -> torch.Tensor:
        """left, right: (B,3,224,224) float32 in [0,1] or uint8 (8-bit renders: scaled by 1/255 inside the first kernel)."""
        outs = list(self._decoded(left, right))
        return outs[0] if len(outs) == 1 else torch.cat(outs, 0)

    def differentiable(self, left: torch.Tensor, right: torch.Tensor, batch_stats: bool = False) -> torch.Tensor:
        """The whole network recorded for autograd on its own parameters: (B,32,32,32) occupancy, B <= MAX_CHUNK, fp32 models only.
        `encoder.differentiable_pair`, `cost_volume.differentiable`, `decoder.differentiable_tail(start="v1")` — every stage on its
        plain standalone kernels, so the value agrees with `forward` (which fuses hand-offs) to fp32 rounding, not bit for bit.
        A training step: `VoxelBCELoss()(model.differentiable(l, r), gt).backward()`.  batch_stats: see `Encoder.differentiable_pair`."""
        self.decoder._fp32_only("Stereo2Voxel.differentiable")
        feats = self.encoder.differentiable_pair(left, right, batch_stats)
        b = feats.shape[0] // 2
        return self.decoder.differentiable_tail(self.cost_volume.differentiable(feats[:b], feats[b:]), "v1", batch_stats)

    @torch.no_grad()
    def trunk_features(self, left: torch.Tensor, right: torch.Tensor, upto: str = "d2") -> torch.Tensor:
        """The frozen trunk — encoder, cost volume, decoder up to the layer `upto` (any decoder layer in front of d4) — without a graph:
        the fp32 activation the layer behind `upto` reads.  `decoder.differentiable_tail(model.trunk_features(l, r, upto="d2"))` is
        the trainable part d3 + d4:
        `VoxelBCELoss()(model.decoder.differentiable_tail(model.trunk_features(l, r, upto="d2")), gt).backward()`.  fp32 models only."""
        self.decoder._fp32_only("Stereo2Voxel.trunk_features")
        if upto not in self.decoder.names[:-1]:
            raise RuntimeError(f"upto must be one of {self.decoder.names[:-1]}, got {upto!r}")
        outs = list(self._decoded(left, right, upto=upto))
        return outs[0] if len(outs) == 1 else torch.cat(outs, 0)

    @torch.no_grad()
    def head_features(self, left: torch.Tensor, right: torch.Tensor) -> torch.Tensor:
        """The frozen trunk alone — encoder, cost volume, decoder up to d3 — without a graph: the fp32 (B,64,32,32,32) activation the
        occupancy head reads (the counterpart of `Stereo2Point.latent`): `trunk_features(upto="d3")`.
        `decoder.differentiable_head(model.head_features(l, r))` is the trainable part.  fp32 models only."""
        self.decoder._fp32_only("Stereo2Voxel.head_features")
        return self.trunk_features(left, right, upto=Decoder.FEATURES)

    @torch.no_grad()
    def autotune(self, left: torch.Tensor, right: torch.Tensor, rounds: int = 3, log=None):
        """Measure-and-pick the per-layer kernel configuration on a representative batch (see
        _HipChain.autotune).  Returns {layer: {tile, ksplit, ms}}."""
        b = left.shape[0]
        images = torch.cat([left, right], 0)                 # (tuning only: one tensor for _HipChain.autotune)
        chosen = dict(self.encoder.autotune(images, rounds=rounds, log=log))
        feats = self.encoder(images)
        vol = self.cost_volume.forward_padded(feats[:b], feats[b:])
        chosen.update(self.decoder.autotune(vol, in_halo=1, rounds=rounds, log=log))
        return chosen


class Stereo2Point(_DisparityMixin, nn.Module):
    """left,right (B,3,224,224) -> (B,2048,3) point cloud.  Keys: encoder.*, decoder.*, point_head.*

    precision="bf16": the convolutional part (encoder, cost volume, v1-v6) on the bf16 MFMA path; the latent is handed
    to the point head as fp32 and the three linear layers stay fp32 (they stream 168 MB of weights: HBM-bound)."""

    def __init__(self, precision: str = "fp32", winograd=None):
        super().__init__()
        self.precision = precision
        self.winograd = winograd
        self.encoder = Encoder(precision, winograd)
        self.cost_volume = CostVolume(precision=precision)
        self.decoder = VolumeEncoder(precision, winograd)
        self.point_head = PointHead()
        self.eval()

    def train(self, mode: bool = True):
        if mode:
            raise RuntimeError("forward/inference path only")
        return super().train(False)

    def _latents(self, left: torch.Tensor, right: torch.Tensor):
        """The trunk — encoder, cost volume, volume encoder — per chunk of MAX_CHUNK pairs: yields the fp32 (b,512,4,4,4) latent.
        `forward` and `latent` both run THIS, so the two cannot drift apart."""
        left = _check_render(left, "left")
        right = _check_render(right, "right")
        if left.shape[0] != right.shape[0]:
            raise RuntimeError("left and right batch sizes differ")
        for s in range(0, max(left.shape[0], 1), MAX_CHUNK):
            l, r = left[s:s + MAX_CHUNK], right[s:s + MAX_CHUNK]
            b = l.shape[0]
            feats = self.encoder.forward_pair(l, r)
            vol, layout = self.cost_volume.forward_for(self.decoder, feats[:b], feats[b:])
            latent = self.decoder.forward_padded(vol, in_layout=layout)
            if latent.dtype != torch.float32:                      # bf16 channels-last view -> fp32 (B,512,4,4,4): HIP kernel
                latent = channels_last_to_f32(latent)
            yield latent

    @torch.no_grad()
    def forward(self, left: torch.Tensor, right: torch.Tensor) -> torch.Tensor:
        outs = [self.point_head(latent) for latent in self._latents(left, right)]
        return outs[0] if len(outs) == 1 else torch.cat(outs, 0)

    def differentiable(self, left: torch.Tensor, right: torch.Tensor, batch_stats: bool = False) -> torch.Tensor:
        """The whole network recorded for autograd on its own parameters: (B,2048,3) points, B <= MAX_CHUNK, fp32 models only.
        `encoder.differentiable_pair`, `cost_volume.differentiable`, `decoder.differentiable_features(start="v1")`,
        `point_head.differentiable`.  A training step: `ChamferDistance()(model.differentiable(l, r), target)`, then `.backward()` on
        the loss built from it.  batch_stats: see `Encoder.differentiable_pair`."""
        feats = self.encoder.differentiable_pair(left, right, batch_stats)
        b = feats.shape[0] // 2
        latent = self.decoder.differentiable_features(self.cost_volume.differentiable(feats[:b], feats[b:]), "v1", batch_stats)
        return self.point_head.differentiable(latent)

    @torch.no_grad()
    def latent(self, left: torch.Tensor, right: torch.Tensor) -> torch.Tensor:
        """The frozen trunk alone — encoder, cost volume, volume encoder — without a graph: the fp32 (B,512,4,4,4) latent that
        `forward` hands to the point head (the same code, the same bits).  `point_head.differentiable(model.latent(l, r))` is the
        trainable part."""
        outs = list(self._latents(left, right))
        return outs[0] if len(outs) == 1 else torch.cat(outs, 0)


_LINEAR_ACTS = ("none", "relu", "sigmoid")


def _check_linear(x, weight, act, who):
    if act not in _LINEAR_ACTS:
        raise RuntimeError(f"{who}: act must be one of {_LINEAR_ACTS}, got {act!r}")
    if x.dim() != 2 or weight.dim() != 2 or x.shape[1] != weight.shape[1]:
        raise RuntimeError(f"{who} expects x (B,Cin) and weight (Cout,Cin), got {tuple(x.shape)} and {tuple(weight.shape)}")
    x = _check_input(x, "x", (weight.shape[1],))
    w = weight.detach()
    if w.device != x.device or w.dtype != torch.float32 or not w.is_contiguous():
        raise RuntimeError(f"{who}: weight must be a contiguous fp32 tensor on {x.device}")
    if w.numel() == 0:
        raise RuntimeError(f"{who} needs a non-empty weight")
    return x, w


@torch.no_grad()
def linear(x: torch.Tensor, weight: torch.Tensor, bias: Optional[torch.Tensor], act: str = "none") -> torch.Tensor:
    """act(x weight^T + bias) on the HIP linear kernels (`s3r_linear_forward`): x (B,Cin), weight (Cout,Cin) in torch layout,
    bias (Cout) or None; act "none", "relu" or "sigmoid".  Records no graph (`differentiable_linear` does)."""
    x, w = _check_linear(x, weight, act, "linear")
    B, cin, cout = x.shape[0], w.shape[1], w.shape[0]
    b = None
    if bias is not None:
        b = bias.detach()
        if b.shape != (cout,) or b.device != x.device or b.dtype != torch.float32 or not b.is_contiguous():
            raise RuntimeError(f"linear: bias must be a contiguous fp32 ({cout},) tensor on {x.device}")
    y = torch.empty((B, cout), dtype=torch.float32, device=x.device)
    if B:
        lib = _lib.load()
        need = _lib.check(lib.s3r_linear_scratch_elems(B, cin, cout), "linear scratch query")
        scratch = torch.empty(max(need, 1), dtype=torch.float32, device=x.device)
        _lib.check(lib.s3r_linear_forward(x.data_ptr(), w.data_ptr(), None if b is None else b.data_ptr(), y.data_ptr(), B, cin, cout,
                                          _lib.ACT[act], scratch.data_ptr(), scratch.numel(), _stream_ptr(x.device)), "linear")
    return y


@torch.no_grad()
def linear_backward(x: torch.Tensor, weight: torch.Tensor, y: Optional[torch.Tensor], grad_y: torch.Tensor, act: str,
                    need_x: bool = True, need_w: bool = True, need_b: bool = True):
    """(grad_x (B,Cin), grad_w (Cout,Cin), grad_bias (Cout)) of y = act(x weight^T + bias) for the output gradient grad_y (B,Cout),
    `None` for the sides not asked for (`s3r_linear_backward`).  y is the layer's output (it may be None when act is "none").  Fixed
    summation orders, no atomics: the same bits on every run.  A side that is not needed costs neither its GEMM nor its traffic."""
    x, w = _check_linear(x, weight, act, "linear_backward")
    if not (need_x or need_w or need_b):
        raise RuntimeError("linear_backward needs need_x, need_w or need_b")
    B, cin, cout = x.shape[0], w.shape[1], w.shape[0]
    gy = _check_input(grad_y, "grad_y", (cout,))
    if gy.shape[0] != B:
        raise RuntimeError(f"grad_y must have batch {B}, got {tuple(gy.shape)}")
    yy = None
    if act != "none":
        if y is None:
            raise RuntimeError(f"linear_backward: act {act!r} needs the layer's output y")
        yy = _check_input(y, "y", (cout,))
        if yy.shape[0] != B:
            raise RuntimeError(f"y must have batch {B}, got {tuple(yy.shape)}")
    dev = x.device
    gx = torch.empty((B, cin), dtype=torch.float32, device=dev) if need_x else None
    gw = torch.empty((cout, cin), dtype=torch.float32, device=dev) if need_w else None
    gb = torch.empty((cout,), dtype=torch.float32, device=dev) if need_b else None
    if B == 0:                                     # an empty sum
        for t in (gw, gb):
            if t is not None:
                t.zero_()
        return gx, gw, gb
    lib = _lib.load()
    need = _lib.check(lib.s3r_linear_backward_scratch_elems(B, cin, cout), "linear backward scratch query")
    scratch = torch.empty(max(need, 1), dtype=torch.float32, device=dev)
    ptr = [None if t is None else t.data_ptr() for t in (yy, gy, gx, gw, gb)]
    _lib.check(lib.s3r_linear_backward(x.data_ptr(), w.data_ptr(), *ptr, B, cin, cout, _lib.ACT[act], scratch.data_ptr(),
                                       scratch.numel(), _stream_ptr(dev)), "linear backward")
    return gx, gw, gb


class _LinearFunction(torch.autograd.Function):
    """`linear` with `linear_backward` as its derivative; saves x, weight and y"""

    @staticmethod
    def forward(ctx, x, weight, bias, act):
        y = linear(x, weight, bias, act)
        ctx.act = act
        ctx.save_for_backward(x, weight, y)
        return y

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_y):
        x, weight, y = ctx.saved_tensors
        need_x, need_w, need_b = ctx.needs_input_grad[:3]
        if not (need_x or need_w or need_b):
            return None, None, None, None
        gx, gw, gb = linear_backward(x, weight, y, grad_y.contiguous().float(), ctx.act, need_x, need_w, need_b)
        return gx, gw, gb, None


def differentiable_linear(x: torch.Tensor, weight: torch.Tensor, bias: Optional[torch.Tensor], act: str = "none") -> torch.Tensor:
    """`linear` recorded for autograd: the same bits, with the deterministic backward `linear_backward`, called with exactly the
    sides autograd needs (`needs_input_grad`).  A B = 0 input gives zero gradients without a kernel call."""
    return _LinearFunction.apply(x, weight, bias, act)


@torch.no_grad()
def chamfer_distance(p: torch.Tensor, q: torch.Tensor):
    """(dist1 (B,N), dist2 (B,M), idx1 (B,N) int32, idx2 (B,M) int32): squared-L2 nearest neighbours (`s3r_chamfer_forward`).
    The distance is ((dx*dx + dy*dy) + dz*dz) in fp32, each operation rounded once.  idx is the FIRST minimum: the lowest index
    holding the smallest distance, as one sequential scan with a strict `<` finds it.  Minima are taken over the distances that are
    not NaN (IEEE minNum); a query with no candidate below +inf gets dist = +inf, idx = 0.  Inputs are expected finite: a
    non-finite point has the distance +inf itself, so it shows up as a non-finite loss and never hides behind a finite one."""
    if p.dim() != 3 or q.dim() != 3 or p.shape[-1] != 3 or q.shape[-1] != 3 or p.shape[0] != q.shape[0]:
        raise RuntimeError(f"chamfer_distance expects (B,N,3) and (B,M,3), got {tuple(p.shape)} and {tuple(q.shape)}")
    p = _check_input(p, "p", p.shape[1:])
    q = _check_input(q, "q", q.shape[1:])
    B, N, M = p.shape[0], p.shape[1], q.shape[1]
    if N == 0 or M == 0:
        raise RuntimeError("chamfer_distance needs non-empty point clouds")
    d1 = torch.empty((B, N), dtype=torch.float32, device=p.device)
    d2 = torch.empty((B, M), dtype=torch.float32, device=p.device)
    i1 = torch.empty((B, N), dtype=torch.int32, device=p.device)
    i2 = torch.empty((B, M), dtype=torch.int32, device=p.device)
    if B:
        _lib.check(_lib.load().s3r_chamfer_forward(p.data_ptr(), q.data_ptr(), d1.data_ptr(), d2.data_ptr(),
                                                   i1.data_ptr(), i2.data_ptr(), B, N, M, _stream_ptr(p.device)),
                   "chamfer")
    return d1, d2, i1, i2


@torch.no_grad()
def chamfer_distance_backward(p: torch.Tensor, q: torch.Tensor, idx1: torch.Tensor, idx2: torch.Tensor, grad_dist1, grad_dist2,
                              need_p: bool = True, need_q: bool = True):
    """(grad_p (B,N,3) or None, grad_q (B,M,3) or None) of sum(grad_dist1 * dist1) + sum(grad_dist2 * dist2), the indices of
    `chamfer_distance` held fixed (`s3r_chamfer_backward`): a gather with a fixed summation order — own term first, then the
    scattered terms in ascending source index, fp32, no fused multiply-adds, no atomics — so the bits do not depend on the run or on
    the batch split.  grad_dist1 / grad_dist2: (B,N) / (B,M) fp32, or None for zeros (not both); need_p / need_q: the sides to compute."""
    if p.dim() != 3 or q.dim() != 3 or p.shape[-1] != 3 or q.shape[-1] != 3 or p.shape[0] != q.shape[0]:
        raise RuntimeError(f"chamfer_distance_backward expects (B,N,3) and (B,M,3), got {tuple(p.shape)} and {tuple(q.shape)}")
    p = _check_input(p, "p", p.shape[1:])
    q = _check_input(q, "q", q.shape[1:])
    B, N, M = p.shape[0], p.shape[1], q.shape[1]
    if N == 0 or M == 0:
        raise RuntimeError("chamfer_distance_backward needs non-empty point clouds")
    if grad_dist1 is None and grad_dist2 is None:
        raise RuntimeError("chamfer_distance_backward needs grad_dist1 or grad_dist2")
    if not (need_p or need_q):
        raise RuntimeError("chamfer_distance_backward needs need_p or need_q")
    idx1 = _check_input(idx1, "idx1", (N,), torch.int32)
    idx2 = _check_input(idx2, "idx2", (M,), torch.int32)
    g1 = None if grad_dist1 is None else _check_input(grad_dist1, "grad_dist1", (N,))
    g2 = None if grad_dist2 is None else _check_input(grad_dist2, "grad_dist2", (M,))
    for t, name in ((idx1, "idx1"), (idx2, "idx2"), (g1, "grad_dist1"), (g2, "grad_dist2")):
        if t is not None and t.shape[0] != B:
            raise RuntimeError(f"{name} must have batch {B}, got {tuple(t.shape)}")
    gp = torch.empty((B, N, 3), dtype=torch.float32, device=p.device) if need_p else None
    gq = torch.empty((B, M, 3), dtype=torch.float32, device=p.device) if need_q else None
    if B:
        ptr = [None if t is None else t.data_ptr() for t in (g1, g2, gp, gq)]
        _lib.check(_lib.load().s3r_chamfer_backward(p.data_ptr(), q.data_ptr(), idx1.data_ptr(), idx2.data_ptr(), *ptr, B, N, M,
                                                    _stream_ptr(p.device)), "chamfer backward")
    return gp, gq


class _ChamferFunction(torch.autograd.Function):
    """`chamfer_distance` with `chamfer_distance_backward` as its derivative (the indices are constants of the graph)"""

    @staticmethod
    def forward(ctx, p, q):
        d1, d2, i1, i2 = chamfer_distance(p, q)
        ctx.mark_non_differentiable(i1, i2)
        ctx.set_materialize_grads(False)                           # an unused dist1 / dist2 arrives as None: NULL, not a zero tensor
        ctx.save_for_backward(p, q, i1, i2)
        return d1, d2, i1, i2

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g1, g2, _gi1, _gi2):
        p, q, i1, i2 = ctx.saved_tensors
        need_p, need_q = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        if (g1 is None and g2 is None) or not (need_p or need_q):
            return None, None
        g1 = None if g1 is None else g1.contiguous().float()
        g2 = None if g2 is None else g2.contiguous().float()
        return chamfer_distance_backward(p, q, i1, i2, g1, g2, need_p, need_q)


def differentiable_chamfer_distance(p: torch.Tensor, q: torch.Tensor):
    """`chamfer_distance` recorded for autograd: (dist1, dist2, idx1, idx2), the same bits; dist1 / dist2 carry the deterministic
    backward `chamfer_distance_backward`, idx1 / idx2 are non-differentiable."""
    return _ChamferFunction.apply(p, q)


class ChamferDistance(nn.Module):
    """Drop-in for the reference's extensions/chamfer_dist module (README.md:64-65): forward(p, q)
    returns mean(dist1) + mean(dist2).  (Whether the reference reduces with mean or sum, squared or
    not, is unknown — SURVEY.md §8a row 5; `chamfer_distance` exposes the unreduced tensors.)
    A loss as well as a metric: with grad mode on and p or q requiring grad the value (the same bits) is recorded for autograd
    through `differentiable_chamfer_distance`; otherwise nothing is recorded."""

    def forward(self, p, q):
        if torch.is_grad_enabled() and (p.requires_grad or q.requires_grad):
            d1, d2, _, _ = differentiable_chamfer_distance(p, q)
        else:
            d1, d2, _, _ = chamfer_distance(p, q)
        return d1.mean() + d2.mean()


def _check_bce(pred, target, who):
    if not isinstance(pred, torch.Tensor) or not isinstance(target, torch.Tensor):
        raise TypeError(f"{who}: pred and target must be torch.Tensors")
    if pred.dim() < 2 or pred.shape != target.shape:
        raise RuntimeError(f"{who} expects pred and target of one shape (B, ...), got {tuple(pred.shape)} and {tuple(target.shape)}")
    p = _check_input(pred.detach(), "pred", pred.shape[1:])
    t = _check_input(target.detach(), "target", target.shape[1:])
    voxels = 1
    for n in pred.shape[1:]:
        voxels *= n
    if voxels == 0:
        raise RuntimeError(f"{who} needs non-empty samples")
    return p, t, pred.shape[0], voxels


@torch.no_grad()
def voxel_bce(pred: torch.Tensor, target: torch.Tensor, elements: bool = False):
    """(loss_sum (B), loss_elem or None) of torch.nn.BCELoss's per-element rule on pred, target (B, ...) (`s3r_voxel_bce_forward`):
    l = -(t * clamp(log p) + (1 - t) * clamp(log(1 - p))), the logs clamped at -100 before the multiplication; loss_sum[b] is the fp32
    sum of sample b's losses in a fixed order that depends on the sample size only (include/s3r.h), so it has the same bits in every
    batch split; loss_elem (the shape of pred) is returned with `elements=True`.  A NaN or out-of-range pred makes that sample's sum
    NaN (torch raises instead).  Records no graph (`differentiable_voxel_bce` does)."""
    p, t, B, V = _check_bce(pred, target, "voxel_bce")
    s = torch.empty((B,), dtype=torch.float32, device=p.device)
    e = torch.empty(p.shape, dtype=torch.float32, device=p.device) if elements else None
    if B:
        _lib.check(_lib.load().s3r_voxel_bce_forward(p.data_ptr(), t.data_ptr(), s.data_ptr(), None if e is None else e.data_ptr(), B, V,
                                                     _stream_ptr(p.device)), "voxel_bce")
    return s, e


@torch.no_grad()
def voxel_bce_backward(pred: torch.Tensor, target: torch.Tensor, grad_scale: torch.Tensor) -> torch.Tensor:
    """grad_pred (the shape of pred) of sum_b grad_scale[b] * loss_sum[b] (`s3r_voxel_bce_backward`): grad_scale[b] * (p - t) /
    max((1 - p) * p, 1e-12), each operation rounded once — torch's binary_cross_entropy_backward, elementwise and bit for bit."""
    p, t, B, V = _check_bce(pred, target, "voxel_bce_backward")
    gs = _check_input(grad_scale, "grad_scale", ())
    if gs.shape[0] != B:
        raise RuntimeError(f"grad_scale must have shape ({B},), got {tuple(gs.shape)}")
    g = torch.empty(p.shape, dtype=torch.float32, device=p.device)
    if B:
        _lib.check(_lib.load().s3r_voxel_bce_backward(p.data_ptr(), t.data_ptr(), gs.data_ptr(), g.data_ptr(), B, V, _stream_ptr(p.device)),
                   "voxel_bce backward")
    return g


class _VoxelBCEFunction(torch.autograd.Function):
    """`voxel_bce`'s loss_sum with `voxel_bce_backward` as its derivative; the gradient goes to pred only"""

    @staticmethod
    def forward(ctx, pred, target):
        s, _ = voxel_bce(pred, target)
        ctx.save_for_backward(pred, target)
        return s

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_sum):
        pred, target = ctx.saved_tensors
        if not ctx.needs_input_grad[0]:
            return None, None
        return voxel_bce_backward(pred, target, grad_sum.contiguous().float()), None


def differentiable_voxel_bce(pred: torch.Tensor, target: torch.Tensor) -> torch.Tensor:
    """`voxel_bce`'s loss_sum (B) recorded for autograd: the same bits, with the elementwise backward `voxel_bce_backward`.  The
    gradient goes to pred only (a target is a constant of the loss)."""
    return _VoxelBCEFunction.apply(pred, target)


class VoxelBCELoss(nn.Module):
    """torch.nn.BCELoss (mean reduction) on occupancy grids: forward(pred, target) with pred, target (B,32,32,32) or any (B, ...)
    returns the mean over all elements, `loss_sum.double().sum() / (B V)` cast to fp32 — the per-sample sums are the HIP kernel's,
    in its fixed order.  With grad mode on and pred requiring grad the value (the same bits) is recorded for autograd through
    `differentiable_voxel_bce`; otherwise nothing is recorded (as `ChamferDistance`)."""

    def forward(self, pred, target):
        if torch.is_grad_enabled() and pred.requires_grad:
            s = differentiable_voxel_bce(pred, target)
        else:
            s, _ = voxel_bce(pred, target)
        return (s.double().sum() / max(pred.numel(), 1)).float()


def _check_head(x, weight, act, who):
    if act not in _LINEAR_ACTS:
        raise RuntimeError(f"{who}: act must be one of {_LINEAR_ACTS}, got {act!r}")
    if not isinstance(x, torch.Tensor) or x.dim() < 3:
        raise RuntimeError(f"{who} expects x (B, C, ...), got {tuple(getattr(x, 'shape', ()))}")
    if weight.numel() != x.shape[1]:
        raise RuntimeError(f"{who} expects a weight of {x.shape[1]} elements (Conv(C -> 1, k = 1)), got {tuple(weight.shape)}")
    x = _check_input(x.detach(), "x", x.shape[1:])
    w = weight.detach()
    if w.device != x.device or w.dtype != torch.float32 or not w.is_contiguous():
        raise RuntimeError(f"{who}: weight must be a contiguous fp32 tensor on {x.device}")
    positions = 1
    for n in x.shape[2:]:
        positions *= n
    if x.shape[1] == 0 or positions == 0:
        raise RuntimeError(f"{who} needs non-empty channels and positions")
    return x, w.view(-1), positions


def _check_head_bias(bias, device, who):
    if bias is None:
        return None
    b = bias.detach()
    if b.numel() != 1 or b.device != device or b.dtype != torch.float32:
        raise RuntimeError(f"{who}: bias must be one fp32 element on {device}")
    return b.reshape(1)


@torch.no_grad()
def head(x: torch.Tensor, weight: torch.Tensor, bias: Optional[torch.Tensor], act: str = "sigmoid") -> torch.Tensor:
    """The pointwise head act(sum_c x[:, c] weight[c] + bias) as `s3r_conv_forward` runs a Conv(C -> 1, k = 1) layer ALONE: x
    (B,C,n,n) or (B,C,n,n,n) with one edge n, weight any shape of C elements (an nn.Conv's (1,C,1,1,1)), bias one element or None;
    act "none", "relu" or "sigmoid".  Returns (B,n,n[,n]).  Records no graph (`differentiable_head` does)."""
    x, w, _ = _check_head(x, weight, act, "head")
    b = _check_head_bias(bias, x.device, "head")
    nd = x.dim() - 2
    n = x.shape[2]
    if nd not in (2, 3) or any(e != n for e in x.shape[2:]):
        raise RuntimeError(f"head expects x (B,C,n,n) or (B,C,n,n,n) with one edge n, got {tuple(x.shape)}")
    B, cin = x.shape[0], x.shape[1]
    y = torch.empty((B,) + tuple(x.shape[2:]), dtype=torch.float32, device=x.device)
    if B == 0:
        return y
    lib = _lib.load()
    desc = _lib.ConvDesc(_lib.OP_CONV, nd, B, cin, 1, n, 1, 1, 0, _lib.ACT[act], 0, -1, 0, 0, 0, 0, 0, 0, 0, 1, 0, 0.0)
    stream = _stream_ptr(x.device)
    elems = C.c_int64(0)
    _lib.check(lib.s3r_conv_packed_elems(C.byref(desc), C.byref(elems)), "head: packed_elems")
    pw = torch.empty(elems.value, dtype=torch.float32, device=x.device)
    _lib.check(lib.s3r_conv_pack_weights(C.byref(desc), w.data_ptr(), pw.data_ptr(), stream), "head: pack_weights")
    need = _lib.check(lib.s3r_conv_scratch_elems(C.byref(desc)), "head: scratch query")
    scratch = torch.empty(max(need, 1), dtype=torch.float32, device=x.device)
    _lib.check(lib.s3r_conv_forward(C.byref(desc), x.data_ptr(), pw.data_ptr(), None, None if b is None else b.data_ptr(), y.data_ptr(),
                                    scratch.data_ptr(), scratch.numel(), stream), "head")
    return y


@torch.no_grad()
def head_backward(x: torch.Tensor, weight: torch.Tensor, y: Optional[torch.Tensor], grad_y: torch.Tensor, act: str,
                  need_x: bool = True, need_w: bool = True, need_b: bool = True, scale: Optional[torch.Tensor] = None):
    """(grad_x (the shape of x), grad_w (C), grad_bias (1)) of y = act((sum_c x[:, c] weight[c]) * scale + bias) for the output
    gradient grad_y (B, ...), `None` for the sides not asked for (`s3r_head_backward`).  x (B,C,...) with any positions per sample, y
    the layer's output (it may be None when act is "none"), scale one frozen fp32 element or None for 1.  One streaming pass, fixed
    summation orders, no atomics: the same bits on every run.  Without need_x grad_x is not written, without need_w x is not read."""
    x, w, S = _check_head(x, weight, act, "head_backward")
    if not (need_x or need_w or need_b):
        raise RuntimeError("head_backward needs need_x, need_w or need_b")
    B, cin, dev = x.shape[0], x.shape[1], x.device

    def flat(t, name):
        t = _check_input(t, name, t.shape[1:])
        if t.shape[0] != B or t.numel() != B * S:
            raise RuntimeError(f"{name} must hold (B, positions) = ({B}, {S}) elements, got {tuple(t.shape)}")
        return t

    gy = flat(grad_y, "grad_y")
    yy = None
    if act != "none":
        if y is None:
            raise RuntimeError(f"head_backward: act {act!r} needs the layer's output y")
        yy = flat(y, "y")
    sc = _check_head_bias(scale, dev, "head_backward (scale)")
    gx = torch.empty(x.shape, dtype=torch.float32, device=dev) if need_x else None
    gw = torch.empty((cin,), dtype=torch.float32, device=dev) if need_w else None
    gb = torch.empty((1,), dtype=torch.float32, device=dev) if need_b else None
    if B == 0:                                     # an empty sum
        for t in (gw, gb):
            if t is not None:
                t.zero_()
        return gx, gw, gb
    lib = _lib.load()
    need = _lib.check(lib.s3r_head_backward_scratch_elems(B, cin, S), "head backward scratch query")
    scratch = torch.empty(max(need, 1), dtype=torch.float32, device=dev)
    ptr = [None if t is None else t.data_ptr() for t in (sc, yy, gy, gx, gw, gb)]
    _lib.check(lib.s3r_head_backward(x.data_ptr(), w.data_ptr(), *ptr, B, cin, S, _lib.ACT[act], scratch.data_ptr(), scratch.numel(),
                                     _stream_ptr(dev)), "head backward")
    return gx, gw, gb


class _HeadFunction(torch.autograd.Function):
    """`head` with `head_backward` as its derivative; saves x, weight and y"""

    @staticmethod
    def forward(ctx, x, weight, bias, act):
        y = head(x, weight, bias, act)
        ctx.act = act
        ctx.save_for_backward(x, weight, y)
        return y

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_y):
        x, weight, y = ctx.saved_tensors
        need_x, need_w, need_b = ctx.needs_input_grad[:3]
        if not (need_x or need_w or need_b):
            return None, None, None, None
        gx, gw, gb = head_backward(x, weight, y, grad_y.contiguous().float(), ctx.act, need_x, need_w, need_b)
        return gx, None if gw is None else gw.view(weight.shape), gb, None


def differentiable_head(x: torch.Tensor, weight: torch.Tensor, bias: Optional[torch.Tensor], act: str = "sigmoid") -> torch.Tensor:
    """`head` recorded for autograd: the same bits (the value of `s3r_conv_forward` on the head layer alone), with the deterministic
    backward `head_backward`, called with exactly the sides autograd needs (`needs_input_grad`); gradients come back in the
    parameters' own shapes.  A B = 0 input gives zero gradients without a kernel call."""
    return _HeadFunction.apply(x, weight, bias, act)


# ---------------------------------------------------------------------------------------------------------------------------------
# One convolution layer under autograd: the forward as a one-layer chain, the backward as s3r_conv_backward + the adjoint layer's forward
_CONV_OPS = ("conv2d", "conv3d", "deconv2d", "deconv3d")
_PACKED_FOR = collections.OrderedDict()      # (id(weight), device, descriptor) -> (weakref to the weight, version, packed image)
_PACKED_MAX = 32


def _packed_for(weight: torch.Tensor, desc) -> torch.Tensor:
    """`weight` (torch layout) packed for `desc`: ONE image per (weight object, layer), valid for the `_version` it was packed at — what
    `_HipChain._ensure_packed` keys on too.  An in-place update of the parameter (an optimizer step) bumps `_version`, and the new image
    REPLACES the old one.  The weak reference tells a live tensor from another one that got a dead one's `id` (an address is no
    identity either: the allocator hands a freed block to the next tensor of the same size)."""
    sig = tuple(getattr(desc, n) for n in ("op", "ndim", "cin", "cout", "in_size", "k", "stride", "pad", "out_pad", "dtype", "algo"))
    key = (id(weight), str(weight.device), sig)
    hit = _PACKED_FOR.get(key)
    if hit is not None and hit[0]() is weight and hit[1] == weight._version:
        _PACKED_FOR.move_to_end(key)
        return hit[2]
    lib = _lib.load()
    one = _lib.ConvDesc.from_buffer_copy(desc)
    one.batch = 1
    n = C.c_int64(0)
    _lib.check(lib.s3r_conv_packed_elems(C.byref(one), C.byref(n)), "packed_elems")
    w = weight.detach().float().contiguous()
    pw = torch.empty(n.value, dtype=torch.float32, device=w.device)
    _lib.check(lib.s3r_conv_pack_weights(C.byref(one), w.data_ptr(), pw.data_ptr(), _stream_ptr(w.device)), "pack_weights")
    _PACKED_FOR[key] = (weakref.ref(weight), weight._version, pw)
    _PACKED_FOR.move_to_end(key)
    for k in [k for k, v in _PACKED_FOR.items() if v[0]() is None]:      # images of tensors that are gone
        del _PACKED_FOR[k]
    while len(_PACKED_FOR) > _PACKED_MAX:
        _PACKED_FOR.popitem(last=False)
    return pw


def _run_one_layer(desc, x: torch.Tensor, pw: torch.Tensor, scale, shift, y: torch.Tensor) -> torch.Tensor:
    """One layer through `s3r_chain_forward`: `s3r_conv_forward` behind the halo-padded copy of an unpadded input that the layer's
    kernel may read its zero padding from (the chain plans that copy itself; a single `s3r_conv_forward` call refuses such a layer)."""
    lib = _lib.load()
    arr = (_lib.Layer * 1)()
    arr[0].desc = desc
    arr[0].packed_w = pw.data_ptr()
    arr[0].scale = scale.data_ptr() if scale is not None else None
    arr[0].shift = shift.data_ptr() if shift is not None else None
    need = _lib.check(lib.s3r_chain_workspace_elems(arr, 1), "workspace query")
    ws = torch.empty(max(need, 1), dtype=torch.float32, device=x.device)
    _lib.check(lib.s3r_chain_forward(arr, 1, x.data_ptr(), y.data_ptr(), ws.data_ptr(), ws.numel(), 1, _stream_ptr(x.device)),
               "one-layer chain")
    return y


def _check_conv(x, weight, layer, who):
    if layer.op not in _CONV_OPS:
        raise RuntimeError(f"{who} takes a conv2d / conv3d / deconv2d / deconv3d layer, got {layer.op!r}")
    if layer.act not in _LINEAR_ACTS:
        raise RuntimeError(f"{who}: act must be one of {_LINEAR_ACTS}, got {layer.act!r}")
    if layer.dil != 1:
        raise RuntimeError(f"{who}: dilation 1 only")
    nd = spec.ndim(layer)
    if not isinstance(x, torch.Tensor) or x.dim() != nd + 2 or x.shape[1] != layer.cin or any(e != x.shape[2] for e in x.shape[2:]):
        raise RuntimeError(f"{who} expects x (B, {layer.cin}, n{', n' * (nd - 1)}) with one edge n, got {tuple(getattr(x, 'shape', ()))}")
    x = _check_input(x.detach(), "x", x.shape[1:])
    want = ((layer.cin, layer.cout) if layer.op.startswith("deconv") else (layer.cout, layer.cin)) + (layer.k,) * nd
    w = weight.detach()
    if tuple(w.shape) != want or w.device != x.device or w.dtype != torch.float32 or not w.is_contiguous():
        raise RuntimeError(f"{who}: weight must be a contiguous fp32 tensor of shape {want} on {x.device}, got {tuple(w.shape)}")
    n = x.shape[2]
    m = spec.out_size(layer, n)
    if m <= 0:
        raise RuntimeError(f"{who}: the layer has no output over an edge of {n}")
    return x, w, n, (x.shape[0], layer.cout) + (m,) * nd


def _check_channel_vector(v, cout, device, who, name):
    if v is None:
        return None
    v = v.detach()
    if tuple(v.shape) != (cout,) or v.device != device or v.dtype != torch.float32:
        raise RuntimeError(f"{who}: {name} must be a fp32 tensor of shape ({cout},) on {device}")
    return v.contiguous()


@torch.no_grad()
def conv_forward(x: torch.Tensor, weight: torch.Tensor, scale: Optional[torch.Tensor], shift: Optional[torch.Tensor],
                 layer: spec.Layer) -> torch.Tensor:
    """act(conv(x, weight) * scale + shift) of ONE arch_spec layer (conv2d / conv3d / deconv2d / deconv3d, dilation 1, act none /
    relu / sigmoid) under the library's AUTO algorithm, as a one-layer `s3r_chain_forward`.  Records no graph."""
    x, w, n, yshape = _check_conv(x, weight, layer, "conv_forward")
    sc = _check_channel_vector(scale, layer.cout, x.device, "conv_forward", "scale")
    sh = _check_channel_vector(shift, layer.cout, x.device, "conv_forward", "shift")
    y = torch.empty(yshape, dtype=torch.float32, device=x.device)
    if x.shape[0] == 0:
        return y
    desc = _lib.make_desc(layer, x.shape[0], n)
    return _run_one_layer(desc, x, _packed_for(weight, desc), sc, sh, y)


@torch.no_grad()
def conv_backward(x: torch.Tensor, weight: torch.Tensor, y: Optional[torch.Tensor], grad_y: torch.Tensor, layer: spec.Layer,
                  scale: Optional[torch.Tensor] = None, need_x: bool = True, need_w: bool = True, need_shift: bool = True):
    """(grad_x, grad_w, grad_shift) of y = act(conv(x, weight) * scale + shift) for the output gradient grad_y, `None` for the sides not
    asked for.  ONE `s3r_conv_backward` call (gs = g * scale, grad_w in the weight's torch shape, grad_shift (cout): fixed summation
    orders, no atomics, the same bits on every run and for every batch a sample appears in) and then, when need_x, the forward of the
    adjoint layer (`s3r_conv_adjoint_desc`) on gs with this layer's own weight tensor, packed once per weight tensor and `_version`.  y may
    be None when the layer's act is "none"; scale (cout) is frozen: it gets no gradient."""
    x, w, n, yshape = _check_conv(x, weight, layer, "conv_backward")
    if not (need_x or need_w or need_shift):
        raise RuntimeError("conv_backward needs need_x, need_w or need_shift")
    B, dev = x.shape[0], x.device
    gy = _check_input(grad_y, "grad_y", yshape[1:])
    if gy.shape[0] != B:
        raise RuntimeError(f"grad_y must hold {B} samples, got {gy.shape[0]}")
    yy = None
    if layer.act != "none":
        if y is None:
            raise RuntimeError(f"conv_backward: act {layer.act!r} needs the layer's output y")
        yy = _check_input(y.detach(), "y", yshape[1:])
        if yy.shape[0] != B:
            raise RuntimeError(f"y must hold {B} samples, got {yy.shape[0]}")
    sc = _check_channel_vector(scale, layer.cout, dev, "conv_backward", "scale")
    gx = torch.empty(x.shape, dtype=torch.float32, device=dev) if need_x else None
    gs = torch.empty(yshape, dtype=torch.float32, device=dev) if need_x else None
    gw = torch.empty(w.shape, dtype=torch.float32, device=dev) if need_w else None
    gb = torch.empty((layer.cout,), dtype=torch.float32, device=dev) if need_shift else None
    if B == 0:                                     # an empty sum
        for t in (gw, gb):
            if t is not None:
                t.zero_()
        return gx, gw, gb
    lib = _lib.load()
    desc = _lib.make_desc(layer, B, n)
    need = _lib.check(lib.s3r_conv_backward_scratch_elems(C.byref(desc)), "conv backward scratch query")
    scratch = torch.empty(max(need, 1), dtype=torch.float32, device=dev)
    ptr = [None if t is None else t.data_ptr() for t in (x if need_w else None, yy, gy, sc, gs, gw, gb)]
    _lib.check(lib.s3r_conv_backward(C.byref(desc), *ptr, scratch.data_ptr(), scratch.numel(), _stream_ptr(dev)), "conv backward")
    if need_x:
        adj = _lib.ConvDesc()
        _lib.check(lib.s3r_conv_adjoint_desc(C.byref(desc), C.byref(adj)), "conv adjoint descriptor")
        _run_one_layer(adj, gs, _packed_for(weight, adj), None, None, gx)
    return gx, gw, gb


class _ConvFunction(torch.autograd.Function):
    """`conv_forward` with `conv_backward` as its derivative; saves x, weight, scale and y"""

    @staticmethod
    def forward(ctx, x, weight, scale, shift, layer):
        y = conv_forward(x, weight, scale, shift, layer)
        ctx.layer = layer
        ctx.has_scale = scale is not None
        ctx.save_for_backward(x, weight, y, *((scale,) if scale is not None else ()))
        return y

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_y):
        x, weight, y = ctx.saved_tensors[:3]
        scale = ctx.saved_tensors[3] if ctx.has_scale else None
        need_x, need_w, need_shift = ctx.needs_input_grad[0], ctx.needs_input_grad[1], ctx.needs_input_grad[3]
        if not (need_x or need_w or need_shift):
            return None, None, None, None, None
        gx, gw, gb = conv_backward(x, weight, y, grad_y.contiguous().float(), ctx.layer, scale, need_x, need_w, need_shift)
        return gx, gw, None, gb, None


def differentiable_conv(x: torch.Tensor, weight: torch.Tensor, scale: Optional[torch.Tensor], shift: Optional[torch.Tensor],
                        layer: spec.Layer) -> torch.Tensor:
    """`conv_forward` recorded for autograd: the value of the layer's kernel under the AUTO algorithm, with the deterministic backward
    `conv_backward`, called with exactly the sides autograd needs (`needs_input_grad` of x, weight and shift).  `scale` is frozen: its
    gradient is `None` (a folded BatchNorm scale: `bn.weight` is not trained through this path)."""
    return _ConvFunction.apply(x, weight, scale, shift, layer)


# ---------------------------------------------------------------------------------------------------------------------------------
# The stem's backward: s3r_stem_backward
def _check_stem_render(x, name):
    if not isinstance(x, torch.Tensor) or x.dim() != 4 or x.shape[1] != 3 or x.shape[2] != x.shape[3] or x.shape[2] < 1:
        raise RuntimeError(f"{name} must be renders (N, 3, n, n), got {tuple(getattr(x, 'shape', ()))}")
    dt = torch.uint8 if x.dtype == torch.uint8 else torch.float32
    return _aligned16(_check_input(x.detach(), name, x.shape[1:], dt))


@torch.no_grad()
def stem_backward(left: torch.Tensor, right: Optional[torch.Tensor], y: Optional[torch.Tensor], grad_y: torch.Tensor,
                  scale: Optional[torch.Tensor] = None, act: str = "relu", need_w: bool = True, need_shift: bool = True):
    """(grad_w, grad_shift) of the stem y = act(conv2d(X, w; 3 -> 32, k 3, s 2, p 1) * scale + shift) for the output gradient grad_y
    (N,32,m,m), `None` for the side not asked for: ONE `s3r_stem_backward` call.  X are the renders as the forward reads them, float32
    or uint8 (scaled by 1/255 as they are read), `left` then `right` (None: one tensor) — no conversion, no concatenation.  Fixed
    summation orders, no atomics: the same bits for one tensor or two, for uint8 renders and their host conversion, and grad_w of a batch
    is the ascending sum of its images' results.  y may be None when act is "none"; scale (32) is frozen."""
    if act not in ("none", "relu"):
        raise RuntimeError(f"stem_backward: act must be 'none' or 'relu', got {act!r}")
    if not (need_w or need_shift):
        raise RuntimeError("stem_backward needs need_w or need_shift")
    left = _check_stem_render(left, "left")
    n, dev = left.shape[2], left.device
    if right is not None:
        right = _check_stem_render(right, "right")
        if tuple(right.shape[1:]) != tuple(left.shape[1:]) or right.dtype != left.dtype or right.device != dev:
            raise RuntimeError("left and right renders must share one edge, dtype and device")
        if right.shape[0] == 0:
            right = None
        elif left.shape[0] == 0:
            left, right = right, None
    N = left.shape[0] + (right.shape[0] if right is not None else 0)
    m = (n - 1) // 2 + 1
    gy = _check_input(grad_y, "grad_y", (32, m, m))
    if gy.shape[0] != N:
        raise RuntimeError(f"grad_y must hold {N} images, got {gy.shape[0]}")
    yy = None
    if act != "none":
        if y is None:
            raise RuntimeError(f"stem_backward: act {act!r} needs the layer's output y")
        yy = _check_input(y.detach(), "y", (32, m, m))
        if yy.shape[0] != N:
            raise RuntimeError(f"y must hold {N} images, got {yy.shape[0]}")
    sc = _check_channel_vector(scale, 32, dev, "stem_backward", "scale")
    gw = torch.empty((32, 3, 3, 3), dtype=torch.float32, device=dev) if need_w else None
    gb = torch.empty((32,), dtype=torch.float32, device=dev) if need_shift else None
    if N == 0:                                     # an empty sum
        for t in (gw, gb):
            if t is not None:
                t.zero_()
        return gw, gb
    lib = _lib.load()
    need = _lib.check(lib.s3r_stem_backward_scratch_elems(N, n), "stem backward scratch query")
    scratch = torch.empty(max(need, 1), dtype=torch.float32, device=dev)
    ptr = [None if t is None else t.data_ptr() for t in (yy, gy, sc, gw, gb)]
    _lib.check(lib.s3r_stem_backward(left.data_ptr(), right.data_ptr() if right is not None else None, left.shape[0],
                                     int(left.dtype == torch.uint8), *ptr, N, n, _lib.ACT[act], scratch.data_ptr(), scratch.numel(),
                                     _stream_ptr(dev)), "stem backward")
    return gw, gb


class _StemFunction(torch.autograd.Function):
    """The encoder's first block with `stem_backward` as its derivative with respect to (weight, shift); the renders get no gradient.
    act "relu": the stem kernel itself on the renders as given — the one-layer chain `encoder._run(left, "e1", 0, right)`, which reads the
    encoder's own e1 parameters (`weight`, `shift` and `scale` ARE those, handed in so that autograd sees them).  act "none" (the
    batch-statistics form; scale None, shift = conv.bias): the stem kernel has no form without its activation, so the forward is
    `conv_forward` on the fp32 conversion of the concatenated renders; the backward reads the renders as given either way."""

    @staticmethod
    def forward(ctx, weight, shift, scale, encoder, left, right, act):
        if act == "none":
            x = left if right is None else torch.cat([left, right], 0)
            if x.dtype == torch.uint8:                             # IEEE division by a device tensor: the kernels' correctly rounded u / 255
                x = x.float() / torch.full((), 255.0, device=x.device)     # (a Python-scalar divisor may be turned into a reciprocal)
            y = conv_forward(x, weight, None, shift, dataclasses.replace(encoder._layers[0], act="none"))
        else:
            y = encoder._run(left, encoder.names[0], 0, right)
        ctx.act, ctx.has_scale, ctx.has_right = act, scale is not None, right is not None
        ctx.save_for_backward(left, y, *((right,) if right is not None else ()), *((scale,) if scale is not None else ()))
        return y

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_y):
        saved = list(ctx.saved_tensors)
        left, y = saved[0], saved[1]
        right = saved[2] if ctx.has_right else None
        scale = saved[-1] if ctx.has_scale else None
        need_w, need_shift = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        if not (need_w or need_shift):
            return (None,) * 7
        gw, gb = stem_backward(left, right, y if ctx.act != "none" else None, grad_y.contiguous().float(), scale, ctx.act, need_w,
                               need_shift)
        return gw, gb, None, None, None, None, None


# ---------------------------------------------------------------------------------------------------------------------------------
# Train-mode BatchNorm (batch statistics) + activation: s3r_batchnorm_train_forward / _backward
def _check_bn(z, who):
    if not isinstance(z, torch.Tensor) or z.dim() < 2:
        raise RuntimeError(f"{who} expects z (B, C, ...), got {tuple(getattr(z, 'shape', ()))}")
    z = _check_input(z.detach(), "z", z.shape[1:])
    S = 1
    for n in z.shape[2:]:
        S *= n
    if z.shape[1] == 0 or S == 0:
        raise RuntimeError(f"{who} needs non-empty channels and positions")
    if z.shape[0] * S < 2:
        raise RuntimeError(f"{who}: batch statistics need more than one value per channel, got z {tuple(z.shape)}")
    return z, S


@torch.no_grad()
def batchnorm_train_forward(z: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, eps: float, act: str = "none"):
    """(y, mean, var, invstd) of train-mode BatchNorm + activation on z (B,C,...) (`s3r_batchnorm_train_forward`): per channel the batch
    mean and the BIASED variance in two passes, invstd = 1 / sqrt(var + eps), y = act(((z - mean) * invstd) * gamma + beta) with nothing
    fused; gamma, beta (C); act "none", "relu" or "sigmoid".  Fixed summation orders, no atomics: the same bits on every run.  A sample's
    result depends on the batch it is in.  Records no graph (`differentiable_batchnorm` does)."""
    if act not in _LINEAR_ACTS:
        raise RuntimeError(f"batchnorm_train_forward: act must be one of {_LINEAR_ACTS}, got {act!r}")
    z, S = _check_bn(z, "batchnorm_train_forward")
    B, ch, dev = z.shape[0], z.shape[1], z.device
    ga = _check_channel_vector(gamma, ch, dev, "batchnorm_train_forward", "gamma")
    be = _check_channel_vector(beta, ch, dev, "batchnorm_train_forward", "beta")
    y = torch.empty_like(z)
    mean, var, invstd = (torch.empty((ch,), dtype=torch.float32, device=dev) for _ in range(3))
    lib = _lib.load()
    need = _lib.check(lib.s3r_batchnorm_train_forward_scratch_elems(B, ch, S), "batchnorm forward scratch query")
    scratch = torch.empty(max(need, 1), dtype=torch.float32, device=dev)
    _lib.check(lib.s3r_batchnorm_train_forward(z.data_ptr(), ga.data_ptr(), be.data_ptr(), float(eps), _lib.ACT[act], y.data_ptr(),
                                               mean.data_ptr(), var.data_ptr(), invstd.data_ptr(), B, ch, S, scratch.data_ptr(),
                                               scratch.numel(), _stream_ptr(dev)), "batchnorm forward")
    return y, mean, var, invstd


@torch.no_grad()
def batchnorm_train_backward(z: torch.Tensor, y: Optional[torch.Tensor], grad_y: torch.Tensor, gamma: torch.Tensor, mean: torch.Tensor,
                             invstd: torch.Tensor, act: str, need_z: bool = True, need_gamma: bool = True, need_beta: bool = True):
    """(grad_z, grad_gamma, grad_beta) of `batchnorm_train_forward` for the output gradient grad_y (the shape of z), `None` for the sides
    not asked for (`s3r_batchnorm_train_backward`): z, y, mean and invstd are the forward's (y may be None when act is "none").  One pass
    for the two sums, a finish, one pass for grad_z; fixed summation orders, no atomics.  A side that is not asked for is not written."""
    if act not in _LINEAR_ACTS:
        raise RuntimeError(f"batchnorm_train_backward: act must be one of {_LINEAR_ACTS}, got {act!r}")
    if not (need_z or need_gamma or need_beta):
        raise RuntimeError("batchnorm_train_backward needs need_z, need_gamma or need_beta")
    z, S = _check_bn(z, "batchnorm_train_backward")
    B, ch, dev = z.shape[0], z.shape[1], z.device
    gy = _check_input(grad_y, "grad_y", z.shape[1:])
    if gy.shape[0] != B:
        raise RuntimeError(f"grad_y must hold {B} samples, got {gy.shape[0]}")
    yy = None
    if act != "none":
        if y is None:
            raise RuntimeError(f"batchnorm_train_backward: act {act!r} needs the layer's output y")
        yy = _check_input(y.detach(), "y", z.shape[1:])
        if yy.shape[0] != B:
            raise RuntimeError(f"y must hold {B} samples, got {yy.shape[0]}")
    ga, mu, iv = (_check_channel_vector(v, ch, dev, "batchnorm_train_backward", n)
                  for v, n in ((gamma, "gamma"), (mean, "mean"), (invstd, "invstd")))
    gz = torch.empty_like(z) if need_z else None
    gg = torch.empty((ch,), dtype=torch.float32, device=dev) if need_gamma else None
    gb = torch.empty((ch,), dtype=torch.float32, device=dev) if need_beta else None
    lib = _lib.load()
    need = _lib.check(lib.s3r_batchnorm_train_backward_scratch_elems(B, ch, S), "batchnorm backward scratch query")
    scratch = torch.empty(max(need, 1), dtype=torch.float32, device=dev)
    ptr = [None if t is None else t.data_ptr() for t in (gz, gg, gb)]
    _lib.check(lib.s3r_batchnorm_train_backward(z.data_ptr(), None if yy is None else yy.data_ptr(), gy.data_ptr(), ga.data_ptr(),
                                                mu.data_ptr(), iv.data_ptr(), _lib.ACT[act], *ptr, B, ch, S, scratch.data_ptr(),
                                                scratch.numel(), _stream_ptr(dev)), "batchnorm backward")
    return gz, gg, gb


class _BatchNormTrainFunction(torch.autograd.Function):
    """`batchnorm_train_forward` with `batchnorm_train_backward` as its derivative; saves z, gamma, y, mean and invstd.  mean and var
    are returned for the running statistics and carry no gradient."""

    @staticmethod
    def forward(ctx, z, gamma, beta, eps, act):
        y, mean, var, invstd = batchnorm_train_forward(z, gamma, beta, eps, act)
        ctx.act = act
        ctx.save_for_backward(z, gamma, y, mean, invstd)
        ctx.mark_non_differentiable(mean, var)
        return y, mean, var

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_y, _gmean, _gvar):
        z, gamma, y, mean, invstd = ctx.saved_tensors
        need_z, need_gamma, need_beta = ctx.needs_input_grad[:3]
        if not (need_z or need_gamma or need_beta):
            return None, None, None, None, None
        gz, gg, gb = batchnorm_train_backward(z, y, grad_y.contiguous().float(), gamma, mean, invstd, ctx.act, need_z, need_gamma, need_beta)
        return gz, gg, gb, None, None


def differentiable_batchnorm(z: torch.Tensor, bn: nn.Module, act: str = "none") -> torch.Tensor:
    """act(bn(z)) of an affine `nn.BatchNorm2d` / `nn.BatchNorm3d` (any `_BatchNorm`) with BATCH statistics — torch's training mode,
    whatever `bn.training` says — recorded for autograd: `batchnorm_train_forward`'s bits, with the deterministic backward
    `batchnorm_train_backward` called with exactly the sides autograd needs (`needs_input_grad` of z, `bn.weight`, `bn.bias`).  When
    `bn.track_running_stats` is set the running statistics and `num_batches_tracked` are updated as torch updates them: with
    `bn.momentum` (None: the cumulative average 1 / num_batches_tracked) and the UNBIASED variance var * N / (N - 1), in torch operations
    on the (C) vectors under no_grad."""
    if not isinstance(bn, nn.modules.batchnorm._BatchNorm) or bn.weight is None or bn.bias is None:
        raise RuntimeError("differentiable_batchnorm takes an affine nn.BatchNorm1d / 2d / 3d module")
    if not isinstance(z, torch.Tensor) or z.dim() < 2 or z.shape[1] != bn.num_features:
        raise RuntimeError(f"differentiable_batchnorm expects z (B, {bn.num_features}, ...), got {tuple(getattr(z, 'shape', ()))}")
    y, mean, var = _BatchNormTrainFunction.apply(z, bn.weight, bn.bias, float(bn.eps), act)
    if bn.track_running_stats and bn.running_mean is not None:
        with torch.no_grad():
            n = z.numel() // z.shape[1]
            bn.num_batches_tracked += 1
            f = 1.0 / float(bn.num_batches_tracked) if bn.momentum is None else float(bn.momentum)
            bn.running_mean.mul_(1.0 - f).add_(mean, alpha=f)
            bn.running_var.mul_(1.0 - f).add_(var * (n / (n - 1.0)), alpha=f)
    return y


@torch.no_grad()
def cost_volume_backward(grad_volume: torch.Tensor, need_left: bool = True, need_right: bool = True):
    """(grad_left, grad_right), (B,C,H,W) each and `None` for the side not asked for, of the plain cost volume for its output gradient
    grad_volume (B,2C,D,H,W): ONE `s3r_cost_volume_backward` call.  Every element is its own sequential fp32 sum in ascending d (no
    atomics: the same bits on every run and for every batch a sample appears in); the volume's structural zeros are never read."""
    if not (need_left or need_right):
        raise RuntimeError("cost_volume_backward needs need_left or need_right")
    if not isinstance(grad_volume, torch.Tensor) or grad_volume.dim() != 5 or grad_volume.shape[1] % 2 or grad_volume.shape[1] == 0:
        raise RuntimeError(f"cost_volume_backward expects grad_volume (B, 2C, D, H, W), got {tuple(getattr(grad_volume, 'shape', ()))}")
    gv = _check_input(grad_volume.detach(), "grad_volume", grad_volume.shape[1:])
    B, C2, D, H, W = gv.shape
    if min(D, H, W) < 1:
        raise RuntimeError(f"cost_volume_backward: D, H and W must be positive, got {tuple(gv.shape)}")
    gl = torch.empty((B, C2 // 2, H, W), dtype=torch.float32, device=gv.device) if need_left else None
    gr = torch.empty((B, C2 // 2, H, W), dtype=torch.float32, device=gv.device) if need_right else None
    if B == 0:
        return gl, gr
    _lib.check(_lib.load().s3r_cost_volume_backward(gv.data_ptr(), None if gl is None else gl.data_ptr(),
                                                    None if gr is None else gr.data_ptr(), B, C2 // 2, D, H, W,
                                                    _stream_ptr(gv.device)), "cost volume backward")
    return gl, gr


class _CostVolumeFunction(torch.autograd.Function):
    """the plain `s3r_cost_volume_forward` (halo 0) with `cost_volume_backward` as its derivative; saves nothing (the operator is linear)"""

    @staticmethod
    def forward(ctx, feat_left, feat_right, max_disp):
        if feat_left.shape != feat_right.shape or feat_left.dim() != 4:
            raise RuntimeError(f"feature maps must both be (B,C,H,W), got {tuple(feat_left.shape)} and {tuple(feat_right.shape)}")
        fl = _check_input(feat_left.detach(), "feat_left", feat_left.shape[1:])
        fr = _check_input(feat_right.detach(), "feat_right", feat_left.shape[1:])
        B, Cc, H, W = fl.shape
        vol = torch.empty((B, 2 * Cc, int(max_disp), H, W), dtype=torch.float32, device=fl.device)
        if B:
            _lib.check(_lib.load().s3r_cost_volume_forward(fl.data_ptr(), fr.data_ptr(), vol.data_ptr(), B, Cc, int(max_disp), H, W, 0,
                                                           _stream_ptr(fl.device)), "cost_volume")
        return vol

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_volume):
        need_l, need_r = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        if not (need_l or need_r):
            return None, None, None
        gl, gr = cost_volume_backward(grad_volume.contiguous().float(), need_l, need_r)
        return gl, gr, None


def differentiable_cost_volume(feat_left: torch.Tensor, feat_right: torch.Tensor, max_disp: int = spec.MAX_DISP) -> torch.Tensor:
    """The plain fp32 cost volume (B,2C,D,H,W) recorded for autograd: the value has the bits of `CostVolume.forward` (the same kernel call),
    the backward is `cost_volume_backward`, called with exactly the sides autograd needs (`needs_input_grad` of the two maps)."""
    return _CostVolumeFunction.apply(feat_left, feat_right, max_disp)


@torch.no_grad()
def voxel_iou(pred: torch.Tensor, gt: torch.Tensor, threshold: float = 0.5) -> torch.Tensor:
    """Per-sample IoU of (pred > th) vs (gt > th), computed on the device: (B,...) -> (B,) (`s3r_voxel_iou`).  Occupied means
    strictly greater than the threshold ROUNDED TO fp32, compared in fp32 (a voxel holding float32(0.3) is not occupied at 0.3);
    NaN is not occupied.  The counts are exact; the result is float32(intersection) / float32(union), conversions
    round-to-nearest-even, 1 for an empty union."""
    if pred.shape != gt.shape:
        raise RuntimeError("pred and gt shapes differ")
    pred = _check_input(pred, "pred", pred.shape[1:])
    gt = _check_input(gt, "gt", gt.shape[1:])
    B = pred.shape[0]
    out = torch.empty((B,), dtype=torch.float32, device=pred.device)
    if B:
        _lib.check(_lib.load().s3r_voxel_iou(pred.data_ptr(), gt.data_ptr(), float(threshold), out.data_ptr(), B,
                                             pred[0].numel(), _stream_ptr(pred.device)), "voxel_iou")
    return out


@torch.no_grad()
def disparity_wta(feat_l: torch.Tensor, feat_r: torch.Tensor, max_disp: int = spec.MAX_DISP):
    """Predicted left / right disparity maps (ground truth: disp_%02d_{l,r}.exr,
    /root/reference/README.md:75-76): winner-take-all over the shift-and-diff costs the cost volume holds, read
    straight from the two feature maps.  (B,C,H,W) x2 fp32 -> two (B,H,W) fp32 maps, integer-valued, in
    feature-resolution pixels; disp_l[b,h,w] = first argmin_d sum_c |L[b,c,h,w] - R[b,c,h,w-d]|, disp_r mirrored."""
    if feat_l.shape != feat_r.shape or feat_l.dim() != 4:
        raise RuntimeError("feat_l / feat_r must be two (B,C,H,W) tensors of one shape")
    feat_l = _check_input(feat_l.float(), "feat_l", feat_l.shape[1:])
    feat_r = _check_input(feat_r.float(), "feat_r", feat_r.shape[1:])
    B, Cc, H, W = feat_l.shape
    dl = torch.empty((B, H, W), dtype=torch.float32, device=feat_l.device)
    dr = torch.empty_like(dl)
    if B:
        _lib.check(_lib.load().s3r_disparity_wta(feat_l.data_ptr(), feat_r.data_ptr(), dl.data_ptr(), dr.data_ptr(), B,
                                                 Cc, H, W, int(max_disp), _stream_ptr(feat_l.device)), "disparity_wta")
    return dl, dr


@torch.no_grad()
def disparity_soft(feat_l: torch.Tensor, feat_r: torch.Tensor, max_disp: int = spec.MAX_DISP, temperature: float = 1.0,
                   out_size: Optional[Sequence[int]] = None, scale: float = 1.0, confidence: bool = False):
    """Sub-pixel disparity read-out (`s3r_disparity_soft`; a stand-in like `disparity_wta`, not a learned head): per pixel the
    soft-argmin sum_d d p_d, p_d = softmax_d(-c(d) / temperature), over the SAME shift-and-diff costs c(d) the WTA takes the argmin
    of, and the confidence p_best = 1 / sum_d exp((min c - c(d)) / temperature).  Features: fp32 (B,C,H,W), or the bf16 encoder's
    logical (B,C,H,W) channels-last tensors as they are (no conversion pass; same bits as the fp32 call on `channels_last_to_f32`).
    out_size=None: (B,H,W) maps; else (B,*out_size), upsampled bilinearly (torch's align_corners=False).  Disparities are
    multiplied by `scale` (8: render pixels).  Returns (dl, dr), or (dl, dr, cl, cr) with confidence=True.  One kernel launch; torch
    only allocates."""
    if feat_l.dim() != 4 or feat_l.shape != feat_r.shape:
        raise RuntimeError("feat_l / feat_r must be two (B,C,H,W) tensors of one shape")
    if feat_l.dtype != feat_r.dtype or feat_l.dtype not in (torch.float32, torch.bfloat16):
        raise RuntimeError(f"features must both be float32 (NCHW) or bfloat16 (channels-last), got {feat_l.dtype} / {feat_r.dtype}")
    bf16 = feat_l.dtype == torch.bfloat16
    chk = _check_input_cl if bf16 else _check_input
    pl, pr = chk(feat_l, "feat_l", feat_l.shape[1:], feat_l.dtype), chk(feat_r, "feat_r", feat_r.shape[1:], feat_r.dtype)
    # (bf16: the kernel reads rows in 16-byte pieces; _check_input_cl copies a view at an odd storage offset once)
    B, Cc, H, W = feat_l.shape
    OH, OW = (H, W) if out_size is None else (int(out_size[0]), int(out_size[1]))
    dev = feat_l.device
    outs = [torch.empty((B, OH, OW), dtype=torch.float32, device=dev) for _ in range(4 if confidence else 2)]
    if B:
        ptr = [o.data_ptr() for o in outs] + [None] * (4 - len(outs))
        _lib.check(_lib.load().s3r_disparity_soft(pl.data_ptr(), pr.data_ptr(), _lib.DTYPE["bf16" if bf16 else "fp32"], *ptr, B,
                                                  Cc, H, W, int(max_disp), float(temperature), OH, OW, float(scale),
                                                  _stream_ptr(dev)), "disparity_soft")
    return tuple(outs)


def _check_soft_features(feat_l, feat_r, who):
    if not isinstance(feat_l, torch.Tensor) or not isinstance(feat_r, torch.Tensor) or feat_l.dim() != 4 or feat_l.shape != feat_r.shape:
        raise RuntimeError(f"{who}: feat_l / feat_r must be two (B,C,H,W) tensors of one shape")
    if feat_l.dtype != torch.float32 or feat_r.dtype != torch.float32:
        raise RuntimeError(f"{who} reads float32 (NCHW) features only (no bf16 backward exists), got {feat_l.dtype} / {feat_r.dtype}")
    return (_check_input(feat_l.detach(), "feat_l", feat_l.shape[1:]), _check_input(feat_r.detach(), "feat_r", feat_r.shape[1:]))


@torch.no_grad()
def disparity_soft_backward(feat_l: torch.Tensor, feat_r: torch.Tensor, grad_disp_l: Optional[torch.Tensor],
                            grad_disp_r: Optional[torch.Tensor], max_disp: int = spec.MAX_DISP, temperature: float = 1.0,
                            out_size: Optional[Sequence[int]] = None, scale: float = 1.0, need_left: bool = True,
                            need_right: bool = True):
    """(grad_left, grad_right), (B,C,H,W) each and `None` for the side not asked for, of `disparity_soft`'s two disparity maps for their
    gradients grad_disp_l / grad_disp_r (B,*out_size) (either may be None: zeros): ONE `s3r_disparity_soft_backward` call with the
    forward's max_disp, temperature, out_size and scale.  Nothing is saved by the forward: the kernel recomputes the costs and the softmax.
    Every output element is its own sequential fp32 sum in ascending d and the upsample's adjoint is a gather in a fixed order (no
    atomics: the same bits on every run and for every batch a sample appears in).  fp32 features only."""
    if not (need_left or need_right):
        raise RuntimeError("disparity_soft_backward needs need_left or need_right")
    if grad_disp_l is None and grad_disp_r is None:
        raise RuntimeError("disparity_soft_backward needs grad_disp_l or grad_disp_r")
    fl, fr = _check_soft_features(feat_l, feat_r, "disparity_soft_backward")
    B, Cc, H, W = fl.shape
    OH, OW = (H, W) if out_size is None else (int(out_size[0]), int(out_size[1]))
    grads = [None if g is None else _check_input(g.detach(), name, (OH, OW))
             for g, name in ((grad_disp_l, "grad_disp_l"), (grad_disp_r, "grad_disp_r"))]
    if any(g is not None and g.shape[0] != B for g in grads):
        raise RuntimeError(f"disparity_soft_backward: the disparity gradients must be ({B},{OH},{OW})")
    gl = torch.empty(fl.shape, dtype=torch.float32, device=fl.device) if need_left else None
    gr = torch.empty(fl.shape, dtype=torch.float32, device=fl.device) if need_right else None
    if B:
        ptr = [None if t is None else t.data_ptr() for t in grads + [gl, gr]]
        _lib.check(_lib.load().s3r_disparity_soft_backward(fl.data_ptr(), fr.data_ptr(), _lib.DTYPE["fp32"], *ptr, B, Cc, H, W,
                                                           int(max_disp), float(temperature), OH, OW, float(scale),
                                                           _stream_ptr(fl.device)), "disparity_soft backward")
    return gl, gr


class _DisparitySoftFunction(torch.autograd.Function):
    """`disparity_soft`'s two disparity maps with `disparity_soft_backward` as their derivative; saves the two feature maps only"""

    @staticmethod
    def forward(ctx, feat_l, feat_r, max_disp, temperature, size, scale):
        fl, fr = _check_soft_features(feat_l, feat_r, "differentiable_disparity_soft")
        ctx.save_for_backward(feat_l, feat_r)
        ctx.args = (int(max_disp), float(temperature), None if size is None else (int(size[0]), int(size[1])), float(scale))
        dl, dr = disparity_soft(fl, fr, ctx.args[0], ctx.args[1], ctx.args[2], ctx.args[3])
        return dl, dr

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_l, grad_r):
        need_l, need_r = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        if not (need_l or need_r):
            return None, None, None, None, None, None
        feat_l, feat_r = ctx.saved_tensors
        max_disp, tau, size, scale = ctx.args
        gl, gr = disparity_soft_backward(feat_l, feat_r, grad_l.contiguous().float(), grad_r.contiguous().float(), max_disp, tau, size,
                                         scale, need_l, need_r)
        return gl, gr, None, None, None, None


def differentiable_disparity_soft(feat_l: torch.Tensor, feat_r: torch.Tensor, max_disp: int = spec.MAX_DISP, temperature: float = 1.0,
                                  size: Optional[Sequence[int]] = None, scale: float = 1.0):
    """`disparity_soft`'s (disp_l, disp_r) recorded for autograd: the values have the bits of `disparity_soft` (the same kernel call), the
    backward is `disparity_soft_backward`, called with exactly the sides autograd needs (`needs_input_grad` of the two maps).  fp32
    features (B,C,H,W); size=None: (B,H,W) maps, else (B,*size) upsampled bilinearly; disparities are multiplied by `scale`.  The
    confidence maps are not returned (they get no gradient), and the temperature is a constant."""
    return _DisparitySoftFunction.apply(feat_l, feat_r, max_disp, temperature, size, scale)


def _check_disparity_loss(pred, gt, beta, who):
    if not isinstance(pred, torch.Tensor) or not isinstance(gt, torch.Tensor):
        raise TypeError(f"{who}: pred and gt must be torch.Tensors")
    if pred.dim() < 2 or pred.shape != gt.shape:
        raise RuntimeError(f"{who} expects pred and gt of one shape (B, ...), got {tuple(pred.shape)} and {tuple(gt.shape)}")
    beta = float(beta)
    if not (beta >= 0.0) or beta == float("inf"):
        raise ValueError(f"{who}: beta must be finite and >= 0, got {beta}")
    p = _check_input(pred.detach(), "pred", pred.shape[1:])
    t = _check_input(gt.detach(), "gt", gt.shape[1:])
    pixels = 1
    for n in pred.shape[1:]:
        pixels *= n
    if pixels == 0:
        raise RuntimeError(f"{who} needs non-empty samples")
    return p, t, pred.shape[0], pixels, beta


@torch.no_grad()
def disparity_loss(pred: torch.Tensor, gt: torch.Tensor, beta: float = 1.0, elements: bool = False):
    """(loss_sum (B), count (B) int32, loss_elem or None) of the smooth-L1 loss on the pixels whose ground truth is valid (finite and
    >= 0, as `disparity_metrics`) (`s3r_disparity_loss_forward`): with e = pred - gt, l = 0.5 e^2 / beta where |e| < beta, else
    |e| - 0.5 beta (beta = 0: plain L1); an invalid pixel counts as +0.0 and its values never enter arithmetic.  loss_sum[b] is the fp32
    sum in `voxel_bce`'s fixed order (a function of the sample size only: the same bits in every batch split), count[b] the valid
    pixels; loss_elem (the shape of pred) is returned with `elements=True`.  Records no graph (`differentiable_disparity_loss` does)."""
    p, t, B, P, beta = _check_disparity_loss(pred, gt, beta, "disparity_loss")
    s = torch.empty((B,), dtype=torch.float32, device=p.device)
    n = torch.empty((B,), dtype=torch.int32, device=p.device)
    e = torch.empty(p.shape, dtype=torch.float32, device=p.device) if elements else None
    if B:
        _lib.check(_lib.load().s3r_disparity_loss_forward(p.data_ptr(), t.data_ptr(), beta, s.data_ptr(), n.data_ptr(),
                                                          None if e is None else e.data_ptr(), B, P, _stream_ptr(p.device)),
                   "disparity_loss")
    return s, n, e


@torch.no_grad()
def disparity_loss_backward(pred: torch.Tensor, gt: torch.Tensor, grad_scale: torch.Tensor, beta: float = 1.0) -> torch.Tensor:
    """grad_pred (the shape of pred) of sum_b grad_scale[b] * loss_sum[b] (`s3r_disparity_loss_backward`): grad_scale[b] *
    clamp((pred - gt) / beta, -1, 1) at a valid pixel (grad_scale[b] * sgn(pred - gt) at beta = 0), exactly +0.0 at an invalid one —
    elementwise and bit for bit."""
    p, t, B, P, beta = _check_disparity_loss(pred, gt, beta, "disparity_loss_backward")
    gs = _check_input(grad_scale, "grad_scale", ())
    if gs.shape[0] != B:
        raise RuntimeError(f"grad_scale must have shape ({B},), got {tuple(gs.shape)}")
    g = torch.empty(p.shape, dtype=torch.float32, device=p.device)
    if B:
        _lib.check(_lib.load().s3r_disparity_loss_backward(p.data_ptr(), t.data_ptr(), gs.data_ptr(), beta, g.data_ptr(), B, P,
                                                           _stream_ptr(p.device)), "disparity_loss backward")
    return g


class _DisparityLossFunction(torch.autograd.Function):
    """`disparity_loss`'s loss_sum with `disparity_loss_backward` as its derivative; the gradient goes to pred only.  count is returned
    beside it as a constant."""

    @staticmethod
    def forward(ctx, pred, gt, beta):
        s, n, _ = disparity_loss(pred, gt, beta)
        ctx.save_for_backward(pred, gt)
        ctx.beta = float(beta)
        ctx.mark_non_differentiable(n)
        return s, n

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_sum, _grad_count):
        pred, gt = ctx.saved_tensors
        if not ctx.needs_input_grad[0]:
            return None, None, None
        return disparity_loss_backward(pred, gt, grad_sum.contiguous().float(), ctx.beta), None, None


def differentiable_disparity_loss(pred: torch.Tensor, gt: torch.Tensor, beta: float = 1.0):
    """`disparity_loss`'s (loss_sum (B), count (B)) with loss_sum recorded for autograd: the same bits, with the elementwise backward
    `disparity_loss_backward`.  The gradient goes to pred only (a ground truth is a constant of the loss)."""
    return _DisparityLossFunction.apply(pred, gt, beta)


class DisparityLoss(nn.Module):
    """Smooth-L1 loss (torch.nn.SmoothL1Loss's rule with `beta`; beta = 0 is L1) of a disparity map against a ground truth with invalid
    pixels: forward(pred, gt) with pred, gt (B,H,W) or any (B, ...) returns the mean over the VALID pixels of the batch (ground truth
    finite and >= 0: the EXR maps mark background as inf or negative), `loss_sum.double().sum() / max(count.sum(), 1)` cast to fp32 —
    the per-sample sums and counts are the HIP kernel's, the sums in its fixed order.  A batch without a valid pixel gives 0 and a
    zero gradient.  With grad mode on and pred requiring grad the value (the same bits) is recorded for autograd through
    `differentiable_disparity_loss`; otherwise nothing is recorded (as `VoxelBCELoss`)."""

    def __init__(self, beta: float = 1.0):
        super().__init__()
        beta = float(beta)
        if not (beta >= 0.0) or beta == float("inf"):
            raise ValueError(f"DisparityLoss: beta must be finite and >= 0, got {beta}")
        self.beta = beta

    def forward(self, pred, gt):
        if torch.is_grad_enabled() and isinstance(pred, torch.Tensor) and pred.requires_grad:
            s, n = differentiable_disparity_loss(pred, gt, self.beta)
        else:
            s, n, _ = disparity_loss(pred, gt, self.beta)
        return (s.double().sum() / n.sum().clamp(min=1).double()).float()


@torch.no_grad()
def disparity_metrics(pred: torch.Tensor, gt: torch.Tensor):
    """Stereo metrics per sample (`s3r_disparity_metrics`) over the pixels whose ground truth is valid (finite, >= 0):
    (B,...) x2 fp32 -> (epe (B,) fp32, equal bit for bit to `disparity_epe`; counts (B,4) int32 = valid pixels, |err| > 1,
    |err| > 3, D1 = |err| > 3 and |err| > 0.05 gt).  Integer counts: rates pool exactly over samples and ranks."""
    if pred.shape != gt.shape:
        raise RuntimeError("pred and gt shapes differ")
    pred = _check_input(pred, "pred", pred.shape[1:])
    gt = _check_input(gt, "gt", gt.shape[1:])
    B = pred.shape[0]
    epe = torch.empty((B,), dtype=torch.float32, device=pred.device)
    counts = torch.empty((B, 4), dtype=torch.int32, device=pred.device)
    if B:
        _lib.check(_lib.load().s3r_disparity_metrics(pred.data_ptr(), gt.data_ptr(), epe.data_ptr(), counts.data_ptr(), B,
                                                     pred[0].numel(), _stream_ptr(pred.device)), "disparity_metrics")
    return epe, counts


@torch.no_grad()
def disparity_epe(pred: torch.Tensor, gt: torch.Tensor):
    """Per-sample end-point error mean|pred - gt| over the pixels whose ground truth is valid (finite and >= 0 — EXR
    disparity maps mark background with inf / negative values), reduced on the device: (B,...) x2 ->
    (epe (B,) fp32, valid pixel count (B,) int32)."""
    if pred.shape != gt.shape:
        raise RuntimeError("pred and gt shapes differ")
    pred = _check_input(pred, "pred", pred.shape[1:])
    gt = _check_input(gt, "gt", gt.shape[1:])
    B = pred.shape[0]
    epe = torch.empty((B,), dtype=torch.float32, device=pred.device)
    cnt = torch.empty((B,), dtype=torch.int32, device=pred.device)
    if B:
        _lib.check(_lib.load().s3r_disparity_epe(pred.data_ptr(), gt.data_ptr(), epe.data_ptr(), cnt.data_ptr(), B,
                                                 pred[0].numel(), _stream_ptr(pred.device)), "disparity_epe")
    return epe, cnt


# the names BASELINE.json's north_star uses for the module API
encoder = Encoder
cost_volume = CostVolume
decoder = Decoder
