"""Host-side mirror of the reference's plugin surface for this path: ordinary `torch.nn.Module`s
named `encoder`, `cost_volume`, `decoder` (BASELINE.json north_star; the reference's own class
names live on unmounted branches, /root/reference/README.md:5) whose parameters are plain
nn.Conv/BatchNorm parameters — so `state_dict()` / `load_state_dict()` behave exactly like a stock
PyTorch model — but whose `forward` enqueues the hand-written HIP kernels of libs3r_hip.so through
its C-ABI.  PyTorch is plumbing here (device memory, streams); no torch conv / BN op runs in any
forward below, and nothing falls back to the CPU: without the HIP library every forward raises.

The networks, for inference and for training.  `forward` (and `disparity`, `latent`, `trunk_features`, ...) is the inference path:
eval-mode BatchNorm folded into each layer's epilogue, whole chains behind one C-ABI call, no autograd graph.  The `differentiable*`
methods record a graph on the modules' own parameters, one stand-alone op of ops.py per layer, with the library's deterministic
backward kernels behind it; BatchNorm stays folded, or runs on batch statistics with `batch_stats=True`.  (`train(True)` is still
refused: the mode flag selects nothing here.)  The tensor contracts both halves share live in _tensors.py.
"""
from __future__ import annotations

import ctypes as C
import dataclasses
import os
from typing import Dict, Optional, Sequence

import torch
import torch.nn as nn

from . import _lib
from . import arch_spec as spec
from ._tensors import _check_input, _check_input_cl, _check_render, _stream_ptr, _to_logical, channels_last_to_f32
from .ops import (_StemFunction, differentiable_batchnorm, differentiable_conv, differentiable_cost_volume, differentiable_disparity_soft,
                  differentiable_head, differentiable_linear, disparity_soft, disparity_wta)

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


def _check_pair(left, right, one_device_and_dtype: bool = False):
    """A (left, right) pair of render batches (`_check_render` each) of one batch size.  The networks ask for that much; the encoder,
    which reads both tensors in one kernel, also for one device and dtype — each in its own words."""
    left, right = _check_render(left, "left"), _check_render(right, "right")
    if one_device_and_dtype:
        if left.shape[0] != right.shape[0] or left.device != right.device or left.dtype != right.dtype:
            raise RuntimeError("left and right must be two batches of one size and dtype on one device")
    elif left.shape[0] != right.shape[0]:
        raise RuntimeError("left and right batch sizes differ")
    return left, right


def _chunks(left, right):
    """(l, r, b): the pair in chunks of b <= MAX_CHUNK pairs (read when called); an empty batch is one empty chunk"""
    for s in range(0, max(left.shape[0], 1), MAX_CHUNK):
        l, r = left[s:s + MAX_CHUNK], right[s:s + MAX_CHUNK]
        yield l, r, l.shape[0]


def _cat(parts):
    """the chunks' results as one tensor; a single chunk's is returned as it is"""
    return parts[0] if len(parts) == 1 else torch.cat(parts, 0)


def _fp32_only(module, what: str, why: str):
    """the training paths and the frozen trunks that feed them exist for fp32 models"""
    if module.precision != "fp32":
        raise RuntimeError(f"{what} is implemented for fp32 models only (this one is {module.precision}): {why}")


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

    def shift_under_grad(self, scale):
        """folded()'s shift evaluated with torch operations under grad, for folded()'s (detached) scale: grad_shift reaches `bn.bias`
        and `conv.bias` through torch; `bn.weight` and the running statistics are frozen."""
        if scale is None:
            return self.conv.bias
        return self.bn.bias + (self.conv.bias - self.bn.running_mean.detach()) * scale


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
            self.eval()              # the mode flag stays False: batch statistics are an argument (`batch_stats`), not a mode

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
        layer's edge % 4 == 0, no sigmoid, ...: the rules live in s3r_plan_algo.hip's resolve_algo, so the question is put to the scratch query of a
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

    def _alloc_out(self, batch: int, n_layers: int, device) -> torch.Tensor:
        """the chain's output as the kernels write it: plain fp32 (B,C,...), or physical channels-last (B,...,C) bf16"""
        shape = self._out_shape(batch, n_layers)
        if self._out_is_bf16(n_layers):
            return torch.empty((shape[0],) + shape[2:] + (shape[1],), dtype=torch.bfloat16, device=device)
        return torch.empty(shape, dtype=torch.float32, device=device)

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
            n = len(self._layers) if upto is None else self.names.index(upto) + 1
            y = self._alloc_out(0, n, device)
            return _to_logical(y) if self._out_is_bf16(n) else y
        arr, n = self._layer_array(batch, device, upto, in_halo, in_layout)
        y = self._alloc_out(batch, n, device)      # (bf16: handed back as a logical (B,C,...) view)
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
            x = differentiable_conv(x, blk.conv.weight, scale, blk.shift_under_grad(scale), l)
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
        left, right = _check_pair(left, right, one_device_and_dtype=True)
        if left.shape[0] == 0:
            return self._run(left)
        return self._run(left, None, 0, right)

    # -- the trainable tower (fp32 models) --------------------------------------------------------------
    def _differentiable(self, left: torch.Tensor, right: Optional[torch.Tensor], batch_stats: bool, who: str) -> torch.Tensor:
        _fp32_only(self, who, "the backward kernels read fp32 activations")
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
            x = _StemFunction.apply(blk.conv.weight, blk.shift_under_grad(scale), scale, self, left, right, l.act)
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
        left, right = _check_pair(left, right, one_device_and_dtype=True)
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
        self._pinned = False                             # set by GraphedForward: a captured HIP graph holds the two buffers' addresses

    def _resident(self, name: str, shape, device, dtype=torch.float32) -> torch.Tensor:
        """The resident buffer `self.<name>` for `shape`: zeroed when (re)allocated — the kernels write the interior only — and never
        replaced once a captured graph holds its address."""
        buf = getattr(self, name)
        if buf is None or tuple(buf.shape) != shape or buf.device != device or buf.dtype != dtype:
            if self._pinned:
                raise RuntimeError("the padded cost volume of this module is captured in a HIP graph for another shape")
            buf = torch.zeros(shape, dtype=dtype, device=device)
            setattr(self, name, buf)
        return buf

    def _bf16(self, feat_left, feat_right, halo, resident):
        """bf16 path: logical (B,C,H,W) channels_last features -> physical (B,D+2h,H+2h,W+2h,2C) volume."""
        if feat_left.shape != feat_right.shape or feat_left.dim() != 4:
            raise RuntimeError("feature maps must both be (B,C,H,W)")
        fl = _check_input_cl(feat_left, "feat_left", feat_left.shape[1:])
        fr = _check_input_cl(feat_right, "feat_right", feat_left.shape[1:])
        B, H, W, Cc = fl.shape
        shape = (B, self.max_disp + 2 * halo, H + 2 * halo, W + 2 * halo, 2 * Cc)
        if resident:
            vol = self._resident("_padded", shape, fl.device, torch.bfloat16)
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
        vol = self._resident("_padded", shape, fl.device)
        if B == 0:
            return vol
        _lib.check(_lib.load().s3r_cost_volume_forward(fl.data_ptr(), fr.data_ptr(), vol.data_ptr(), B, Cc,
                                                       self.max_disp, H, W, halo, _stream_ptr(fl.device)),
                   "cost_volume")
        return vol

    @torch.no_grad()
    def forward_wino(self, feat_left: torch.Tensor, feat_right: torch.Tensor) -> torch.Tensor:
        """fp32 internal hand-off to a decoder whose first 3D conv runs the Winograd kernel (`takes_wino_input`): the volume
        written directly as the six F(4,3)-along-H plane sets of its halo-1 padded form, (6,B,2C,D+2,H/4,W+2) — bit-identical
        to the consumer's own input transform, without the volume's round trip through HBM."""
        fl = _check_input(feat_left, "feat_left", feat_left.shape[1:])
        fr = _check_input(feat_right, "feat_right", feat_left.shape[1:])
        B, Cc, H, W = fl.shape
        shape = (6, B, 2 * Cc, self.max_disp + 2, H // 4, W + 2)      # F(4,3) along H: six plane sets, one row per four outputs
        planes = self._resident("_planes", shape, fl.device)
        _lib.check(_lib.load().s3r_cost_volume_forward_wino(fl.data_ptr(), fr.data_ptr(), planes.data_ptr(), B, Cc,
                                                            self.max_disp, H, W, _stream_ptr(fl.device)), "cost_volume (wino)")
        return planes

    @torch.no_grad()
    def forward_wino2(self, feat_left: torch.Tensor, feat_right: torch.Tensor) -> torch.Tensor:
        """The same hand-off for a decoder whose first 3D conv runs the TWO-AXIS Winograd kernel: the 36 F(4,3) x F(4,3) plane
        sets of the halo-1 padded volume, (36,B,2C,D/4,H/4,W+2), each value bit-identical to the consumer's own input transform.  In
        memory the column lies OUTSIDE the row group, (36,B,2C,D/4,W+2,H/4) — what S3R_LAYOUT_WINO_DH is — so the tensor handed back
        is a transposed VIEW of the resident buffer (the way the bf16 modules hand each other logical views of channels-last buffers):
        Decoder.forward_padded(in_layout=LAYOUT_WINO_DH) takes it as it is; its first layer skips the K tiles that hold the volume's
        structural zeros."""
        fl = _check_input(feat_left, "feat_left", feat_left.shape[1:])
        fr = _check_input(feat_right, "feat_right", feat_left.shape[1:])
        B, Cc, H, W = fl.shape
        shape = (36, B, 2 * Cc, self.max_disp // 4, W + 2, H // 4)
        planes = self._resident("_planes", shape, fl.device)
        _lib.check(_lib.load().s3r_cost_volume_forward_wino2(fl.data_ptr(), fr.data_ptr(), planes.data_ptr(), B, Cc,
                                                             self.max_disp, H, W, _stream_ptr(fl.device)), "cost_volume (wino2)")
        return planes.transpose(-1, -2)

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
        _fp32_only(self, "CostVolume.differentiable", "the cost-volume backward kernel reads fp32 tensors")
        return differentiable_cost_volume(feat_left, feat_right, self.max_disp)


def _check_wino_planes(v: torch.Tensor, layout: int = _lib.LAYOUT_WINO_H) -> torch.Tensor:
    if layout == _lib.LAYOUT_WINO_DH:
        ncls, want = 36, (2 * spec.FEAT_C, spec.MAX_DISP // 4, spec.FEAT_HW // 4, spec.FEAT_HW + 2)
    else:
        ncls, want = 6, (2 * spec.FEAT_C, spec.MAX_DISP + 2, spec.FEAT_HW // 4, spec.FEAT_HW + 2)
    if not isinstance(v, torch.Tensor) or not v.is_cuda or v.dtype != torch.float32 or v.dim() != 6 or v.shape[0] != ncls or \
            tuple(v.shape[2:]) != want or (layout != _lib.LAYOUT_WINO_DH and not v.is_contiguous()):
        raise RuntimeError(f"transformed volume must be a contiguous float32 HIP tensor ({ncls}, B, {', '.join(map(str, want))})")
    if layout == _lib.LAYOUT_WINO_DH:      # in memory (.., W+2, H/4): CostVolume.forward_wino2's view passes through, anything else is copied once
        phys = v.transpose(-1, -2)
        return (phys if phys.is_contiguous() else phys.contiguous()).transpose(-1, -2)
    return v


class _VolumeChain(_HipChain):
    """A chain that reads the cost volume (Decoder, VolumeEncoder): the volume's validation in its three forms — plain, halo-padded,
    Winograd-transformed planes."""
    _entry = "s3r_decoder_forward"

    def __init__(self, layers, precision: str, winograd):
        super().__init__(layers, spec.MAX_DISP, tag_base=200, precision=precision, winograd=winograd)

    def _run_plain(self, volume: torch.Tensor, upto: Optional[str] = None) -> torch.Tensor:
        tail = (2 * spec.FEAT_C, spec.MAX_DISP, spec.FEAT_HW, spec.FEAT_HW)
        check = _check_input_cl if self.precision == "bf16" else _check_input
        return self._run(check(volume, "volume", tail), upto)

    def _run_padded(self, volume_padded: torch.Tensor, halo: int, in_layout: int, upto: Optional[str] = None) -> torch.Tensor:
        """The chain on the halo-padded volume CostVolume.forward_padded produced (no pad copy; bf16: physical
        (B,D+2h,H+2h,W+2h,2C)), or (in_layout = LAYOUT_WINO_H / LAYOUT_WINO_DH) on the transformed planes CostVolume.forward_wino /
        forward_wino2 produced (LAYOUT_WINO_DH: exactly that call's output — the first layer relies on the cost volume's mask)."""
        if in_layout in (_lib.LAYOUT_WINO_H, _lib.LAYOUT_WINO_DH):
            return self._run(_check_wino_planes(volume_padded, in_layout), upto, in_halo=1, in_layout=in_layout)
        n = (spec.MAX_DISP + 2 * halo, spec.FEAT_HW + 2 * halo, spec.FEAT_HW + 2 * halo)
        if self.precision == "bf16":
            x = _check_input(volume_padded, "volume_padded", n + (2 * spec.FEAT_C,), torch.bfloat16)
        else:
            x = _check_input(volume_padded, "volume_padded", (2 * spec.FEAT_C,) + n)
        return self._run(x, upto, in_halo=halo)


class Decoder(_VolumeChain):
    """3D conv hourglass: cost volume (B,64,28,28,28) -> occupancy probabilities (B,32,32,32)."""

    def __init__(self, precision: str = "fp32", winograd=None):
        super().__init__(spec.DECODER, precision, winograd)

    def forward(self, volume: torch.Tensor, upto: Optional[str] = None) -> torch.Tensor:
        y = self._run_plain(volume, upto)
        return y.squeeze(1) if upto is None or upto == self.names[-1] else y

    def forward_padded(self, volume_padded: torch.Tensor, halo: int = 1, in_layout: int = 0, upto: Optional[str] = None) -> torch.Tensor:
        """`forward` on the cost volume's internal hand-off forms (`_run_padded`)."""
        y = self._run_padded(volume_padded, halo, in_layout, upto)
        return y.squeeze(1) if upto is None or upto == self.names[-1] else y

    # -- the trainable occupancy head (fp32 models) ---------------------------------------------------
    FEATURES = "d3"          # the layer whose output the occupancy head reads

    def _fp32_only(self, what: str):
        _fp32_only(self, what, "the head backward and the BCE kernels read fp32 tensors")

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


class VolumeEncoder(_VolumeChain):
    """The down half of the hourglass alone (Stereo2Point): cost volume -> (B,512,4,4,4) latent."""

    def __init__(self, precision: str = "fp32", winograd=None):
        super().__init__(spec.DECODER_DOWN, precision, winograd)

    def forward(self, volume: torch.Tensor) -> torch.Tensor:
        return self._run_plain(volume)

    def forward_padded(self, volume_padded: torch.Tensor, halo: int = 1, in_layout: int = 0) -> torch.Tensor:
        return self._run_padded(volume_padded, halo, in_layout)

    def differentiable_features(self, x: torch.Tensor, start: str = "v1", batch_stats: bool = False) -> torch.Tensor:
        """Layers `start` .. v6 recorded for autograd on this module's own parameters, by the loop of `Decoder.differentiable_features`
        (`bn.weight` frozen, `bn.bias` and `conv.bias` reached through the folded shift): x is `start`'s input — for "v1" the plain
        (B,64,28,28,28) volume `CostVolume.differentiable` returns —, the result the (B,512,4,4,4) latent
        `PointHead.differentiable` reads.  fp32 models only.  batch_stats=True: every BatchNorm layer in training form, as
        `Decoder.differentiable_features` describes."""
        _fp32_only(self, "VolumeEncoder.differentiable_features", "the conv backward kernels read fp32 tensors")
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
        dls, drs = [], []
        for l, r, b in _chunks(*_check_pair(left, right)):
            feats = self.encoder.forward_pair(l, r)
            if feats.dtype != torch.float32:                     # bf16 path: channels-last bf16 -> fp32 NCHW (HIP kernel)
                feats = channels_last_to_f32(feats)
            dl, dr = disparity_wta(feats[:b], feats[b:], self.cost_volume.max_disp)
            dls.append(dl), drs.append(dr)
        scale = float(spec.IMG_HW // spec.FEAT_HW) if in_pixels else 1.0
        return _cat(dls) * scale, _cat(drs) * scale

    def _disparity_soft(self, left, right, in_pixels, temperature, full_resolution, confidence):
        tau = float(self.disparity_temperature if temperature is None else temperature)
        left, right = _check_pair(left, right)
        scale = float(spec.IMG_HW // spec.FEAT_HW) if in_pixels else 1.0
        size = (spec.IMG_HW, spec.IMG_HW) if full_resolution else None
        parts = []
        for l, r, b in _chunks(left, right):
            feats = self.encoder.forward_pair(l, r)            # fp32 NCHW, or the bf16 channels-last features as they are
            parts.append(disparity_soft(feats[:b], feats[b:], self.cost_volume.max_disp, tau, size, scale, confidence))
        return tuple(_cat(p) for p in zip(*parts))

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
        _fp32_only(self, "stereo_features", "the cost-volume backward kernel reads fp32 tensors")
        fls, frs = [], []
        for l, r, b in _chunks(*_check_pair(left, right)):
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
        for l, r, b in _chunks(*_check_pair(left, right)):
            feats = self.encoder.forward_pair(l, r)          # (2b,32,28,28): left batch, then right batch
            # (v1 on a Winograd kernel: the volume goes over in the transformed layout that kernel reads)
            vol, layout = self.cost_volume.forward_for(self.decoder, feats[:b], feats[b:])
            yield self.decoder.forward_padded(vol, in_layout=layout, upto=upto)

    @torch.no_grad()
    def forward(self, left: torch.Tensor, right: torch.Tensor) -> torch.Tensor:
        """left, right: (B,3,224,224) float32 in [0,1] or uint8 (8-bit renders: scaled by 1/255 inside the first kernel)."""
        return _cat(list(self._decoded(left, right)))

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
        return _cat(list(self._decoded(left, right, upto=upto)))

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
        for l, r, b in _chunks(*_check_pair(left, right)):
            feats = self.encoder.forward_pair(l, r)
            vol, layout = self.cost_volume.forward_for(self.decoder, feats[:b], feats[b:])
            latent = self.decoder.forward_padded(vol, in_layout=layout)
            if latent.dtype != torch.float32:                      # bf16 channels-last view -> fp32 (B,512,4,4,4): HIP kernel
                latent = channels_last_to_f32(latent)
            yield latent

    @torch.no_grad()
    def forward(self, left: torch.Tensor, right: torch.Tensor) -> torch.Tensor:
        return _cat([self.point_head(latent) for latent in self._latents(left, right)])

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
        return _cat(list(self._latents(left, right)))


# the names BASELINE.json's north_star uses for the module API
encoder = Encoder
cost_volume = CostVolume
decoder = Decoder
