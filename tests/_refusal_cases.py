"""The host-side refusals of the C-ABI entry points (csrc/s3r_api_layers.hip, csrc/s3r_api_tasks.hip and the thin fronts of
csrc/s3r_conv_forward.hip), as tests/golden/abi_refusals.json pins them: which check fires first, with which code and in which words.

One ROW per entry point: its smallest valid argument list (the baseline) and its checks in source order, each as (label, mutation of
the baseline).  Pointers are distinct dummy addresses, 16 MiB apart and 16-byte aligned, that are never dereferenced: every case is
refused (or returns for an empty batch) before anything is enqueued.  From a row come
  - every single mutation, and every pair of adjacent mutations applied together (the order of the checks); `no_pair` names the pairs
    left out because both mutations need the same argument;
  - with `scratch`: the baseline with scratch = NULL and with one float too few;
  - with `empty`: batch = 0 with valid pointers and with the listed pointers NULL;
  - with `shapes`: for the *_scratch_elems queries the baseline, larger shapes and a refused one; for entries that accept an empty
    batch, batch = 0 with a per-sample extent past the limit (refused or not: the order of the limit and the empty-batch return).
Each case records [rc, s3r_last_error() text]; the text only when rc < 0 (it is stale after a success).

Shared by tests/golden/make_abi_refusals_golden.py (which writes the file) and tests/test_abi_refusals_cpu.py (which compares).  The
calls are made by `python -m tests._refusal_cases` in a child process whose environment hides every device: a case that stopped
refusing would find no device to launch on (and answer S3R_ERR_HIP, which neither the generator nor the test accepts).
"""
from __future__ import annotations

import dataclasses
import json
import math
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IMAX = 2 ** 31 - 1
ERR_HIP = -2
NO_DEVICE_STATUS = 3               # the child's exit status when a device is visible to it
HIDE_DEVICES = {"HIP_VISIBLE_DEVICES": "-1", "ROCR_VISIBLE_DEVICES": "-1", "CUDA_VISIBLE_DEVICES": "-1"}


def dummy(i):
    return (1 << 20) + i * (1 << 24)


def off(n):                        # the argument's own dummy + n bytes: a misaligned pointer
    return ("off", n)


def same(other):                   # the dummy of another argument: two tensors at one address
    return ("same", other)


@dataclasses.dataclass(frozen=True)
class Row:
    entry: str
    args: tuple                    # of (name, kind, baseline): kind "ptr" (a dummy), "val", "struct" (baseline: a factory), "need" (scratch size)
    checks: tuple                  # of (label, {argument or argument.field: value})
    no_pair: tuple = ()            # of (label, next label): both mutations need the same argument
    scratch: tuple = None          # (query, its argument names, the scratch pointer's name)
    empty: tuple = None            # (the batch argument, the pointers that may then be NULL)
    shapes: tuple = ()             # of (tag, mutation): further calls without pairs (a query's shapes; an empty batch of a too large sample)
    launches: bool = True          # the baseline reaches a launch (False: the entry enqueues nothing, its baseline is a case)


def _args(spec, **structs):
    """'x* batch=1 d& need@ stream': name* a pointer, name=value a number, name& a struct (its factory by keyword), name@ the scratch size"""
    out = []
    for tok in spec.split():
        if tok == "stream":
            out.append(("stream", "val", None))
        elif tok.endswith("*"):
            out.append((tok[:-1], "ptr", None))
        elif tok.endswith("&"):
            out.append((tok[:-1], "struct", structs[tok[:-1]]))
        elif tok.endswith("@"):
            out.append((tok[:-1], "need", None))
        else:
            name, v = tok.split("=")
            out.append((name, "val", float(v) if "." in v or "e" in v else int(v)))
    return tuple(out)


def _lib():
    import s3r
    return s3r._lib


# ---------------------------------------------------------------- descriptors of the baselines
def _conv_desc(**kw):
    def make():
        f = dict(op=0, ndim=2, batch=1, cin=16, cout=16, in_size=4, k=3, stride=1, pad=1, act=0, tag=0, tile=-1, in_halo=0, out_halo=0,
                 ksplit=0, dtype=0, in_layout=0, out_layout=0, algo=0, dilation=1, out_pad=0, act_param=0.0)
        f.update(kw)
        return _lib().ConvDesc(**f)
    return make


def _layers(*descs, pointers=True):
    def make():
        P = _lib()
        arr = (P.Layer * len(descs))()
        for i, d in enumerate(descs):
            arr[i].desc = d()
            if pointers:
                arr[i].packed_w, arr[i].scale, arr[i].shift = dummy(40 + 3 * i), dummy(41 + 3 * i), dummy(42 + 3 * i)
        return arr
    return make


LINEAR = _conv_desc(op=2, ndim=1, cin=1, cout=1, in_size=1, k=1, pad=0)
STEM = _conv_desc(cin=3, cout=32, in_size=16, stride=2, act=1, batch=2)
CONV3D = _conv_desc(ndim=3)
BWD = _conv_desc()


def _optim_desc():
    return _lib().OptimDesc(kind=1, flags=4, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.0, max_norm=1.0)      # Adam, norm clip


def _optim_list(n=1, elems=1, pointers=True, same_param=False):
    def make():
        arr = (_lib().OptimTensor * n)()
        for i in range(n):
            arr[i].elems = elems
            if pointers:
                base = 48 + 4 * (0 if same_param else i)
                arr[i].param, arr[i].grad, arr[i].m, arr[i].v = dummy(base), dummy(48 + 4 * i + 1), dummy(48 + 4 * i + 2), dummy(48 + 4 * i + 3)
        return arr
    return make


def _augment_desc():
    return _lib().AugmentDesc(seed=0, channels=3, max_shift=0, flags=0, bg_lo=0, bg_hi=255, brightness_lo=1.0, brightness_hi=1.0,
                              contrast_lo=0.5, contrast_hi=1.5, saturation_lo=1.0, saturation_hi=1.0, noise_sigma=0.0)


def _out_desc():
    return _lib().ConvDesc()


# ---------------------------------------------------------------- the rows
_CONVBWD = (("null-desc", {"d": None}), ("dtype", {"d.dtype": 1}), ("op", {"d.op": 2}), ("dilation", {"d.dilation": 2}),
            ("plain", {"d.in_halo": 1}), ("act", {"d.act": 3}), ("batch", {"d.batch": -1}), ("geometry", {"d.k": 0}),
            ("weight", {"d.cin": 30000, "d.cout": 30000}), ("tiling", {"d.cout": 1, "d.k": 5000, "d.in_size": 5000, "d.pad": 0}),
            ("workgroups", {"d.ndim": 3, "d.cout": 1, "d.k": 200, "d.in_size": 1, "d.pad": 100, "d.batch": 2000}))
_CONVBWD_NO_PAIR = (("null-desc", "dtype"), ("weight", "tiling"), ("tiling", "workgroups"))
_SOFT = "batch=1 channels=1 height=1 width=1 max_disp=1 temperature=1.0 out_height=1 out_width=1 disp_scale=1.0 stream"
_AUG_SHAPE = (("null-desc", {"d": None}), ("channels", {"d.channels": 2}), ("dims", {"batch": 0}), ("plane", {"height": 65536, "width": 32768}),
              ("too-large", {"batch": IMAX}), ("shift", {"d.max_shift": 4097}), ("flags", {"d.flags": 2}), ("background", {"d.bg_hi": 256}),
              ("brightness", {"d.brightness_lo": -1.0}), ("contrast", {"d.contrast_lo": 2.0}), ("saturation", {"d.saturation_lo": -1.0}),
              ("noise", {"d.noise_sigma": -1.0}))
_SURFACE_SHAPE = (("batch", {"batch": 0}), ("edges", {"depth": 257}), ("volume", {"depth": 256, "height": 256, "width": 33}),
                  ("scratch-size", {"batch": IMAX}))
_OPTIM_LIST = (("null-list", {"t": None}), ("count", {"n_tensors": 0}), ("count-max", {"n_tensors": 4097}), ("elems", {"t.0.elems": 0}))

ROWS = (
    # ---- the thin fronts of the forward convolution (csrc/s3r_conv_forward.hip)
    Row("s3r_conv_pack_weights", _args("d& w* packed* stream", d=CONV3D),
        (("null-desc", {"d": None}), ("dims", {"d.batch": 0}), ("route", {"d.dtype": 1}), ("null-w", {"w": None}), ("null-packed", {"packed": None})),
        no_pair=(("null-desc", "dims"),)),
    Row("s3r_conv_forward", _args("d& x* w* scale* shift* y* scratch* need@ stream", d=LINEAR),
        (("null-desc", {"d": None}), ("dims", {"d.cin": 0}), ("halo", {"d.in_halo": 1}), ("null-x", {"x": None}), ("null-w", {"w": None}),
         ("null-y", {"y": None}), ("scratch", {"scratch": None})),
        no_pair=(("null-desc", "dims"),), scratch=("s3r_conv_scratch_elems", "d", "scratch")),
    Row("s3r_chain_forward", _args("layers& n_layers=1 x* y* ws* need@ ws_fresh=0 stream", layers=_layers(CONV3D)),
        (("null-chain", {"layers": None}), ("count", {"n_layers": 0}), ("null-x", {"x": None}), ("null-y", {"y": None}), ("workspace", {"ws": None})),
        scratch=("s3r_chain_workspace_elems", "layers n_layers", "ws")),
    Row("s3r_encoder_forward", _args("layers& n_layers=1 images_left* images_right* features* ws* ws_elems=0 ws_fresh=0 stream", layers=_layers(STEM)),
        (("null-chain", {"layers": None}), ("first-layer", {"layers.0.desc.cin": 16}), ("pair", {"layers.0.desc.batch": 3}),
         ("null-left", {"images_left": None}), ("null-features", {"features": None}), ("align-left", {"images_left": off(4)}),
         ("align-right", {"images_right": off(4)})),
        no_pair=(("null-chain", "first-layer"),)),
    Row("s3r_encoder_forward_u8", _args("layers& n_layers=1 images_left* images_right* features* ws* ws_elems=0 ws_fresh=0 stream", layers=_layers(STEM)),
        (("count", {"n_layers": 0}), ("first-layer", {"layers.0.desc.ndim": 3}), ("pair", {"layers.0.desc.batch": 1}),
         ("null-left", {"images_left": None}), ("null-features", {"features": None}), ("align-left", {"images_left": off(4)}))),
    Row("s3r_decoder_forward", _args("layers& n_layers=1 volume* occupancy* ws* need@ ws_fresh=0 stream", layers=_layers(CONV3D)),
        (("null-chain", {"layers": None}), ("layer-2d", {"layers.0.desc.ndim": 2}), ("null-volume", {"volume": None}),
         ("null-occupancy", {"occupancy": None}), ("workspace", {"ws": None})),
        no_pair=(("null-chain", "layer-2d"),),
        scratch=("s3r_chain_workspace_elems", "layers n_layers", "ws")),
    # ---- layer-level ops (csrc/s3r_api_layers.hip)
    Row("s3r_channels_last_to_f32", _args("x* y* batch=1 channels=1 positions=1 stream"),
        (("null-x", {"x": None}), ("null-y", {"y": None}), ("align", {"x": off(2)}), ("dims", {"channels": 0}), ("batch-max", {"batch": 65536}),
         ("too-large", {"positions": 2 ** 31}))),
    Row("s3r_linear_scratch_elems", _args("batch=1 cin=1 cout=1"), (("dims", {"batch": 0}),), launches=False,
        shapes=(("9x33x100", {"batch": 9, "cin": 33, "cout": 100}), ("64x1024x1024", {"batch": 64, "cin": 1024, "cout": 1024}),
                ("refused", {"cout": -1}))),
    Row("s3r_linear_forward", _args("x* w* bias* y* batch=1 cin=1 cout=1 act=0 scratch* need@ stream"),
        (("null", {"y": None}), ("dims", {"cin": 0}), ("act", {"act": 3}), ("scratch", {"scratch": None})),
        scratch=("s3r_linear_scratch_elems", "batch cin cout", "scratch")),
    Row("s3r_linear_backward_scratch_elems", _args("batch=1 cin=1 cout=1"),
        (("dims", {"cout": 0}), ("too-large", {"batch": 2 ** 16, "cin": 2 ** 15}), ("too-large-max", {"batch": IMAX, "cin": IMAX, "cout": IMAX})),
        no_pair=(("too-large", "too-large-max"),), launches=False,
        shapes=(("9x33x100", {"batch": 9, "cin": 33, "cout": 100}), ("64x1024x1024", {"batch": 64, "cin": 1024, "cout": 1024}),
                ("refused", {"batch": 2 ** 20, "cout": 2 ** 10}))),
    Row("s3r_linear_backward", _args("x* w* y* grad_y* grad_x* grad_w* grad_bias* batch=1 cin=1 cout=1 act=0 scratch* need@ stream"),
        (("all-null", {"grad_x": None, "grad_w": None, "grad_bias": None}), ("act", {"act": 3}), ("null-grad-y", {"grad_y": None}),
         ("null-x", {"x": None}), ("null-w", {"w": None}), ("null-y", {"act": 1, "y": None}), ("dims", {"cin": 0}),
         ("too-large", {"batch": IMAX, "cout": IMAX}), ("scratch", {"scratch": None})),
        scratch=("s3r_linear_backward_scratch_elems", "batch cin cout", "scratch")),
    Row("s3r_head_backward_scratch_elems", _args("batch=1 channels=1 voxels=1"),
        (("dims", {"channels": 0}), ("too-large", {"voxels": 2 ** 31}), ("too-large-bytes", {"batch": 2 ** 30}),
         ("too-large-max", {"batch": IMAX, "channels": IMAX, "voxels": IMAX})),
        no_pair=(("too-large-bytes", "too-large-max"),), launches=False,
        shapes=(("empty", {"batch": 0}), ("3x32x4096", {"batch": 3, "channels": 32, "voxels": 4096}),
                ("2x8x32768", {"batch": 2, "channels": 8, "voxels": 32768}), ("refused", {"batch": -1}))),
    Row("s3r_head_backward", _args("x* w* scale* y* grad_y* grad_x* grad_w* grad_shift* batch=1 channels=1 voxels=1 act=0 scratch* need@ stream"),
        (("all-null", {"grad_x": None, "grad_w": None, "grad_shift": None}), ("act", {"act": -1}), ("dims", {"voxels": 0}),
         ("too-large", {"channels": 2 ** 16, "voxels": 2 ** 15}), ("null-grad-y", {"grad_y": None}), ("null-x", {"x": None}), ("null-w", {"w": None}),
         ("null-y", {"act": 2, "y": None}), ("scratch", {"scratch": None})),
        no_pair=(("dims", "too-large"),),
        scratch=("s3r_head_backward_scratch_elems", "batch channels voxels", "scratch"), empty=("batch", "x w y grad_y scratch"),
        shapes=(("empty-large", {"batch": 0, "voxels": 2 ** 31}),)),
    Row("s3r_conv_adjoint_desc", _args("d& adj&", d=BWD, adj=_out_desc),
        (("null-adj", {"adj": None}),) + _CONVBWD[:6] + (("batch", {"d.batch": 0}),) + _CONVBWD[7:] +
        (("no-adjoint", {"d.k": 1, "d.pad": 1, "d.in_size": 4}),),
        no_pair=_CONVBWD_NO_PAIR + (("workgroups", "no-adjoint"),), launches=False),
    Row("s3r_conv_backward_scratch_elems", _args("d&", d=BWD), _CONVBWD, no_pair=_CONVBWD_NO_PAIR, launches=False,
        shapes=(("empty", {"d.batch": 0}), ("conv3d-32to16-e8-B2", {"d.ndim": 3, "d.cin": 32, "d.in_size": 8, "d.batch": 2}),
                ("deconv3d-16to32-k4s2-e4-B3", {"d.op": 1, "d.ndim": 3, "d.cout": 32, "d.k": 4, "d.stride": 2, "d.batch": 3}),
                ("refused", {"d.ndim": 4}))),
    Row("s3r_conv_backward", _args("d& x* y* grad_y* scale* gs* grad_w* grad_shift* scratch* need@ stream", d=BWD),
        (("all-null", {"gs": None, "grad_w": None, "grad_shift": None}),) + _CONVBWD +
        (("null-grad-y", {"grad_y": None}), ("null-x", {"x": None}), ("null-y", {"d.act": 1, "y": None}), ("scratch", {"scratch": None})),
        no_pair=_CONVBWD_NO_PAIR, scratch=("s3r_conv_backward_scratch_elems", "d", "scratch"), empty=("d.batch", "x y grad_y scratch")),
    Row("s3r_stem_backward_scratch_elems", _args("n_images=1 in_size=1"),
        (("dims", {"n_images": -1}), ("too-large-plane", {"in_size": 16383}), ("too-large", {"n_images": IMAX})), launches=False,
        shapes=(("empty", {"n_images": 0}), ("4x137", {"n_images": 4, "in_size": 137}), ("64x224", {"n_images": 64, "in_size": 224}),
                ("refused", {"in_size": 0}))),
    Row("s3r_stem_backward", _args("images_left* images_right* n_left=1 renders_u8=0 y* grad_y* scale* grad_w* grad_shift* n_images=2 in_size=1 "
                                   "act=0 scratch* need@ stream"),
        (("all-null", {"grad_w": None, "grad_shift": None}), ("act", {"act": 2}), ("dims", {"in_size": 0}), ("too-large", {"n_images": IMAX}),
         ("n-left", {"n_left": 3}), ("n-left-one-tensor", {"images_right": None}), ("null-left", {"images_left": None}),
         ("null-grad-y", {"grad_y": None}), ("null-y", {"act": 1, "y": None}), ("align-left", {"images_left": off(4)}),
         ("align-right", {"images_right": off(4)}), ("scratch", {"scratch": None})),
        scratch=("s3r_stem_backward_scratch_elems", "n_images in_size", "scratch"), empty=("n_images", "images_left images_right y grad_y scratch"),
        shapes=(("empty-large", {"n_images": 0, "in_size": 16383}),)),
    Row("s3r_batchnorm_train_forward_scratch_elems", _args("batch=1 channels=1 positions=2"),
        (("dims", {"positions": 0}), ("too-large", {"channels": IMAX}), ("too-large-max", {"batch": IMAX, "channels": IMAX, "positions": IMAX})),
        no_pair=(("too-large", "too-large-max"),), launches=False,
        shapes=(("empty", {"batch": 0}), ("3x32x4096", {"batch": 3, "channels": 32, "positions": 4096}),
                ("2x5x100003", {"batch": 2, "channels": 5, "positions": 100003}), ("refused", {"channels": 0}))),
    Row("s3r_batchnorm_train_backward_scratch_elems", _args("batch=1 channels=1 positions=2"),
        (("dims", {"batch": -1}), ("too-large", {"positions": 2 ** 31}), ("too-large-bytes", {"batch": 2 ** 29})), launches=False,
        shapes=(("empty", {"batch": 0}), ("3x32x4096", {"batch": 3, "channels": 32, "positions": 4096}),
                ("2x5x100003", {"batch": 2, "channels": 5, "positions": 100003}), ("refused", {"positions": -5}))),
    Row("s3r_batchnorm_train_forward", _args("z* gamma* beta* eps=1e-5 act=0 y* save_mean* save_var* save_invstd* batch=1 channels=1 positions=2 "
                                             "scratch* need@ stream"),
        (("act", {"act": 3}), ("dims", {"batch": -1}), ("too-large", {"channels": IMAX}), ("one-value", {"positions": 1}),
         ("null", {"save_invstd": None}), ("scratch", {"scratch": None})),
        scratch=("s3r_batchnorm_train_forward_scratch_elems", "batch channels positions", "scratch"),
        empty=("batch", "z gamma beta y save_mean save_var save_invstd scratch"), shapes=(("empty-large", {"batch": 0, "positions": 2 ** 31}),)),
    Row("s3r_batchnorm_train_backward", _args("z* y* grad_y* gamma* save_mean* save_invstd* act=0 grad_z* grad_gamma* grad_beta* batch=1 channels=1 "
                                              "positions=2 scratch* need@ stream"),
        (("all-null", {"grad_z": None, "grad_gamma": None, "grad_beta": None}), ("act", {"act": 3}), ("dims", {"batch": -1}),
         ("too-large", {"channels": IMAX}), ("one-value", {"positions": 1}), ("null-grad-y", {"grad_y": None}), ("null-z", {"z": None}),
         ("null-gamma", {"gamma": None}), ("null-y", {"act": 1, "y": None}), ("scratch", {"scratch": None})),
        scratch=("s3r_batchnorm_train_backward_scratch_elems", "batch channels positions", "scratch"),
        empty=("batch", "z y grad_y gamma save_mean save_invstd scratch"), shapes=(("empty-large", {"batch": 0, "channels": IMAX}),)),
    Row("s3r_optim_scratch_elems", _args("t& n_tensors=1", t=_optim_list(pointers=False)),
        _OPTIM_LIST + (("chunks", {"t": _optim_list(512, IMAX, pointers=False), "n_tensors": 512}),),
        no_pair=(("count", "count-max"), ("elems", "chunks")), launches=False,
        shapes=(("3x1000", {"t": _optim_list(3, 1000, pointers=False), "n_tensors": 3}),
                ("70x100003", {"t": _optim_list(70, 100003, pointers=False), "n_tensors": 70}), ("refused", {"t.0.elems": 2 ** 31}))),
    Row("s3r_optim_state_init", _args("state* lr=0.1 stream"), (("null", {"state": None}), ("lr", {"lr": -1.0}))),
    Row("s3r_optim_set_lr", _args("state* lr=0.1 stream"), (("null", {"state": None}), ("lr", {"lr": math.inf}))),
    Row("s3r_optim_step", _args("d& t& n_tensors=1 state* scratch* need@ stream", d=_optim_desc, t=_optim_list()),
        (("null-desc", {"d": None}), ("kind", {"d.kind": 2}), ("flags", {"d.flags": 16}), ("beta1", {"d.beta1": 1.0}), ("beta2", {"d.beta2": -0.5}),
         ("eps", {"d.eps": -1.0}), ("weight-decay", {"d.weight_decay": math.inf}), ("max-norm", {"d.max_norm": -1.0}),
         ("nesterov", {"d.flags": 6}), ("decoupled", {"d.kind": 0, "d.flags": 5}), ("null-state", {"state": None})) + _OPTIM_LIST +
        (("null-grad", {"t.0.grad": None}), ("null-m", {"t.0.m": None}), ("null-v", {"t.0.v": None}), ("scratch", {"scratch": None}),
         ("overlap", {"t.0.v": dummy(48)}), ("same-param", {"t": _optim_list(2, same_param=True), "n_tensors": 2})),
        no_pair=(("null-desc", "kind"), ("nesterov", "decoupled"), ("count", "count-max"), ("overlap", "same-param")),
        scratch=("s3r_optim_scratch_elems", "t n_tensors", "scratch")),
    # ---- stereo and shape ops (csrc/s3r_api_tasks.hip)
    Row("s3r_cost_volume_forward", _args("fl* fr* vol* batch=1 channels=1 max_disp=1 height=1 width=1 out_halo=0 stream"),
        (("null", {"fr": None}), ("dims", {"max_disp": 0}), ("lds", {"height": 128, "width": 65}), ("halo", {"out_halo": 9}),
         ("too-large", {"batch": IMAX}))),
    Row("s3r_cost_volume_forward_wino", _args("fl* fr* planes* batch=1 channels=1 max_disp=1 height=4 width=1 stream"),
        (("null", {"planes": None}), ("shape", {"channels": 0}), ("shape-h", {"height": 6}), ("disp", {"max_disp": 128}),
         ("lds", {"height": 128, "width": 65}), ("too-large", {"batch": IMAX}))),
    Row("s3r_cost_volume_forward_wino2", _args("fl* fr* planes* batch=1 channels=1 max_disp=4 height=4 width=4 stream"),
        (("null", {"fl": None}), ("shape", {"height": 2}), ("shape-d", {"max_disp": 6}), ("disp", {"max_disp": 128}),
         ("lds", {"height": 128, "width": 65}), ("too-large", {"batch": IMAX})),
        no_pair=(("shape-d", "disp"),)),
    Row("s3r_cost_volume_forward_bf16", _args("fl* fr* vol* batch=1 channels=8 max_disp=1 height=1 width=1 out_halo=0 stream"),
        (("null", {"vol": None}), ("align-left", {"fl": off(2)}), ("align-right", {"fr": off(2)}), ("align-volume", {"vol": off(2)}),
         ("dims", {"width": 0}), ("channels", {"channels": 4}), ("halo", {"out_halo": -1}), ("too-large", {"batch": IMAX}))),
    Row("s3r_cost_volume_backward", _args("grad_volume* grad_left* grad_right* batch=1 channels=1 max_disp=1 height=1 width=1 stream"),
        (("all-null", {"grad_left": None, "grad_right": None}), ("dims", {"batch": -1}), ("lds", {"height": 128, "width": 65}),
         ("too-large", {"batch": IMAX}), ("null", {"grad_volume": None})),
        empty=("batch", "grad_volume")),
    Row("s3r_disparity_wta", _args("feat_l* feat_r* disp_l* disp_r* batch=1 channels=1 height=1 width=1 max_disp=1 stream"),
        (("null", {"disp_r": None}), ("dims", {"max_disp": 0}), ("lds", {"channels": 8193}))),
    Row("s3r_disparity_epe", _args("pred* gt* epe* count* batch=1 pixels=1 stream"), (("null", {"count": None}), ("dims", {"pixels": 0}))),
    Row("s3r_disparity_soft", _args("feat_l* feat_r* feat_dtype=0 disp_l* disp_r* conf_l* conf_r* " + _SOFT),
        (("temperature", {"temperature": 0.0}), ("dims", {"out_width": 0}), ("dtype", {"feat_dtype": 2}), ("bf16-channels", {"feat_dtype": 1, "channels": 4}),
         ("bf16-align", {"feat_dtype": 1, "channels": 8, "feat_r": off(2)}), ("lds", {"width": 8192}), ("too-large", {"out_height": 65536, "out_width": 32768}),
         ("rows", {"batch": 2 ** 24}), ("null", {"feat_l": None})),
        no_pair=(("dtype", "bf16-channels"), ("bf16-channels", "bf16-align")), empty=("batch", "feat_l feat_r"),
        shapes=(("empty-large", {"batch": 0, "channels": 2, "height": IMAX}),)),
    Row("s3r_disparity_metrics", _args("pred* gt* epe* counts* batch=1 pixels=1 stream"),
        (("dims", {"pixels": -1}), ("batch-max", {"batch": 65536}), ("too-large", {"pixels": 2 ** 31}), ("null", {"counts": None})),
        empty=("batch", "pred gt epe counts"), shapes=(("empty-large", {"batch": 0, "pixels": 2 ** 31}),)),
    Row("s3r_disparity_soft_backward", _args("feat_l* feat_r* feat_dtype=0 grad_disp_l* grad_disp_r* grad_left* grad_right* " + _SOFT),
        (("null-grad-disp", {"grad_disp_l": None, "grad_disp_r": None}), ("null-grad-feat", {"grad_left": None, "grad_right": None}),
         ("temperature", {"temperature": math.inf}), ("dims", {"channels": 0}), ("bf16", {"feat_dtype": 1}), ("dtype", {"feat_dtype": -1}),
         ("lds", {"width": 8192}), ("too-large", {"channels": 2, "height": IMAX}), ("rows-out", {"out_height": 2 ** 24}),
         ("rows", {"height": 2 ** 24}), ("null", {"feat_r": None})),
        no_pair=(("bf16", "dtype"),), empty=("batch", "feat_l feat_r"), shapes=(("empty-large", {"batch": 0, "channels": 2, "height": IMAX}),)),
    Row("s3r_disparity_loss_forward", _args("pred* gt* beta=1.0 loss_sum* count* loss_elem* batch=1 pixels=1 stream"),
        (("beta", {"beta": -1.0}), ("dims", {"pixels": 0}), ("too-large", {"batch": IMAX}), ("null", {"count": None})),
        empty=("batch", "pred gt loss_sum count"), shapes=(("empty-large", {"batch": 0, "pixels": 2 ** 31}),)),
    Row("s3r_disparity_loss_backward", _args("pred* gt* grad_scale* beta=1.0 grad_pred* batch=1 pixels=1 stream"),
        (("beta", {"beta": math.inf}), ("dims", {"batch": -1}), ("too-large", {"pixels": 2 ** 31}), ("null", {"grad_scale": None})),
        empty=("batch", "pred gt grad_scale grad_pred"), shapes=(("empty-large", {"batch": 0, "pixels": 2 ** 31}),)),
    Row("s3r_augment_scratch_elems", _args("d& batch=1 height=1 width=1", d=_augment_desc), _AUG_SHAPE, no_pair=(("null-desc", "channels"),),
        launches=False,
        shapes=(("no-contrast", {"d.contrast_lo": 1.0, "d.contrast_hi": 1.0}), ("4x137x137", {"batch": 4, "height": 137, "width": 137}),
                ("64x224x224", {"batch": 64, "height": 224, "width": 224}), ("refused", {"d.channels": 5}))),
    Row("s3r_augment_pair", _args("d& left* right* sample_ids* disp_left* disp_right* out_left* out_right* out_disp_left* out_disp_right* "
                                  "batch=1 height=1 width=1 scratch* need@ stream", d=_augment_desc),
        _AUG_SHAPE + (("null-input", {"sample_ids": None}), ("null-output", {"out_right": None}), ("disparity-some", {"disp_left": None}),
                      ("scratch", {"scratch": None}), ("overlap-outputs", {"out_disp_left": same("out_left")}),
                      ("overlap-input", {"right": same("out_right")})),
        no_pair=(("null-desc", "channels"),),
        scratch=("s3r_augment_scratch_elems", "d batch height width", "scratch")),
    Row("s3r_chamfer_forward", _args("p* q* dist1* dist2* idx1* idx2* batch=1 n=1 m=1 stream"),
        (("null", {"idx2": None}), ("empty-cloud", {"n": 0}), ("batch-max", {"batch": 65536}))),
    Row("s3r_chamfer_backward", _args("p* q* idx1* idx2* grad_dist1* grad_dist2* grad_p* grad_q* batch=1 n=1 m=1 stream"),
        (("null", {"q": None}), ("null-grad-dist", {"grad_dist1": None, "grad_dist2": None}), ("null-grad-cloud", {"grad_p": None, "grad_q": None}),
         ("empty-cloud", {"m": 0}), ("batch-max", {"batch": 65536}), ("too-large", {"n": IMAX}))),
    Row("s3r_voxel_iou", _args("pred* gt* threshold=0.5 iou* batch=1 voxels=1 stream"), (("null", {"iou": None}), ("dims", {"voxels": 0}))),
    Row("s3r_voxel_bce_forward", _args("pred* target* loss_sum* loss_elem* batch=1 voxels=1 stream"),
        (("all-null", {"loss_sum": None, "loss_elem": None}), ("dims", {"voxels": 0}), ("too-large", {"batch": IMAX}), ("null", {"target": None})),
        empty=("batch", "pred target"), shapes=(("empty-large", {"batch": 0, "voxels": 2 ** 31}),)),
    Row("s3r_voxel_bce_backward", _args("pred* target* grad_scale* grad_pred* batch=1 voxels=1 stream"),
        (("dims", {"batch": -1}), ("too-large", {"voxels": 2 ** 31}), ("too-large-max", {"batch": IMAX, "voxels": IMAX}), ("null", {"grad_pred": None})),
        no_pair=(("too-large", "too-large-max"),), empty=("batch", "pred target grad_scale grad_pred"),
        shapes=(("empty-large", {"batch": 0, "voxels": 2 ** 31}),)),
    Row("s3r_voxel_surface_points_scratch_elems", _args("batch=1 depth=1 height=1 width=1"), _SURFACE_SHAPE, no_pair=(("edges", "volume"),),
        launches=False,
        shapes=(("3x32x32x32", {"batch": 3, "depth": 32, "height": 32, "width": 32}), ("2x128x128x128", {"batch": 2, "depth": 128, "height": 128, "width": 128}),
                ("refused", {"height": 0}))),
    Row("s3r_voxel_surface_points", _args("occupancy* threshold=0.5 sample_ids* seed=0 points* n_faces* batch=1 depth=1 height=1 width=1 n_points=1 "
                                          "scratch* need@ stream"),
        _SURFACE_SHAPE + (("null", {"sample_ids": None}), ("points", {"n_points": 0}), ("points-max", {"n_points": IMAX}),
                          ("threshold", {"threshold": math.inf}), ("scratch", {"scratch": None}), ("overlap-outputs", {"n_faces": same("points")}),
                          ("overlap-input", {"occupancy": same("scratch")})),
        no_pair=(("edges", "volume"), ("points", "points-max")),
        scratch=("s3r_voxel_surface_points_scratch_elems", "batch depth height width", "scratch")),
)

# fail( sites of the entry-point sources that no host call reaches, each with the earlier check that precludes it
UNREACHABLE = {
    "s3r_conv_adjoint_desc: internal: adjoint output edge %d != input edge %d":
        "out_pad is set to the remainder that makes the adjoint's output edge the input edge, and geometry has accepted both layers.",
    "stem backward: render tensor of 2^31 elements / 4 GiB or more: split the batch":
        "stembwd_dims bounds y = n_images 32 m^2 below 2^31 with m >= in_size / 2, and the renders hold at most 3/8 as many elements.",
}


# the entry-point sources whose fail( sites the golden must reach (csrc/)
ENTRY_SOURCES = ("s3r_api_layers.hip", "s3r_api_tasks.hip", "s3r_host.h")
_FAIL = re.compile(r'(?<![A-Za-z0-9_])fail\(\s*[A-Za-z0-9_]+\s*,\s*((?:"(?:[^"\\]|\\.)*"\s*)+)')
_CONVERSION = re.compile(r"%[-+ #0]*\d*(?:\.\d+)?(?:ll|l|h|z)?[diuxXgfsp]")


def fail_formats(text):
    """the format string of every fail( call in a source text (adjacent literals joined)"""
    out = []
    for m in _FAIL.finditer(text):
        lits = re.findall(r'"((?:[^"\\]|\\.)*)"', m.group(1))
        out.append("".join(lits).replace('\\"', '"').replace("\\\\", "\\"))
    return out


def format_pattern(fmt):
    """a format string as a regular expression: every conversion matches anything"""
    parts, at = [], 0
    for m in _CONVERSION.finditer(fmt):
        parts += [re.escape(fmt[at:m.start()].replace("%%", "%")), ".*"]
        at = m.end()
    return re.compile("".join(parts) + re.escape(fmt[at:].replace("%%", "%")), re.S)


# ---------------------------------------------------------------- cases of a row
def _conflict(a, b):
    ka, kb = set(a), set(b)
    heads = lambda ks: {k.split(".")[0] for k in ks if "." not in k}
    return bool(ka & kb) or any(k.split(".")[0] in heads(kb) for k in ka) or any(k.split(".")[0] in heads(ka) for k in kb)


def cases_of(row):
    """[(case id, kind, mutation)]: kind 'call' (apply the mutation), 'scratch-null' / 'scratch-short', 'empty-valid' / 'empty-null'"""
    out = []
    if not row.launches:
        out.append((f"{row.entry}:baseline", "call", {}))
    for label, mut in row.checks:
        out.append((f"{row.entry}:{label}", "call", mut))
    for (la, ma), (lb, mb) in zip(row.checks, row.checks[1:]):
        if not _conflict(ma, mb):
            out.append((f"{row.entry}:{la}+{lb}", "call", {**ma, **mb}))
    if row.scratch:
        out += [(f"{row.entry}:scratch-null", "scratch-null", {}), (f"{row.entry}:scratch-short", "scratch-short", {})]
    if row.empty:
        out += [(f"{row.entry}:empty-valid", "empty-valid", {}), (f"{row.entry}:empty-null", "empty-null", {})]
    for tag, mut in row.shapes:
        out.append((f"{row.entry}:shape-{tag}", "call", mut))
    return out


def _no_pair_errors():
    """no_pair must name exactly the adjacent pairs that cannot be applied together"""
    out = []
    for row in ROWS:
        cannot = {(la, lb) for (la, ma), (lb, mb) in zip(row.checks, row.checks[1:]) if _conflict(ma, mb)}
        out += [f"{row.entry}: {a} + {b} is left out but not listed" for a, b in sorted(cannot - set(row.no_pair))]
        out += [f"{row.entry}: {a} + {b} is listed but can be applied" for a, b in sorted(set(row.no_pair) - cannot)]
    return out


assert not _no_pair_errors(), "\n".join(_no_pair_errors())
CASE_IDS = [cid for row in ROWS for cid, _, _ in cases_of(row)]
assert len(set(CASE_IDS)) == len(CASE_IDS)


# ---------------------------------------------------------------- the child: makes the calls
def _values(row, mut):
    names = [a[0] for a in row.args]
    vals = {}
    for i, (name, kind, base) in enumerate(row.args):
        vals[name] = dummy(i) if kind == "ptr" else base() if kind == "struct" else base
    for key, v in mut.items():
        head, *path = key.split(".")
        if isinstance(v, tuple):
            v = dummy(names.index(head)) + v[1] if v[0] == "off" else dummy(names.index(v[1]))
        elif callable(v):
            v = v()
        if not path:
            vals[head] = v
            continue
        obj = vals[head]
        for p in path[:-1]:
            obj = obj[int(p)] if p.isdigit() else getattr(obj, p)
        setattr(obj, path[-1], v)
    return vals


def _call(lib, row, vals):
    rc = getattr(lib, row.entry)(*[vals[a[0]] for a in row.args])
    return [rc, lib.s3r_last_error().decode() if rc < 0 else None]


def run_row(lib, row, check_baseline=False):
    """{case id: [rc, text]} of the row; check_baseline (the generator): also that the baseline passes every check (it reaches the launch,
    which finds no device)"""
    need_name = next((a[0] for a in row.args if a[1] == "need"), None)

    def values(mut):
        vals = _values(row, mut)
        if need_name:
            vals[need_name] = 0
            if row.scratch and all(vals[n] is not None for n in row.scratch[1].split()):
                vals[need_name] = getattr(lib, row.scratch[0])(*[vals[n] for n in row.scratch[1].split()])
        return vals

    out = {}
    for cid, kind, mut in cases_of(row):
        vals = values(mut)
        if kind.startswith("scratch"):
            assert vals[need_name] > 0, (cid, vals[need_name])
            if kind == "scratch-null":
                vals[row.scratch[2]] = None
            else:
                vals[need_name] -= 1
        elif kind.startswith("empty"):
            vals = values({row.empty[0]: 0})
            if kind == "empty-null":
                for n in row.empty[1].split():
                    vals[n] = None
        out[cid] = _call(lib, row, vals)
    if check_baseline and row.launches:
        rc, text = _call(lib, row, values({}))
        assert rc == ERR_HIP, f"{row.entry}: the baseline does not reach its launch: {rc} {text}"
    return out


def run_all(lib, check_baseline=False):
    out = {}
    for row in ROWS:
        out.update(run_row(lib, row, check_baseline))
    return out


def child_main(argv):
    import torch
    if torch.cuda.device_count() != 0:
        return NO_DEVICE_STATUS
    import s3r
    json.dump(run_all(s3r.load_library(), check_baseline="--check-baseline" in argv), sys.stdout)
    return 0


def run_in_child(check_baseline=False):
    """The calls of every row, made by a fresh child process that sees no device; raises when the child finds one or fails"""
    cmd = [sys.executable, "-m", "tests._refusal_cases"] + (["--check-baseline"] if check_baseline else [])
    r = subprocess.run(cmd, cwd=ROOT, env=dict(os.environ, **HIDE_DEVICES), capture_output=True, text=True, timeout=300)
    assert r.returncode != NO_DEVICE_STATUS, "the child process sees a device: the refusal calls were not made"
    assert r.returncode == 0, f"the child process failed ({r.returncode}):\n{r.stderr[-4000:]}"
    return json.loads(r.stdout)


if __name__ == "__main__":
    sys.exit(child_main(sys.argv[1:]))
