"""The case table of tests/test_streams_gpu.py, shared with tests/test_streams_cpu.py: every entry point of include/s3r.h that takes a
`void* stream`, at the smallest shapes that still take every launch of the entry point.

A case is a recipe, not data: `case.plan(lib, dev)` returns a `Plan` —

  args     the buffers of the call, `Arg(name, shape, dtype, role)`; roles:
             "in"    an input; two data sets exist for it (`data(0)`, `data(1)`)
             "out"   an output the call must write whole (poison-filled in front of the call, no poison may remain)
             "zero"  an output the CALLER zeroes and the call writes in part (the plane layouts of the cost volume)
             "scr"   scratch / workspace / the packed-weight image of a pack + forward pair: NaN-filled in front of the call
  data(k)  name -> host tensor for every "in" argument (set k), plus "_ref": whatever `check` needs of the logical problem
  call     (ptr: name -> device address, stream) -> return code; a case may make several library calls (pack + forward; a chain with
           ws_fresh = 1 and then 0 on another input), every one on `stream`
  check    (data(k), results: name -> host tensor) -> None: the entry's existing reference — bit equality with the restated order
           where the contract is bits, the per-element fp64 bound (tests/_ref64.py at HALF, tests/_linear64.py, tests/_bce64.py,
           tests/test_disparity_soft_gpu.py's) otherwise
  refuse   training entries only: (ptr, stream) -> (return code, the code the header promises): the same call with a scratch one
           element short, or with the arguments the header names as invalid; it must enqueue nothing

`plan(lib, None)` plans sizes only (no device): what tests/test_streams_cpu.py reads.  The layer arrays of the chain and stage
entries point at parameter images that are packed BEFORE an instrument starts and stay constant through it; the pack entry itself is
under the instruments in every convolution case.

PRESTATE names the bit pattern every buffer holds before anything is queued (tests/_guard.py's patterns); `safe_prestate` says why
the header allows the library to read it.
"""
from __future__ import annotations

import ctypes as C
import re
from dataclasses import dataclass
from typing import Callable, Optional

import numpy as np
import torch

import s3r
from s3r import arch_spec as spec
from tests import _bce64 as B64
from tests import _buffer_cases as BC
from tests import _chamfer64 as C64
from tests import _disp64 as D64
from tests import _guard as G
from tests import _head64 as H64
from tests import _linear64 as L64
from tests import _ref64 as R
from tests import _select_ref as SR

L = spec.Layer
F32, BF16, I32, U8 = torch.float32, torch.bfloat16, torch.int32, torch.uint8
CAP_BYTES = 64 << 20
HALF = 0.5
TRAINING = ("s3r_linear_backward", "s3r_chamfer_backward", "s3r_voxel_bce_forward", "s3r_voxel_bce_backward", "s3r_head_backward")
FAMILIES = ("conv", "chain", "linear_backward", "head_backward", "chamfer", "bce", "disparity")   # one misplaced-stream mutant each


@dataclass(frozen=True)
class Arg:
    name: str
    shape: tuple
    dtype: torch.dtype
    role: str

    @property
    def nbytes(self):
        n = 1
        for s in self.shape:
            n *= s
        return n * torch.empty(0, dtype=self.dtype).element_size()


@dataclass
class Plan:
    args: list
    data: Callable
    call: Callable
    check: Callable
    refuse: Optional[Callable] = None
    keep: object = None

    @property
    def nbytes(self):
        return sum(a.nbytes for a in self.args)


@dataclass(frozen=True)
class Case:
    id: str
    entries: tuple          # the prototypes of include/s3r.h this case calls with its stream
    family: str
    make: Callable          # (lib, dev or None) -> Plan
    mutant: bool = False    # the family's misplaced-stream case

    def plan(self, lib, dev=None):
        return self.make(lib, dev)


# ---------------------------------------------------------------- pre-states
def prestate(arg):
    """the bits `arg` holds before anything is queued (a value of the signed bit view of tests/_guard.py): inputs the poison,
    outputs and scratch the scratch NaN, int32 index inputs the int32 guard pattern, 8-bit renders the byte guard.  An int32 OUTPUT
    (indices, counts) has no NaN, and its poison IS the guard pattern (tests/_guard.py), so its pre-state is the int32 halo sentinel:
    negative like both, which no index or count is, and different from the poison the stream fills it with"""
    bits = G._BITS[arg.dtype]
    if arg.dtype == U8:
        return bits[1]
    if arg.dtype == I32:
        return bits[1] if arg.role == "in" else bits[3]
    return bits[2] if arg.role == "in" else bits[4]


# what a header comment has to say for a pre-state to count as documented: NaN in its arithmetic, indices clamped
_NAN_WORDING = r"\bNaN\b"
_INDEX_WORDING = r"garbage\s+index\s+never\s+reads\s+outside"


def safe_prestate(arg, entry_comment):
    """why the library may READ `arg`'s pre-state (None: it may not), from the comment in front of the entry's prototype.

    float, fp32 or bf16: the pattern must be a NaN.  Where the entry's comment says what a NaN does (the selection, loss and backward
    entries: skipped by the minimum, "not occupied", poisons one sample, propagates through the arithmetic) the answer names that
    wording: "NaN (header)".  The other entries (convolutions, chains, stages, cost volumes, linear forward, disparity read-outs)
    say nothing of non-finite values — their NaN rules are not pinned — and the answer is the weaker "NaN (data only)": in every
    prototype a float tensor is an operand of arithmetic or of a comparison and never an index, an offset or a count, so no float
    value can move an address.  test_streams_cpu.py pins which entries are in the first group.
    int32: an INPUT is an index, safe only where the comment says that a garbage index never reads outside; an output is never read.
    8-bit: every byte is a render sample."""
    v = prestate(arg)
    if arg.dtype in (F32, BF16):
        as_f32 = np.array([v if arg.dtype == F32 else v << 16], np.int64).astype(np.int32).view(np.float32)[0]
        if not np.isnan(as_f32):
            return None
        return "NaN (header)" if re.search(_NAN_WORDING, entry_comment) else "NaN (data only)"
    if arg.dtype == U8:
        return "any byte is a render sample"
    if arg.role != "in":
        return "never read"
    return "clamped" if re.search(_INDEX_WORDING, entry_comment) else None


def stream_prototypes(header_text):
    """name -> the comment block in front of it, for every prototype of include/s3r.h with a `void* stream` parameter"""
    out = {}
    for m in re.finditer(r"\b(?:int|int64_t)\s+(s3r_\w+)\s*\(([^;{}]*?)\)\s*;", header_text, re.S):
        if re.search(r"void\s*\*\s*stream\b", m.group(2)):
            before = header_text[:m.start()]
            out[m.group(1)] = before[before.rfind("/*"):]
    return out


# ---------------------------------------------------------------- helpers
def _t(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return t if dtype is None else t.to(dtype)


def _np(t):
    return t.detach().cpu().numpy()


def _same(got, want, what):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    v = np.int32 if got.dtype == np.float32 else got.dtype
    bad = np.argwhere(got.view(v) != want.view(v))
    assert not bad.size, f"{what}: first of {len(bad)} differing elements at {tuple(bad[0])}: got {got[tuple(bad[0])]!r}, want {want[tuple(bad[0])]!r}"


def _within(got, ref, bnd, what):
    ratio, i = R.worst(got, ref, bnd)
    assert ratio <= HALF, (what, ratio, i)


def _within_np(got, ref, bnd, what):
    got = np.asarray(got, np.float64)
    assert not np.isnan(got).any(), what
    over = np.abs(got - ref) > bnd
    assert not over.any(), (what, int(over.sum()), float(np.abs(got - ref).max()))


# ---------------------------------------------------------------- s3r_conv_pack_weights + s3r_conv_forward
def _conv(cc, refused_out_halo=None):
    """refused_out_halo: the forward with this out_halo in the descriptor is refused with S3R_ERR_INVALID (the plan's `refuse`)"""
    l, nd, bf, B = cc.layer, R.ndim(cc.layer), cc.dtype == "bf16", cc.B
    stem, head = BC._stem(l), BC._head(l, cc.n_in)
    cl_in, cl_out = bf and not stem, bf and not head

    def make(lib, dev):
        from tests._abi_calls import pad
        ih = BC.need_halo(l, cc.n_in, cc.dtype)
        desc = s3r._lib.make_desc(l, B, cc.n_in, tile=cc.tile, in_halo=ih, out_halo=0, ksplit=cc.ksplit, dtype=s3r._lib.DTYPE[cc.dtype],
                                  algo=cc.algo)
        npk = C.c_int64(0)
        assert lib.s3r_conv_packed_elems(C.byref(desc), C.byref(npk)) == 0, lib.s3r_last_error()
        need = lib.s3r_conv_scratch_elems(C.byref(desc))
        assert need >= 0, lib.s3r_last_error()
        n_out = lib.s3r_conv_out_size(C.byref(desc))
        xsp, ysp = (cc.n_in + 2 * ih,) * nd, (n_out,) * nd
        xshape = (B,) + xsp + (l.cin,) if cl_in else (B, l.cin) + xsp
        yshape = (B,) + ysp + (l.cout,) if cl_out else (B, l.cout) + ysp
        wshape = tuple(R.make_params(l, 0)["w"].shape)
        args = [Arg("x", xshape, BF16 if cl_in else F32, "in"), Arg("w", wshape, F32, "in"), Arg("shift", (l.cout,), F32, "in")]
        if l.bn:
            args.append(Arg("scale", (l.cout,), F32, "in"))
        args += [Arg("packed", (npk.value,), F32, "scr"), Arg("y", yshape, BF16 if cl_out else F32, "out"), Arg("scratch", (need,), F32, "scr")]

        def data(k):
            p = R.make_params(l, 17 + 5 * k)
            if bf and not stem and not head:
                p["w"] = p["w"].to(BF16).float()
            x = torch.randn((B, l.cin) + (cc.n_in,) * nd, generator=torch.Generator().manual_seed(100 + k))
            if bf and not stem:
                x = x.to(BF16).float()
            xp, _ = pad(x.to(BF16) if cl_in else x, ih, cl_in)
            d = {"x": xp, "w": p["w"], "shift": p["shift"], "_ref": (x, p)}
            if l.bn:
                d["scale"] = p["scale"]
            return d

        def call(ptr, st):
            rc = lib.s3r_conv_pack_weights(C.byref(desc), ptr["w"], ptr["packed"], st)
            if rc:
                return rc
            return lib.s3r_conv_forward(C.byref(desc), ptr["x"], ptr["packed"], ptr.get("scale"), ptr["shift"], ptr["y"], ptr["scratch"], need, st)

        def check(d, res):
            x, p = d["_ref"]
            y = res["y"]
            got = y.permute(0, y.dim() - 1, *range(1, y.dim() - 1)) if cl_out else y
            ref, mag = R.ref64(l, x, p)
            _within(got.float(), ref, R.bound(l, ref, mag, cc.form), cc.id)

        refuse = None
        if refused_out_halo is not None:               # (the forward alone: a refused call reads no packed weights)
            bad = s3r._lib.make_desc(l, B, cc.n_in, tile=cc.tile, in_halo=ih, out_halo=refused_out_halo, ksplit=cc.ksplit,
                                     dtype=s3r._lib.DTYPE[cc.dtype], algo=cc.algo)
            assert lib.s3r_conv_scratch_elems(C.byref(bad)) == -1, "expected to be refused"
            refuse = lambda ptr, st: (lib.s3r_conv_forward(C.byref(bad), ptr["x"], ptr["packed"], ptr.get("scale"), ptr["shift"], ptr["y"],
                                                           ptr["scratch"], need, st), -1)
        return Plan(args, data, call, check, refuse=refuse, keep=desc)

    return make


W, DIRECT = s3r.ALGO_WINOGRAD, s3r.ALGO_DIRECT
_CC = BC.ConvCase
CONV = [
    _CC("direct-conv3d-32to32-e8", L("t", "conv3d", 32, 32, 3, 1, 1), 8, 2, algo=DIRECT),
    _CC("splitk2-leaky-finish-conv3d-64to32-s2-e9", L("t", "conv3d", 64, 32, 3, 2, 1, True, "leaky_relu", 1, 0, 0.3), 9, 2, ksplit=2),
    _CC("wino2-class-parallel-conv3d-32to32-e8", L("t", "conv3d", 32, 32, 3, 1, 1), 8, 2, algo=W, tile=4),
    _CC("transposed-f22-classes-deconv3d-32to32-e4", L("t", "deconv3d", 32, 32, 4, 2, 1), 4, 2, algo=W, tile=1),
    _CC("wino3-deconv3d-64to32-e8", L("t", "deconv3d", 64, 32, 4, 2, 1), 8, 2, algo=W, tile=6),
    _CC("staged-tanh-conv2d-20to33-k5-e9", L("t", "conv2d", 20, 33, 5, 1, 2, True, "tanh"), 9, 2),
    _CC("unfolded-conv2d-3to16-e17", L("t", "conv2d", 3, 16, 3, 1, 1), 17, 2),
    _CC("tclass-deconv2d-32to16-k4s2-e9", L("t", "deconv2d", 32, 16, 4, 2, 1), 9, 2),
    _CC("d2s-deconv2d-16to16-k2s2-e9", L("t", "deconv2d", 16, 16, 2, 2, 0), 9, 2),
    _CC("bf16-conv3d-32to96-e7", L("t", "conv3d", 32, 96, 3, 1, 1), 7, 2, dtype="bf16"),
]


# ---------------------------------------------------------------- s3r_chain_forward
def _chain(name, parts, B=2):
    layers = [q.layer for q in parts]

    def make(lib, dev):
        if dev is None:                                            # sizes only: descriptors without parameter images
            arr = (s3r._lib.Layer * len(parts))()
            for i, q in enumerate(parts):
                arr[i].desc = s3r._lib.make_desc(q.layer, B, q.n_in, tag=i, algo=q.algo, tile=q.tile)
            params, keep = None, None
        else:
            from tests import _abi_bodies as AB
            _, params, arr, keep = AB.chain_case(s3r, lib, parts, B, 0)
        n = len(parts)
        need = lib.s3r_chain_workspace_elems(arr, n)
        assert need > 0, lib.s3r_last_error()
        first, last = parts[0], parts[-1]
        n_out = lib.s3r_conv_out_size(C.byref(arr[n - 1].desc))
        xshape = (B, first.layer.cin) + (first.n_in,) * R.ndim(first.layer)
        yshape = (B, last.layer.cout) + (() if last.layer.op == "linear" else (n_out,) * R.ndim(last.layer))
        args = [Arg("xa", xshape, F32, "in"), Arg("xb", xshape, F32, "in"), Arg("ya", yshape, F32, "out"), Arg("yb", yshape, F32, "out"),
                Arg("ws", (need,), F32, "scr")]

        def data(k):
            g = torch.Generator().manual_seed(50 + k)
            xa, xb = torch.randn(xshape, generator=g), torch.randn(xshape, generator=g)
            return {"xa": xa, "xb": xb}

        def call(ptr, st):                                         # ws_fresh = 1, then the same arena, not re-zeroed, on another input
            rc = lib.s3r_chain_forward(arr, n, ptr["xa"], ptr["ya"], ptr["ws"], need, 1, st)
            if rc:
                return rc
            return lib.s3r_chain_forward(arr, n, ptr["xb"], ptr["yb"], ptr["ws"], need, 0, st)

        def check(d, res):
            forms = ["wino" if BC.has_wino(_CC("", q.layer, q.n_in, B, algo=q.algo, tile=q.tile)) else "direct" for q in parts]
            for xi, yi in (("xa", "ya"), ("xb", "yb")):
                ref, bnd = R.chain_ref64(layers, forms, d[xi], [{k: (None if v is None else v.cpu()) for k, v in p.items()} for p in params])
                _within(res[yi], ref, bnd, (name, yi))

        return Plan(args, data, call, check, keep=(arr, keep))

    return make


_PAIRS = {p[0]: p for p in BC.CHAIN_PAIRS}
CHAINS = {
    "handoff-b-k3-e8": [BC.Part(L("ha", "conv3d", 32, 32, 3, 1, 1), 8, W, 4), BC.Part(L("hb", "conv3d", 32, 32, 3, 1, 1), 8)],
    "staged-to-d2s": list(_PAIRS["staged->d2s"][1:3]),
}


# ---------------------------------------------------------------- s3r_encoder_forward, _u8, s3r_decoder_forward (B = 1)
def _stage_descs(layers, n0, batch, dtype):
    arr = (s3r._lib.Layer * len(layers))()
    for i, (l, n, _) in enumerate(spec.trace(layers, n0)):
        arr[i].desc = s3r._lib.make_desc(l, batch, n, tag=i, dtype=dtype)
    return arr, len(layers)


def _encoder(precision, u8):
    bf = precision == "bf16"

    def make(lib, dev):
        B = 1
        if dev is None:
            mod, (arr, n) = None, _stage_descs(spec.ENCODER, spec.IMG_HW, 2 * B, s3r._lib.DTYPE[precision])
        else:
            mod = s3r.Encoder(precision=precision)
            s3r.seed_module(mod, 3)
            mod.to(dev)
            arr, n = mod._layer_array(2 * B, torch.device(dev))
        need = lib.s3r_chain_workspace_elems(arr, n)
        assert need > 0, lib.s3r_last_error()
        ishape = (B, 3, spec.IMG_HW, spec.IMG_HW)
        fshape = (2 * B, spec.FEAT_HW, spec.FEAT_HW, spec.FEAT_C) if bf else (2 * B, spec.FEAT_C, spec.FEAT_HW, spec.FEAT_HW)
        args = [Arg("left", ishape, U8 if u8 else F32, "in"), Arg("right", ishape, U8 if u8 else F32, "in"),
                Arg("features", fshape, BF16 if bf else F32, "out"), Arg("ws", (need,), F32, "scr")]
        fn = lib.s3r_encoder_forward_u8 if u8 else lib.s3r_encoder_forward

        def data(k):
            g = torch.Generator().manual_seed(7 + k)
            l8, r8 = (torch.randint(0, 256, ishape, generator=g, dtype=U8) for _ in range(2))
            lf, rf = l8.float() / 255.0, r8.float() / 255.0
            return {"left": l8 if u8 else lf, "right": r8 if u8 else rf, "_ref": (lf, rf)}

        def call(ptr, st):
            return fn(arr, n, ptr["left"], ptr["right"], ptr["features"], ptr["ws"], need, 1, st)

        def check(d, res):                                         # the module on the same renders (tests/_abi_bodies.py::encoder_forward):
            # the module calls this entry itself, so this pins the layout and the call, not the values (tests/test_parity_gpu.py does)
            lf, rf = d["_ref"]
            want = mod.forward_pair(lf.to(dev), rf.to(dev)).cpu()
            got = res["features"].permute(0, 3, 1, 2) if bf else res["features"]
            assert torch.equal(got.float(), want.float()), "the entry differs from the module on the same renders"

        return Plan(args, data, call, check, keep=(mod, arr))

    return make


def _decoder(precision):
    bf = precision == "bf16"

    def make(lib, dev):
        B = 1
        if dev is None:
            mod, (arr, n) = None, _stage_descs(spec.DECODER, spec.MAX_DISP, B, s3r._lib.DTYPE[precision])
        else:
            mod = s3r.Decoder(precision=precision)
            s3r.seed_module(mod, 4)
            mod.to(dev)
            arr, n = mod._layer_array(B, torch.device(dev))
        need = lib.s3r_chain_workspace_elems(arr, n)
        assert need > 0, lib.s3r_last_error()
        Cc, D, H = 2 * spec.FEAT_C, spec.MAX_DISP, spec.FEAT_HW
        vshape = (B, D, H, H, Cc) if bf else (B, Cc, D, H, H)
        args = [Arg("volume", vshape, BF16 if bf else F32, "in"), Arg("occupancy", (B, 1, spec.VOX, spec.VOX, spec.VOX), F32, "out"),
                Arg("ws", (need,), F32, "scr")]

        def data(k):
            vol = torch.randn((B, Cc, D, H, H), generator=torch.Generator().manual_seed(11 + k))
            if bf:
                vol = vol.to(BF16)
                return {"volume": vol.permute(0, 2, 3, 4, 1).contiguous(), "_ref": vol}
            return {"volume": vol, "_ref": vol}

        def call(ptr, st):
            return lib.s3r_decoder_forward(arr, n, ptr["volume"], ptr["occupancy"], ptr["ws"], need, 1, st)

        def check(d, res):                                         # the module on the same volume (tests/_abi_bodies.py::decoder_forward):
            # not an independent reference either, as for the encoder
            vol = d["_ref"].to(dev)
            want = mod(vol.permute(0, 2, 3, 4, 1).contiguous().permute(0, 4, 1, 2, 3) if bf else vol).cpu()
            assert torch.equal(res["occupancy"].reshape(want.shape), want), "the entry differs from the module on the same volume"

        return Plan(args, data, call, check, keep=(mod, arr))

    return make


# ---------------------------------------------------------------- hand-off, cost volume
def _cl_to_f32(lib, dev):
    B, Cc, P = 2, 32, 100
    args = [Arg("x", (B, P, Cc), BF16, "in"), Arg("y", (B, Cc, P), F32, "out")]

    def data(k):
        return {"x": torch.randn(B, P, Cc, generator=torch.Generator().manual_seed(3 + k)).to(BF16)}

    return Plan(args, data, lambda ptr, st: lib.s3r_channels_last_to_f32(ptr["x"], ptr["y"], B, Cc, P, st),
                lambda d, res: _same(_np(res["y"]), _np(d["x"].float().permute(0, 2, 1).contiguous()), "channels_last_to_f32"))


CV_SHAPE = (2, 8, 8, 8, 12)                                        # B, C, D, H, W


def _cost_volume(kind):
    B, Cc, D, H, Wd = CV_SHAPE

    def make(lib, dev):
        from oracle import s2v_oracle as O
        bf = kind == "bf16"
        fshape = (B, H, Wd, Cc) if bf else (B, Cc, H, Wd)
        if kind == "plain":
            out, fn = Arg("volume", (B, 2 * Cc, D, H, Wd), F32, "out"), lib.s3r_cost_volume_forward
        elif bf:
            out, fn = Arg("volume", (B, D, H, Wd, 2 * Cc), BF16, "out"), lib.s3r_cost_volume_forward_bf16
        elif kind == "wino":                                        # the caller zeroes the planes: the depth-halo planes are never written
            out, fn = Arg("volume", (6 * B * 2 * Cc * (D + 2) * (H // 4) * (Wd + 2),), F32, "zero"), lib.s3r_cost_volume_forward_wino
        else:
            out, fn = Arg("volume", (36 * B * 2 * Cc * (D // 4) * (H // 4) * (Wd + 2),), F32, "zero"), lib.s3r_cost_volume_forward_wino2
        args = [Arg("left", fshape, BF16 if bf else F32, "in"), Arg("right", fshape, BF16 if bf else F32, "in"), out]

        def data(k):
            g = torch.Generator().manual_seed(11 + k)
            fl, fr = torch.randn(B, Cc, H, Wd, generator=g), torch.randn(B, Cc, H, Wd, generator=g)
            if bf:
                fl, fr = fl.to(BF16), fr.to(BF16)
                return {"left": fl.permute(0, 2, 3, 1).contiguous(), "right": fr.permute(0, 2, 3, 1).contiguous(), "_ref": (fl.float(), fr.float())}
            return {"left": fl, "right": fr, "_ref": (fl, fr)}

        def call(ptr, st):
            if kind in ("plain", "bf16"):
                return fn(ptr["left"], ptr["right"], ptr["volume"], B, Cc, D, H, Wd, 0, st)
            return fn(ptr["left"], ptr["right"], ptr["volume"], B, Cc, D, H, Wd, st)

        def check(d, res):
            fl, fr = d["_ref"]
            want = O.cost_volume(fl, fr, D)
            if kind == "plain":
                assert torch.equal(res["volume"], want)
            elif bf:
                assert torch.equal(res["volume"].permute(0, 4, 1, 2, 3), want.to(BF16))
            # (the plane layouts' existing reference, tests/_abi_bodies.py::cost_volume_planes, is the same call into a plain zeroed
            # buffer, which is the NULL-stream run every case is compared with; their values are pinned by tests/test_exact_gpu.py)

        return Plan(args, data, call, check)

    return make


# ---------------------------------------------------------------- linear forward / backward
def _linear_forward(shape, act):
    B, cin, cout = shape
    l = L("t", "linear", cin, cout, 1, 1, 0, False, act)

    def make(lib, dev):
        need = lib.s3r_linear_scratch_elems(B, cin, cout)
        args = [Arg("x", (B, cin), F32, "in"), Arg("w", (cout, cin), F32, "in"), Arg("bias", (cout,), F32, "in"), Arg("y", (B, cout), F32, "out"),
                Arg("scratch", (need,), F32, "scr")]

        def data(k):
            p = R.make_params(l, cin + cout + k)
            x = torch.randn(B, cin, generator=torch.Generator().manual_seed(B + k))
            return {"x": x, "w": p["w"], "bias": p["shift"], "_ref": p}

        def call(ptr, st):
            return lib.s3r_linear_forward(ptr["x"], ptr["w"], ptr["bias"], ptr["y"], B, cin, cout, s3r._lib.ACT[act], ptr["scratch"], need, st)

        def check(d, res):
            ref, mag = R.ref64(l, d["x"], d["_ref"])
            _within(res["y"], ref, R.bound(l, ref, mag, "direct"), shape)

        return Plan(args, data, call, check)

    return make


def _linear_backward(shape, act, outs=("grad_x", "grad_w", "grad_bias")):
    B, cin, cout = shape

    def make(lib, dev):
        need = lib.s3r_linear_backward_scratch_elems(B, cin, cout)
        oshape = {"grad_x": (B, cin), "grad_w": (cout, cin), "grad_bias": (cout,)}
        args = [Arg("x", (B, cin), F32, "in"), Arg("w", (cout, cin), F32, "in"), Arg("y", (B, cout), F32, "in"), Arg("grad_y", (B, cout), F32, "in")]
        args += [Arg(o, oshape[o], F32, "out") for o in outs] + [Arg("scratch", (need,), F32, "scr")]

        def data(k):
            rng = np.random.default_rng(shape[1] + k)
            x = rng.standard_normal((B, cin)).astype(np.float32)
            w = (rng.standard_normal((cout, cin)) / np.sqrt(cin)).astype(np.float32)
            y = L64.forward32(x, w, 0.1 * rng.standard_normal(cout), act)
            gy = rng.standard_normal((B, cout)).astype(np.float32)
            return {"x": _t(x), "w": _t(w), "y": _t(y), "grad_y": _t(gy)}

        def _call(ptr, st, elems):
            return lib.s3r_linear_backward(ptr["x"], ptr["w"], ptr["y"], ptr["grad_y"], ptr.get("grad_x"), ptr.get("grad_w"), ptr.get("grad_bias"),
                                           B, cin, cout, s3r._lib.ACT[act], ptr["scratch"], elems, st)

        def check(d, res):
            x, w, y, gy = (_np(d[n]) for n in ("x", "w", "y", "grad_y"))
            g = L64.g32(y, gy, act)
            (gw, kw, mw), (gx, kx, mx) = L64.backward64(x, w, g)
            if "grad_bias" in res:
                _same(_np(res["grad_bias"]), L64.grad_bias32(g), "grad_bias")
            if "grad_w" in res:
                _within_np(_np(res["grad_w"]), gw, L64.bound32(kw, mw), "grad_w")
            if "grad_x" in res:
                _within_np(_np(res["grad_x"]), gx, L64.bound32(kx, mx), "grad_x")

        return Plan(args, data, lambda ptr, st: _call(ptr, st, need), check,
                    refuse=lambda ptr, st: (_call(ptr, st, need - 1), -3))       # a scratch one element short: S3R_ERR_WORKSPACE

    return make


# ---------------------------------------------------------------- Chamfer, IoU
CH = (2, 300, 257)


def _chamfer_clouds(k):
    B, N, M = CH
    g = torch.Generator().manual_seed(N * 7 + M + k)
    return torch.rand(B, N, 3, generator=g), torch.rand(B, M, 3, generator=g)


def _chamfer_forward(lib, dev):
    B, N, M = CH
    args = [Arg("p", (B, N, 3), F32, "in"), Arg("q", (B, M, 3), F32, "in"), Arg("dist1", (B, N), F32, "out"), Arg("dist2", (B, M), F32, "out"),
            Arg("idx1", (B, N), I32, "out"), Arg("idx2", (B, M), I32, "out")]

    def data(k):
        p, q = _chamfer_clouds(k)
        return {"p": p, "q": q}

    def check(d, res):
        for name, want in zip(("dist1", "dist2", "idx1", "idx2"), SR.chamfer_scan(_np(d["p"]), _np(d["q"]))):
            _same(_np(res[name]), want, name)

    return Plan(args, data, lambda ptr, st: lib.s3r_chamfer_forward(ptr["p"], ptr["q"], ptr["dist1"], ptr["dist2"], ptr["idx1"], ptr["idx2"],
                                                                   B, N, M, st), check)


def _chamfer_backward(lib, dev):
    B, N, M = CH
    args = [Arg("p", (B, N, 3), F32, "in"), Arg("q", (B, M, 3), F32, "in"), Arg("idx1", (B, N), I32, "in"), Arg("idx2", (B, M), I32, "in"),
            Arg("grad_dist1", (B, N), F32, "in"), Arg("grad_dist2", (B, M), F32, "in"), Arg("grad_p", (B, N, 3), F32, "out"),
            Arg("grad_q", (B, M, 3), F32, "out")]

    def data(k):
        p, q = _chamfer_clouds(k)
        _, _, i1, i2 = SR.chamfer_scan(_np(p), _np(q))
        g = torch.Generator().manual_seed(91 + k)
        return {"p": p, "q": q, "idx1": _t(i1), "idx2": _t(i2), "grad_dist1": torch.randn(B, N, generator=g), "grad_dist2": torch.randn(B, M, generator=g)}

    def _call(ptr, st, g1, g2):
        return lib.s3r_chamfer_backward(ptr["p"], ptr["q"], ptr["idx1"], ptr["idx2"], g1, g2, ptr["grad_p"], ptr["grad_q"], B, N, M, st)

    def check(d, res):
        gp, gq = C64.backward32(*(_np(d[n]) for n in ("p", "q", "idx1", "idx2", "grad_dist1", "grad_dist2")))
        _same(_np(res["grad_p"]), gp, "grad_p")
        _same(_np(res["grad_q"]), gq, "grad_q")

    return Plan(args, data, lambda ptr, st: _call(ptr, st, ptr["grad_dist1"], ptr["grad_dist2"]), check,
                refuse=lambda ptr, st: (_call(ptr, st, None, None), -1))         # both grad_dist NULL: S3R_ERR_INVALID


def _voxel_iou(lib, dev):
    B, V = 3, 2500
    args = [Arg("pred", (B, V), F32, "in"), Arg("gt", (B, V), F32, "in"), Arg("iou", (B,), F32, "out")]

    def data(k):
        g = torch.Generator().manual_seed(V + k)
        return {"pred": torch.rand(B, V, generator=g), "gt": torch.rand(B, V, generator=g)}

    return Plan(args, data, lambda ptr, st: lib.s3r_voxel_iou(ptr["pred"], ptr["gt"], 0.5, ptr["iou"], B, V, st),
                lambda d, res: _same(_np(res["iou"]), SR.iou_ref(_np(d["pred"]), _np(d["gt"]), 0.5), "iou"))


# ---------------------------------------------------------------- voxel BCE (B 3, V 2500: three chunks, the last short)
BCE = (3, 2500)


def _bce_data(k):
    B, V = BCE
    g = torch.Generator().manual_seed(V + 13 * k)
    pred = torch.rand(B, V, generator=g).clamp(1e-4, 1 - 1e-4)
    target = (torch.rand(B, V, generator=g) > 0.6).float()
    target[:, ::7] = torch.rand(B, len(range(0, V, 7)), generator=g)           # some soft targets
    return pred, target


def _bce_forward(lib, dev):
    B, V = BCE
    args = [Arg("pred", (B, V), F32, "in"), Arg("target", (B, V), F32, "in"), Arg("loss_sum", (B,), F32, "out"), Arg("loss_elem", (B, V), F32, "out")]

    def data(k):
        p, t = _bce_data(k)
        return {"pred": p, "target": t}

    def _call(ptr, st, v):
        return lib.s3r_voxel_bce_forward(ptr["pred"], ptr["target"], ptr["loss_sum"], ptr["loss_elem"], B, v, st)

    def check(d, res):
        p, t, le = _np(d["pred"]), _np(d["target"]), _np(res["loss_elem"])
        _within_np(le, B64.loss_elem64(p, t), B64.elem_bound(p, t), "loss_elem")
        _same(_np(res["loss_sum"]), np.array([B64.sum_order32(le[b]) for b in range(B)], np.float32), "loss_sum")

    return Plan(args, data, lambda ptr, st: _call(ptr, st, V), check, refuse=lambda ptr, st: (_call(ptr, st, 0), -1))   # voxels = 0: S3R_ERR_INVALID


def _bce_backward(lib, dev):
    B, V = BCE
    args = [Arg("pred", (B, V), F32, "in"), Arg("target", (B, V), F32, "in"), Arg("grad_scale", (B,), F32, "in"), Arg("grad_pred", (B, V), F32, "out")]

    def data(k):
        p, t = _bce_data(k)
        return {"pred": p, "target": t, "grad_scale": torch.randn(B, generator=torch.Generator().manual_seed(k)) / V}

    def _call(ptr, st, v):
        return lib.s3r_voxel_bce_backward(ptr["pred"], ptr["target"], ptr["grad_scale"], ptr["grad_pred"], B, v, st)

    return Plan(args, data, lambda ptr, st: _call(ptr, st, V),
                lambda d, res: _same(_np(res["grad_pred"]), B64.grad32(_np(d["pred"]), _np(d["target"]), _np(d["grad_scale"])), "grad_pred"),
                refuse=lambda ptr, st: (_call(ptr, st, 0), -1))


# ---------------------------------------------------------------- head backward (B 2, C 64, S 1100: three chunks)
def _head_backward(outs):
    B, Cc, S, act = 2, 64, 1100, "sigmoid"

    def make(lib, dev):
        need = lib.s3r_head_backward_scratch_elems(B, Cc, S)
        oshape = {"grad_x": (B, Cc, S), "grad_w": (Cc,), "grad_shift": (1,)}
        args = [Arg("x", (B, Cc, S), F32, "in"), Arg("w", (Cc,), F32, "in"), Arg("scale", (1,), F32, "in"), Arg("y", (B, S), F32, "in"),
                Arg("grad_y", (B, S), F32, "in")] + [Arg(o, oshape[o], F32, "out") for o in outs] + [Arg("scratch", (need,), F32, "scr")]

        def data(k):
            rng = np.random.default_rng(S + k)
            x = rng.standard_normal((B, Cc, S)).astype(np.float32)
            w = (rng.standard_normal(Cc) / 8).astype(np.float32)
            scale = np.array([1.25 + k], np.float32)
            y = H64.forward64(x, w, 0.1, act, scale[0])[0].astype(np.float32)
            gy = rng.standard_normal((B, S)).astype(np.float32)
            return {"x": _t(x), "w": _t(w), "scale": _t(scale), "y": _t(y), "grad_y": _t(gy)}

        def _call(ptr, st, elems):
            return lib.s3r_head_backward(ptr["x"], ptr["w"], ptr["scale"], ptr["y"], ptr["grad_y"], ptr.get("grad_x"), ptr.get("grad_w"),
                                         ptr.get("grad_shift"), B, Cc, S, s3r._lib.ACT[act], ptr["scratch"], elems, st)

        def check(d, res):
            x, w, scale, y, gy = (_np(d[n]) for n in ("x", "w", "scale", "y", "grad_y"))
            g = H64.g32(y, gy, act)
            gs = H64.gs32(g, scale[0])
            if "grad_x" in res:
                _same(_np(res["grad_x"]), H64.grad_x32(gs, w), "grad_x")
            if "grad_w" in res:
                _same(_np(res["grad_w"]), H64.grad_w32(gs, x), "grad_w")
            if "grad_shift" in res:
                _same(_np(res["grad_shift"]), np.asarray(H64.grad_shift32(g), np.float32).reshape(1), "grad_shift")

        return Plan(args, data, lambda ptr, st: _call(ptr, st, need), check, refuse=lambda ptr, st: (_call(ptr, st, need - 1), -3))

    return make


# ---------------------------------------------------------------- disparity read-outs and metrics
DSHAPE = (2, 16, 8, 20, 6)                                         # B, C, H, W, max_disp


def _disp_feats(k, bf=False):
    B, Cc, H, Wd, _ = DSHAPE
    g = torch.Generator().manual_seed(Wd + k)
    fl, fr = torch.randn(B, Cc, H, Wd, generator=g), torch.randn(B, Cc, H, Wd, generator=g)
    return (fl.to(BF16), fr.to(BF16)) if bf else (fl, fr)


def _disparity_wta(lib, dev):
    from oracle import s2v_oracle as O
    B, Cc, H, Wd, D = DSHAPE
    args = [Arg("left", (B, Cc, H, Wd), F32, "in"), Arg("right", (B, Cc, H, Wd), F32, "in"), Arg("disp_l", (B, H, Wd), F32, "out"),
            Arg("disp_r", (B, H, Wd), F32, "out")]

    def data(k):
        fl, fr = _disp_feats(k)
        return {"left": fl, "right": fr}

    def check(d, res):
        want = O.disparity_wta(d["left"], d["right"], D)
        assert torch.equal(res["disp_l"], want[0]) and torch.equal(res["disp_r"], want[1])

    return Plan(args, data, lambda ptr, st: lib.s3r_disparity_wta(ptr["left"], ptr["right"], ptr["disp_l"], ptr["disp_r"], B, Cc, H, Wd, D, st), check)


def _disparity_soft(bf):
    B, Cc, H, Wd, D = DSHAPE
    TAU = 0.7

    def make(lib, dev):
        fshape = (B, H, Wd, Cc) if bf else (B, Cc, H, Wd)
        names = ("disp_l", "disp_r", "conf_l", "conf_r")
        args = [Arg("left", fshape, BF16 if bf else F32, "in"), Arg("right", fshape, BF16 if bf else F32, "in")] + \
               [Arg(n, (B, H, Wd), F32, "out") for n in names]

        def data(k):
            fl, fr = _disp_feats(k, bf)
            if bf:
                return {"left": fl.permute(0, 2, 3, 1).contiguous(), "right": fr.permute(0, 2, 3, 1).contiguous(), "_ref": (fl.float(), fr.float())}
            return {"left": fl, "right": fr, "_ref": (fl, fr)}

        def call(ptr, st):
            return lib.s3r_disparity_soft(ptr["left"], ptr["right"], 1 if bf else 0, *(ptr[n] for n in names), B, Cc, H, Wd, D, TAU, H, Wd, 1.0, st)

        def check(d, res):                                         # tests/test_disparity_soft_gpu.py::test_feature_resolution_matches_fp64
            fl, fr = d["_ref"]
            (wl, wr), (ql, qr) = D64.soft(_np(fl), _np(fr), D, TAU)
            for n, want in (("disp_l", wl), ("disp_r", wr)):
                assert np.abs(_np(res[n]).astype(np.float64) - want).max() <= 2e-5 * D, n
            for n, want in (("conf_l", ql), ("conf_r", qr)):
                assert (np.abs(_np(res[n]).astype(np.float64) - want) / want).max() <= 1e-5, n

        return Plan(args, data, call, check)

    return make


def _disparity_epe(lib, dev):
    from oracle import s2v_oracle as O
    B, P = 3, 1000
    args = [Arg("pred", (B, P), F32, "in"), Arg("gt", (B, P), F32, "in"), Arg("epe", (B,), F32, "out"), Arg("count", (B,), I32, "out")]

    def data(k):
        g = torch.Generator().manual_seed(P + k)
        pred, gt = torch.rand(B, P, generator=g) * 200, torch.rand(B, P, generator=g) * 200
        gt[:, ::3] = float("inf")
        gt[:, 1::5] = -1.0
        return {"pred": pred, "gt": gt}

    def check(d, res):
        want_e, want_n = O.disparity_epe(d["pred"], d["gt"])
        assert torch.equal(res["count"], want_n)
        assert (res["epe"] - want_e).abs().max().item() <= 1e-6 * want_e.abs().max().item()

    return Plan(args, data, lambda ptr, st: lib.s3r_disparity_epe(ptr["pred"], ptr["gt"], ptr["epe"], ptr["count"], B, P, st), check)


def _disparity_metrics(lib, dev):
    B, P = 5, 1000
    args = [Arg("pred", (B, P), F32, "in"), Arg("gt", (B, P), F32, "in"), Arg("epe", (B,), F32, "out"), Arg("counts", (B, 4), I32, "out")]

    def data(k):
        from tests._abi_bodies import metric_case
        pred, gt = metric_case(B, P)
        return {"pred": pred + k, "gt": gt}

    def check(d, res):
        want_e, want_c = D64.metrics(_np(d["pred"]), _np(d["gt"]))
        assert np.array_equal(_np(res["counts"]), want_c)
        assert (np.abs(_np(res["epe"]).astype(np.float64) - want_e) <= 1e-6 * want_e.max()).all()

    return Plan(args, data, lambda ptr, st: lib.s3r_disparity_metrics(ptr["pred"], ptr["gt"], ptr["epe"], ptr["counts"], B, P, st), check)


# ---------------------------------------------------------------- the table
_CONV_E = ("s3r_conv_pack_weights", "s3r_conv_forward")
CASES = [Case(f"conv:{c.id}", _CONV_E, "conv", _conv(c), mutant=c.id.startswith("splitk2")) for c in CONV]
# the two-axis Conv2d at its largest edge; with out_halo 3 its padded plane (130^2 floats) passes the finish kernel's 64 KiB of LDS:
# refused when the algorithm is resolved (include/s3r.h, s3r_algo) — the launcher used to refuse it behind an enqueued input transform
CONV_AT_THE_LDS_LIMIT = "conv:wino2-conv2d-32to2-e124"
CASES.append(Case(CONV_AT_THE_LDS_LIMIT, _CONV_E, "conv",
                  _conv(_CC("wino2-conv2d-32to2-e124", L("t", "conv2d", 32, 2, 3, 1, 1), 124, 1, algo=W, tile=3), refused_out_halo=3)))
CASES += [Case(f"chain:{n}", ("s3r_chain_forward",), "chain", _chain(n, parts), mutant=n.startswith("handoff")) for n, parts in CHAINS.items()]
CASES += [
    Case("encoder:fp32", ("s3r_encoder_forward",), "stage", _encoder("fp32", False)),
    Case("encoder:bf16", ("s3r_encoder_forward",), "stage", _encoder("bf16", False)),
    Case("encoder_u8:fp32", ("s3r_encoder_forward_u8",), "stage", _encoder("fp32", True)),
    Case("encoder_u8:bf16", ("s3r_encoder_forward_u8",), "stage", _encoder("bf16", True)),
    Case("decoder:fp32", ("s3r_decoder_forward",), "stage", _decoder("fp32")),
    Case("decoder:bf16", ("s3r_decoder_forward",), "stage", _decoder("bf16")),
    Case("channels_last_to_f32", ("s3r_channels_last_to_f32",), "pointwise", _cl_to_f32),
    Case("cost_volume:plain", ("s3r_cost_volume_forward",), "cost_volume", _cost_volume("plain")),
    Case("cost_volume:wino", ("s3r_cost_volume_forward_wino",), "cost_volume", _cost_volume("wino")),
    Case("cost_volume:wino2", ("s3r_cost_volume_forward_wino2",), "cost_volume", _cost_volume("wino2")),
    Case("cost_volume:bf16", ("s3r_cost_volume_forward_bf16",), "cost_volume", _cost_volume("bf16")),
    Case("linear_forward:3x50x7-relu", ("s3r_linear_forward",), "linear", _linear_forward((3, 50, 7), "relu")),
    Case("linear_forward:splitk-5x1024x6144", ("s3r_linear_forward",), "linear", _linear_forward((5, 1024, 6144), "none")),
    Case("linear_forward:elu-pass-4x50x7", _CONV_E, "linear", _conv(_CC("linear-elu-4x50x7", L("t", "linear", 50, 7, 1, 1, 0, False, "elu"), 1, 4))),
    Case("linear_backward:3x96x40-sigmoid", ("s3r_linear_backward",), "linear_backward", _linear_backward((3, 96, 40), "sigmoid"), mutant=True),
    # grad_x in two K slices: s3r_linear_bwd.hip cuts Cout into whole 128-o chunks, so Cout = 129 is the smallest with two
    Case("linear_backward:2x33x129-relu-two-slices", ("s3r_linear_backward",), "linear_backward", _linear_backward((2, 33, 129), "relu")),
    Case("linear_backward:3x96x40-grad_w-only", ("s3r_linear_backward",), "linear_backward", _linear_backward((3, 96, 40), "relu", ("grad_w",))),
    Case("chamfer_forward", ("s3r_chamfer_forward",), "chamfer", _chamfer_forward),
    Case("chamfer_backward", ("s3r_chamfer_backward",), "chamfer", _chamfer_backward, mutant=True),
    Case("voxel_iou", ("s3r_voxel_iou",), "iou", _voxel_iou),
    Case("voxel_bce_forward", ("s3r_voxel_bce_forward",), "bce", _bce_forward, mutant=True),
    Case("voxel_bce_backward", ("s3r_voxel_bce_backward",), "bce", _bce_backward),
    Case("head_backward:all", ("s3r_head_backward",), "head_backward", _head_backward(("grad_x", "grad_w", "grad_shift")), mutant=True),
    Case("head_backward:grad_x-only", ("s3r_head_backward",), "head_backward", _head_backward(("grad_x",))),
    Case("disparity_wta", ("s3r_disparity_wta",), "disparity", _disparity_wta),
    Case("disparity_epe", ("s3r_disparity_epe",), "disparity", _disparity_epe),
    Case("disparity_soft:fp32", ("s3r_disparity_soft",), "disparity", _disparity_soft(False), mutant=True),
    Case("disparity_soft:bf16", ("s3r_disparity_soft",), "disparity", _disparity_soft(True)),
    Case("disparity_metrics", ("s3r_disparity_metrics",), "disparity", _disparity_metrics),
]
BY_ID = {c.id: c for c in CASES}
# both instruments run the whole table (tests/test_streams_gpu.py parametrises over these lists)
INSTRUMENTS = {"delayed_producer": CASES, "capture_replay": CASES}
MUTANTS = [c for c in CASES if c.mutant]
REFUSALS = [c for c in CASES if c.entries[0] in TRAINING and c.id in (
    "linear_backward:3x96x40-sigmoid", "chamfer_backward", "voxel_bce_forward", "voxel_bce_backward", "head_backward:all")]
REFUSALS.append(BY_ID[CONV_AT_THE_LDS_LIMIT])
