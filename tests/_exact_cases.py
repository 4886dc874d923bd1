"""The cases of tests/test_exact_gpu.py, shared with the harness's self-test in tests/test_exact_cpu.py.

A case is a descriptor (layer, size, batch, dtype, tile, split-K, algo, halos) plus the recipe of its lattice data (`data`: what
tests/_lattice.py::lattice_case takes).  Cases that differ only in HOW the layer is launched share their data, and with it the
reference and the CPU self-test.
"""
from __future__ import annotations

import dataclasses
import math
from dataclasses import dataclass

import s3r
import torch
from s3r import arch_spec as spec

from tests import _buffer_cases as BC
from tests import _lattice as LT
from tests import _linear_cases as LC
from tests import _ref64 as R

L = spec.Layer
DIRECT, WINO = s3r.ALGO_DIRECT, s3r.ALGO_WINOGRAD


@dataclass(frozen=True)
class Data:
    layer: L
    B: int
    n_in: int
    seed: int
    form: str = "direct"
    xmax: int = 2
    wmax: int = 1
    density: float = 1.0
    dtype: str = "fp32"
    xdensity: float = 1.0
    ep: str = "ss"             # the epilogue's vector form (tests/_lattice.py::lattice_case): "0s" scale NULL, "s0" shift NULL, "00" both

    def make(self):
        return LT.lattice_case(self.layer, self.B, self.n_in, self.seed, self.form, self.xmax, self.wmax, self.density, self.xdensity,
                               self.ep)

    @property
    def bf16_out(self):
        return self.dtype == "bf16" and not BC._head(self.layer, self.n_in)

    @property
    def id(self):
        l = self.layer
        return (f"{l.name}-{l.op}-{l.cin}to{l.cout}-k{l.k}s{l.s}p{l.p}d{l.dil}o{l.opad}-{l.act}{l.act_param or ''}-e{self.n_in}-B{self.B}-"
                f"{self.dtype}-{self.form}-x{self.xmax}w{self.wmax}-s{self.seed}" + ("" if self.ep == "ss" else f"-ep{self.ep}"))


@dataclass(frozen=True)
class XCase:
    id: str
    data: Data
    tile: int = -1
    ksplit: int = 0
    algo: int = 0
    in_halo: int = -1          # -1: what the layer's kernel needs
    out_halo: int = 0
    refused: bool = False      # the library refuses this configuration: asserted refused, never launched
    twice: bool = False        # also run over zero-filled scratch (descriptors tests/test_buffers_gpu.py does not run)
    ran: tuple = ()            # the profiler record's `ran` must be one of these (s3r._lib.RAN); (): not asserted

    layer = property(lambda self: self.data.layer)
    n_in = property(lambda self: self.data.n_in)
    B = property(lambda self: self.data.B)
    dtype = property(lambda self: self.data.dtype)


def network():
    rows = []
    for layers, n0 in ((spec.ENCODER, spec.IMG_HW), (spec.DECODER, spec.MAX_DISP)):
        rows += [(l, n) for l, n, _ in spec.trace(layers, n0)]
    return rows


def _bf16_data(layer, B, n_in, seed):
    a, b = LT.bf16_magnitudes(R.k_terms(layer))
    return Data(layer, B, n_in, seed, xmax=a, wmax=b, dtype="bf16")


# ---------------------------------------------------------------- direct fp32
def _direct_fp32():
    cases = []
    # all 18 network layers at their own sizes; the head with act none and ReLU (its sigmoid cannot be exact)
    for i, (l, n) in enumerate(network()):
        variants = [l] if l.act != "sigmoid" else [dataclasses.replace(l, act="none"), dataclasses.replace(l, act="relu")]
        for lv in variants:
            for B in (1, 3):
                cases.append(XCase(f"{lv.name}-{lv.act}-B{B}", Data(lv, B, n, 100 + i), algo=DIRECT))
    # tests/test_parity_gpu.py::test_every_tile_configuration: nine shapes x 8 tiles x both gather widths
    for kind, (l, n, B, _) in {
        "conv3d_s1": (L("t", "conv3d", 32, 96, 3, 1, 1), 7, 3, 0),
        "conv3d_s1_w8": (L("t", "conv3d", 32, 96, 3, 1, 1), 8, 3, 0),
        "conv3d_s2": (L("t", "conv3d", 16, 160, 3, 2, 1), 9, 2, 0),
        "deconv": (L("t", "deconv3d", 32, 48, 4, 2, 1), 5, 3, 0),
        "deconv_w4": (L("t", "deconv3d", 32, 48, 4, 2, 1), 4, 3, 0),
        "conv2d_s2": (L("t", "conv2d", 48, 64, 3, 2, 1), 13, 5, 0),
        "conv2d_s1_w12": (L("t", "conv2d", 48, 64, 3, 1, 1), 12, 5, 0),
        "conv3d_k4_valid": (L("t", "conv3d", 16, 40, 4, 1, 0), 7, 2, 0),
    }.items():
        d = Data(l, B, n, 200)
        out_w = n if l.op == "deconv3d" else spec.out_size(l, n)
        for vec in (0, 1):
            dword = vec == 1 or (l.op != "deconv3d" and l.s != 1) or out_w % 4 != 0
            for tile in range(8):
                # (the 64 x 512 tile is wider than one dword-gather row piece allows: refused, as that test expects)
                cases.append(XCase(f"tile{tile}-vec{vec}-{kind}", d, tile=tile + 16 * vec, algo=DIRECT, refused=tile == 5 and dword, twice=True))
    # tests/test_parity_gpu.py::test_split_k's shapes (their sigmoid replaced), and v5, v6, d1 at network size under forced split-K
    for kind, (l, n, B) in {
        "conv3d_k4_valid": (L("t", "conv3d", 64, 40, 4, 1, 0), 7, 3),
        "deconv": (L("t", "deconv3d", 64, 48, 4, 2, 1), 5, 3),
        "conv3d_s2": (L("t", "conv3d", 128, 160, 3, 2, 1, bn=False, act="none"), 9, 2),
    }.items():
        for ks in (1, 2, 4):
            cases.append(XCase(f"splitk{ks}-{kind}", Data(l, B, n, 300), ksplit=ks, algo=DIRECT, twice=True))
    net = dict((l.name, (l, n)) for l, n in network())
    for name in ("v5", "v6", "d1"):
        l, n = net[name]
        for ks in (1, 2, 4, 8, 16):                    # cin / 16 >= 16 chunks: every power of two up to 16 divides them
            cases.append(XCase(f"splitk{ks}-{name}-network", Data(l, 1, n, 310), ksplit=ks, algo=DIRECT, twice=True))
    # the general-layer families of tests/_buffer_cases.py with an exact activation substituted
    for c in BC.CONV_CASES:
        fam = c.id.split("-")[0]
        if c.dtype != "fp32" or fam not in ("general", "staged", "tclass", "unfolded", "d2s", "dilated", "leaky", "tanh", "elu", "head"):
            continue
        l = LT.exact_act(c.layer)
        # (with its Tanh replaced, AUTO would pick a Winograd form for that layer, and this data is on the direct lattice)
        algo = DIRECT if BC.has_wino(dataclasses.replace(c, layer=l)) else c.algo
        cases.append(XCase("g-" + c.id, Data(l, c.B, c.n_in, 400), tile=c.tile, ksplit=c.ksplit, algo=algo, in_halo=c.in_halo,
                           out_halo=c.out_halo))
    # LeakyReLU: slope 1/2 fused in the split-K finish and in the direct kernel's own epilogue, slope 2 (> 1: the separate pass) behind a direct and a staged layer
    cases += [
        XCase("leaky-half-splitk2-finish", Data(L("t", "conv3d", 64, 32, 3, 2, 1, True, "leaky_relu", 1, 0, 0.5), 2, 9, 410), ksplit=2, twice=True),
        XCase("leaky-half-fused-epilogue", Data(L("t", "conv3d", 32, 32, 3, 1, 1, True, "leaky_relu", 1, 0, 0.5), 2, 8, 413), ksplit=1, algo=DIRECT,
              twice=True),
        XCase("leaky-2-pass-conv3d", Data(L("t", "conv3d", 32, 32, 3, 1, 1, True, "leaky_relu", 1, 0, 2.0), 2, 8, 411), algo=DIRECT, twice=True),
        XCase("leaky-2-pass-staged-conv2d", Data(L("t", "conv2d", 20, 33, 5, 1, 2, True, "leaky_relu", 1, 0, 2.0), 2, 9, 412), twice=True),
    ]
    return cases


DIRECT_CASES = _direct_fp32()

# ---------------------------------------------------------------- linear
LIN_SHAPES = [(32, 8192, 1024), (5, 1024, 6144), (33, 96, 40), (3, 50, 7), (70, 4096, 100), (4, 1, 9), (3, 7, 1), (2, 64, 7),
              (7, 7, 7), (1, 256, 1), (32, 32768, 1024)]


def _linear():
    out = []
    for B, cin, cout in LIN_SHAPES:
        for act in ("none", "relu"):
            # (K = 1, 7: a wider weight range, so that enough outputs clear the ReLU and differ from their neighbours)
            out.append(XCase(f"linear-{B}x{cin}x{cout}-{act}", Data(L("t", "linear", cin, cout, 1, 1, 0, False, act), B, 1, 500,
                                                                    wmax=1 if cin > 7 else 4), twice=cin == 32768))
    for i, l in enumerate(spec.POINT_HEAD):
        for B in (1, 3):
            out.append(XCase(f"{l.name}-B{B}", Data(l, B, 1, 510 + i), twice=True))
    # every branch of the launch plan (tests/_linear_cases.py::SWEEP holds the reason for each shape)
    for B, cin, cout in LC.SWEEP:
        for act in ("none", "relu"):
            out.append(XCase(f"linear-{B}x{cin}x{cout}-{act}", Data(L("t", "linear", cin, cout, 1, 1, 0, False, act), B, 1, 522), twice=True))
    return out


LINEAR_CASES = _linear()

# ---------------------------------------------------------------- bf16
BF16_KINDS = {
    "conv3d_s1": (L("t", "conv3d", 32, 96, 3, 1, 1), 7, 3, 0),
    "conv3d_s2": (L("t", "conv3d", 64, 160, 3, 2, 1), 9, 2, 0),
    "deconv": (L("t", "deconv3d", 32, 48, 4, 2, 1), 5, 3, 0),
    "conv2d_s2": (L("t", "conv2d", 64, 64, 3, 2, 1), 13, 5, 0),
    "conv3d_k4_valid_ks2": (L("t", "conv3d", 64, 40, 4, 1, 0), 7, 2, 2),
    "cout32": (L("t", "conv2d", 256, 32, 1, 1, 0), 9, 3, 4),
    "conv2d_s1_w28": (L("t", "conv2d", 64, 64, 3, 1, 1), 28, 3, 0),
    "conv3d_s1_w14": (L("t", "conv3d", 32, 64, 3, 1, 1), 14, 2, 0),
    "conv3d_s1_c64": (L("t", "conv3d", 64, 96, 3, 1, 1), 7, 3, 0),
    "deconv_c64": (L("t", "deconv3d", 64, 48, 4, 2, 1), 5, 3, 0),
    "deconv_c128_w8": (L("t", "deconv3d", 128, 64, 4, 2, 1), 8, 2, 0),
    "conv3d_k4_valid_c128_ks2": (L("t", "conv3d", 128, 40, 4, 1, 0), 7, 2, 2),
    "conv2d_s1_c128_w9": (L("t", "conv2d", 128, 64, 3, 1, 1), 9, 21, 0),
    "cout36_narrow_stores": (L("t", "conv2d", 64, 36, 3, 1, 1), 9, 3, 0),
    "cout100_s2": (L("t", "conv3d", 32, 100, 3, 2, 1), 9, 2, 0),
    "c128_cout128_ks2": (L("t", "conv3d", 128, 128, 3, 1, 1), 6, 2, 2),
}
BF16_TILES = (1, 2, 3, 4, 5, 6, 9, 10, 17, 18, 19, 20, 21, 22, 23)


def bf16_refused(tm, kind):
    """tests/test_bf16_gpu.py::test_bf16_tiles_and_split_k's refusal rules, verbatim.  (20 — 512-position per-tap tiles with 32-channel
    K tiles — has none, like 1, 2, 4, 17 and 18: one 64-cout tile per workgroup, no reuse image to fit)"""
    layer, n_in, B, ks = BF16_KINDS[kind]
    kc = 64 if tm in (5, 6) else 32
    plane_ok = (layer.s == 1 or layer.op == "deconv3d") and layer.cin % kc == 0 and (ks == 0 or (layer.cin // kc) % ks == 0)
    if tm in (6, 22, 23) and kind in ("conv3d_k4_valid_c128_ks2", "conv3d_k4_valid_ks2"):
        plane_ok = False
    if tm == 6 and kind == "c128_cout128_ks2":
        plane_ok = False
    wide_ok = (-(-layer.cout // 64)) % 2 == 0
    return (tm == 10 and kind in ("conv3d_s2", "cout100_s2")) or (tm in (5, 6, 21, 22, 23) and not plane_ok) or \
        (tm in (3, 19, 23) and not wide_ok)


def _bf16():
    cases = []
    for i, (l, n) in enumerate(network()):
        lv = dataclasses.replace(l, act="none") if l.act == "sigmoid" else l
        for B in (1, 3):
            cases.append(XCase(f"{lv.name}-bf16-B{B}", _bf16_data(lv, B, n, 600 + i)))
    for kind, (l, n, B, ks) in BF16_KINDS.items():
        d = _bf16_data(l, B, n, 700)
        for tm in BF16_TILES:
            cases.append(XCase(f"bf16-tile{tm}-{kind}", d, tile=tm, ksplit=ks, refused=bf16_refused(tm, kind), twice=True))
    return cases


BF16_CASES = _bf16()



# ---------------------------------------------------------------- Winograd fp32 (weights on the form's lattice)
def _wino_data(layer, B, n_in, seed, form):
    """two-axis F(4, 3) x F(4, 3): the flow through |B^T|, |G|, the channel sum and |A^T| grows with cin x (taps left in a class) and
    must stay below 2^24 (tests/_lattice.py::exactness), so x and w are thinned by sqrt(50 / that) each; x in {-1, 0, 1} throughout"""
    units = layer.cin * (3 if layer.op == "conv3d" else 1)
    dn = min(1.0, round(math.sqrt(50 / units), 2)) if form == "f43x2" else 1.0
    return Data(layer, B, n_in, seed, form, xmax=1, wmax=1, density=dn, xdensity=dn)


def _wino():
    cases = []
    net = dict((l.name, (l, n)) for l, n in network())
    names = {0: "serial", 1: "class-parallel", 2: "dual"}
    # one axis, F(4, 3) along H, in its three launch forms
    for tag, l, n, B in (("conv2d-32to48-e40", L("t", "conv2d", 32, 48, 3, 1, 1), 40, 3), ("conv3d-64to64-e12", L("t", "conv3d", 64, 64, 3, 1, 1), 12, 2),
                         ("e2", *net["e2"], 2), ("e4", *net["e4"], 2)):
        d = _wino_data(l, B, n, 800, "f43-h")
        for t in (0, 1, 2):
            cases.append(XCase(f"wino1-{names[t]}-{tag}", d, tile=t, algo=WINO, twice=tag in ("e2", "e4")))
    # two axes: 3 the two-axis algorithm, 4 its class-parallel form, 5 its semi-fused form
    for tag, l, n, B in (("e6", *net["e6"], 2), ("e7", *net["e7"], 2), ("conv2d-64to96-e20", L("t", "conv2d", 64, 96, 3, 1, 1), 20, 3),
                         ("v1", *net["v1"], 2), ("v3", *net["v3"], 2), ("v5", *net["v5"], 2)):
        d = _wino_data(l, B, n, 810, "f43x2")
        for t in (3, 4, 5):
            cases.append(XCase(f"wino2-tile{t}-{tag}", d, tile=t, algo=WINO, twice=len(tag) == 2))
    d = _wino_data(net["v6"][0], 2, net["v6"][1], 820, "f24x2")
    for t in (3, 4, 5):                                # (F(2, 4) x F(2, 4) has no semi-fused form: tile 5 is refused)
        cases.append(XCase(f"wino2-tile{t}-v6", d, tile=t, algo=WINO, refused=t == 5, twice=True))
    # transposed: F(2, 2) along D and H inside the parity classes (the library's pick and the three launch forms), and the three-axis form
    for name in ("d1", "d2"):
        l, n = net[name]
        d = Data(l, 2, n, 830, "f22x2")
        for t in (-1, 0, 1, 2):
            cases.append(XCase(f"dwino-tile{t}-{name}", d, tile=t, algo=WINO, twice=True))
    t3 = L("t", "deconv3d", 64, 32, 4, 2, 1)
    for n in (8, 16):
        d = Data(t3, 2, n, 840, "f22x3")
        for t in (6, 7, 8):
            cases.append(XCase(f"wino3-tile{t}-deconv3d-64to32-e{n}", d, tile=t, algo=WINO))
    cases.append(XCase("wino3-tile6-d3", Data(net["d3"][0], 1, net["d3"][1], 841, "f22x3"), tile=6, algo=WINO, twice=True))
    return cases


WINO_CASES = _wino()

# ---------------------------------------------------------------- Winograd fp32 at ragged shapes and at the LDS limits
ONE_AXIS_RAN = ("winograd-serial", "winograd-class-parallel", "winograd-dual")
DUAL_CASE = "ws1-dual-conv2d-32to130-e41-B13"      # asserted to have run the dual form: 276 serial workgroups on 256 compute units


def serial_workgroups(l, n_in, B):
    """workgroups of the one-axis kernel's serial form (tests/test_wino_gpu.py::_positions): 64-cout x 64-position tiles"""
    n = B * (n_in if l.op == "conv3d" else 1) * -(-n_in // 4) * n_in
    return -(-l.cout // 64) * -(-n // 64)


def _wino_shapes():
    """The smallest shapes at which each branch of the Winograd kernels is taken that the network's own sizes never reach: edges
    with n mod 4 = 1, 2, 3 (the dword-gather instantiation of the one-axis kernel, ragged last groups along one or both axes), couts
    2 / 33 / 70 / 130 over position counts that end inside a 64-position tile, ragged last packs of the two finish kernels (B % PL,
    PL and SUB shrunk by LDS under out_halo = 8), and the largest padded planes / slices that fit 64 KiB of LDS.  Every launch form
    of an algorithm is a case of its own over ONE Data; out_halo cycles through 0 .. 3 over the rows that fix none."""
    cases = []
    seed = 850
    names = {0: "serial", 1: "class-parallel", 2: "dual"}
    c2 = lambda ci, co: L("t", "conv2d", ci, co, 3, 1, 1)
    c3 = lambda ci, co: L("t", "conv3d", ci, co, 3, 1, 1)
    row = [0]

    def halo():
        row[0] += 1
        return (row[0] - 1) % 4

    # one axis, F(4, 3) along H: 0 serial, 1 class-parallel, 2 dual.  B = 13 at edge 41: 13 x 11 x 41 positions in 92 tiles x 3
    # cout tiles = 276 serial workgroups, past the 256 compute units — what the dual form needs to cut inside the layer
    for l, n, B in ((c2(32, 33), 5, 3), (c2(32, 33), 6, 3), (c2(32, 33), 7, 3), (c2(32, 48), 4, 1), (c3(32, 40), 9, 1), (c3(96, 70), 6, 2),
                    (c3(32, 2), 4, 1), (c2(32, 130), 41, 13), (c2(64, 2), 30, 1)):
        d, oh = _wino_data(l, B, n, seed, "f43-h"), halo()
        tag = f"{l.op}-{l.cin}to{l.cout}-e{n}-B{B}"
        for t in (0, 1, 2):
            cid = f"ws1-{names[t]}-{tag}"
            ran = (ONE_AXIS_RAN[t],) if t < 2 or cid == DUAL_CASE else ONE_AXIS_RAN      # (dual falls back where no cut exists)
            cases.append(XCase(cid, d, tile=t, algo=WINO, out_halo=oh, twice=True, ran=ran))
        if n > 28:                                     # AUTO takes the one-axis kernel above the two-axis form's edge 28
            cases.append(XCase(f"ws1-auto-{tag}", d, out_halo=oh, twice=True, ran=ONE_AXIS_RAN))
    assert serial_workgroups(c2(32, 130), 41, 13) == 276
    # two axes, F(4, 3) x F(4, 3): 3 the library's launch form, 4 class-parallel, 5 semi-fused; AUTO up to edge 28
    two = [(c2(32, 33), n, 3, None) for n in (4, 5, 6, 7, 9, 10, 11)]
    two += [(c2(32, 64), 28, 7, None),                 # 49 groups per sample: PL = 5 samples per finish workgroup, packs of 5 + 2
            (c2(32, 2), 12, 23, 8),                    # 9 groups: PL = 23 by the batch, 20 by LDS (28^2 floats a plane), packs of 20 + 3
            (c2(64, 130), 29, 2, None), (c2(64, 130), 30, 1, None)]
    two += [(c3(32, 40), n, B, None) for n, B in ((4, 3), (5, 3), (6, 3), (9, 2), (10, 2), (11, 1))]
    two += [(c3(96, 70), 6, 2, None),
            (c3(32, 2), 8, 5, 8)]                      # SUB = 10 (sample, depth group) pairs, 7 by LDS (four 24^2 slices each): items of 7 + 3
    for l, n, B, oh in two:
        d, oh = _wino_data(l, B, n, seed, "f43x2"), halo() if oh is None else oh
        tag = f"{l.op}-{l.cin}to{l.cout}-e{n}-B{B}-oh{oh}"
        for t in (3, 4, 5) + ((0,) if n <= 28 else ()):
            if t:
                cases.append(XCase(f"ws2-tile{t}-{tag}", d, tile=t, algo=WINO, out_halo=oh, twice=True, ran=("winograd-2axis",)))
            else:
                cases.append(XCase(f"ws2-auto-{tag}", d, out_halo=oh, twice=True, ran=("winograd-2axis",)))
    # the limits (include/s3r.h, s3r_algo): a padded plane of 128^2 floats, four padded slices of 64^2, are exactly 64 KiB
    d = _wino_data(c2(32, 2), 1, 124, seed, "f43x2")
    for oh in (0, 2):
        for t in (3, 4, 5):
            cases.append(XCase(f"ws2-tile{t}-conv2d-32to2-e124-B1-oh{oh}", d, tile=t, algo=WINO, out_halo=oh, twice=True, ran=("winograd-2axis",)))
    d = _wino_data(c3(32, 2), 1, 60, seed, "f43x2")
    for oh in (0, 2):
        for t in (4, 5):
            cases.append(XCase(f"ws2-tile{t}-conv3d-32to2-e60-B1-oh{oh}", d, tile=t, algo=WINO, out_halo=oh, twice=True, ran=("winograd-2axis",)))
    # F(2, 4) x F(2, 4): output edges 2, 3, 5, 6 (v6 has 4); no semi-fused form
    for l, n, B in ((L("t", "conv3d", 32, 48, 4, 1, 0), 5, 3), (L("t", "conv3d", 32, 48, 4, 1, 0), 6, 3), (L("t", "conv3d", 32, 48, 4, 1, 0), 8, 3),
                    (L("t", "conv3d", 64, 20, 4, 1, 0), 9, 2)):
        d, oh = _wino_data(l, B, n, seed, "f24x2"), halo()
        tag = f"conv3d-k4-{l.cin}to{l.cout}-e{n}-B{B}-oh{oh}"
        for t in (3, 4):
            cases.append(XCase(f"ws2-tile{t}-{tag}", d, tile=t, algo=WINO, out_halo=oh, twice=True, ran=("winograd-2axis",)))
        cases.append(XCase(f"ws2-auto-{tag}", d, out_halo=oh, twice=True, ran=("winograd-2axis",)))
    # transposed: F(2, 2) along D and H (the library's pick and the three launch forms), and the three-axis form
    for l, n, B in ((L("t", "deconv3d", 32, 24, 4, 2, 1), 4, 3), (L("t", "deconv3d", 32, 24, 4, 2, 1), 12, 1), (L("t", "deconv3d", 64, 72, 4, 2, 1), 8, 1)):
        d, oh = Data(l, B, n, seed, "f22x2"), halo()
        for t in (-1, 0, 1, 2):
            cases.append(XCase(f"wsd-tile{t}-deconv3d-{l.cin}to{l.cout}-e{n}-B{B}-oh{oh}", d, tile=t, algo=WINO, out_halo=oh, twice=True,
                               ran=(ONE_AXIS_RAN[t],) if t in (0, 1) else ONE_AXIS_RAN))
    for l, n, B in ((L("t", "deconv3d", 16, 40, 4, 2, 1), 8, 3), (L("t", "deconv3d", 48, 24, 4, 2, 1), 16, 1)):
        d, oh = Data(l, B, n, seed, "f22x3"), halo()
        for t in (6, 7, 8):
            cases.append(XCase(f"ws3-tile{t}-deconv3d-{l.cin}to{l.cout}-e{n}-B{B}-oh{oh}", d, tile=t, algo=WINO, out_halo=oh, twice=True,
                               ran=("winograd-3axis", "winograd-3axis-class-parallel")))
    return cases


WINO_SHAPE_CASES = _wino_shapes()


# ---------------------------------------------------------------- every epilogue site under the four vector forms
THREE_AXIS_RAN = ("winograd-3axis", "winograd-3axis-class-parallel")


def three_axis_ran(tile):
    """s3r_plan_algo.hip, resolve_algo: tile 6 the library's launch form (either), 7 class-parallel, 8 the one-kernel form: both run"""
    return {6: THREE_AXIS_RAN, 7: THREE_AXIS_RAN[1:], 8: THREE_AXIS_RAN[:1]}[tile]


def _ep_sites():
    """(site, dtype route, the site's Data in the "ss" form, [(launch, XCase keywords)]): the smallest shape the suite has for each
    kernel that ends in `scale ? scale[m] : 1, shift ? shift[m] : 0`, forced onto that kernel by algo / tile / ksplit.  Layers that
    fold no BatchNorm elsewhere in the suite (head, linear) get bn=True here, so that their scale[] branch holds a real vector"""
    c2 = lambda ci, co: L("t", "conv2d", ci, co, 3, 1, 1)
    c3 = lambda ci, co: L("t", "conv3d", ci, co, 3, 1, 1)
    up = lambda ci, co: L("t", "deconv3d", ci, co, 4, 2, 1)
    seed = 940
    two = ("winograd-2axis",)
    sites = [
        ("direct", Data(L("t", "conv3d", 64, 33, 3, 2, 1), 2, 9, seed),
         [("epilogue", dict(ksplit=1, algo=DIRECT)), ("splitk2-finish", dict(ksplit=2, algo=DIRECT))]),
        ("tclass", Data(L("t", "deconv2d", 32, 7, 4, 2, 1), 2, 7, seed), [("residue-classes", {})]),
        ("d2s", Data(L("t", "deconv2d", 32, 24, 3, 3, 0), 2, 7, seed), [("depth-to-space", {})]),
        ("wino1", _wino_data(c2(32, 33), 3, 5, seed, "f43-h"),
         [(f"tile{t}", dict(tile=t, algo=WINO, ran=(ONE_AXIS_RAN[t],) if t < 2 else ONE_AXIS_RAN)) for t in (0, 1, 2)]),
        ("wino2-conv2d", _wino_data(c2(32, 33), 3, 4, seed, "f43x2"), [(f"tile{t}", dict(tile=t, algo=WINO, ran=two)) for t in (3, 4, 5)]),
        ("wino2-conv3d", _wino_data(c3(32, 40), 3, 4, seed, "f43x2"), [(f"tile{t}", dict(tile=t, algo=WINO, ran=two)) for t in (3, 4, 5)]),
        ("wino2-k4", _wino_data(L("t", "conv3d", 32, 48, 4, 1, 0), 3, 5, seed, "f24x2"),
         [(f"tile{t}", dict(tile=t, algo=WINO, ran=two)) for t in (3, 4)]),
        ("dwino2", Data(up(32, 24), 3, 4, seed, "f22x2"),
         [(f"tile{t}", dict(tile=t, algo=WINO, ran=(ONE_AXIS_RAN[t],) if t < 2 else ONE_AXIS_RAN)) for t in (0, 1, 2)]),
        ("dwino3", Data(up(16, 40), 3, 8, seed, "f22x3"), [(f"tile{t}", dict(tile=t, algo=WINO, ran=three_axis_ran(t))) for t in (6, 7, 8)]),
        ("head", Data(L("t", "conv2d", 48, 1, 1, 1, 0, True, "relu"), 3, 6, seed + 1, wmax=2), [("kernel", {})]),      # (one channel: a seed with scale != 1)
    ]
    for name, (B, cin, cout) in LC.PER_KERNEL.items():          # an S3R_OP_LINEAR descriptor: the route that has a scale
        sites.append((f"linear-{name}", Data(L("t", "linear", cin, cout, 1, 1, 0, True, "relu"), B, 1, seed), [("descriptor", {})]))
    sites += [
        ("bf16-mfma", _bf16_data(c3(32, 96), 3, 7, seed), [("epilogue", {})]),
        ("bf16-splitk", _bf16_data(L("t", "conv3d", 64, 40, 4, 1, 0), 2, 7, seed), [("splitk2-finish", dict(ksplit=2))]),
        ("bf16-head", _bf16_data(L("t", "conv3d", 64, 1, 1, 1, 0, True, "relu"), 3, 4, seed), [("kernel", {})]),
    ]
    return sites


def _ep_cases():
    cases, groups = [], []
    for site, d, launches in _ep_sites():
        forms = [dataclasses.replace(d, ep=ep) for ep in LT.EP_FORMS]
        groups.append((site, forms))
        for f in forms:
            for tag, kw in launches:
                cases.append(XCase(f"ep-{site}-{tag}-{f.ep}", f, twice=True, **kw))
    return cases, groups


EP_CASES, EP_GROUPS = _ep_cases()
# s3r_linear_forward has no scale: bias = NULL is its one other form, once per kernel of the plan (the given-bias run is the sweep's)
LINEAR_NULL_BIAS = [XCase(f"linear-{name}-{B}x{cin}x{cout}-null-bias",
                          Data(L("t", "linear", cin, cout, 1, 1, 0, False, "relu"), B, 1, 522, wmax=4 if cin < 64 else 1, ep="00"), twice=True)
                    for name, (B, cin, cout) in LC.PER_KERNEL.items()]


def auto_form(c):
    """the Winograd form include/s3r.h's policy resolves an AUTO convolution of the sweep to: the two-axis algorithm for every stride-1
    layer that has it and an edge <= 28, the one-axis kernel above"""
    l = c.layer
    if (l.k, l.p) == (4, 0):
        return "f24x2"
    return "f43x2" if c.n_in <= 28 else "f43-h"


# ---------------------------------------------------------------- producers that hand a consumer its input: cost volume, chains
@dataclass(frozen=True)
class CVCase:
    """s3r_cost_volume_forward_wino / _wino2 writing v1's transformed planes (in_layout), v1 on the form's lattice.  The features are
    integers in {-1, 0, 1}, the volume their differences in {-2 .. 2}: exact, and on v1's input lattice"""
    id: str
    kind: str                  # "wino": six F(4, 3)-along-H plane sets, "wino2": the 36 two-axis ones
    B: int
    seed: int
    fdensity: float
    data: Data                 # v1's (the cost volume stands in for its x)

    def features(self):
        g = torch.Generator().manual_seed(self.seed)
        shape = (self.B, spec.FEAT_C, spec.FEAT_HW, spec.FEAT_HW)
        return tuple(torch.randint(-1, 2, shape, generator=g).float() * (torch.rand(shape, generator=g) < self.fdensity).float() for _ in range(2))

    def make(self):
        """(volume, v1's parameters): the volume from the oracle's own formulation, exact on integers"""
        from oracle import s2v_oracle as O
        _, p = self.data.make()
        return O.cost_volume(*self.features(), spec.MAX_DISP), p


def _cv():
    v1, n = dict((l.name, (l, n)) for l, n in network())["v1"]
    return [CVCase("cost-volume-wino->v1", "wino", 2, 900, 1.0, _wino_data(v1, 2, n, 901, "f43-h")),
            # (|x| up to 2 doubles the two-axis flow: the features are thinned to a third, on top of v1's own thinning)
            CVCase("cost-volume-wino2->v1", "wino2", 2, 910, 0.35, _wino_data(v1, 2, n, 911, "f43x2"))]


CV_CASES = _cv()


@dataclass(frozen=True)
class ChainCase:
    """two layers through s3r_chain_forward; the first has a ReLU and an epilogue that keeps the intermediate on the integer lattice.
    pep, the producer's epilogue: "unit" scale 1 / shift 0 as vectors; "null" both NULL; "int" scale in {1, 2} and an integer shift
    in [-4, 8] per channel (seeded by the first Data's seed)"""
    id: str
    first: Data
    second: Data               # (its x is the first layer's output: only the parameters of second.make() are used)
    dtype: str = "fp32"
    pep: str = "unit"
    algo: int = 0              # of the first layer
    tile: int = -1
    ran: tuple = ()            # the first layer's profiler record must name one of these; (): not asserted
    fused: bool = False        # the head must have run inside the first layer's launch: no head record

    def make(self):
        x, p0 = self.first.make()
        if self.pep == "unit":
            p0 = dict(p0, scale=None if p0["scale"] is None else torch.ones_like(p0["scale"]), shift=torch.zeros_like(p0["shift"]))
        elif self.pep == "null":
            p0 = dict(p0, scale=None, shift=None)
        else:
            g = torch.Generator().manual_seed(self.first.seed + 31)
            co = self.first.layer.cout
            p0 = dict(p0, scale=torch.randint(1, 3, (co,), generator=g).float(), shift=torch.randint(-4, 9, (co,), generator=g).float())
        _, p1 = dataclasses.replace(self.second, B=1).make()      # (the parameters do not depend on the batch; its x is not used)
        return x, [p0, p1]

    def intermediate(self, x, p0):
        """the first layer's exact output in the second layer's geometry (rounded to bf16 on that path: exact when |h| <= 256)"""
        h = LT.expected(self.first.layer, x, p0, "fp32")
        return h.to(torch.bfloat16).float() if self.dtype == "bf16" else h


def _chains():
    net = dict((l.name, (l, n)) for l, n in network())
    (e1, n1), (e2, n2), (d3, n3), (d4, n4) = net["e1"], net["e2"], net["d3"], net["d4"]
    head = dataclasses.replace(d4, act="none")
    return [
        # the stem writes e2's F(4, 3)-along-H plane sets (the library's own pick for this pair): e2 on that form's lattice
        ChainCase("stem->e2", Data(e1, 2, n1, 920, xmax=1), _wino_data(e2, 2, n2, 921, "f43-h")),
        # bf16: d3 with the head fused into its launch (d3's output is never materialised).  d3's data is thinned until its output stays
        # within +-256, where bf16 holds every integer: the intermediate is then the same number whether or not the kernel rounds it
        ChainCase("d3+head-bf16", Data(d3, 2, n3, 930, xmax=1, density=0.25, xdensity=0.25, dtype="bf16"), Data(head, 2, n4, 931, wmax=2, dtype="bf16"),
                  dtype="bf16"),
    ]


CHAIN_CASES = _chains()

TILE1_WORKGROUPS, TILE1_POSITIONS = 2000, 256      # conv_head_fused: the 64 x 256 tile from 2000 workgroups of it on


def tile1_batch(n_out):
    """smallest batch of a 3D layer over output edge n_out at which the fused launch of a 33 .. 64-cout convolution takes the
    64 x 256 tile: ceil(B n^3 / 256) >= 2000"""
    return -(-((TILE1_WORKGROUPS - 1) * TILE1_POSITIONS + 1) // n_out ** 3)


def _head_chains():
    """the fp32 conv + head launch (s3r_conv_forward.hip: conv_head_fused, which rides on run_dwino / run_dwino3 or launches the direct kernel
    itself), one row per route, each under the head's four epilogue forms and
    the producer forms null and int.  The head has bn=True so that head_scale is a real vector, and act none: negative sums count.
    (Its one channel draws its scale from four values: seed 997 gives scale 2, a non-zero shift and non-zero weights on the first and the
    last input channel at cin 24, 40 and 64 — with seed 961 the last weight at cin 40 was 0, and a head that skipped its last channel passed;
    tests/test_exact_cpu.py keeps the condition)"""
    net = dict((l.name, (l, n)) for l, n in network())
    (d3, n3), (d4, n4) = net["d3"], net["d4"]
    c3 = lambda ci, co: L("t", "conv3d", ci, co, 3, 1, 1)
    up = lambda ci, co: L("t", "deconv3d", ci, co, 4, 2, 1)
    head = lambda ci: L("h", "conv3d", ci, 1, 1, 1, 0, True, "none")
    B1 = tile1_batch(8)
    rows = [  # (route, first layer's Data, head edge, ChainCase keywords)
        ("direct-c24-tile2", Data(c3(32, 24), 2, 4, 950), 4, dict(algo=DIRECT)),
        ("direct-c40-tile7", Data(c3(16, 40), 2, 4, 951), 4, dict(algo=DIRECT)),
        (f"direct-c40-tile1-B{B1}", Data(L("t", "conv3d", 16, 40, 1, 1, 0), B1, 8, 952), 8, dict(algo=DIRECT)),      # (1 x 1 x 1: a large batch stays cheap)
        ("transposed-direct", Data(up(32, 24), 2, 4, 953), 8, dict(algo=DIRECT)),
    ]
    rows += [(f"dwino2-tile{t}", Data(up(32, 24), 2, 4, 954, "f22x2"), 8,
              dict(algo=WINO, tile=t, ran=(ONE_AXIS_RAN[t],) if t < 2 else ONE_AXIS_RAN)) for t in (0, 1, 2)]
    rows += [(f"dwino3-tile{t}", Data(up(16, 40), 2, 8, 955, "f22x3"), 16, dict(algo=WINO, tile=t, ran=three_axis_ran(t))) for t in (6, 7, 8)]
    rows.append(("d3+d4", Data(d3, 1, n3, 956, xmax=1), n4, {}))
    out = []
    for route, first, n_head, kw in rows:
        for pep in ("null", "int"):
            for ep in LT.EP_FORMS:
                out.append(ChainCase(f"{route}+head-p{pep}-h{ep}", first, Data(head(first.layer.cout), first.B, n_head, 997, wmax=2, ep=ep),
                                     pep=pep, fused=True, **kw))
    return out


HEAD_CHAIN_CASES = _head_chains()
ALL_CHAIN_CASES = CHAIN_CASES + HEAD_CHAIN_CASES       # (CHAIN_CASES alone: the hand-offs tests/test_alignment_gpu.py runs at skewed pointers)

ALL_CASES = DIRECT_CASES + LINEAR_CASES + BF16_CASES + WINO_CASES + WINO_SHAPE_CASES + EP_CASES + LINEAR_NULL_BIAS


def unique_data(cases=None):
    seen, out = set(), []
    for c in (ALL_CASES if cases is None else cases):
        if c.data not in seen:
            seen.add(c.data)
            out.append(c.data)
    return out
