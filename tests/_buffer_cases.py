"""The cases of tests/test_buffers_gpu.py, shared with the checker's self-test in tests/test_buffers_cpu.py.

CONV_CASES: s3r_conv_forward / s3r_conv_pack_weights, one per (layer or shape, form).  CHAIN_PAIRS: the producer x consumer
composition matrix of s3r_chain_forward (host-only planning on the CPU, the pairs that plan on the GPU).
"""
from __future__ import annotations

from dataclasses import dataclass

import s3r
from s3r import arch_spec as spec

L = spec.Layer
DIRECT, WINO = s3r.ALGO_DIRECT, s3r.ALGO_WINOGRAD


@dataclass(frozen=True)
class ConvCase:
    id: str
    layer: L
    n_in: int
    B: int
    dtype: str = "fp32"
    tile: int = -1
    ksplit: int = 0
    algo: int = 0
    in_halo: int = -1          # -1: what the layer's kernel needs
    out_halo: int = 0

    @property
    def form(self):
        return "bf16" if self.dtype == "bf16" else ("wino" if has_wino(self) else "direct")


def _stem(l):
    return l.op == "conv2d" and l.cin == 3 and l.cout == 32 and l.k == 3 and l.s == 2 and l.p == 1 and l.act == "relu" and l.dil == 1


def _head(l, n):
    return l.op in ("conv2d", "conv3d") and l.cout == 1 and l.k == 1 and l.s == 1 and l.p == 0 and l.act in ("none", "relu", "sigmoid") \
        and n ** spec.ndim(l) % 4 == 0


def staged(l, n, dtype="fp32"):
    if dtype != "fp32" or l.op == "linear" or _stem(l) or _head(l, n):
        return False
    if l.op.startswith("deconv"):
        return not (l.op == "deconv3d" and (l.k, l.s, l.p, l.dil, l.opad) == (4, 2, 1, 1, 0) and l.cin % 16 == 0)
    return l.cin % 16 != 0


def need_halo(l, n, dtype="fp32"):
    if l.op == "linear" or _stem(l) or _head(l, n) or staged(l, n, dtype):
        return 0
    return 1 if l.op.startswith("deconv") else l.p


def has_wino(c):
    """whether the form that runs may be a Winograd one (its bound is the looser: a direct run checked with it only loses strictness)"""
    l = c.layer
    if c.dtype != "fp32" or c.algo == DIRECT or (c.algo == 0 and (c.tile >= 0 or c.ksplit > 0)) or l.act == "sigmoid":
        return False
    if l.op in ("conv2d", "conv3d"):
        return l.cin % 32 == 0 and l.cout > 1 and l.dil == 1 and l.s == 1 and ((l.k, l.p) == (3, 1) or (l.op == "conv3d" and (l.k, l.p) == (4, 0)))
    if l.op != "deconv3d" or (l.k, l.s, l.p, l.dil, l.opad) != (4, 2, 1, 1, 0):
        return False
    if c.algo == WINO and c.tile in (6, 7, 8):         # the three-axis form: 16-channel K tiles, edges 8 / 16 / 32
        return l.cin % 16 == 0 and c.n_in in (8, 16, 32)
    return l.cin % 32 == 0 and c.n_in % 4 == 0


def zero_halo_writer(c):
    """the two-axis Conv2d form: its finish kernel stores whole padded planes, the halo as +0.0; the FORCED semi-fused form of the
    two-axis Conv3d k3: whole padded slices, the depth halo too (include/s3r.h, Halos).  (Where the library picks the Conv3d's launch
    form, the cases here have batches at which it is the class-parallel one, which writes interiors only: held to that.)"""
    l = c.layer
    if not has_wino(c):
        return False
    if l.op == "conv3d":
        return c.algo == WINO and c.tile == 5 and l.k == 3
    if l.op != "conv2d":
        return False
    return c.tile in (3, 4, 5) or (c.algo == 0 and c.tile < 0 and c.n_in <= 28)


def _network():
    rows = []
    for layers, n0 in ((spec.ENCODER, spec.IMG_HW), (spec.DECODER, spec.MAX_DISP)):
        rows += [(l, n) for l, n, _ in spec.trace(layers, n0)]
    return rows


def _conv_cases():
    cases = []
    for i, (l, n) in enumerate(_network()):
        for dt in ("fp32", "bf16"):
            for B in (1, 3):
                oh = 0 if _head(l, n) else (i + B) % 4
                cases.append(ConvCase(f"{l.name}-{dt}-B{B}-oh{oh}", l, n, B, dt, out_halo=oh))
    # forced direct tiles and split-K on ragged shapes
    t = L("t", "conv3d", 64, 70, 3, 1, 1)
    for cfg in range(8):        # (edge 12: rows of a multiple of 4 positions, which tile 5's 16-byte gather needs; 3456 positions)
        cases.append(ConvCase(f"tile{cfg}-conv3d-64to70-e12", t, 12, 2, tile=cfg, out_halo=cfg % 3))
    for ks in (1, 2, 4):
        cases.append(ConvCase(f"splitk{ks}-conv3d-64to33-s2-e9", L("t", "conv3d", 64, 33, 3, 2, 1), 9, 3, ksplit=ks, out_halo=1))
        cases.append(ConvCase(f"splitk{ks}-deconv3d-tuned-64to16-e5", L("t", "deconv3d", 64, 16, 4, 2, 1), 5, 2, ksplit=ks, algo=DIRECT))
    # Winograd one-axis launch forms, two-axis, three-axis
    for form, name in ((0, "serial"), (1, "class-parallel"), (2, "dual")):
        cases.append(ConvCase(f"wino1-{name}-conv2d-32to48-e40", L("t", "conv2d", 32, 48, 3, 1, 1), 40, 3, algo=WINO, tile=form, out_halo=1))
        cases.append(ConvCase(f"wino1-{name}-conv3d-64to64-e12", L("t", "conv3d", 64, 64, 3, 1, 1), 12, 2, algo=WINO, tile=form))
    for form in (3, 4, 5):
        cases.append(ConvCase(f"wino2-tile{form}-conv2d-64to96-e20", L("t", "conv2d", 64, 96, 3, 1, 1), 20, 3, algo=WINO, tile=form, out_halo=2))
        cases.append(ConvCase(f"wino2-tile{form}-conv3d-32to64-e12", L("t", "conv3d", 32, 64, 3, 1, 1), 12, 1, algo=WINO, tile=form))
    for form in (6, 7, 8):
        for n in (8, 16):
            cases.append(ConvCase(f"wino3-tile{form}-deconv3d-64to32-e{n}", L("t", "deconv3d", 64, 32, 4, 2, 1), n, 2, algo=WINO, tile=form,
                                  out_halo=1))
    # general layers: cout 1 / 7 / 33 / 70 / 130, ragged position counts
    for co in (1, 7, 33, 70, 130):
        cases.append(ConvCase(f"general-conv2d-16to{co}-k3-e13", L("t", "conv2d", 16, co, 3, 1, 1), 13, 3, out_halo=co % 4))
        cases.append(ConvCase(f"general-conv3d-32to{co}-k3s2-e11", L("t", "conv3d", 32, co, 3, 2, 1), 11, 2, algo=DIRECT))
        cases.append(ConvCase(f"staged-conv2d-20to{co}-k5-e9", L("t", "conv2d", 20, co, 5, 1, 2, True, "leaky_relu"), 9, 2, out_halo=1))
        cases.append(ConvCase(f"tclass-deconv2d-32to{co}-k4s2-e7", L("t", "deconv2d", 32, co, 4, 2, 1), 7, 2, out_halo=2))
    cases += [
        ConvCase("staged-conv3d-5to7-k1-e6", L("t", "conv3d", 5, 7, 1, 1, 0), 6, 2),
        ConvCase("unfolded-conv2d-3to16-k7s2-e33", L("t", "conv2d", 3, 16, 7, 2, 3), 33, 2, out_halo=3),
        ConvCase("unfolded-conv3d-2to24-k4s2-elu-e10", L("t", "conv3d", 2, 24, 4, 2, 1, True, "elu"), 10, 2),
        ConvCase("unfolded-subbatch-conv2d-8to16-k7-e200", L("t", "conv2d", 8, 16, 7, 1, 3, True, "leaky_relu", 1, 0, 0.1), 200, 20),
        ConvCase("tclass-noTap-deconv2d-16to16-k2s3-e5", L("t", "deconv2d", 16, 16, 2, 3, 0), 5, 2, out_halo=1),
        ConvCase("tclass-deconv3d-16to16-k3s2p1op1-e5", L("t", "deconv3d", 16, 16, 3, 2, 1, True, "relu", 1, 1), 5, 2),
        ConvCase("tclass-staged-deconv3d-8to12-k4s2-e5", L("t", "deconv3d", 8, 12, 4, 2, 1), 5, 2, out_halo=1),
        # 4^3 = 64 residue classes, more than one class table holds (kTClsMax = 27): one launch per class; output edge 13
        ConvCase("tclass-perclass-deconv3d-16to16-k5s4-e3", L("t", "deconv3d", 16, 16, 5, 4, 0), 3, 2),
        ConvCase("tclass-inplace-h3-deconv2d-32to16-k7s2-e8", L("t", "deconv2d", 32, 16, 7, 2, 0), 8, 2, in_halo=3),
        ConvCase("tclass-inplace-h1-deconv2d-64to32-k4s2-e16", L("t", "deconv2d", 64, 32, 4, 2, 1), 16, 2, in_halo=1, out_halo=1),
        ConvCase("d2s-deconv2d-32to24-k3s3-e7", L("t", "deconv2d", 32, 24, 3, 3, 0), 7, 2, out_halo=2),
        ConvCase("d2s-deconv3d-24to10-k2s2-leaky-e5", L("t", "deconv3d", 24, 10, 2, 2, 0, True, "leaky_relu"), 5, 2),
        ConvCase("d2s-deconv2d-16to40-k4s4-sigmoid-e5", L("t", "deconv2d", 16, 40, 4, 4, 0, True, "sigmoid"), 5, 3),
        ConvCase("dilated-deconv2d-16to16-k3s2p2d2-e6", L("t", "deconv2d", 16, 16, 3, 2, 2, True, "none", 2, 1), 6, 2, out_halo=1),
        ConvCase("dilated-conv2d-32to32-d2-e16", L("t", "conv2d", 32, 32, 3, 1, 2, True, "relu", 2), 16, 2),
        ConvCase("dilated-conv3d-16to16-d3-e9", L("t", "conv3d", 16, 16, 3, 1, 3, True, "none", 3), 9, 1, out_halo=2),
        ConvCase("leaky-splitk2-finish-conv3d-64to32-s2-e9", L("t", "conv3d", 64, 32, 3, 2, 1, True, "leaky_relu", 1, 0, 0.3), 9, 2, ksplit=2),
        ConvCase("leaky-splitk4-finish-conv3d-128to32-e6", L("t", "conv3d", 128, 32, 3, 1, 1, True, "leaky_relu", 1, 0, 0.2), 6, 2, ksplit=4,
                 algo=DIRECT, out_halo=1),
        ConvCase("tanh-pass-conv2d-32to16-e8", L("t", "conv2d", 32, 16, 3, 1, 1, True, "tanh"), 8, 2, out_halo=1),
        ConvCase("elu-pass-conv3d-32to32-e8", L("t", "conv3d", 32, 32, 3, 1, 1, True, "elu"), 8, 2),
        ConvCase("head-conv2d-48to1-sigmoid-e6", L("t", "conv2d", 48, 1, 1, 1, 0, False, "sigmoid"), 6, 3),
    ]
    return cases + _wino_shape_cases()


def _wino_shape_cases():
    """one guarded case per branch of tests/_exact_cases.py::_wino_shapes (that table holds the reasons for each shape): random data
    in poisoned buffers is the half that catches a READ outside the tensor, which integers in plain allocations cannot"""
    c2 = lambda ci, co: L("t", "conv2d", ci, co, 3, 1, 1)
    c3 = lambda ci, co: L("t", "conv3d", ci, co, 3, 1, 1)
    k4 = L("t", "conv3d", 32, 48, 4, 1, 0)
    forms = ("serial", "class-parallel", "dual")
    cases = []
    # one axis: every row at one launch form, the forms rotating; the last row under AUTO too (the one-axis kernel above edge 28)
    for i, (l, n, B) in enumerate(((c2(32, 33), 5, 3), (c2(32, 33), 6, 3), (c2(32, 33), 7, 3), (c2(32, 48), 4, 1), (c3(32, 40), 9, 1),
                                   (c3(96, 70), 6, 2), (c3(32, 2), 4, 1), (c2(32, 130), 41, 13), (c2(64, 2), 30, 1))):
        cases.append(ConvCase(f"ws1-{forms[(i + 1) % 3]}-{l.op}-{l.cin}to{l.cout}-e{n}-B{B}", l, n, B, algo=WINO, tile=(i + 1) % 3, out_halo=i % 4))
    cases.append(ConvCase("ws1-auto-conv2d-64to2-e30-B1", c2(64, 2), 30, 1, out_halo=1))
    # two axes: ragged groups, ragged packs (B % PL, PL and SUB shrunk by LDS under out_halo 8), the largest plane / slices that fit
    for l, n, B, tile, oh in ((c2(32, 33), 5, 3, 3, 1), (c2(32, 33), 6, 3, 4, 2), (c2(32, 33), 7, 3, 5, 3), (c2(32, 64), 28, 7, 3, 0),
                              (c2(32, 2), 12, 23, 4, 8), (c2(32, 2), 124, 1, 5, 2),
                              (c3(32, 40), 5, 3, 3, 1), (c3(32, 40), 6, 3, 4, 2), (c3(32, 40), 9, 2, 5, 3), (c3(32, 2), 8, 5, 5, 8),
                              (c3(32, 2), 60, 1, 5, 2),
                              (k4, 5, 3, 3, 0), (k4, 6, 3, 4, 1), (k4, 8, 3, 3, 2)):
        cases.append(ConvCase(f"ws2-tile{tile}-{l.op}-k{l.k}-{l.cin}to{l.cout}-e{n}-B{B}-oh{oh}", l, n, B, algo=WINO, tile=tile, out_halo=oh))
    # transposed: the two-axis classes at edge 12, the three-axis form at cin 16 / cout 40
    cases.append(ConvCase("wsd-class-parallel-deconv3d-32to24-e12-B1", L("t", "deconv3d", 32, 24, 4, 2, 1), 12, 1, algo=WINO, tile=1, out_halo=1))
    cases.append(ConvCase("ws3-tile6-deconv3d-16to40-e8-B3", L("t", "deconv3d", 16, 40, 4, 2, 1), 8, 3, algo=WINO, tile=6, out_halo=2))
    return cases


CONV_CASES = _conv_cases()


# ---------------------------------------------------------------- chain composition matrix
@dataclass(frozen=True)
class Part:
    layer: L
    n_in: int
    algo: int = 0
    tile: int = -1


def _consumers():
    """name -> (input geometry (C, n, nd) or None = any, builder)"""
    c = {}
    for p in range(4):
        c[f"direct-p{p}"] = ((32, 12, 2), lambda C, n, nd, p=p: Part(L("c", "conv2d", C, 24, 2 * p + 1, 1, p), n, DIRECT))
    c["staged"] = ((24, 10, 2), lambda C, n, nd: Part(L("c", "conv2d", C, 16, 3, 1, 1), n))
    c["unfolded"] = ((3, 12, 2), lambda C, n, nd: Part(L("c", "conv2d", C, 16, 3, 1, 1), n))
    c["unfolded-c1"] = ((1, 8, 2), lambda C, n, nd: Part(L("c", "conv2d", C, 16, 3, 1, 1), n))
    c["wino1"] = ((32, 40, 2), lambda C, n, nd: Part(L("c", "conv2d", C, 32, 3, 1, 1), n, WINO, 0))
    c["wino2-2d"] = ((32, 8, 2), lambda C, n, nd: Part(L("c", "conv2d", C, 32, 3, 1, 1), n, WINO, 3))
    c["wino2-3d"] = ((32, 8, 3), lambda C, n, nd: Part(L("c", "conv3d", C, 32, 3, 1, 1), n, WINO, 3))
    c["tuned-deconv3d"] = ((32, 8, 3), lambda C, n, nd: Part(L("c", "deconv3d", C, 16, 4, 2, 1), n))
    c["tclass-h1"] = ((32, 8, 2), lambda C, n, nd: Part(L("c", "deconv2d", C, 16, 4, 2, 1), n))
    c["tclass-h2"] = ((32, 8, 2), lambda C, n, nd: Part(L("c", "deconv2d", C, 16, 5, 2, 0), n))
    c["tclass-h3"] = ((32, 8, 2), lambda C, n, nd: Part(L("c", "deconv2d", C, 16, 7, 2, 0), n))
    c["tclass-h9-staged"] = ((32, 4, 2), lambda C, n, nd: Part(L("c", "deconv2d", C, 8, 19, 2, 0), n))
    c["d2s"] = ((32, 8, 2), lambda C, n, nd: Part(L("c", "deconv2d", C, 16, 2, 2, 0), n))
    c["head-2d"] = ((32, 8, 2), lambda C, n, nd: Part(L("c", "conv2d", C, 1, 1, 1, 0, False, "sigmoid"), n))
    c["head-3d"] = ((32, 8, 3), lambda C, n, nd: Part(L("c", "conv3d", C, 1, 1, 1, 0, False, "sigmoid"), n))
    c["direct3d-e16"] = ((32, 16, 3), lambda C, n, nd: Part(L("c", "conv3d", C, 16, 3, 1, 1), n, DIRECT))
    c["head-3d-e32"] = ((32, 32, 3), lambda C, n, nd: Part(L("c", "conv3d", C, 1, 1, 1, 0, False, "sigmoid"), n))
    c["linear"] = (None, lambda C, n, nd: Part(L("c", "linear", C * n ** nd, 10, 1, 1, 0, False, "none"), 1))
    return c


def _producers():
    """name -> builder(C, n, nd) -> Part with output (C, n, nd), or None where the producer cannot make it; `natural` geometry for
    consumers that take any input (the linear one), kept to K = C n^nd <= 4096: a linear consumer's dropped term must stand out of
    the checker's bound (tests/_ref64.py); None: no such pair (tuned-deconv3d-e16 writes 32^3 positions per channel)"""
    def conv(cin, algo=0, tile=-1, ok=lambda C, n, nd: True):
        return lambda C, n, nd: Part(L("p", f"conv{nd}d", cin, C, 3, 1, 1), n, algo, tile) if ok(C, n, nd) else None

    def up(C, n, nd, k, s, p, ok):
        return Part(L("p", f"deconv{nd}d", 32, C, k, s, p), n // s) if ok else None

    pr = {
        "linear": (lambda C, n, nd: Part(L("p", "linear", 40, C * n ** nd, 1, 1, 0, False, "relu"), 1), (32, 8, 2)),
        "head": (lambda C, n, nd: Part(L("p", f"conv{nd}d", 32, 1, 1, 1, 0, False, "sigmoid"), n) if C == 1 else None, (1, 8, 2)),
        "direct": (conv(16, DIRECT), (32, 8, 2)),
        "staged": (conv(24), (32, 8, 2)),
        "unfolded": (conv(3), (16, 8, 2)),
        "wino1-e40": (conv(32, WINO, 0, ok=lambda C, n, nd: C > 1 and n >= 4), (16, 8, 2)),
        "wino2-2d": (conv(32, WINO, 3, ok=lambda C, n, nd: nd == 2 and C > 1 and n % 4 == 0 and n <= 28), (32, 8, 2)),
        "wino2-3d": (conv(32, WINO, 3, ok=lambda C, n, nd: nd == 3 and C > 1 and n % 4 == 0 and n <= 28), (8, 8, 3)),
        "tclass": (lambda C, n, nd: up(C, n, nd, 4, 2, 1, nd == 2 and n % 2 == 0), (32, 8, 2)),
        "d2s": (lambda C, n, nd: up(C, n, nd, 2, 2, 0, nd == 2 and n % 2 == 0), (32, 8, 2)),
        "reshape-conv": (lambda C, n, nd: Part(L("p", f"conv{nd}d", 16, C * 2 ** nd, 3, 1, 1), n // 2, DIRECT) if n % 2 == 0 else None,
                         (32, 8, 2)),
    }
    for e, natural in ((4, (8, 8, 3)), (8, (1, 16, 3)), (16, None)):
        pr[f"tuned-deconv3d-e{e}"] = (lambda C, n, nd, e=e: up(C, n, nd, 4, 2, 1, nd == 3 and n == 2 * e), natural)
    return pr


RESHAPING = ("linear", "reshape-conv")
# consumers whose kernel reads its zero padding from the producer's halo: behind a reshaping producer they are refused
# (include/s3r.h, s3r_chain_forward): the reshaped activation has no halo in the consumer's geometry
HALO_READERS = ("direct-p1", "direct-p2", "direct-p3", "wino1", "wino2-2d", "wino2-3d", "tuned-deconv3d", "direct3d-e16")


def _pairs():
    out = []
    cons, prods = _consumers(), _producers()
    for pn, (pb, natural) in prods.items():
        for cn, (geo, cb) in cons.items():
            if geo is None and natural is None:
                continue
            C, n, nd = geo if geo is not None else natural
            p = pb(C, n, nd)
            if p is None:
                continue
            c = cb(C, n, nd)
            refused = pn in RESHAPING and cn in HALO_READERS
            out.append((f"{pn}->{cn}", p, c, refused))
    return out


CHAIN_PAIRS = _pairs()
