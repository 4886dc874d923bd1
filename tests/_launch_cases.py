"""The launch forms launch_conv_mfma (csrc/s3r_conv_glds.hip) takes by itself above one round of workgroups on the compute units, and
the cases of tests/test_launch_forms_cpu.py / tests/test_launch_forms_gpu.py that reach them.

No tile code and no descriptor field forces these forms: the launcher plans them from the layer's workgroup count and the device's
compute units.  So the tests need to know, WITHOUT asking the library, what it must have done — this file restates the plan:

    TILE_DIMS, KTUNED   kTileDims and the keys of kTuned
    pick_tile           conv_pick_tile's rules (the part below the kTuned lookup; no case may match a kTuned row: asserted)
    pick_vec            conv_pick_vec
    tail_cut            plan_tail_cut line by line, the one-launch ("dual") and the two-launch cost model included
    ring                sparse_launch
    plan, form          launch_conv_mfma's own sequence: what s3r_prof_record.launch_form and .launches must read

It MIRRORS the kernel file and must move with it: a change to plan_tail_cut's constants, to the 384-workgroup ring threshold, to the
tiles the dual kernel is built for or to conv_pick_tile's rules is made here too, and the GPU test (record == form(case, cus) on the
device's own compute-unit count) says so when it is not.  The CPU test computes, from this file alone at 256 compute units, that every
row of the table takes the form it names and what the rows reach between them.

The cases are XCases over "direct" lattices (tests/_lattice.py); on the device they go through tests/_abi_bodies.py::conv_forward
(guarded buffers, NaN-filled and zero-filled scratch) and tests/test_exact_gpu.py's bit comparison with the float64 reference.
Unless a row says otherwise: cin 16, k3 s1 p1, BatchNorm folded, ReLU.  Positions are output positions (input positions for a
transposed layer, whose eight residue classes each walk all of them).
"""
from __future__ import annotations

from dataclasses import dataclass
from types import SimpleNamespace

from s3r import arch_spec as spec

from tests._exact_cases import DIRECT, Data, L, XCase

FORM_CUT, FORM_ONE_LAUNCH, FORM_RING = 1, 2, 4          # s3r_prof_record.launch_form (include/s3r.h)

# kTileDims: cfg -> (BM couts, BN positions)
TILE_DIMS = ((128, 128), (64, 256), (32, 256), (64, 64), (128, 256), (64, 512), (128, 64), (64, 128))
DUAL_TILES = (0, 1, 4, 7)                               # launch_dual: the bulk tiles conv_glds_dual_kernel is instantiated for
RING_MAX_WGS = 384                                      # sparse_launch
# kTuned's keys: (cin, cout, T, stride, S per sample, transposed)
KTUNED = ((32, 64, 9, 1, 12544, 0), (64, 64, 9, 2, 3136, 0), (64, 128, 9, 1, 3136, 0), (128, 128, 9, 2, 784, 0), (128, 256, 9, 1, 784, 0),
          (256, 256, 9, 1, 784, 0), (256, 32, 1, 1, 784, 0), (64, 64, 27, 1, 21952, 0), (64, 128, 27, 2, 2744, 0), (128, 128, 27, 1, 2744, 0),
          (128, 256, 27, 2, 343, 0), (256, 256, 27, 1, 343, 0), (256, 512, 64, 1, 64, 0), (512, 256, 8, 1, 64, 1), (256, 128, 8, 1, 512, 1),
          (128, 64, 8, 1, 4096, 1))


def cdiv(a, b):
    return -(-a // b)


# ---------------------------------------------------------------- the layer as the launcher sees it (make_params)
def geometry(layer, n_in, B):
    """what ConvParams holds of a case: positions per sample S and in all (Ntotal), the row width Nw, taps T, the key stride (a fast
    ConvTranspose k4 s2 p1 is eight stride-1 classes of 2 x 2 x 2 taps over the INPUT positions)"""
    nd = spec.ndim(layer)
    transposed = layer.op == "deconv3d"
    if transposed:
        assert (layer.k, layer.s, layer.p, layer.dil, layer.opad) == (4, 2, 1, 1, 0) and layer.cin % 16 == 0
        nw, T, stride = n_in, 8, 1
    else:
        assert layer.cin % 16 == 0 and layer.dil == 1
        nw, T, stride = spec.out_size(layer, n_in), layer.k ** nd, layer.s
    S = nw ** nd
    return SimpleNamespace(transposed=transposed, Nw=nw, S=S, Ntotal=B * S, T=T, stride=stride, cin=layer.cin, cout=layer.cout, nd=nd)


def matches_ktuned(g):
    return (g.cin, g.cout, g.T, g.stride, g.S, int(g.transposed)) in KTUNED


def pick_tile(cout, ntotal, transposed, ksplit=1):
    """conv_pick_tile below its kTuned lookup"""
    classes = (8 if transposed else 1) * (ksplit if ksplit > 1 else 1)

    def wgs(cfg):
        bm, bn = TILE_DIMS[cfg]
        return cdiv(cout, bm) * cdiv(ntotal, bn) * classes

    if cout <= 32:
        return 2 if wgs(2) >= 128 else 3
    if cout <= 64:
        return 1 if wgs(1) >= 2000 else (7 if wgs(7) >= 2000 else 3)
    if wgs(2) >= 1500:
        return 2
    return 7 if wgs(7) >= 1500 else 3


def pick_vec(g):
    """conv_pick_vec: 16-byte gathers for stride-1 rows of a multiple of 4 positions, dword gathers otherwise"""
    if g.stride != 1:
        return 1
    return 4 if g.Nw % 4 == 0 else 1


def tail_cut(cout, ntotal, cfg, transposed, dual_built, cus, ksplit=1):
    """plan_tail_cut: n_cut, or None where the layer goes out uncut.  dual_built: the process may put bulk and remainder into one
    launch (False under S3R_NO_DUAL); the one-launch cost model then holds for the tiles that launch exists for"""
    if ksplit != 1 or cout <= 32 or cfg == 3:
        return None
    classes = 8 if transposed else 1
    bm, bn = TILE_DIMS[cfg]
    m_tiles, n_tiles = cdiv(cout, bm), cdiv(ntotal, bn)
    W = m_tiles * n_tiles * classes
    rounds, rem = W // cus, W % cus
    dual = (not transposed) and cfg in DUAL_TILES and dual_built
    if rounds < 1 or rounds >= (64 if dual else 16) or rem == 0:
        return None
    n_main = (rounds * cus) // (m_tiles * classes)                  # whole N tiles in the bulk
    if n_main < 1 or n_main >= n_tiles:
        return None
    pos_tail = ntotal - n_main * bn
    W_tail = cdiv(pos_tail, 64) * cdiv(cout, 64) * classes
    before = float(cdiv(W, cus))
    bulk = float(cdiv(n_main * m_tiles * classes, cus))
    small = (64.0 * 64.0) / float(bm * bn)
    if dual:
        after = bulk + float(W_tail) / float(cus) * small / 0.85
    else:
        after = bulk + float(cdiv(W_tail, cus)) * small / 0.8
    if after > (0.99 if dual else 0.97) * before:
        return None
    return n_main * bn


def ring(workgroups):
    """sparse_launch: a launch of the 64 x 64 tile with at most 384 workgroups runs the six-stage ring"""
    return workgroups <= RING_MAX_WGS


def plan(case, cus, dual_built=True):
    """launch_conv_mfma for the case on a device of `cus` compute units: the tile, the gather width, the cut and the launches"""
    l = case.layer
    assert case.ksplit == 0 and l.cin // 16 % 2 == 1, "the cases here are unsplit: conv_pick_ksplit must answer 1"
    assert l.act in ("none", "relu") or (l.act == "leaky_relu" and spec.act_param(l) <= 1), "a separate activation pass is one launch more"
    g = geometry(l, case.n_in, case.B)
    assert not matches_ktuned(g), (case.id, "matches a kTuned row: its tile would not follow the rules")
    cfg = case.tile & 15 if case.tile >= 0 else pick_tile(g.cout, g.Ntotal, g.transposed)
    classes = 8 if g.transposed else 1
    q = SimpleNamespace(g=g, cfg=cfg, vec=pick_vec(g), n_cut=tail_cut(g.cout, g.Ntotal, cfg, g.transposed, dual_built, cus), bits=0)
    if q.n_cut is not None:
        q.tail = g.Ntotal - q.n_cut
        q.bits |= FORM_CUT
        if dual_built and not g.transposed and g.cout > 32 and cfg in DUAL_TILES:
            q.bits |= FORM_ONE_LAUNCH                  # (the remainder inside the bulk's launch runs the two-stage loop)
            q.launches = 1
        else:
            q.launches = 2                             # the remainder: tile 3 over [n_cut, Ntotal)
            if ring(cdiv(g.cout, 64) * cdiv(q.tail, 64) * classes):
                q.bits |= FORM_RING
    else:
        q.tail = 0
        q.launches = 1
        bm, bn = TILE_DIMS[cfg]
        if cfg == 3 and ring(cdiv(g.cout, bm) * cdiv(g.Ntotal, bn) * classes):
            q.bits |= FORM_RING
    return q


def form(case, cus, dual_built=True):
    """(launch_form, launches) the profiler record of the case must hold"""
    q = plan(case, cus, dual_built)
    return q.bits, q.launches


def kind(bits, case):
    """one-launch / two-launch cut, or (uncut 64 x 64 tile) ring / two-stage; None for anything else"""
    if bits & FORM_ONE_LAUNCH:
        return "one-launch"
    if bits & FORM_CUT:
        return "two-launch"
    if case.tile >= 0 and (case.tile & 15) == 3:
        return "ring" if bits & FORM_RING else "two-stage"
    return None


# ---------------------------------------------------------------- the table
@dataclass(frozen=True)
class Row:
    name: str
    want: str                  # the form the row is in the table for, at 256 compute units
    tile: int                  # -1: the library's own pick
    layer: L
    n_in: int
    B: int
    n_cut: int = 0             # at 256 compute units (0: uncut)


c2 = lambda co, **kw: L("t", "conv2d", 16, co, 3, 1, 1, **kw)
c3 = lambda co, **kw: L("t", "conv3d", 16, co, 3, 1, 1, **kw)
dc = lambda co, **kw: L("t", "deconv3d", 16, co, 4, 2, 1, **kw)

ROWS = (
    # cut inside a sample and a row, tail of 2.5 tiles, half-empty 128-cout tile
    Row("t0-conv2d-16to48-e28-B42", "one-launch", 0, c2(48), 28, 42, 32768),
    # two cout tiles in both parts, tail % 64 = 48
    Row("t1-conv2d-16to70-e28-B43", "one-launch", 1, c2(70), 28, 43, 32768),
    # 128 x 256 bulk, three 64-cout tiles in the remainder
    Row("t4-conv2d-16to130-e28-B42", "one-launch", 4, c2(130), 28, 42, 32768),
    # a remainder of ONE partial tile (16 positions)
    Row("t7-conv2d-16to70-e20-B41", "one-launch", 7, c2(70), 20, 41, 16384),
    # dword gathers (edge % 4 != 0), odd Ntotal, tail % 64 = 39
    Row("t7-conv3d-16to70-e7-B49", "one-launch", 7, c3(70), 7, 49, 16384),
    # cut exactly on a sample boundary, 16-byte gathers
    Row("t0-conv3d-16to48-e8-B65", "one-launch", 0, c3(48), 8, 65, 32768),
    # stride-2 gather on both sides of the cut
    Row("t1-conv2d-16to70-s2-e56-B43", "one-launch", 1, L("t", "conv2d", 16, 70, 3, 2, 1), 56, 43, 32768),
    # a tile with no dual kernel; remainder = ring with n_begin != 0
    Row("t2-conv2d-16to70-e28-B28", "two-launch", 2, c2(70), 28, 28, 21760),
    # the same with a 128 x 64 bulk
    Row("t6-conv2d-16to48-e20-B41", "two-launch", 6, c2(48), 20, 41, 16384),
    # transposed: eight classes in both launches, tail % 64 = 13
    Row("t7-deconv3d-16to70-e5-B17", "two-launch", 7, dc(70), 5, 17, 2048),
    # 8-position remainder x 8 classes
    Row("t0-deconv3d-16to48-e6-B19", "two-launch", 0, dc(48), 6, 19, 4096),
    Row("t2-deconv3d-16to70-e6-B12", "two-launch", 2, dc(70), 6, 12, 2560),
    # the library's own pick (>= 1500 workgroups of the 64 x 128 tile) followed by a cut
    Row("auto-conv2d-16to130-e20-B164", "one-launch", -1, c2(130), 20, 164, 65536),
    # LeakyReLU with slope 1/2 in the epilogue of both parts; couts that fill their tiles (128 = 2 x 64), dword gathers
    Row("t7-conv3d-16to128-leaky-e7-B49", "one-launch", 7, c3(128, act="leaky_relu", act_param=0.5), 7, 49, 16384),
    # no BatchNorm (no scale vector) on a transposed cut
    Row("t7-deconv3d-16to70-nobn-e5-B17", "two-launch", 7, dc(70, bn=False), 5, 17, 2048),
    # the 64 x 64 tile forced: 2 x 196 = 392 workgroups run the two-stage K loop, 2 x 184 = 368 the six-stage ring
    Row("t3-conv2d-16to70-e28-B16", "two-stage", 3, c2(70), 28, 16),
    Row("t3-conv2d-16to70-e28-B15", "ring", 3, c2(70), 28, 15),
)


def _cases():
    out = []
    for i, r in enumerate(ROWS):                       # out_halo cycles through 0 .. 3 (tests/_exact_cases.py::_wino_shapes)
        out.append(XCase("lf-" + r.name, Data(r.layer, r.B, r.n_in, 1000 + i), tile=r.tile, algo=DIRECT, out_halo=i % 4, twice=True,
                         ran=("direct",)))
    return out


CASES = _cases()
ROW_OF = {c.id: r for c, r in zip(CASES, ROWS)}
ONE_LAUNCH = [c for c in CASES if ROW_OF[c.id].want == "one-launch"]


# ---------------------------------------------------------------- what a mistake in the cut's arithmetic would produce
def by_position(y, g):
    """the logical output (B, cout, ...) as (cout, classes, Ntotal): the axis the launches tile and the cut divides"""
    B, co = y.shape[0], y.shape[1]
    if not g.transposed:
        return y.reshape(B, co, 1, g.S).permute(1, 2, 0, 3).reshape(co, 1, g.Ntotal)
    n = g.Nw
    v = y.reshape(B, co, n, 2, n, 2, n, 2).permute(1, 3, 5, 7, 0, 2, 4, 6)          # (cout, rd, rh, rw, B, pd, ph, pw)
    return v.reshape(co, 8, g.Ntotal)


def cut_mutants(ref, q):
    """{name: wrong output in position space} for a cut plan q (plan()), from the exact output `ref`; only those that apply:
    shifted-back / shifted-on   the first (up to) 64 positions after n_cut hold the tile before / the tile after (a remainder that
                                starts at the wrong position: n_begin, the dual kernel's workgroup rebasing)
    ragged-zeroed               the last tail % 64 positions are missing (a ragged last tile dropped)
    halves-swapped              the two 64-cout tiles of the remainder's first position tile trade places (m / n tile decode)"""
    p = by_position(ref, q.g)
    first = min(64, q.tail)
    out = {}
    m = p.clone()
    m[..., q.n_cut:q.n_cut + first] = p[..., q.n_cut - 64:q.n_cut - 64 + first]
    out["shifted-back"] = m
    if q.tail >= 128:
        m = p.clone()
        m[..., q.n_cut:q.n_cut + 64] = p[..., q.n_cut + 64:q.n_cut + 128]
        out["shifted-on"] = m
    if q.tail % 64:
        m = p.clone()
        m[..., q.g.Ntotal - q.tail % 64:] = 0.0
        out["ragged-zeroed"] = m
    if q.g.cout > 64:
        h = min(64, q.g.cout - 64)
        m = p.clone()
        m[:h, :, q.n_cut:q.n_cut + first] = p[64:64 + h, :, q.n_cut:q.n_cut + first]
        m[64:64 + h, :, q.n_cut:q.n_cut + first] = p[:h, :, q.n_cut:q.n_cut + first]
        out["halves-swapped"] = m
    return p, out
