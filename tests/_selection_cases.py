"""The inputs of tests/test_selection_{cpu,gpu}.py: tie-dense and special-value data placed where the selection kernels branch, and
the COVERAGE CONDITIONS each case must meet.  The conditions are computed from the references alone (tests/_select_ref.py,
tests/_disp64.py), are stated here once and are asserted by both test files, so a case cannot quietly stop covering its boundary.

Chamfer (csrc/s3r_chamfer.hip): a direction's candidates are staged in passes of 2048, a pass is cut into four slices of
ceil(count / 4), a slice is taken in blocks of 8 and a tail of < 8.  Direction 0 is p's queries against q's candidates, direction 1
the reverse.  A direction is MULTI-PASS when it has more than 2048 candidates.

  C1  lattice cases, every direction with at least 2048 candidates: >= 90 % of its queries have two or more equal minima;
  C2  lattice cases, every multi-pass direction; shuffled-copies cases, direction 0 (the one whose candidates hold the copies):
      >= 50 % of its queries have equal minima in two different passes;
  C3  the same directions: >= 100 queries have their FIRST minimum outside pass 0;
  EXEMPT lists, with the reason, the (case, direction, condition) triples that cannot meet C2 / C3 by their shape.  Nothing is
  exempt from C1.  The shifted variant of a case (p moved by half a cell: a query's nearest candidates are then the corners of its
  cell, and one of the eight is nearly always in pass 0) must meet C1 and C2; C3 is a condition of the plain variant.

Read-outs: in every WTA / soft case >= 25 % of the 2 B H W pixels have a minimum shared by two or more but not all of their
disparities, with the first of them at d > 0.
"""
from __future__ import annotations

import functools

import numpy as np
import torch

from tests import _disp64 as D64
from tests import _select_ref as SR

TIES_SHARE, CROSS_PASS_SHARE, LATE_FIRST_QUERIES, READOUT_SHARE = 0.90, 0.50, 100, 0.25

# ---------------------------------------------------------------- Chamfer: lattice clouds
# coordinates k / L per axis, L in {4, 8, 16}: every difference, square and sum is exact in fp32, so equal minima are EQUAL.
# The number of lattice points (the product of the three L) is chosen against the cloud size: few enough that nearly every query
# has several equal minima, many enough (5000 x 4500) that some lattice points first appear after the first pass.
LATTICE = {  # id: ((B, N, M), (Lx, Ly, Lz))
    "lat-5000x4500": ((2, 5000, 4500), (8, 8, 8)),
    "lat-2049x6200": ((2, 2049, 6200), (4, 4, 4)),
    "lat-300x2100": ((3, 300, 2100), (4, 4, 4)),
    "lat-2048x2048": ((1, 2048, 2048), (8, 4, 4)),
    "lat-37x4097": ((2, 37, 4097), (16, 4, 4)),
    "lat-4097x37": ((2, 4097, 37), (16, 4, 4)),
}
# q holds every distinct point two or three times at uniformly random positions; p is the distinct points
SHUFFLED = {"shuf-2048": 2048, "shuf-2049": 2049, "shuf-4100": 4100, "shuf-6151": 6151}

EXEMPT = {
    ("lat-2049x6200", 0, "C3"): "64 lattice points among 2048 candidates: every one of them occurs in pass 0",
    ("lat-2049x6200", 1, "C2"): "2049 candidates: the second pass holds one",
    ("lat-2049x6200", 1, "C3"): "2049 candidates: the second pass holds one",
    ("lat-300x2100", 0, "C3"): "64 lattice points among 2048 candidates: every one of them occurs in pass 0",
    ("lat-37x4097", 0, "C3"): "74 queries",
    ("lat-4097x37", 1, "C3"): "74 queries",
    ("shuf-2049", 0, "C2"): "2049 candidates: the second pass holds one",
    ("shuf-2049", 0, "C3"): "2049 candidates: the second pass holds one",
}


def _seed(name):
    return sum((i + 1) * ord(ch) for i, ch in enumerate(name))


@functools.lru_cache(maxsize=None)
def chamfer_case(name, shifted=False):
    """(p, q) float32 numpy of a LATTICE or SHUFFLED case; shifted: p moved by a constant, so the tied minimum is not zero"""
    g = torch.Generator().manual_seed(_seed(name))
    if name in LATTICE:
        (B, N, M), L = LATTICE[name]
        Lt = torch.tensor(L, dtype=torch.float32)
        p = torch.stack([torch.randint(0, l, (B, N), generator=g) for l in L], -1).float() / Lt
        q = torch.stack([torch.randint(0, l, (B, M), generator=g) for l in L], -1).float() / Lt
        if shifted:
            p = p + 1 / (2 * Lt)                                   # half a cell: exact
    else:
        M = SHUFFLED[name]
        K = 2 * M // 5                                             # every point twice, M - 2 K of them a third time
        pts = torch.rand(2, K, 3, generator=g)
        q = torch.empty(2, M, 3)
        for b in range(2):
            src = torch.cat([torch.arange(K), torch.arange(K), torch.randperm(K, generator=g)[:M - 2 * K]])
            q[b] = pts[b, src[torch.randperm(M, generator=g)]]
        p = pts + 0.03125 if shifted else pts
    return p.numpy().copy(), q.numpy().copy()


@functools.lru_cache(maxsize=None)
def chamfer_want(name, shifted=False):
    return SR.chamfer_scan(*chamfer_case(name, shifted))


def chamfer_conditions(name):
    """[(direction, condition)] a case must meet"""
    lattice = name in LATTICE
    p, q = chamfer_case(name)
    out = []
    for direction, cands in ((0, q.shape[1]), (1, p.shape[1])):
        if lattice and cands >= SR.CH_TILE:
            out.append((direction, "C1"))
        if cands > SR.CH_TILE and (lattice or direction == 0):
            out += [(direction, c) for c in ("C2", "C3") if (name, direction, c) not in EXEMPT]
    return out


@functools.lru_cache(maxsize=None)
def chamfer_coverage(name, shifted=False):
    """{direction: (queries, share with >= 2 equal minima, share with equal minima in >= 2 passes, queries whose first minimum is
    outside pass 0)} from the reference alone"""
    p, q = chamfer_case(name, shifted)
    d1, d2, i1, i2 = chamfer_want(name, shifted)
    out = {}
    for direction, (a, c, d, i) in enumerate(((p, q, d1, i1), (q, p, d2, i2))):
        count, passes = SR.chamfer_tie_stats(a, c, d)
        out[direction] = (d.size, float((count >= 2).mean()), float((passes >= 2).mean()), int((i >= SR.CH_TILE).sum()))
    return out


def check_chamfer_coverage(name, shifted=False):
    cov = chamfer_coverage(name, shifted)
    for direction, cond in chamfer_conditions(name):
        n, ties, cross, late = cov[direction]
        what = f"{name}{'+shift' if shifted else ''} direction {direction}: {n} queries, {ties:.1%} tied, {cross:.1%} across passes, {late} late firsts"
        if cond == "C1":
            assert ties >= TIES_SHARE, what
        elif cond == "C2":
            assert cross >= CROSS_PASS_SHARE, what
        elif not (shifted and name in LATTICE):
            assert late >= LATE_FIRST_QUERIES, what
    return cov


# ---------------------------------------------------------------- Chamfer: planted indices
# a far, all-distinct filler cloud of M candidates; the one near point is copied to every index of J: every query's first minimum
# is min(J).  M = 6200: three full passes (slices of 512: blocks only) and a last pass of 56 (slices of 14: one block, a tail of 6).
PLANT_M, PLANT_N = 6200, 130
PLANTED = {
    "block-7|8": (7, 8),
    "slice-511|512": (511, 512),
    "pass-2047|2048": (2047, 2048),
    "pass0-slice3|pass1-slice0": (1600, 2100),      # an earlier pass in a later slice against a later pass in slice 0
    "pass1|pass2-same-slice": (2053, 4097),
    "last": (PLANT_M - 1,),
    "first|last": (0, PLANT_M - 1),
    "last-pass-block|tail": (6144 + 7, 6144 + 8),   # slice 0 of the last pass: the end of its block, the start of its tail
    "last-block|last-tail": (6144 + 49, 6144 + 50),  # slice 3 of the last pass
    "last-pass-slices": (6144 + 13, 6144 + 14, 6144 + 27, 6144 + 28, 6144 + 41, 6144 + 42),
    "same-block": (4096 + 9, 4096 + 11, 4096 + 15),
    "every-pass": (6190, 4100, 2060, 2040),
}


@functools.lru_cache(maxsize=None)
def planted_case(name):
    """(queries (B,PLANT_N,3), candidates (B,PLANT_M,3)); run it as (p, q) and, swapped, as (q, p)"""
    g = torch.Generator().manual_seed(_seed(name))
    queries = torch.rand(2, PLANT_N, 3, generator=g)
    cands = 10 + torch.rand(2, PLANT_M, 3, generator=g)
    near = torch.tensor([[0.5, 0.25, 0.75], [0.125, 0.5, 0.375]])
    for j in PLANTED[name]:
        cands[:, j] = near
    return queries.numpy().copy(), cands.numpy().copy()


# ---------------------------------------------------------------- Chamfer: non-finite input
# q: 2100 candidates, a full pass (slices of 512, blocks only) and a pass of 52 (slices of 13: one block, a tail of 5);
# p: 300 candidates of the other direction, one pass, slices of 75 (nine blocks, a tail of 3).  Lattice of 64 points: every query
# has equal minima all over the other cloud, so a special value at any of these places moves some query's first minimum.
NF_SHAPE = (2, 300, 2100)
NF_Q_AT = (3, 515, 1027, 1539, 2047, 2048 + 2, 2048 + 10, 2048 + 13 + 2, 2048 + 13 + 10, 2048 + 26 + 9, 2048 + 39 + 12)
NF_P_AT = (5, 73, 75 + 4, 150 + 74, 225 + 10, 299)
NONFINITE = ("nan", "+inf", "-inf", "inf-inf", "mixed")


@functools.lru_cache(maxsize=None)
def nonfinite_case(kind):
    B, N, M = NF_SHAPE
    g = torch.Generator().manual_seed(_seed(kind))
    p = (torch.randint(0, 4, (B, N, 3), generator=g).float() / 4).numpy()
    q = (torch.randint(0, 4, (B, M, 3), generator=g).float() / 4).numpy()
    nan, inf = np.float32("nan"), np.float32("inf")
    for n, j in enumerate(NF_Q_AT):
        axis = n % 3
        if kind == "nan":
            q[:, j, axis] = nan
        elif kind in ("+inf", "inf-inf"):
            q[:, j, axis] = inf
        elif kind == "-inf":
            q[:, j, axis] = -inf
        else:
            q[:, j, axis] = (nan, inf, -inf)[n % 3]
            q[0, j, (axis + 1) % 3] = (inf, nan, nan)[n % 3]
    for n, i in enumerate(NF_P_AT):
        axis = n % 3
        if kind == "nan":
            p[:, i, axis] = nan
        elif kind == "+inf":
            p[:, i, axis] = -inf                                   # the opposite sign: no inf - inf, every such distance is +inf
        elif kind == "-inf":
            p[:, i, axis] = inf
        elif kind == "inf-inf":
            p[:, i, :] = inf                                       # against q's +inf on any axis: an inf - inf = NaN distance
        else:
            p[:, i, axis] = (inf, -inf, nan)[n % 3]
    return p, q


# ---------------------------------------------------------------- read-outs
READOUT_SHAPES = [(3, 32, 28, 28, 28), (2, 5, 7, 13, 40), (2, 8, 12, 40, 40)]      # (B, C, H, W, max_disp)
READOUT_UP = {(3, 32, 28, 28, 28): (224, 224), (2, 5, 7, 13, 40): (37, 100), (2, 8, 12, 40, 40): (30, 64)}
_KEEP = {32: 0.08, 5: 0.2, 8: 0.3}      # share of the feature entries kept non-zero: one to two and a half per pixel


@functools.lru_cache(maxsize=None)
def readout_feats(shape):
    """integer features in {-2..2}, thinned: costs are small integers, so two disparities often share the minimum"""
    B, Cc, H, W, _ = shape
    g = torch.Generator().manual_seed(sum(shape))
    out = []
    for _ in range(2):
        v = torch.randint(-2, 3, (B, Cc, H, W), generator=g).float()
        out.append((v * (torch.rand(B, Cc, H, W, generator=g) < _KEEP[Cc])).numpy())
    return tuple(out)


@functools.lru_cache(maxsize=None)
def readout_ties(shape):
    """per direction: (costs (B,H,W,Dm) fp32 with +inf outside a pixel's range, the mask of the pixels whose minimum is shared by two
    or more but not all of its disparities with the first at d > 0, the mean index of the minimum set)"""
    fl, fr = readout_feats(shape)
    out = []
    for right in (False, True):
        c = D64.costs(fl, fr, shape[4], right)
        n = np.isfinite(c).sum(-1)
        m = c[..., 0].copy()
        for d in range(1, c.shape[-1]):                            # (costs are finite non-negative integers inside the range)
            m = np.where(c[..., d] < m, c[..., d], m)
        at = c == m[..., None]
        k = at.sum(-1)
        marked = (k >= 2) & (k < n) & ~at[..., 0]
        mean = (at * np.arange(c.shape[-1])).sum(-1) / k
        out.append((c, marked, mean))
    return out


def check_readout_coverage(shape):
    marked = np.stack([m for _, m, _ in readout_ties(shape)])
    share = float(marked.mean())
    assert share >= READOUT_SHARE, f"{shape}: {share:.1%} of the pixels have a partly shared minimum with the first at d > 0"
    return share


# ---------------------------------------------------------------- IoU
IOU_V = (1, 255, 256, 257, 32768)
IOU_BIG_V = 2 ** 24 + 1027      # an odd count above 2^24 whose round-to-nearest-even and truncated fp32 values differ
IOU_BIG_UNSET = 26              # voxels of gt left empty in the big case: the intersection is such a count too, and rounds DOWN where
                                # the union rounds up, so a truncating conversion moves the quotient by two ulps


def iou_palette(th):
    t = np.float32(th)
    return np.array([t, np.nextafter(t, np.float32(-1)), np.nextafter(t, np.float32(2)), 0.0, -0.0, 1.0, np.nan, np.inf, -np.inf],
                    np.float32)


@functools.lru_cache(maxsize=None)
def iou_case(V, th):
    """(pred, gt) (4,V): two samples drawn from the palette, one whose pred is all above and gt from the palette, one with nothing
    above the threshold on either side (an empty union)"""
    g = torch.Generator().manual_seed(V * 31 + int(th * 100))
    pal = iou_palette(th)
    draw = lambda n=len(pal): pal[torch.randint(0, n, (V,), generator=g).numpy()]      # noqa: E731
    low = pal[[0, 1, 3, 4, 6, 8]]                                  # th itself, below it, +-0, NaN, -inf: none is occupied
    pred = np.stack([draw(), draw(), pal[[2, 5, 7]][torch.randint(0, 3, (V,), generator=g).numpy()],
                     low[torch.randint(0, 6, (V,), generator=g).numpy()]])
    gt = np.stack([draw(), draw(), draw(), low[torch.randint(0, 6, (V,), generator=g).numpy()]])
    return pred, gt


def iou_big_case():
    """(pred, gt) (1, IOU_BIG_V): every voxel of pred set, all but IOU_BIG_UNSET of gt: union and intersection both pass 2^24"""
    pred = np.ones((1, IOU_BIG_V), np.float32)
    gt = np.ones((1, IOU_BIG_V), np.float32)
    gt[0, 1000:1000 + IOU_BIG_UNSET] = 0
    return pred, gt


# ---------------------------------------------------------------- metrics
FLT_MAX = np.finfo(np.float32).max


def metrics_case(P=1000):
    """(pred, gt) (5,P): ground truth of -0.0 (valid), subnormal ground truth, FLT_MAX against -FLT_MAX (the fp32 difference
    overflows: an infinite error, an infinite EPE), errors exactly on 1, 3 and 0.05 gt, and a sample mixing them with invalid pixels"""
    g = torch.Generator().manual_seed(77)
    pred = (torch.rand(5, P, generator=g) * 8).numpy()
    gt = (torch.rand(5, P, generator=g) * 8).numpy()
    gt[0] = -0.0
    pred[0, ::4] = 1.0
    pred[0, 1::4] = 3.0
    pred[0, 2::4] = -0.0
    gt[1] = np.float32(1e-45)
    gt[1, ::2] = np.float32(1e-40)
    pred[1, ::3] = 0.0
    pred[1, 1::3] = np.float32(1e-40)
    pred[1, 2::3] = np.float32(2.0 ** -126)                        # the smallest normal number
    gt[2, 17] = FLT_MAX
    pred[2, 17] = -FLT_MAX
    gt[3, :3] = (10.0, 10.0, 100.0)
    pred[3, :3] = (11.0, 13.0, 105.0)
    gt[4, ::5] = -0.0
    gt[4, 1::5] = np.float32(1e-45)
    gt[4, 2::5] = np.inf
    gt[4, 3::5] = np.nan
    gt[4, 4::5] = -np.float32(1e-45)                               # a negative subnormal is below zero: invalid
    gt[4, 7] = FLT_MAX
    pred[4, 7] = FLT_MAX
    return pred.astype(np.float32), gt.astype(np.float32)
