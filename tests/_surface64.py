"""numpy restatement of s3r_voxel_surface_points (include/s3r.h) for tests/test_surface_points_{cpu,gpu}.py: integers, and one rounded
fp32 operation per line; no notion of launches or chunks.  Philox and `unit` are tests/_augment64.py's.

  exposure(grid, threshold)    (D, H, W) uint8: bit f = 2 a + side set where that face of an occupied voxel is exposed
  faces(grid, threshold)       the exposed faces' numbers e = 6 v + f, ascending
  surface32(grids, ids, n_points, seed, threshold, mutant)
                               ((B, n_points, 3) fp32 points, (B,) int32 face counts); `mutant` builds the wrong versions the cases
                               must tell from the right one (MUTANTS)
  drawn(grid, id, n_points, seed, threshold)
                               the face numbers e the points of one sample land on (what the coverage conditions are about)
  CASES / grid(kind, shape, seed)
                               the device test's table: grid kinds, shapes, ids, point counts
"""
import numpy as np

from tests._augment64 import _id, _key, philox, unit

F = np.float32
PURPOSE = 0x100
MUTANTS = ("descending_faces", "side_major_faces", "modulo_index", "swapped_units", "side_ignored", "not_strict", "fused_scale")
SEED = 7


def occupied(grid, threshold, mutant=None):
    g = np.asarray(grid, F)
    with np.errstate(invalid="ignore"):
        return (g >= F(threshold)) if mutant == "not_strict" else (g > F(threshold))


def exposure(grid, threshold=0.5, mutant=None):
    occ = occupied(grid, threshold, mutant)
    mask = np.zeros(occ.shape, np.uint8)
    for a in range(3):
        for side in range(2):
            nb = np.zeros_like(occ)                                      # the neighbour's occupancy; outside the grid: empty
            src = [slice(None)] * 3
            dst = [slice(None)] * 3
            if side == 0:
                dst[a], src[a] = slice(1, None), slice(0, -1)
            else:
                dst[a], src[a] = slice(0, -1), slice(1, None)
            nb[tuple(dst)] = occ[tuple(src)]
            f = 2 * side + a if mutant == "side_major_faces" else 2 * a + side
            mask |= ((occ & ~nb).astype(np.uint8) << np.uint8(f))
    return mask


def faces(grid, threshold=0.5, mutant=None):
    mask = exposure(grid, threshold, mutant).reshape(-1)
    bits = (mask[:, None] >> np.arange(6, dtype=np.uint8)[None, :]) & np.uint8(1)
    e = np.flatnonzero(bits.reshape(-1)).astype(np.int64)               # 6 v + f, ascending
    return e[::-1].copy() if mutant == "descending_faces" else e


def _words(sample_id, n_points, seed):
    i0, i1 = _id(sample_id)
    return philox((i0, i1, PURPOSE, np.arange(n_points, dtype=np.uint32)), _key(seed))


def _index(w0, N, mutant=None):
    if mutant == "modulo_index":
        return (w0.astype(np.uint64) % np.uint64(N)).astype(np.int64)
    return ((w0.astype(np.uint64) * np.uint64(N)) >> np.uint64(32)).astype(np.int64)


def drawn(grid, sample_id, n_points, seed=SEED, threshold=0.5):
    e = faces(grid, threshold)
    if not e.size:
        return e
    return e[_index(_words(sample_id, n_points, seed)[0], e.size)]


def _sample(grid, sample_id, n_points, seed, threshold, mutant):
    size = grid.shape
    e = faces(grid, threshold, mutant)
    out = np.zeros((n_points, 3), F)
    if not e.size:
        return out, 0
    w = _words(sample_id, n_points, seed)
    e = e[_index(w[0], e.size, mutant)]
    v, f = e // 6, e % 6
    a, side = f // 2, f % 2                                              # (the side-major mutant mis-builds the mask only)
    if mutant == "side_ignored":
        side = np.zeros_like(side)
    idx = [v // (size[1] * size[2]), (v // size[2]) % size[1], v % size[2]]
    u1, u2 = unit(w[1]), unit(w[2])
    if mutant == "swapped_units":
        u1, u2 = u2, u1
    first = np.where(a == 0, 1, 0)                                       # the lower in-plane axis
    for c in range(3):
        inv = F(F(1) / F(size[c]))
        normal = (idx[c] + side).astype(F)
        u = np.where(c == first, u1, u2).astype(F)
        if mutant == "fused_scale":                                      # (i + u) * inv rounded once
            plane = ((idx[c].astype(np.float64) + u.astype(np.float64)) * np.float64(inv)).astype(F)
            t = np.where(a == c, (normal * inv).astype(F), plane).astype(F)
        else:
            plane = (idx[c].astype(F) + u).astype(F)
            t = np.where(a == c, normal, plane).astype(F)
            t = (t * inv).astype(F)
        out[:, c] = (t - F(0.5)).astype(F)
    return out, int(faces(grid, threshold, mutant).size)


def surface32(grids, ids, n_points, seed=SEED, threshold=0.5, mutant=None):
    assert mutant is None or mutant in MUTANTS
    grids = np.asarray(grids, F)
    pts = np.zeros((grids.shape[0], n_points, 3), F)
    n = np.zeros(grids.shape[0], np.int32)
    for b in range(grids.shape[0]):
        pts[b], n[b] = _sample(grids[b], ids[b], n_points, seed, threshold, mutant)
    return pts, n


# ---------------------------------------------------------------- the device test's table
SHAPES = [(1, 1, 1), (2, 3, 5), (5, 7, 9), (8, 8, 8), (4, 4, 17), (1, 1, 256)]
KINDS = ["full", "empty", "corner", "checkerboard", "half", "specials"]
N_POINTS = [1, 63, 64, 65, 257]
BIG = (32, 32, 32)
ABOVE_LDS = (8, 256, 256)           # 8192 chunks: the draw kernel reads the prefix from global memory above 4096
# per batch row; the middle row of a B = 3 batch is the empty grid.  Row 0's id was searched on the CPU: under SEED with 257 points it draws
# face 0, face N - 1 and all six directions of every half-full grid of the table (tests/test_surface_points_cpu.py asserts it)
IDS = [1, 0, 2 ** 32 + 5]


def grid(kind, shape, seed=0):
    r = np.random.default_rng(1000 * seed + 7 * shape[0] + 11 * shape[1] + 13 * shape[2])
    g = np.zeros(shape, F)
    if kind == "full":
        g[:] = 1
    elif kind == "corner":
        g[-1, -1, -1] = 1
    elif kind == "checkerboard":
        i = np.indices(shape).sum(0)
        g[i % 2 == 0] = 1
    elif kind in ("half", "specials"):
        g = (r.random(shape) < 0.5).astype(F)
        if kind == "specials":
            flat = g.reshape(-1)
            pick = r.integers(0, 4, flat.size)
            flat[pick == 1] = np.nan
            flat[(pick == 2) & (flat > 0)] = np.inf
            flat[(pick == 2) & (flat == 0)] = -np.inf
            flat[pick == 3] = F(0.5)                                     # the threshold itself: empty
    elif kind == "ball":
        c = (np.indices(shape) - (np.array(shape).reshape(3, 1, 1, 1) - 1) / 2.0)
        g[(c ** 2).sum(0) <= 144] = 1
    elif kind == "gap":                                                  # occupied only in the first and the last 64-voxel chunk
        flat = g.reshape(-1)
        flat[:min(64, flat.size)] = 1
        flat[-min(64, flat.size):] = 1
    else:
        assert kind == "empty", kind
    return g


def batch(kind, shape, seed=0):
    """the B = 3 batch of a table row: the kind, an empty grid in the middle, the kind from another seed"""
    return np.stack([grid(kind, shape, seed), grid("empty", shape), grid(kind, shape, seed + 1)])


CASES = [(kind, shape) for shape in SHAPES for kind in KINDS] + [("gap", (5, 7, 9)), ("gap", (4, 4, 17))]
