"""s3r_voxel_surface_points without a device: the header and bindings, every refusal (host-side: nothing is enqueued), the scratch
query's formula, the restatement's facts on named grids (tests/_surface64.py), every restated point on an exposed face of its grid (in
integers), the coverage the device test's table must have, and the mutants its bit-for-bit comparison must catch."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests import _surface64 as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32


@pytest.fixture(scope="module")
def lib(s3r):
    return s3r.load_library()


@pytest.fixture(autouse=True)
def _the_entry_exists(s3r, lib):
    """every test of this file is about s3r_voxel_surface_points: a restatement pins nothing without the entry point it restates"""
    assert hasattr(lib, "s3r_voxel_surface_points") and hasattr(s3r, "voxel_surface_points")


@pytest.fixture(scope="module")
def header():
    with open(os.path.join(ROOT, "include", "s3r.h")) as f:
        return f.read()


# ---------------------------------------------------------------- header, bindings
def _proto(header, ret, name):
    plain = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    m = re.search(r"\b%s\s+%s\s*\(([^)]*)\)\s*;" % (ret, name), plain)
    assert m, f"{name} is not declared in include/s3r.h"
    return [" ".join(a.split()) for a in m.group(1).split(",")]


def test_header_prototypes_match_the_bindings(s3r, lib, header):
    L = s3r._lib
    assert _proto(header, "int64_t", "s3r_voxel_surface_points_scratch_elems") == ["int batch", "int depth", "int height", "int width"]
    assert _proto(header, "int", "s3r_voxel_surface_points") == [
        "const float* occupancy", "float threshold", "const int64_t* sample_ids", "uint64_t seed", "float* points", "int32_t* n_faces",
        "int batch", "int depth", "int height", "int width", "int n_points", "float* scratch", "int64_t scratch_elems", "void* hip_stream"]
    assert L.SIGNATURES["s3r_voxel_surface_points_scratch_elems"] == (C.c_int64, [C.c_int] * 4)
    res, args = L.SIGNATURES["s3r_voxel_surface_points"]
    assert res == C.c_int and args == [C.c_void_p, C.c_float, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p] + [C.c_int] * 5 + \
        [C.c_void_p, C.c_int64, C.c_void_p]
    assert lib.s3r_voxel_surface_points.argtypes == args
    assert lib.s3r_abi_version() == 8 and "#define S3R_ABI_VERSION 8" in header
    assert {"voxel_surface_points", "SurfacePoints"} <= set(s3r.__all__) and s3r.ops.voxel_surface_points is s3r.voxel_surface_points


def test_the_header_states_the_rule(header):
    at = header.index("int64_t s3r_voxel_surface_points_scratch_elems")
    comment = " ".join(re.sub(r"\n \*", " ", header[header[:at].rfind("/* Ground-truth point clouds"):at]).split())
    for wording in ("occupied iff v > threshold", "a NaN is empty", "f = 2 a + side", "0 = D, 1 = H, 2 = W", "outside the grid or empty",
                    "ascending e = 6 * ((i0 * H + i1) * W + i2) + f", "Philox4x32-10", "(float)(w >> 8) * 2^-24", "purpose 0x100, j",
                    "k = (uint64)w0 * N >> 32", "inv_c = 1.f / (float)size_c", "t = (float)(i_a + side)", "u(w1) then u(w2)",
                    "t = (float)i_c + u", "t = t * inv_c; p_c = t - 0.5f", "uniformly by area", "uniformly by face count",
                    "(+0.0, +0.0, +0.0)", "no floating-point sum", "B (17 ceil(D H W / 64) + 1)", "before anything is enqueued",
                    "Every node is a kernel", "no atomics", "nothing is read on the host", "hip_stream", "hipStream_t",
                    "INVENTED by this build", "Profiler: no record"):
        assert wording in comment, wording


# ---------------------------------------------------------------- refusals and the scratch query (host-only)
A = 0x10000000      # non-NULL addresses far apart: every case is refused before anything could dereference them


def _call(lib, **kw):
    p = dict(occ=A * 1, thr=0.5, ids=A * 2, seed=7, points=A * 3, n_faces=A * 4, B=2, D=8, H=8, W=8, n=64, scratch=A * 5, elems=1 << 24)
    p.update(kw)
    return lib.s3r_voxel_surface_points(p["occ"], p["thr"], p["ids"], p["seed"], p["points"], p["n_faces"], p["B"], p["D"], p["H"], p["W"],
                                        p["n"], p["scratch"], p["elems"], None)


def _refused(lib, rc, *words):
    assert rc == -1, rc
    msg = lib.s3r_last_error().decode()
    assert msg.startswith("surface points")
    for w in words:
        assert w in msg, (w, msg)


@pytest.mark.parametrize("name", ["occ", "ids", "points"])
def test_a_null_pointer_is_refused(lib, name):
    _refused(lib, _call(lib, **{name: None}), "null")


@pytest.mark.parametrize("kw,word", [(dict(B=0), "batch"), (dict(B=-1), "batch"), (dict(n=0), "n_points"), (dict(n=-5), "n_points")])
def test_a_non_positive_count_is_refused(lib, kw, word):
    _refused(lib, _call(lib, **kw), word, "positive")


@pytest.mark.parametrize("kw", [dict(D=0), dict(H=0), dict(W=0), dict(D=257), dict(H=257), dict(W=257), dict(W=-1)])
def test_an_edge_outside_1_to_256_is_refused(lib, kw):
    _refused(lib, _call(lib, **kw), "1..256")
    g = dict(B=2, D=8, H=8, W=8)
    g.update(kw)
    assert lib.s3r_voxel_surface_points_scratch_elems(g["B"], g["D"], g["H"], g["W"]) == -1


def test_a_grid_above_2_21_voxels_is_refused(lib):
    _refused(lib, _call(lib, D=129, H=128, W=128), "2^21")
    assert lib.s3r_voxel_surface_points_scratch_elems(1, 129, 128, 128) == -1
    assert lib.s3r_voxel_surface_points_scratch_elems(1, 128, 128, 128) == 17 * 32768 + 1          # 2^21 itself is served
    assert lib.s3r_voxel_surface_points_scratch_elems(0, 8, 8, 8) == -1


def test_a_cloud_tensor_of_2_31_elements_is_refused(lib):
    _refused(lib, _call(lib, B=1 << 10, D=1, H=1, W=1, n=699051), "2^31")                         # 1024 * 699051 * 3 >= 2^31
    assert _call(lib, B=1 << 10, D=1, H=1, W=1, n=699050, points=None) == -1                     # ... one fewer gets past that check
    assert b"null" in lib.s3r_last_error()


@pytest.mark.parametrize("thr", [float("nan"), float("inf"), float("-inf")])
def test_a_non_finite_threshold_is_refused(lib, thr):
    _refused(lib, _call(lib, thr=thr), "threshold", "finite")


def test_scratch_is_checked_against_the_query(lib):
    need = lib.s3r_voxel_surface_points_scratch_elems(2, 8, 8, 8)
    assert need == 2 * (17 * 8 + 1)
    _refused(lib, _call(lib, scratch=None), "scratch", str(need))
    _refused(lib, _call(lib, elems=need - 1), "scratch", str(need))
    _refused(lib, _call(lib, elems=0), "scratch")


def test_overlaps_are_refused(lib):
    need = lib.s3r_voxel_surface_points_scratch_elems(2, 8, 8, 8)
    occ_bytes, pts_bytes = 4 * 2 * 512, 12 * 2 * 64
    _refused(lib, _call(lib, points=A * 1), "overlap", "occupancy")
    _refused(lib, _call(lib, points=A * 1 + occ_bytes - 4), "overlap", "occupancy")
    _refused(lib, _call(lib, points=A * 2 + 12), "overlap", "sample_ids")
    _refused(lib, _call(lib, n_faces=A * 1 + 8), "overlap", "occupancy")
    _refused(lib, _call(lib, n_faces=A * 2 + 4), "overlap", "sample_ids")
    _refused(lib, _call(lib, n_faces=A * 3 + pts_bytes - 4), "overlap", "points", "n_faces")
    _refused(lib, _call(lib, scratch=A * 1 + 16, elems=need), "overlap", "occupancy")
    _refused(lib, _call(lib, scratch=A * 2, elems=need), "overlap", "sample_ids")
    _refused(lib, _call(lib, scratch=A * 3 + 4, elems=need), "overlap", "points", "scratch")
    _refused(lib, _call(lib, scratch=A * 4 - 4 * need + 4, elems=need), "overlap", "n_faces", "scratch")


def test_scratch_query_formula(lib):
    for B, D, H, W in ((1, 1, 1, 1), (3, 2, 3, 5), (3, 5, 7, 9), (2, 8, 8, 8), (1, 4, 4, 17), (1, 1, 1, 256), (32, 32, 32, 32), (1, 8, 256, 256)):
        assert lib.s3r_voxel_surface_points_scratch_elems(B, D, H, W) == B * (17 * -(-(D * H * W) // 64) + 1)
    assert lib.s3r_voxel_surface_points_scratch_elems(4096, 128, 128, 128) == -1      # 2^31 elements or more: split the batch


def test_python_surface_refuses_host_tensors(s3r):
    import torch
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        s3r.voxel_surface_points(torch.zeros(1, 4, 4, 4), torch.zeros(1, dtype=torch.int64))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        s3r.SurfacePoints(8)(torch.zeros(1, 4, 4, 4), torch.zeros(1, dtype=torch.int64))
    cfg = s3r.TrainConfig(variant="point")
    assert (cfg.cloud_points, cfg.cloud_seed) == (2048, 0) and cfg.as_dict()["cloud_points"] == 2048


# ---------------------------------------------------------------- the restatement's facts, one named grid each
def _on_the_cube_surface(p):
    return np.all(np.abs(p) <= 0.5) and np.all(np.max(np.abs(p), axis=-1) == 0.5)


def test_one_voxel_in_a_1x1x1_grid():
    p, n = R.surface32(np.ones((1, 1, 1, 1), F), [3], 257)
    assert n.tolist() == [6] and _on_the_cube_surface(p[0])
    assert set(R.drawn(np.ones((1, 1, 1), F), 3, 257).tolist()) == set(range(6))


def test_the_full_32_cube_has_6144_faces():
    p, n = R.surface32(R.grid("full", R.BIG)[None], [1], 2048)
    assert n.tolist() == [6 * 32 * 32] and _on_the_cube_surface(p[0])


def test_the_32_cube_checkerboard_has_98304_faces():
    _, n = R.surface32(R.grid("checkerboard", R.BIG)[None], [1], 8)
    assert n.tolist() == [98304] == [6 * 32 ** 3 // 2]


def test_a_radius_12_ball_in_the_32_cube_has_2688_faces():
    p, n = R.surface32(R.grid("ball", R.BIG)[None], [1], 2048)
    assert n.tolist() == [2688]
    r = np.sqrt((p[0].astype(np.float64) ** 2).sum(-1)) * 32
    assert r.max() <= 12 + np.sqrt(3) and r.min() >= 12 - 2 * np.sqrt(3)


def test_an_empty_grid_gives_zeros_and_count_0():
    p, n = R.surface32(np.zeros((1, 5, 7, 9), F), [9], 65)
    assert n.tolist() == [0] and not p.view(np.uint32).any()               # +0.0, not -0.0


def test_a_nan_voxel_is_empty():
    g = np.zeros((1, 3, 3, 3), F)
    g[0, 1, 1, 1] = np.nan
    assert R.surface32(g, [0], 4)[1].tolist() == [0]
    g[:] = 1
    g[0, 1, 1, 1] = np.nan                                                 # a NaN hole in a full grid exposes its six neighbours' faces
    assert R.surface32(g, [0], 4)[1].tolist() == [6 * 9 + 6]
    g[0, 1, 1, 1] = 0.5                                                    # the threshold itself: empty as well
    assert R.surface32(g, [0], 4)[1].tolist() == [6 * 9 + 6]


@pytest.mark.parametrize("kind,shape", R.CASES + [("ball", R.BIG), ("checkerboard", R.BIG)], ids=lambda v: str(v).replace(" ", ""))
def test_every_restated_point_lies_on_an_exposed_face(kind, shape):
    """in integers: the normal-axis coordinate times the edge is an integer, and the voxel pair next to it is (occupied, empty or outside)"""
    g = R.grid(kind, shape)
    occ = R.occupied(g, 0.5)
    p, n = R.surface32(g[None], [R.IDS[2]], 257)
    if n[0] == 0:
        assert not p.any()
        return
    size = np.array(shape)
    x = (p[0].astype(np.float64) + 0.5) * size
    assert np.all(p[0] >= -0.5) and np.all(p[0] <= 0.5)

    def filled(cell):
        return all(0 <= cell[c] < size[c] for c in range(3)) and bool(occ[tuple(cell)])

    for q, pt in zip(x, p[0]):
        ok = False
        for a in range(3):
            m = int(round(q[a]))                                           # the plane: p_a must be the image of the INTEGER m, bit for bit
            inv = F(F(1) / F(size[a]))
            if F(F(F(m) * inv) - F(0.5)).view(np.int32) != pt[a].view(np.int32):
                continue
            others = [c for c in range(3) if c != a]
            # (float)i + u may round up to i + 1: a point on a cell's border belongs to both cells
            cand = [sorted({int(np.clip(np.floor(q[c] + d), 0, size[c] - 1)) for d in (-1e-4, 1e-4)}) for c in others]
            for i in cand[0]:
                for j in cand[1]:
                    lower, upper = [0, 0, 0], [0, 0, 0]
                    lower[others[0]] = upper[others[0]] = i
                    lower[others[1]] = upper[others[1]] = j
                    lower[a], upper[a] = m - 1, m
                    ok |= filled(lower) != filled(upper)                   # (occupied, empty or outside), either way round
        assert ok, (kind, shape, q)


# ---------------------------------------------------------------- coverage of the device test's table
def _chunk_of(e):
    return e // 6 // 64


def test_the_device_tests_table_covers_the_paths():
    assert R.SEED == 7 and any(i >= 2 ** 32 for i in R.IDS) and R.N_POINTS == [1, 63, 64, 65, 257]
    assert R.SHAPES == [(1, 1, 1), (2, 3, 5), (5, 7, 9), (8, 8, 8), (4, 4, 17), (1, 1, 256)]
    assert R.KINDS == ["full", "empty", "corner", "checkerboard", "half", "specials"]
    ends = ragged = directions = gap = False
    for shape in ((2, 3, 5), (5, 7, 9), (8, 8, 8), (4, 4, 17)):
        g = R.grid("half", shape)
        e, d = R.faces(g), R.drawn(g, R.IDS[0], 257)
        V = int(np.prod(shape))
        assert e[0] in d and e[-1] in d, shape                             # face 0 and face N - 1 drawn (R.IDS[0] was searched for it)
        ends = True
        assert set((d % 6).tolist()) == set(range(6)), shape             # all six directions
        directions = True
        if V > 64:
            assert _chunk_of(d).min() == 0 and _chunk_of(d).max() == (V - 1) // 64       # the first and the last chunk
        ragged |= V % 64 != 0 and V > 64 and _chunk_of(d).max() == V // 64
    for shape in ((5, 7, 9), (4, 4, 17)):                                  # a chunk with zero faces between two drawn chunks
        g = R.grid("gap", shape)
        counts = np.bincount(_chunk_of(R.faces(g)), minlength=-(-g.size // 64))
        chunks = set(_chunk_of(R.drawn(g, R.IDS[0], 257)).tolist())
        assert any(counts[c] == 0 and min(chunks) < c < max(chunks) for c in range(len(counts))), (counts, chunks)
        gap = True
    assert ends and ragged and directions and gap
    # the specials hold NaN, both infinities and the threshold itself
    s = R.grid("specials", (5, 7, 9))
    assert np.isnan(s).any() and np.isposinf(s).any() and np.isneginf(s).any() and (s == F(0.5)).any()
    # both draw paths of the kernel: the prefix staged (<= 4096 chunks) and read from global memory
    assert -(-int(np.prod(R.BIG)) // 64) <= 4096 < -(-int(np.prod(R.ABOVE_LDS)) // 64)


def test_mutants_of_the_restatement_change_the_device_tests_result():
    hit = {m: False for m in R.MUTANTS}
    for kind, shape in (("half", (5, 7, 9)), ("specials", (4, 4, 17)), ("half", (8, 8, 8))):
        assert (kind, shape) in R.CASES
        grids = R.batch(kind, shape)
        want = R.surface32(grids, R.IDS, 257)
        for m in R.MUTANTS:
            got = R.surface32(grids, R.IDS, 257, mutant=m)
            if any(not np.array_equal(g.view(np.int32), w.view(np.int32)) for g, w in zip(got, want)):
                hit[m] = True
    assert all(hit.values()), hit
