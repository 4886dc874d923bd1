"""s3r_cost_volume_backward without a GPU: the declaration and its binding, the formula against torch's float64 autograd through the
oracle's own forward, the restated fp32 order against float64 (exact on integer lattices, inside the derived bound on random data),
the mutants of the order that the GPU table's data sets must tell apart, and the host-side half of the entry point (every refusal
happens before anything is launched: a HIP call would have given S3R_ERR_HIP on a host without a device)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests import _costvol64 as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, INVALID = 0, -1
_ids = R.case_id


@pytest.fixture(scope="module")
def lib(s3r):
    import __graft_entry__ as g
    if not os.path.exists(s3r.LIB_PATH):
        g.build()
    return s3r.load_library()


@pytest.fixture(scope="module")
def header():
    with open(os.path.join(ROOT, "include", "s3r.h")) as f:
        return f.read()


# ---------------------------------------------------------------- the declaration
def test_header_declares_the_entry_point_and_the_binding_matches(s3r, header):
    assert re.search(r"#define\s+S3R_ABI_VERSION\s+8\b", header) and s3r._lib.ABI_VERSION == 8
    m = re.search(r"\bint\s+s3r_cost_volume_backward\s*\(([^;{}]*?)\)\s*;", header, re.S)
    assert m, "include/s3r.h does not declare s3r_cost_volume_backward"
    params = [" ".join(p.split()) for p in m.group(1).split(",")]
    assert params == ["const float* grad_volume", "float* grad_left", "float* grad_right", "int batch", "int channels", "int max_disp",
                      "int height", "int width", "void* hip_stream"]
    res, args = s3r._lib.SIGNATURES["s3r_cost_volume_backward"]
    assert res is C.c_int
    assert args == [C.c_void_p if "*" in p else C.c_int for p in params]
    comment = header[header[:m.start()].rfind("/*"):m.start()]
    for phrase in ("ascending d", "starts AS t_0", "no atomics", "hipStream_t", "NaN", "propagates", "both NULL", "family 3"):
        assert phrase in comment, phrase


def test_the_header_wording_admits_the_poison_pre_state(header):
    """tests/_stream_cases.safe_prestate: a float buffer's NaN pre-state counts as documented where the entry's comment says what a
    NaN does"""
    from tests import _stream_cases as SC
    at = header.index("int s3r_cost_volume_backward(")
    comment = header[header[:at].rfind("/*"):at]
    for role in ("in", "out"):
        assert SC.safe_prestate(SC.Arg("t", (2, 2), SC.F32, role), comment) == "NaN (header)"
    assert "s3r_cost_volume_backward" not in SC.stream_prototypes(header)      # `hip_stream`: its stream contract has a file of its own


# ---------------------------------------------------------------- the mathematics
@pytest.mark.parametrize("case", R.CASES, ids=_ids)
def test_float64_restatement_equals_autograd_through_the_oracle(oracle, case):
    """integer data: both sides are exact in float64, so they must be EQUAL; random data: the same real terms in another order"""
    gv = R.lattice_gv(case)
    gl, gr, nl, nr, ml, mr = R.backward64(gv)
    wl, wr = R.oracle_backward64(gv, oracle)
    assert np.array_equal(gl, wl) and np.array_equal(gr, wr)
    if case in R.SMALL:
        gv = R.random_gv(case)
        gl, gr, nl, nr, ml, mr = R.backward64(gv)
        wl, wr = R.oracle_backward64(gv, oracle)
        assert (np.abs(gl - wl) <= 2.0 ** -50 * nl * ml).all() and (np.abs(gr - wr) <= 2.0 ** -50 * nr * mr).all()
    B, Cc, D, H, W = case
    assert nl.max() == nr.max() == min(D, W) and nl.min() == nr.min() == 1


@pytest.mark.parametrize("case", R.CASES, ids=_ids)
def test_fp32_order_is_exact_on_integer_lattices(case):
    gv = R.lattice_gv(case)
    gl32, gr32 = R.backward32(gv)
    gl, gr, *_ = R.backward64(gv)
    assert gl32.dtype == np.float32 and np.array_equal(gl32.astype(np.float64), gl) and np.array_equal(gr32.astype(np.float64), gr)
    assert np.abs(gl).max() > 0 and np.abs(gr).max() > 0


@pytest.mark.parametrize("case", R.CASES, ids=_ids)
def test_fp32_order_is_inside_the_derived_bound_on_random_data(case):
    gv = R.random_gv(case)
    gl32, gr32 = R.backward32(gv)
    gl, gr, nl, nr, ml, mr = R.backward64(gv)
    for got, ref, n, mag in ((gl32, gl, nl, ml), (gr32, gr, nr, mr)):
        err, lim = np.abs(got.astype(np.float64) - ref), R.bound32(n, mag)
        assert (err <= lim).all(), (err / lim).max()
        # the bound must be able to see a mistake: far below the values it is applied to
        assert lim.max() <= 1e-5 * np.abs(ref).max()


def test_structural_zero_classes_and_live_positions_partition_the_volume():
    for case in R.CASES:
        m = R.structural_zero_masks(case)
        total = sum(v.astype(np.int64) for v in m.values()) + R.live_mask(case)
        assert (total == 1).all()
        B, Cc, D, H, W = case
        assert m["plane d >= W"].any() == (D > W)
        # the forward writes constants exactly there: its float64 autograd gives those positions no path to the features
        gv = np.where(R.live_mask(case), 0.0, 1.0)
        gl, gr, *_ = R.backward64(gv)
        assert not gl.any() and not gr.any()


# ---------------------------------------------------------------- mutants
def _datasets(case):
    """every data set the GPU table runs on `case`: name -> gv"""
    sets = {"random": R.random_gv(case), "lattice": R.lattice_gv(case), "signed zeros": R.signed_zero_gv(case)}
    for name, mask in R.structural_zero_masks(case).items():
        if mask.any():
            sets["NaN in " + name] = np.where(mask, np.float32(np.nan), R.random_gv(case)).astype(np.float32)
    return sets


def _equal(a, b):
    """bit-equal where neither is NaN, and NaN in the same places"""
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb) and np.array_equal(R.bits(a)[~na], R.bits(b)[~nb]))


@pytest.mark.parametrize("mutant", R.MUTANTS)
def test_each_mutant_is_caught_by_the_gpu_tables_data(mutant):
    """descending d, a start from +0.0, n_L off by one, the slabs swapped, a mask by multiplication: each differs from the defined order
    on at least one (case, data set) of the GPU table — by bits, or by where the NaN are"""
    caught = []
    for case in R.SMALL:
        for name, gv in _datasets(case).items():
            want, got = R.backward32(gv), R.backward32(gv, mutant)
            if not (_equal(want[0], got[0]) and _equal(want[1], got[1])):
                caught.append((R.case_id(case), name))
    assert caught, mutant
    expect = {"start from +0.0": "signed zeros", "mask by multiplication": "NaN in left slab w < d"}.get(mutant)
    if expect:
        assert any(n == expect for _, n in caught), caught


def test_a_nan_at_a_structural_zero_changes_nothing_in_the_restatement():
    for case in R.SMALL:
        base = R.backward32(R.random_gv(case))
        for name, gv in _datasets(case).items():
            if name.startswith("NaN in"):
                got = R.backward32(gv)
                assert np.array_equal(R.bits(got[0]), R.bits(base[0])) and np.array_equal(R.bits(got[1]), R.bits(base[1])), (case, name)


def test_a_nan_at_a_live_position_reaches_exactly_two_outputs():
    """gv[b, c, d, h, w] is in grad_left[b,c,h,w] and grad_right[b,c,h,w-d]; gv[b, C+c, d, h, w] in grad_right[b,c,h,w] and
    grad_left[b,c,h,w+d]"""
    case = R.CASES[4]
    B, Cc, D, H, W = case
    gv = R.random_gv(case).copy()
    gv[1, 1, 2, 3, 7] = np.nan                  # left slab, c = 1, d = 2, w = 7
    gv[2, Cc + 0, 3, 4, 5] = np.nan             # right slab, c = 0, d = 3, w = 5
    gl, gr = R.backward32(gv)
    assert sorted(map(tuple, np.argwhere(np.isnan(gl)))) == [(1, 1, 3, 7), (2, 0, 4, 8)]
    assert sorted(map(tuple, np.argwhere(np.isnan(gr)))) == [(1, 1, 3, 5), (2, 0, 4, 5)]


# ---------------------------------------------------------------- the host-side half of the entry point
def test_refusals_need_no_device(lib):
    one = C.c_void_p(256)           # a non-NULL address that is never dereferenced: every call below returns before a launch
    call = lambda gv, gl, gr, *dims: lib.s3r_cost_volume_backward(gv, gl, gr, *dims, None)
    assert call(one, None, None, 1, 2, 3, 4, 5) == INVALID
    assert "both NULL" in lib.s3r_last_error().decode()
    for dims in ((1, 0, 3, 4, 5), (1, 2, 0, 4, 5), (1, 2, 3, 0, 5), (1, 2, 3, 4, 0), (-1, 2, 3, 4, 5), (1, -2, 3, 4, 5)):
        assert call(one, one, one, *dims) == INVALID, dims
        assert "dims must be positive" in lib.s3r_last_error().decode(), dims
    assert call(one, one, one, 1, 2, 3, 128, 128) == INVALID                    # the forward refuses this plane: 2 H W floats > 64 KiB
    assert "128x128" in lib.s3r_last_error().decode()
    assert call(one, one, one, 1 << 12, 1 << 8, 1 << 5, 8, 8) == INVALID        # 2^32 elements
    assert "split the batch" in lib.s3r_last_error().decode()
    assert call(None, one, one, 1, 2, 3, 4, 5) == INVALID
    assert "null tensor pointer" in lib.s3r_last_error().decode()
    for gl, gr in ((one, one), (one, None), (None, one)):
        assert call(one, gl, gr, 0, 2, 3, 4, 5) == OK                            # batch 0: nothing to launch
    assert call(one, None, None, 0, 2, 3, 4, 5) == INVALID                      # ... but both NULL stays an error


def test_python_surface_validates_before_it_touches_a_device(s3r):
    import torch
    with pytest.raises(RuntimeError, match="need_left or need_right"):
        s3r.cost_volume_backward(torch.zeros(1, 2, 1, 1, 1), need_left=False, need_right=False)
    with pytest.raises(RuntimeError, match=r"\(B, 2C, D, H, W\)"):
        s3r.cost_volume_backward(torch.zeros(1, 3, 1, 1, 1))
    with pytest.raises(RuntimeError, match="HIP device"):
        s3r.cost_volume_backward(torch.zeros(1, 2, 1, 1, 1))
    with pytest.raises(RuntimeError, match="fp32 models only"):
        s3r.CostVolume(precision="bf16").differentiable(torch.zeros(1, 8, 4, 4), torch.zeros(1, 8, 4, 4))
    with pytest.raises(RuntimeError, match="fp32 models only"):
        s3r.VolumeEncoder(precision="bf16").differentiable_features(torch.zeros(1, 64, 28, 28, 28))
