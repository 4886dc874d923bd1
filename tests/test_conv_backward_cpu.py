"""s3r_conv_backward / s3r_conv_adjoint_desc without a GPU: the mathematics the design rests on (the weight-gradient formula and the two
adjoint identities against torch's own float64 autograd), the mutants the cases must tell apart, the tiling restatement (geo(), pinned
against the library's scratch query) and the branches the sweep SHAPES reaches, the declarations and their bindings, and the host-side half of the entry points (the adjoint descriptor's fields, the scratch query, every refusal — each happens before
anything is launched: a HIP call would have given S3R_ERR_HIP on a host without a device)."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from tests import _convbwd64 as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID, WORKSPACE = -1, -3
ALL = R.CASES + R.D3[:1] + R.LONG_ROWS
RUNS = [(i, c, a) for i, c in enumerate(R.CASES) for a in R.acts_of(i)] + [(-1, c, a) for c in (R.D3[0], R.LONG_ROWS[0]) for a in ("none", "relu")]
RUNS += [(20 + i, c, a) for i, c in enumerate(R.SHAPES) for a in ("none", "relu")]
OLD12 = R.CASES + R.D3 + R.LONG_ROWS


@pytest.fixture(scope="module")
def lib(s3r):
    import __graft_entry__ as g
    if not os.path.exists(s3r.LIB_PATH):
        g.build()
    return s3r.load_library()


def desc_of(s3r, c, act_name="none", **over):
    L = s3r._lib
    d = L.ConvDesc(L.OP_DECONV if c.op == "deconv" else L.OP_CONV, c.nd, c.B, c.cin, c.cout, c.n, c.k, c.s, c.p, L.ACT[act_name], 7, -1, 0, 0, 0, 0,
                   0, 0, 0, 1, c.opad, 0.0)
    for k, v in over.items():
        setattr(d, k, v)
    return d


# ---------------------------------------------------------------- the mathematics
@pytest.mark.parametrize("i,c,act", RUNS, ids=[f"{R.case_id(c)}-{a}" for _, c, a in RUNS])
def test_formula_and_adjoint_identities_against_float64_autograd(i, c, act):
    """grad_w64 (the header's formula), grad_x64 (the adjoint layer's forward on the layer's own weight) and sum(g) against
    torch.autograd.grad in float64.  Both sides add the same real terms in float64 in different orders."""
    x, w, scale, shift, _, gy = R.make(c, seed=100 + i, act=act)
    want_x, want_w, want_b, y64 = R.autograd64(c, x, w, scale, shift, act, gy)
    gy64 = gy.astype(np.float64)
    g = {"none": gy64, "relu": np.where(y64 > 0, gy64, 0.0), "sigmoid": gy64 * (y64 * (1.0 - y64))}[act]
    gs = g if scale is None else g * scale.astype(np.float64).reshape((1, -1) + (1,) * c.nd)
    gw, K, mag = R.grad_w64(c, x, gs)
    assert gw.shape == want_w.shape == R.weight_shape(c)
    assert (np.abs(gw - want_w) <= R.lim64(K, mag)).all()
    gx = R.grad_x64(c, w, gs)
    assert gx.shape == want_x.shape == R.x_shape(c)
    kx = c.cout * c.k ** c.nd
    wabs = np.abs(w.astype(np.float64))
    assert (np.abs(gx - want_x) <= R.lim64(kx, R.grad_x64(c, wabs, np.abs(gs)))).all()
    gb = g.sum(axis=(0,) + tuple(range(2, 2 + c.nd)))
    assert (np.abs(gb - want_b) <= R.lim64(g[:, 0].size, np.abs(g).sum(axis=(0,) + tuple(range(2, 2 + c.nd))))).all()
    # every in-grid count is positive somewhere and never above B Q
    Q = (c.n if c.op == "deconv" else R.out_edge(c)) ** c.nd
    assert K.max() <= c.B * Q and K.min() >= 0


@pytest.mark.parametrize("c", R.CASES, ids=R.case_id)
def test_mutants_fail_the_comparison(c):
    """the ConvTranspose roles swapped (the channel axes exchanged) or the kernel flipped: the cases can tell them from the formula"""
    x, w, scale, shift, _, gy = R.make(c, seed=5, act="none")
    _, want_w, _, _ = R.autograd64(c, x, w, scale, shift, "none", gy)
    gs = gy.astype(np.float64) * scale.astype(np.float64).reshape((1, -1) + (1,) * c.nd)
    gw, K, mag = R.grad_w64(c, x, gs)
    ok = lambda got: bool((np.abs(got - want_w) <= R.bound32(K, mag)).all())      # (the DEVICE test's tolerance: the mutants are far outside it)
    assert ok(gw)
    assert not ok(R.grad_w64(c, x, gs, mutant="swap")[0])
    if c.k > 1:
        assert not ok(R.grad_w64(c, x, gs, mutant="flip")[0])


def test_cases_cover_the_paths():
    cs = R.CASES
    assert len(cs) == 9 and {c.op for c in cs} == {"conv", "deconv"} and {c.nd for c in cs} == {2, 3}
    assert any(R.adjoint_out_pad(c) for c in cs) and any(c.opad for c in cs)
    S = [R.out_edge(c) ** c.nd for c in cs]
    assert 512 in S and any(512 < s < 1024 and s % 512 for s in S)      # a whole chunk, and a chunk boundary with a tail
    assert any(c.cin % 32 and c.cout % 32 for c in cs) and any(c.k == c.s for c in cs)
    assert R.out_edge(R.D3[0]) == 32 and R.LONG_ROWS[0].n > 64


# ---------------------------------------------------------------- the tiling sweep
@pytest.mark.parametrize("c", OLD12 + R.SHAPES, ids=R.case_id)
def test_geo_restatement_is_pinned_by_the_scratch_query(s3r, lib, c):
    """s3r_conv_backward_scratch_elems = B cout S + cout B ceil(S / 512) + (B nsl > 1 ? B nsl Ca Cf k^nd : 0) with geo()'s nsl (the host
    library plans without a device); at B = 2 as well where the case has B = 1, so that nsl always shows.  The staged tiles fit the LDS."""
    g = R.geo(c)
    assert g is not None and g.lds_bytes <= 65536 and g.run in (64, 32) and g.WLP % 2 == 0 and g.WL <= g.WLP <= g.run
    S, Ca, Cf = R.out_edge(c) ** c.nd, *((c.cin, c.cout) if c.op == "deconv" else (c.cout, c.cin))
    for B in sorted({c.B, 2}):
        want = B * c.cout * S + c.cout * B * ((S + 511) // 512) + (B * g.nsl * Ca * Cf * c.k ** c.nd if B * g.nsl > 1 else 0)
        got = lib.s3r_conv_backward_scratch_elems(C.byref(desc_of(s3r, c, "relu", batch=B)))
        assert got == want == R.scratch_elems(c, B), (B, got, want, vars(g))


_mc = lambda c: c.n if c.op == "deconv" else R.out_edge(c)
_Ca = lambda c: c.cin if c.op == "deconv" else c.cout
BRANCHES = {                                              # branch of convbwd_geo / convbwd_gw_kernel / convbwd_shift_finish_kernel -> (case, geo) hits it
    "a partial second tap group along W": lambda c, g: g.ntg == 2 and c.k % 4 != 0,
    "a second 128-row group with inactive waves": lambda c, g: g.nag >= 2 and _Ca(c) % 128 != 0,
    "run halved, whole rows": lambda c, g: g.run == 32 and g.nseg == 1,
    "run halved, segments": lambda c, g: g.run == 32 and g.nseg > 1,
    "a ragged last K slice": lambda c, g: g.nchunks % g.cps != 0,
    "segments of a strided Conv": lambda c, g: g.nseg > 1 and c.s > 1 and c.op == "conv",
    "segments of a strided ConvTranspose": lambda c, g: g.nseg > 1 and c.s > 1 and c.op == "deconv",
    "segments in 3D": lambda c, g: g.nseg > 1 and c.nd == 3,
    "mc = 64, the last whole-row shape": lambda c, g: g.mc == 64 and g.nseg == 1,
    "mc = 65, a second segment of one position": lambda c, g: g.mc == 65 and g.nseg == 2 and g.mc - g.WL == 1,
    "stride 3": lambda c, g: c.s == 3,
    "k < stride": lambda c, g: c.k < c.s,
    "coarse edge 1": lambda c, g: g.mc == 1,
    "the finish kernels' second 64-sample block": lambda c, g: c.B > 64,
}


def test_shapes_cover_the_tiling():
    assert len(R.SHAPES) == 20 and len(set(R.SHAPES)) == 20 and not set(R.SHAPES) & set(OLD12)
    for name, hit in BRANCHES.items():
        assert any(hit(c, R.geo(c)) for c in R.SHAPES), f"no case of SHAPES reaches: {name}"
    # why the sweep exists: none of the twelve earlier geometries takes any of the first five
    for name in list(BRANCHES)[:5]:
        assert not any(BRANCHES[name](c, R.geo(c)) for c in OLD12), f"an earlier case already reaches: {name}"
    assert all(_mc(c) == R.geo(c).mc for c in R.SHAPES)
    # what the single cases are listed for (tests/_convbwd64.py's comments)
    G = [R.geo(c) for c in R.SHAPES]
    assert (G[0].ntg, G[0].nag, R.SHAPES[0].k - 4) == (2, 2, 1) and (G[1].nag, G[1].R) == (2, 16) and (G[2].nag, G[2].nft) == (3, 2)
    assert (G[3].nchunks, G[3].cps, G[3].nsl, G[3].nrows % G[3].R) == (7, 2, 4, 2)
    assert (G[5].R, G[5].nsl) == (8, 2) and (G[6].ntg, G[6].tiles) == (2, 98) and (G[7].R, G[7].run) == (8, 32)
    assert (G[8].WL, G[8].nseg, G[8].mc, G[8].ntg) == (32, 2, 63, 2) and (G[9].mc, G[9].WLP, G[9].R, G[9].nsl) == (33, 34, 1, 7)
    assert (G[10].nseg, G[10].nsl) == (2, 16) and (G[11].mc, G[11].nsl) == (71, 21) and (G[12].nchunks, G[12].cps, G[12].nsl) == (8712, 1089, 8)
    assert G[17].tiles == 1 and (G[18].WLP, G[18].WL) == (2, 1)
    # every tensor stays small: a case takes well under a second on the device
    for c in R.SHAPES:
        assert max(np.prod(R.x_shape(c)), np.prod(R.y_shape(c)), np.prod(R.weight_shape(c))) < 600_000


@pytest.mark.parametrize("c", R.SHAPES, ids=R.case_id)
def test_tiling_mutants_fail_the_comparison(c):
    """the last K slice dropped (a wrong cend) or the second tap group dropped (a wrong tw0 mask): on random data each falls outside the
    DEVICE test's bound32 on every case it applies to (nsl > 1, respectively k >= 5), and the true formula stays inside.
    The data are the device test's: normal draws with R.data_mean's mean 1, so that a sum grows like K and the any-order bound, which
    grows like K^2 u, stays below it at every K of the sweep.  On zero-mean data the 3D segment case (K = 66^3) could not reject
    "drop_tail_slice": there the bound is 1 / 0.646 of the largest |grad_w| and the missing slice moves no element by more than 0.162 of
    it; with the mean it is 5.6 bounds outside, the smallest figure of all cases (R.data_mean's estimate: 5)."""
    g = R.geo(c)
    x, w, scale, shift, _, gy = R.make(c, seed=5, act="none", mean=R.data_mean(c))
    _, want_w, _, _ = R.autograd64(c, x, w, scale, shift, "none", gy)
    gs = gy.astype(np.float64) * scale.astype(np.float64).reshape((1, -1) + (1,) * c.nd)
    gw, K, mag = R.grad_w64(c, x, gs)
    lim = R.bound32(K, mag)
    ok = lambda got: bool((np.abs(got - want_w) <= lim).all())
    assert ok(gw)
    m = R.tail_slice_mask(c)
    assert m.any() and (g.nsl == 1) == bool(m.all())
    rel = lambda d: np.divide(np.abs(d), lim, out=np.zeros_like(lim), where=lim > 0).max()      # (a tap that never meets the grid: 0 / 0)
    print(f"max |grad_w| / bound {rel(want_w):.3e}")
    for mutant, applies in (("drop_tail_slice", g.nsl > 1), ("drop_tap_group", c.k >= 5)):
        if applies:
            got = R.grad_w64(c, x, gs, mutant=mutant)[0]
            worst = rel(got - want_w)
            print(f"{mutant}: max |change| / bound {worst:.3e}")
            assert not ok(got), f"{mutant} stays inside bound32: max |change| / bound {worst:.3e}"


@pytest.mark.parametrize("c", R.SHAPES, ids=R.case_id)
def test_lattice_sums_of_the_sweep_stay_below_2_24_and_tell_the_mutants(c):
    """what test_integer_lattice_is_exact (GPU) relies on, checked here first: the float64 sum of |terms| of every element is below 2^24
    (the largest is the 3D n = 66 case: at most 18 * 66^3 = 5.2 M).  That test asks for equality, and on its data (same seed) both
    tiling mutants differ from the formula on every case they apply to"""
    g = R.geo(c)
    x, _, scale, _, _, gy = R.make(c, seed=7, lattice=True)
    gs = R.gs32(gy, scale)
    gw, _, mag = R.grad_w64(c, x, gs)
    assert mag.max() < 2 ** 24 and np.abs(gy).sum() < 2 ** 24
    if g.nsl > 1:
        assert not np.array_equal(R.grad_w64(c, x, gs, mutant="drop_tail_slice")[0], gw)
    if c.k >= 5:
        assert not np.array_equal(R.grad_w64(c, x, gs, mutant="drop_tap_group")[0], gw)


def test_nan_taps_is_the_formulas_support():
    """nan_taps against the formula itself: plant one 1.0 in an all-zero F under an all-ones A; grad_w64 is non-zero exactly there"""
    for c, pos in ((R.SHAPES[4], (0, 11)), (R.SHAPES[15], (14, 7)), (R.SHAPES[16], (8, 0, 4)), (R.SHAPES[9], (130, 64)), (R.CASES[7], (9, 4))):
        x, gs = np.zeros(R.x_shape(c, 1)), np.ones(R.y_shape(c, 1))
        Fi = gs if c.op == "deconv" else x
        if c.op == "deconv":
            x[:] = 1.0
            gs[:] = 0.0
        Fi[(0, 0) + pos] = 1.0
        gw = R.grad_w64(c, x, gs)[0]
        assert np.array_equal(gw[0, 0] != 0, R.nan_taps(c, pos)), (c, pos)
        assert not gw[:, 1:].any()


def test_grad_shift_order_is_the_head_backwards():
    """reduce32 over (B, cout, S) is, per channel, the head backward's restated order on that channel's rows"""
    from tests import _head64 as H
    g = torch.randn(3, 4, 529, generator=torch.Generator().manual_seed(0)).numpy()
    got = R.grad_shift32(g.reshape(3, 4, 23, 23))
    for o in range(4):
        assert R.bits(got[o:o + 1])[0] == R.bits(H.grad_shift32(g[:, o, :]))[()]
    sc = np.array([0.5, 1.5, 0.75, 3.0], np.float32)
    assert (R.bits(R.gs32(g, sc)[:, 2]) == R.bits(H.gs32(g[:, 2], 0.75))).all()


# ---------------------------------------------------------------- declarations and bindings
def _args(header, ret, name):
    m = re.search(r"\b%s\s+%s\s*\(([^)]*)\)\s*;" % (ret, name), re.sub(r"/\*.*?\*/", "", header, flags=re.S))
    assert m, f"{name} is not declared in include/s3r.h"
    return [" ".join(a.split()) for a in m.group(1).split(",")]


def test_header_prototypes_match_the_bindings(s3r, lib):
    header = open(os.path.join(ROOT, "include", "s3r.h")).read()
    assert "#define S3R_ABI_VERSION 8" in header                  # additive entry points: no version step
    assert _args(header, "int", "s3r_conv_adjoint_desc") == ["const s3r_conv_desc* d", "s3r_conv_desc* adj"]
    assert _args(header, "int64_t", "s3r_conv_backward_scratch_elems") == ["const s3r_conv_desc* d"]
    assert _args(header, "int", "s3r_conv_backward") == [
        "const s3r_conv_desc* d", "const float* x", "const float* y", "const float* grad_y", "const float* scale", "float* gs",
        "float* grad_w", "float* grad_shift", "float* scratch", "int64_t scratch_elems", "void* hip_stream"]
    res, args = s3r._lib.SIGNATURES["s3r_conv_backward"]
    assert res is C.c_int and args == [C.POINTER(s3r._lib.ConvDesc)] + [C.c_void_p] * 8 + [C.c_int64, C.c_void_p]
    assert lib.s3r_abi_version() == 8
    assert "#define S3R_CONV_BACKWARD_TAG 1000000" in header and s3r._lib.CONV_BACKWARD_TAG == 1000000
    names = {"conv_backward", "differentiable_conv"}
    assert names <= set(s3r.__all__) and all(callable(getattr(s3r, n)) for n in names)
    assert all(callable(f) for f in (s3r.Decoder.differentiable_tail, s3r.Decoder.differentiable_features, s3r.Stereo2Voxel.trunk_features))
    flat = " ".join(header.replace("\n *", " ").split())
    for sentence in ("in ascending (sample, slice) order", "a slice never spans two samples", "replaced by 0 in BOTH operands",
                     "with any scratch contents on entry", "a sample's partial is the same in every batch", "No atomics".lower(),
                     "out_pad = (n + 2 p - k) mod s", "the version stays 8"):
        assert sentence in flat, sentence


# ---------------------------------------------------------------- the adjoint descriptor
@pytest.mark.parametrize("c", ALL, ids=R.case_id)
def test_adjoint_descriptor(s3r, lib, c):
    L = s3r._lib
    d, adj = desc_of(s3r, c, "relu"), L.ConvDesc()
    assert lib.s3r_conv_adjoint_desc(C.byref(d), C.byref(adj)) == 0, lib.s3r_last_error()
    assert adj.op == (L.OP_CONV if c.op == "deconv" else L.OP_DECONV)
    assert (adj.cin, adj.cout, adj.in_size) == (c.cout, c.cin, R.out_edge(c))
    assert (adj.k, adj.stride, adj.pad, adj.out_pad, adj.dilation) == (c.k, c.s, c.p, R.adjoint_out_pad(c), 1)
    assert (adj.ndim, adj.batch, adj.tag) == (c.nd, c.B, 7)
    assert (adj.act, adj.in_halo, adj.out_halo, adj.in_layout, adj.out_layout, adj.algo, adj.dtype, adj.tile, adj.ksplit) == (0, 0, 0, 0, 0, 0, 0, -1, 0)
    assert lib.s3r_conv_out_size(C.byref(adj)) == c.n                       # the adjoint's output is the layer's input
    packed = C.c_int64(0)
    assert lib.s3r_conv_packed_elems(C.byref(adj), C.byref(packed)) == 0 and packed.value >= int(np.prod(R.weight_shape(c)))


def test_adjoint_out_pad_rule_over_every_residue(s3r, lib):
    """Conv over every edge n that leaves another remainder (n + 2 p - k) mod s; ConvTranspose with every out_pad < s"""
    L = s3r._lib
    for nd in (2, 3):
        for (k, s, p) in ((3, 2, 1), (4, 2, 1), (3, 3, 1), (3, 2, 0), (1, 1, 0), (4, 1, 0), (5, 4, 2)):
            for n in range(k + 1, k + 1 + 2 * s):
                c = R.Case("conv", nd, 4, 6, k, s, p, 0, n, 2)
                adj = L.ConvDesc()
                assert lib.s3r_conv_adjoint_desc(C.byref(desc_of(s3r, c)), C.byref(adj)) == 0
                assert adj.out_pad == (n + 2 * p - k) % s and lib.s3r_conv_out_size(C.byref(adj)) == n
            for op in range(s):
                c = R.Case("deconv", nd, 4, 6, k, s, p, op, 5, 2)
                adj = L.ConvDesc()
                assert lib.s3r_conv_adjoint_desc(C.byref(desc_of(s3r, c)), C.byref(adj)) == 0
                assert adj.out_pad == 0 and adj.op == L.OP_CONV and lib.s3r_conv_out_size(C.byref(adj)) == 5


# ---------------------------------------------------------------- refusals and the scratch query
_P = C.cast(C.create_string_buffer(64), C.c_void_p).value      # a non-NULL host address: validation rejects each case before a dereference
_REFUSED = {
    "bf16": dict(dtype=1), "linear": dict(op=2), "dilation-2": dict(dilation=2), "act-leaky": dict(act=3), "act-tanh": dict(act=5),
    "act-negative": dict(act=-1), "in-layout": dict(in_layout=2), "out-layout": dict(out_layout=5), "in-halo": dict(in_halo=1),
    "out-halo": dict(out_halo=1), "ndim-4": dict(ndim=4), "k-zero": dict(k=0), "batch-negative": dict(batch=-1), "cin-zero": dict(cin=0),
    "out-pad-on-conv": dict(out_pad=1), "empty-output": dict(in_size=1, k=3, pad=0),
}


def _backward(lib, d, x=_P, y=_P, gy=_P, scale=_P, gs=_P, gw=_P, gb=_P, scratch=_P, elems=1 << 50):
    return lib.s3r_conv_backward(C.byref(d), x, y, gy, scale, gs, gw, gb, scratch, elems, None)


@pytest.mark.parametrize("case", list(_REFUSED), ids=list(_REFUSED))
def test_refusals_on_the_host(s3r, lib, case):
    d = desc_of(s3r, R.CASES[0], "relu", **_REFUSED[case])
    assert _backward(lib, d) == INVALID and lib.s3r_last_error().decode()
    assert lib.s3r_conv_backward_scratch_elems(C.byref(d)) == INVALID
    assert lib.s3r_conv_adjoint_desc(C.byref(d), C.byref(s3r._lib.ConvDesc())) == INVALID


def test_null_rules_and_workspace(s3r, lib):
    for c in (R.CASES[0], R.CASES[5]):
        d = desc_of(s3r, c, "relu")
        need = lib.s3r_conv_backward_scratch_elems(C.byref(d))
        assert need > 0
        assert _backward(lib, d, gs=None, gw=None, gb=None) == INVALID and b"all NULL" in lib.s3r_last_error()
        assert _backward(lib, d, y=None) == INVALID and b"y is NULL" in lib.s3r_last_error()
        assert _backward(lib, d, gy=None) == INVALID
        assert _backward(lib, d, x=None) == INVALID                          # grad_w asked for
        assert _backward(lib, d, elems=need - 1) == WORKSPACE and b"s3r_conv_backward_scratch_elems" in lib.s3r_last_error()
        assert _backward(lib, d, scratch=None) == WORKSPACE
        # the allowed NULL forms get past every check but the last
        assert _backward(lib, d, x=None, gw=None, elems=1) == WORKSPACE
        assert _backward(lib, d, scale=None, elems=1) == WORKSPACE
        assert _backward(lib, desc_of(s3r, c, "none"), y=None, elems=1) == WORKSPACE
        assert lib.s3r_conv_adjoint_desc(C.byref(d), None) == INVALID
    d0 = desc_of(s3r, R.CASES[0], "relu", batch=0)
    assert _backward(lib, d0, scratch=None, elems=0) == 0                    # S3R_OK with no device: nothing was enqueued
    assert _backward(lib, d0, gs=None, gw=None, gb=None) == INVALID
    assert lib.s3r_conv_backward_scratch_elems(C.byref(d0)) == 0


@pytest.mark.parametrize("c", ALL, ids=R.case_id)
def test_scratch_query_is_monotone_in_batch(s3r, lib, c):
    sizes = [lib.s3r_conv_backward_scratch_elems(C.byref(desc_of(s3r, c, "relu", batch=b))) for b in range(0, 40)]
    assert sizes[0] == 0 and sizes[1] > 0 and all(a <= b for a, b in zip(sizes, sizes[1:])), sizes[:6]
    S = R.out_edge(c) ** c.nd
    assert sizes[1] >= c.cout * S + c.cout * ((S + 511) // 512)             # gs and one chunk sum per channel and chunk at least
    # per-sample slabs: the slab count grows by the same whole number of weight-sized slabs with every sample
    W = int(np.prod(R.weight_shape(c)))
    step = {(b - a) for a, b in zip(sizes[2:], sizes[3:])}
    assert len(step) == 1 and (step.pop() - c.cout * S - c.cout * ((S + 511) // 512)) % W == 0


def test_python_layer_checks_before_the_device(s3r):
    L = s3r.arch_spec.Layer("t", "conv3d", 5, 7, 3, 1, 1, True, "relu")
    x, w = torch.zeros(2, 5, 5, 5, 5), torch.zeros(7, 5, 3, 3, 3)
    y = torch.zeros(2, 7, 5, 5, 5)
    with pytest.raises(RuntimeError, match="HIP device"):         # no CPU fallback
        s3r.conv_backward(x, w, y, y, L)
    with pytest.raises(RuntimeError, match="HIP device"):
        s3r.differentiable_conv(x, w.requires_grad_(), None, torch.zeros(7), L)
