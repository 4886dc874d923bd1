"""Every convolution, linear and bf16 kernel against the float64 reference BIT FOR BIT, on integer-lattice data.

tests/_lattice.py holds the argument: with the input, the weights and the folded epilogue on an integer (dyadic) lattice and the
absolute-value flow below 2^24, no fp32 operation of ANY summation order rounds, so the kernel's output must equal the float64
reference bit for bit; on the bf16 path it must equal RNE_bf16(exact value).  There is no tolerance, so one missing or doubled
(channel, tap) term is a mismatch at any reduction depth — the network's p1 (K = 32768), v6 (16384), v5 (6912), d1 (4096) and
the 32768-wide linear shape included, where tests/_ref64.py's bound cannot see a term.  tests/test_exact_cpu.py proves, without a
GPU, that every case here is admissible and that bit equality catches the single-term, shifted-output and rounding-mode mutants.

Bit patterns are compared (`view(int32)` / `view(int16)`), so -0.0 against +0.0 would be reported: the reference of no case holds a
-0.0 (asserted on the CPU: the epilogue adds a +0.0-or-non-zero shift last), so the contract here is +0.0.

Every call goes through the C-ABI (s3r_conv_pack_weights + s3r_conv_forward, s3r_linear_forward, s3r_chain_forward) with NaN-filled
scratch and a NaN-filled output; the descriptors tests/test_buffers_gpu.py does not run (forced tiles and split-K, the bf16 tile
matrix, the deep linear shapes) run a second time over zero-filled scratch.  Guards and poisons are that file's subject, values
are this one's.  A configuration the library refuses (tests/test_parity_gpu.py's and tests/test_bf16_gpu.py's rules) is asserted
refused — fp32 tiles by the scratch query, bf16 tiles by the forward call, which must return an error and leave the output
untouched — and never compared.

A mismatch is reported as the first differing element with its (b, cout, position), the exact value, the value got and their
difference in lattice units (2^-f): a difference equal to one `w x` product names the tap.

Cases: direct fp32 233 (18 network layers x B 1 / 3, 8 shapes x 8 tiles x 2 gather widths, split-K 1 / 2 / 4 and v5 / v6 / d1 at
network size under split-K 1 .. 16, the general-layer families), linear 28 + the 14 shapes of the launch plan's sweep x act none /
ReLU + bias = NULL once per kernel (tests/_linear_cases.py: every branch of linear_wgk_ok / linear_split / launch_linear), bf16 276 under each of the two matrix instructions
(18 layers x B 1 / 3, the 15 x 16 tile matrix), Winograd 48 (one-axis x 3 launch forms, two-axis tiles 3 / 4 / 5 incl. F(2,4) x F(2,4),
transposed F(2,2) classes and the three-axis form), Winograd at ragged shapes and at the LDS limits 143 (tests/_exact_cases.py::
_wino_shapes: the smallest shapes at which each branch of those kernels is taken — edges with n mod 4 = 1, 2, 3 and the dword-gather
instantiation of the one-axis kernel, F(2,4) x F(2,4) at output edges 2, 3, 5, 6, couts 2 / 33 / 70 / 130, ragged last packs of the
two finish kernels, PL and SUB shrunk by LDS under out_halo 8, a padded plane of 128^2 and four padded slices of 64^2 floats; every
launch form and AUTO, the profiler record naming the form that ran), the cost volume writing v1's plane sets in both layouts, the
stem -> e2 hand-off, the bf16 d3 + head fused launch, and four runs that drop ONE term on the device and require the mismatch.  On
an MI355X every one of them is bit-exact: the tests found no kernel or pack bug.

Epilogue forms (tests/_exact_cases.py::_ep_sites, 116 cases): `scale` and `shift` each given or a NULL POINTER — ss / 0s / s0 / 00 — at
every kernel that ends in `scale ? scale[m] : 1, shift ? shift[m] : 0`: direct epilogue and split-K finish, residue classes,
depth-to-space, every Winograd launch form, head_kernel, the four linear kernels behind an S3R_OP_LINEAR descriptor with a folded
BatchNorm, the bf16 MFMA epilogue, bf16 split-K finish and head_bf16_kernel.  The fp32 conv + head launch (_head_chains, 88 cases): one
row per route of conv_head_fused (direct tiles 2 / 7 / 1, transposed direct, transposed two-axis tiles 0 / 1 / 2, three-axis tiles
6 / 7 / 8, d3 + d4) x the head's four forms x a NULL / NULL and an integer producer epilogue; no head record may appear.  All bit-exact
at first contact on an MI355X.

Past the LDS limits (a padded plane of 130^2, four slices of 66^2) the descriptor is refused by the scratch query and by the forward,
with the NaN fill of the output and the scratch intact, and the library's own launch form at such a shape is the class-parallel one:
three tests beside the sweep (the planner half is tests/test_exact_cpu.py::test_two_axis_lds_rule_is_the_planners).

Staying on tests/_ref64.py's bound (tests/test_buffers_gpu.py's chain matrix): the e6 -> e7 two-axis hand-off AS A CHAIN.  The
producer's weights must be multiples of 576 (wax_g in s3r_wino.h folds 1/24 per axis into them), so the intermediate is
a multiple of 576, and the consumer's weights bring another 576: one unit product is 3.3e5 and the flow passes 2^24 after a few
dozen terms, whatever the data.  e6 and e7 are held exactly one at a time (wino2-tile3/4/5-e6, -e7).  The activations Sigmoid, ELU
and Tanh stay there too (transcendental), and the 8-bit stem entry (it scales by 1/255; it is tied to the fp32 entry bit for bit).

Wall time on an MI355X: `pytest tests -m gpu` without this file 144 s (1181 tests); this file 6 s (838 tests).  With the shape
sweep: 8.5 s (984 tests) — summed per-test times of one run, the 838 earlier tests 4.1 s, the 146 new ones 2.1 s, of which the
library-pick case at edge 60 (B = 2, its fp64 reference included) 1.8 s and the first edge-124 case 0.6 s (it makes the data);
every other new case is below 0.12 s.  With the epilogue forms, the fused-head chains and the linear sweep (236 more tests): 1252 tests,
`--durations` of one run of the whole GPU suite: 22 of the new ones take 5 ms or more, 0.67 s together, the slowest 0.07 s (linear
3 x 4096 x 4065, whose case makes 16.6 M weights) against 1.8 s for the slowest earlier case; the other 214 are below 5 ms each.
"""
import ctypes as C

import pytest
import torch

from tests import _buffer_cases as BC
from tests import _exact_cases as X
from tests import _lattice as LT
from tests import _linear_cases as LC
from tests._abi_calls import DEV, interior, pad, rc_ok, sync

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib(s3r):
    return s3r.load_library()


@pytest.fixture(params=[32, 16], ids=["mfma32x32x16", "mfma16x16x32"])
def mfma_shape(request, monkeypatch):
    """both matrix instructions the bf16 kernels are built for (S3R_BF16_MFMA, read per call)"""
    monkeypatch.setenv("S3R_BF16_MFMA", str(request.param))
    return request.param


_DATA = {}


def _data(d):
    """(x, params, expected) of a case's data on the device; the reference in float64 on the device, kept for the cases that share it"""
    if d not in _DATA:
        if len(_DATA) >= 4:
            _DATA.pop(next(iter(_DATA)))
        x, p = d.make()
        x = x.to(DEV)
        p = {k: None if v is None else v.to(DEV) for k, v in p.items()}
        _DATA[d] = (x, p, LT.expected(d.layer, x, p, "bf16" if d.bf16_out else "fp32"))
    return _DATA[d]


def assert_bits(got, want, d, p, what):
    """bit equality, or the first differing element: (b, cout, position), exact, got, difference in lattice units"""
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    view = torch.int16 if got.dtype == torch.bfloat16 else torch.int32
    gb, wb = got.contiguous().view(view), want.contiguous().view(view)
    if torch.equal(gb, wb):
        return
    bad = (gb != wb)
    i = int(bad.reshape(-1).nonzero()[0, 0])
    idx = tuple(int(v) for v in torch.unravel_index(torch.tensor(i), want.shape))
    g, w = float(got.reshape(-1)[i]), float(want.reshape(-1)[i])
    unit = 2.0 ** -LT.frac_bits(d.layer, p)
    raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} elements differ; first at (b, cout, position) = "
                         f"({idx[0]}, {idx[1] if len(idx) > 1 else '-'}, {idx[2:]}): exact {w!r}, got {g!r}, difference {(g - w) / unit!r} "
                         f"lattice units of {unit}")


def make_desc(s3r, c):
    ih = c.in_halo if c.in_halo >= 0 else BC.need_halo(c.layer, c.n_in, c.dtype)
    return ih, s3r._lib.make_desc(c.layer, c.B, c.n_in, tile=c.tile, in_halo=ih, out_halo=c.out_halo, ksplit=c.ksplit,
                                  dtype=s3r._lib.DTYPE[c.dtype], algo=c.algo)


def run_conv(s3r, lib, c):
    """the case through s3r_conv_pack_weights + s3r_conv_forward; the logical (B, cout, ...) output"""
    l, nd, bf = c.layer, LT.R.ndim(c.layer), c.dtype == "bf16"
    ih, desc = make_desc(s3r, c)
    need = lib.s3r_conv_scratch_elems(C.byref(desc))
    if c.refused and not bf:                          # fp32: the planner refuses the descriptor (checked on the CPU too)
        assert need == -1 and lib.s3r_last_error(), (c.id, "expected to be refused", need)
        return None
    assert need >= 0, (c.id, lib.s3r_last_error())
    x, p, _ = _data(c.data)
    n = C.c_int64(0)
    rc_ok(lib, lib.s3r_conv_packed_elems(C.byref(desc), C.byref(n)), "packed_elems")
    w = p["w"].contiguous()
    pk = torch.full((n.value,), float("nan"), device=DEV)
    rc_ok(lib, lib.s3r_conv_pack_weights(C.byref(desc), w.data_ptr(), pk.data_ptr(), None), "pack_weights")
    cl_in, cl_out = bf and not BC._stem(l), bf and not BC._head(l, c.n_in)
    xp, _ = pad(x.to(torch.bfloat16) if cl_in else x, ih, cl_in)
    xp = xp.contiguous()
    n_out = lib.s3r_conv_out_size(C.byref(desc))
    oh = c.out_halo
    ysp = (n_out + 2 * oh,) * nd
    yshape = (c.B,) + ysp + (l.cout,) if cl_out else (c.B, l.cout) + ysp
    sp = tuple(range(1, 1 + nd)) if cl_out else tuple(range(2, 2 + nd))
    sc = None if p["scale"] is None else p["scale"].contiguous()
    sh = None if p["shift"] is None else p["shift"].contiguous()      # (None: a NULL pointer, not a vector of ones / zeros)
    outs = []
    if c.ran:
        s3r.profile_enable(8)
    try:
        for fill in (("nan", "zero") if c.twice else ("nan",)):
            y = torch.full(yshape, float("nan"), dtype=torch.bfloat16 if cl_out else torch.float32, device=DEV)
            scr = torch.full((max(need, 1),), float("nan") if fill == "nan" else 0.0, device=DEV)
            rc = lib.s3r_conv_forward(C.byref(desc), xp.data_ptr(), pk.data_ptr(), sc.data_ptr() if sc is not None else None,
                                      sh.data_ptr() if sh is not None else None, y.data_ptr(), scr.data_ptr(), need, None)
            sync()
            if c.refused:                             # bf16: the forced tile is refused when the launch is resolved, before any kernel
                assert rc < 0 and lib.s3r_last_error() and bool(torch.isnan(y).all()), (c.id, "expected to be refused", rc)
                return None
            rc_ok(lib, rc, c.id)
            outs.append(interior(y, oh, sp, cl_out).contiguous())
        rec = [r for r in s3r.profile_read(8) if r["family"] == "conv_mfma"] if c.ran else []
    finally:
        if c.ran:
            s3r.profile_enable(0)
    if c.ran:                                         # the algorithm and launch form under test are the ones that ran
        assert len(rec) == len(outs) and all(r["ran"] in c.ran for r in rec), (c.id, c.ran, rec)
    if len(outs) == 2:
        view = torch.int16 if cl_out else torch.int32
        assert torch.equal(outs[0].view(view), outs[1].view(view)), "the result depends on the scratch contents"
    return outs[0]


def _check_conv(s3r, lib, c):
    got = run_conv(s3r, lib, c)
    if got is None:
        return
    x, p, want = _data(c.data)
    assert_bits(got, want, c.data, p, c.id)


# ---------------------------------------------------------------- direct fp32
@pytest.mark.parametrize("case", X.DIRECT_CASES, ids=[c.id for c in X.DIRECT_CASES])
def test_direct_fp32(s3r, lib, case):
    _check_conv(s3r, lib, case)


# ---------------------------------------------------------------- linear
LINEAR_RUNS = X.LINEAR_CASES + X.LINEAR_NULL_BIAS


@pytest.mark.parametrize("case", LINEAR_RUNS, ids=[c.id for c in LINEAR_RUNS])
def test_linear(s3r, lib, case):
    """s3r_linear_forward: the shapes the suite began with, the point head, every branch of the launch plan (tests/_linear_cases.py)
    and, once per kernel of the plan, bias = NULL"""
    l, B = case.layer, case.B
    x, p, want = _data(case.data)
    need = lib.s3r_linear_scratch_elems(B, l.cin, l.cout)
    assert need >= 0, lib.s3r_last_error()
    w, b = p["w"].contiguous(), None if p["shift"] is None else p["shift"].contiguous()
    outs = []
    for fill in (("nan", "zero") if case.twice else ("nan",)):
        y = torch.full((B, l.cout), float("nan"), device=DEV)
        scr = torch.full((max(need, 1),), float("nan") if fill == "nan" else 0.0, device=DEV)
        rc_ok(lib, lib.s3r_linear_forward(x.data_ptr(), w.data_ptr(), b.data_ptr() if b is not None else None, y.data_ptr(), B, l.cin,
                                          l.cout, s3r._lib.ACT[l.act], scr.data_ptr(), need, None), case.id)
        sync()
        outs.append(y)
    if len(outs) == 2:
        assert torch.equal(outs[0].view(torch.int32), outs[1].view(torch.int32)), "the result depends on the scratch contents"
    assert_bits(outs[0], want, case.data, p, case.id)


# ---------------------------------------------------------------- bf16
@pytest.mark.parametrize("case", X.BF16_CASES, ids=[c.id for c in X.BF16_CASES])
def test_bf16(s3r, lib, case, mfma_shape):
    _check_conv(s3r, lib, case)


# ---------------------------------------------------------------- Winograd fp32
@pytest.mark.parametrize("case", X.WINO_CASES, ids=[c.id for c in X.WINO_CASES])
def test_winograd_fp32(s3r, lib, case):
    _check_conv(s3r, lib, case)


@pytest.mark.parametrize("case", X.WINO_SHAPE_CASES, ids=[c.id for c in X.WINO_SHAPE_CASES])
def test_winograd_shapes(s3r, lib, case):
    """tests/_exact_cases.py::_wino_shapes: ragged edges, couts and packs, and the LDS limits; the profiler record names the form
    that ran — for the dual case unconditionally (276 serial workgroups: more than this device's compute units, or B must grow)"""
    if case.id == X.DUAL_CASE:
        cus = torch.cuda.get_device_properties(0).multi_processor_count
        assert X.serial_workgroups(case.layer, case.n_in, case.B) > cus, ("raise B of the dual case: this device has", cus, "compute units")
        assert case.ran == ("winograd-dual",)
    _check_conv(s3r, lib, case)


# ---------------------------------------------------------------- every epilogue site under the four vector forms
@pytest.mark.parametrize("case", X.EP_CASES, ids=[c.id for c in X.EP_CASES])
def test_epilogue_forms(s3r, lib, case, monkeypatch):
    """tests/_exact_cases.py::_ep_sites: scale and shift each given or NULL (a NULL POINTER) at every kernel that ends in
    `scale ? scale[m] : 1, shift ? shift[m] : 0`; the linear sites through an S3R_OP_LINEAR descriptor, the one route with a scale"""
    if case.dtype == "bf16":
        monkeypatch.setenv("S3R_BF16_MFMA", "32" if case.data.ep in ("ss", "00") else "16")      # (both matrix instructions over the forms)
    if case.layer.op == "linear":
        desc = make_desc(s3r, case)[1]
        assert lib.s3r_conv_scratch_elems(C.byref(desc)) == LC.plan(case.B, case.layer.cin, case.layer.cout).scratch
    _check_conv(s3r, lib, case)


def _semi_fused_batch(l, n):
    """smallest batch at which the library takes the semi-fused form of a two-axis Conv3d on this device (s3r_wino_axis2.hip,
    wino2_form: six workgroups per 64-cout x 64-position tile fill the compute units' four slots twice over)"""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    B = 1
    while -(-l.cout // 64) * -(-(B * (-(-n // 4)) ** 2 * n) // 64) * 6 < 8 * cus:
        B += 1
    return B


ERR_INVALID = -1          # S3R_ERR_INVALID (include/s3r.h)
REFUSED_AT_THE_LIMIT = [("conv2d", 124, 3, 3, b"128"), ("conv3d", 60, 3, 5, b"64")]


@pytest.mark.parametrize("op,n,oh,tile,bound", REFUSED_AT_THE_LIMIT, ids=[f"{r[0]}-e{r[1]}-oh{r[2]}-tile{r[3]}" for r in REFUSED_AT_THE_LIMIT])
def test_past_the_lds_limit_is_refused_before_anything_is_enqueued(s3r, lib, op, n, oh, tile, bound):
    """one padded plane of 130^2 floats, four padded slices of 66^2: refused by the scratch query AND by the forward — called with
    the scratch the planner used to grant such a descriptor (what the same descriptor needs at out_halo = 2, where it fits: the
    scratch of these forms does not depend on the output's halo) — with S3R_ERR_INVALID, a message that names the bound, and the
    output and the scratch still holding their NaN fill.  (The forward used to enqueue the input transform and fail in the launcher.)"""
    l = X.L("t", op, 32, 2, 3, 1, 1)
    nd = 2 if op == "conv2d" else 3
    desc = s3r._lib.make_desc(l, 1, n, tile=tile, in_halo=1, out_halo=oh, algo=X.WINO)
    assert lib.s3r_conv_scratch_elems(C.byref(desc)) == ERR_INVALID and bound in lib.s3r_last_error(), lib.s3r_last_error()
    fits = s3r._lib.make_desc(l, 1, n, tile=tile, in_halo=1, out_halo=2, algo=X.WINO)
    need = lib.s3r_conv_scratch_elems(C.byref(fits))
    assert need > 0, lib.s3r_last_error()
    npk = C.c_int64(0)
    rc_ok(lib, lib.s3r_conv_packed_elems(C.byref(fits), C.byref(npk)), "packed_elems")      # (the packed layout knows no halo)
    g = torch.Generator().manual_seed(n)
    w = torch.randn((2, 32) + (3,) * nd, generator=g).to(DEV)
    pk = torch.zeros(npk.value, device=DEV)
    rc_ok(lib, lib.s3r_conv_pack_weights(C.byref(fits), w.data_ptr(), pk.data_ptr(), None), "pack_weights")
    x = torch.randn((1, 32) + (n + 2,) * nd, generator=g).to(DEV)
    sc, sh = torch.ones(2, device=DEV), torch.zeros(2, device=DEV)
    y = torch.full((1, 2) + (n + 2 * oh,) * nd, float("nan"), device=DEV)
    scr = torch.full((need,), float("nan"), device=DEV)
    rc = lib.s3r_conv_forward(C.byref(desc), x.data_ptr(), pk.data_ptr(), sc.data_ptr(), sh.data_ptr(), y.data_ptr(), scr.data_ptr(), need, None)
    err = lib.s3r_last_error()
    sync()
    assert rc == ERR_INVALID and bound in err, (rc, err)
    assert bool(torch.isnan(y).all()) and bool(torch.isnan(scr).all()), "a refused call wrote to its output or its scratch"


def test_library_pick_past_the_semi_fused_limit_runs_class_parallel(s3r, lib):
    """Conv3d 32 -> 2 over edge 60 with out_halo 3 under the two-axis algorithm in the LIBRARY's launch form (algo = WINOGRAD,
    tile = 3), at the smallest batch at which the library takes the semi-fused form on this device: four 66^2 slices do not fit
    its finish kernel, so the plan is the class-parallel form — the call used to fail in the launcher with an opaque HIP error.
    That the semi-fused form did not run follows from the launcher's own check, which the refusal test above shows intact at
    this very shape.  Bit-exact like every other form.  (tile = -1 resolves an edge above 28 to the one-axis kernel.)"""
    l = X.L("t", "conv3d", 32, 2, 3, 1, 1)
    B = _semi_fused_batch(l, 60)
    assert B >= 2 and B <= 4, ("the semi-fused form from batch", B)
    c = X.XCase("ws2-library-form-conv3d-32to2-e60-oh3", X._wino_data(l, B, 60, 850, "f43x2"), tile=3, algo=X.WINO, out_halo=3,
                ran=("winograd-2axis",))
    x, p = c.data.make()
    assert LT.admissible(LT.exactness(l, x, p, "f43x2")) is None
    _check_conv(s3r, lib, c)


# ---------------------------------------------------------------- producers that write a consumer's input
@pytest.mark.parametrize("case", X.CV_CASES, ids=[c.id for c in X.CV_CASES])
def test_cost_volume_planes_feed_v1(s3r, lib, case):
    """the cost volume written as v1's transformed plane sets (never as a volume), v1 reading them through in_layout"""
    l, B, D, H, W, Cc = case.data.layer, case.B, X.spec.MAX_DISP, X.spec.FEAT_HW, X.spec.FEAT_HW, X.spec.FEAT_C
    vol, p = case.make()
    vol = vol.to(DEV)
    p = {k: None if v is None else v.to(DEV).contiguous() for k, v in p.items()}
    want = LT.expected(l, vol, p)
    fl, fr = (t.to(DEV).contiguous() for t in case.features())
    if case.kind == "wino":
        n, fn, layout = 6 * B * 2 * Cc * (D + 2) * (H // 4) * (W + 2), lib.s3r_cost_volume_forward_wino, s3r._lib.LAYOUT_WINO_H
    else:
        n, fn, layout = 36 * B * 2 * Cc * (D // 4) * (H // 4) * (W + 2), lib.s3r_cost_volume_forward_wino2, s3r._lib.LAYOUT_WINO_DH
    planes = torch.zeros(n, device=DEV)                        # (the plane layouts are written into a zero-initialised buffer: include/s3r.h)
    rc_ok(lib, fn(fl.data_ptr(), fr.data_ptr(), planes.data_ptr(), B, Cc, D, H, W, None), case.id)
    desc = s3r._lib.make_desc(l, B, D, in_halo=1, algo=X.WINO, in_layout=layout)
    need = lib.s3r_conv_scratch_elems(C.byref(desc))
    assert need >= 0, lib.s3r_last_error()
    npk = C.c_int64(0)
    rc_ok(lib, lib.s3r_conv_packed_elems(C.byref(desc), C.byref(npk)), "packed_elems")
    pk = torch.full((npk.value,), float("nan"), device=DEV)
    rc_ok(lib, lib.s3r_conv_pack_weights(C.byref(desc), p["w"].data_ptr(), pk.data_ptr(), None), "pack_weights")
    outs = []
    for fill in ("nan", "zero"):
        y = torch.full((B, l.cout, D, H, W), float("nan"), device=DEV)
        scr = torch.full((max(need, 1),), float("nan") if fill == "nan" else 0.0, device=DEV)
        rc_ok(lib, lib.s3r_conv_forward(C.byref(desc), planes.data_ptr(), pk.data_ptr(), p["scale"].data_ptr(), p["shift"].data_ptr(),
                                        y.data_ptr(), scr.data_ptr(), need, None), case.id)
        sync()
        outs.append(y)
    assert torch.equal(outs[0].view(torch.int32), outs[1].view(torch.int32)), "the result depends on the scratch contents"
    assert_bits(outs[0], want, case.data, p, case.id)


_INTER = {}


def _intermediate(case, x, p0):
    """the first layer's exact output, kept for the cases that share (first Data, producer form)"""
    key = (case.first, case.pep, case.dtype)
    if key not in _INTER:
        _INTER.clear()
        _INTER[key] = case.intermediate(x, p0)
    return _INTER[key]


CHAIN_RUNS = [(c, m) for c in X.ALL_CHAIN_CASES for m in ((32, 16) if c.dtype == "bf16" else (None,))]


@pytest.mark.parametrize("case,mfma", CHAIN_RUNS, ids=[c.id + (f"-mfma{m}" if m else "") for c, m in CHAIN_RUNS])
def test_chain_handoff(s3r, lib, case, mfma, monkeypatch):
    """two layers through s3r_chain_forward: the stem writing e2's transformed planes; bf16 d3 with the head fused into its launch
    (under both matrix instructions); every route of the fp32 conv + head launch (tests/_exact_cases.py::_head_chains) under the
    head's four epilogue forms and a NULL / NULL and an integer producer epilogue"""
    bf = case.dtype == "bf16"
    if mfma:
        monkeypatch.setenv("S3R_BF16_MFMA", str(mfma))
    x, ps = case.make()
    x = x.to(DEV)
    ps = [{k: None if v is None else v.to(DEV).contiguous() for k, v in p.items()} for p in ps]
    parts = (case.first, case.second)
    want = LT.expected(case.second.layer, _intermediate(case, x, ps[0]), ps[1])       # (every chain here ends in fp32)
    B = case.first.B
    arr = (s3r._lib.Layer * 2)()
    keep = []
    for i, (d, p) in enumerate(zip(parts, ps)):
        desc = s3r._lib.make_desc(d.layer, B, d.n_in, tag=i, dtype=s3r._lib.DTYPE[case.dtype], algo=0 if i else case.algo,
                                  tile=-1 if i else case.tile)
        npk = C.c_int64(0)
        rc_ok(lib, lib.s3r_conv_packed_elems(C.byref(desc), C.byref(npk)), "packed_elems")
        pk = torch.full((npk.value,), float("nan"), device=DEV)
        rc_ok(lib, lib.s3r_conv_pack_weights(C.byref(desc), p["w"].data_ptr(), pk.data_ptr(), None), "pack_weights")
        arr[i].desc, arr[i].packed_w = desc, pk.data_ptr()
        arr[i].scale = p["scale"].data_ptr() if p["scale"] is not None else None
        arr[i].shift = p["shift"].data_ptr() if p["shift"] is not None else None
        keep.append(pk)
    need = lib.s3r_chain_workspace_elems(arr, 2)
    assert need > 0 or (need == 0 and case.fused), lib.s3r_last_error()      # (a fused pair over an unpadded input needs no workspace)
    xin = x.to(torch.bfloat16).permute(0, *range(2, x.dim()), 1).contiguous() if bf else x.contiguous()
    outs = []
    s3r.profile_enable(16)
    try:
        for fill in ("nan", "zero"):
            y = torch.full(want.shape, float("nan"), device=DEV)
            ws = torch.full((max(need, 1),), float("nan") if fill == "nan" else 0.0, device=DEV)
            rc_ok(lib, lib.s3r_chain_forward(arr, 2, xin.data_ptr(), y.data_ptr(), ws.data_ptr(), need, 1, None), case.id)
            sync()
            outs.append(y)
        rec = s3r.profile_read(16)
    finally:
        s3r.profile_enable(0)
    assert torch.equal(outs[0].view(torch.int32), outs[1].view(torch.int32)), "the result depends on the workspace contents"
    if case.fused:    # the head rode in the first layer's launch, on the forced form
        first = [r for r in rec if r["family"] == "conv_mfma" and r["tag"] == 0]
        assert not [r for r in rec if r["family"] == "head"] and len(first) == 2, rec
        assert not case.ran or all(r["ran"] in case.ran for r in first), (case.ran, first)
    elif bf:          # the hand-off under test is the one that ran: the head inside d3's launch; e2 on a Winograd form
        assert not [r for r in rec if r["family"] == "head"] and [r for r in rec if r["family"] == "conv_mfma" and r["tag"] == 0], rec
    else:
        assert [r for r in rec if r["family"] == "conv_mfma" and r["tag"] == 1 and r["ran"].startswith("winograd")], rec
    assert_bits(outs[0], want, case.second, ps[1], case.id)


# ---------------------------------------------------------------- the instrument itself, on the device
@pytest.mark.parametrize("case", [c for c in X.ALL_CASES if c.id in ("p1-B1", "linear-32x32768x1024-none", "v6-relu-B1", "wino2-tile3-v5")],
                         ids=lambda c: c.id)
def test_one_dropped_term_is_a_mismatch(s3r, lib, case, monkeypatch):
    """ONE (channel, tap) weight zeroed in what the kernel is given: the output must differ from the untouched reference, and equal
    the reference of the mutated weights bit for bit — at K = 32768 and 16384, below tests/_ref64.py's bound"""
    x, p, want = _data(case.data)
    w = p["w"]
    t = int(w.reshape(-1).nonzero()[0, 0])
    q = dict(p, w=w.clone())
    q["w"].reshape(-1)[t] = 0.0
    monkeypatch.setitem(_DATA, case.data, (x, q, LT.expected(case.layer, x, q)))
    if case.layer.op == "linear":
        y = torch.full((case.B, case.layer.cout), float("nan"), device=DEV)
        need = lib.s3r_linear_scratch_elems(case.B, case.layer.cin, case.layer.cout)
        scr = torch.full((max(need, 1),), float("nan"), device=DEV)
        rc_ok(lib, lib.s3r_linear_forward(x.data_ptr(), q["w"].data_ptr(), q["shift"].data_ptr(), y.data_ptr(), case.B, case.layer.cin,
                                          case.layer.cout, s3r._lib.ACT[case.layer.act], scr.data_ptr(), need, None), case.id)
        sync()
        got = y
    else:
        got = run_conv(s3r, lib, case)
    assert not torch.equal(got.view(torch.int32), want.view(torch.int32)), "a dropped term went unseen"
    assert_bits(got, _DATA[case.data][2], case.data, q, case.id)
