"""s3r_cost_volume_backward on the device, through the C-ABI in guarded, poisoned buffers unless stated: bit for bit against the restated
fp32 order (tests/_costvol64.py), per element within the derived bound of float64, exact on integer lattices, blind to NaN and
infinity at every class of structural-zero position, a NaN at a live position in exactly the outputs whose sums hold it, run /
address / output-content / output-subset / batch invariance, the profiler record, and the autograd surface.

There is no measured tolerance in this file."""
import functools

import numpy as np
import pytest
import torch

from tests import _costvol64 as R
from tests import _guard as G

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32 = torch.float32
POISON = G._BITS[F32][2]
INVALID = -1
_ids = R.case_id


@pytest.fixture(scope="module")
def lib(s3r):
    return s3r.load_library()


def _same_bits(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.argwhere(R.bits(got) != R.bits(want))
    assert bad.size == 0, f"{what}: {len(bad)} elements differ, first at {tuple(bad[0])}: got {got[tuple(bad[0])]!r} want {want[tuple(bad[0])]!r}"


def run(lib, gv, need=(True, True), expect=0, prefill=None, dims=None):
    """One guarded call on a numpy fp32 grad_volume.  Returns (grad_left, grad_right) as numpy, None for a side not asked for.  BOTH
    outputs are allocated, poisoned (or filled with `prefill`) and guarded; a side that is not asked for is passed as NULL and must hold
    what it held.  `expect` != 0: the call must be refused with that code and leave both outputs untouched.  Skews come from an
    enclosing `with G.skews(...)`."""
    B, C2, D, H, W = gv.shape
    src = G.Guarded("grad_volume", gv.shape, F32, DEV, "in", data=torch.from_numpy(np.array(gv, np.float32)))
    outs = [G.Guarded(n, (B, C2 // 2, H, W), F32, DEV, "out") for n in ("grad_left", "grad_right")]
    if prefill is not None:
        for o in outs:
            o.t.fill_(prefill)
    before = [G._as_bits(o.t).clone() for o in outs]
    ptrs = [o.ptr if n else None for o, n in zip(outs, need)]
    rc = lib.s3r_cost_volume_backward(src.ptr, *ptrs, *(dims or (B, C2 // 2, D, H, W)), None)
    torch.cuda.synchronize()
    G.check_all(src)
    if expect:
        assert rc == expect and lib.s3r_last_error().decode(), (rc, expect)
        need = (False, False)
    else:
        assert rc == 0, f"{lib.s3r_last_error().decode()} ({rc})"
    res = []
    for o, n, b in zip(outs, need, before):
        if n:
            G.check_all(o)
            res.append(o.t.cpu().numpy())
        else:
            o.role = "scratch"                                     # nothing may have been written: guards intact, every element as before
            G.check_all(o)
            assert torch.equal(G._as_bits(o.t), b), f"{o.name} was not asked for but was written"
            res.append(None)
    return tuple(res)


@functools.lru_cache(maxsize=None)
def reference(case, data):
    """(gv, backward32, backward64) of a (case, data set), computed once and shared (left unchanged by the tests)"""
    gv = {"random": R.random_gv, "lattice": R.lattice_gv, "signed zeros": R.signed_zero_gv}[data](case)
    return gv, R.backward32(gv), R.backward64(gv)


@functools.lru_cache(maxsize=None)
def device_result(case, data="random"):
    import s3r
    return run(s3r.load_library(), reference(case, data)[0])


# ---------------------------------------------------------------- values
@pytest.mark.parametrize("case", R.CASES, ids=_ids)
def test_bits_equal_the_defined_order(lib, case):
    for data in ("random", "signed zeros"):
        gv, (wl, wr), _ = reference(case, data)
        gl, gr = device_result(case, data)
        _same_bits(gl, wl, f"grad_left, {data}")
        _same_bits(gr, wr, f"grad_right, {data}")
    assert np.signbit(device_result(case, "signed zeros")[0]).all()          # -0.0: the accumulator started as t_0


@pytest.mark.parametrize("case", R.CASES, ids=_ids)
def test_within_the_derived_bound_of_float64(lib, case):
    _, _, (gl64, gr64, nl, nr, ml, mr) = reference(case, "random")
    gl, gr = device_result(case)
    worst = 0.0
    for got, ref, n, mag in ((gl, gl64, nl, ml), (gr, gr64, nr, mr)):
        ratio = np.abs(got.astype(np.float64) - ref) / R.bound32(n, mag)
        worst = max(worst, ratio.max())
    print(f"{R.case_id(case)}: largest error / bound {worst:.3e}")
    assert worst <= 1.0


@pytest.mark.parametrize("case", R.CASES, ids=_ids)
def test_integer_lattice_is_exact(lib, case):
    gv, _, (gl64, gr64, *_) = reference(case, "lattice")
    assert np.abs(gv).max() <= 8
    gl, gr = device_result(case, "lattice")
    assert np.array_equal(gl.astype(np.float64), gl64) and np.array_equal(gr.astype(np.float64), gr64)
    assert np.abs(gl64).max() > 0


# ---------------------------------------------------------------- non-finite values
@pytest.mark.parametrize("value", [np.nan, np.inf], ids=["nan", "inf"])
@pytest.mark.parametrize("case", R.SMALL + R.CASES[6:7], ids=_ids)
def test_structural_zeros_are_not_read_into_the_arithmetic(lib, case, value):
    """a NaN, and separately +inf, at EVERY position of a class of structural zeros (left slab w < d, right slab w + d >= W, the planes
    d >= W) changes no output bit"""
    gv = reference(case, "random")[0]
    base = device_result(case)
    planted = 0
    for name, mask in R.structural_zero_masks(case).items():
        if not mask.any():
            continue
        planted += 1
        gl, gr = run(lib, np.where(mask, np.float32(value), gv).astype(np.float32))
        _same_bits(gl, base[0], f"grad_left, {value} in {name}")
        _same_bits(gr, base[1], f"grad_right, {value} in {name}")
    B, Cc, D, H, W = case
    assert planted == (3 if D > W else 2 if D > 1 else 0)


def test_a_nan_at_a_live_position_poisons_exactly_the_outputs_that_hold_it(lib):
    case = R.CASES[4]
    B, Cc, D, H, W = case
    gv = reference(case, "random")[0].copy()
    gv[1, 1, 2, 3, 7] = np.nan                  # left slab: grad_left[1,1,3,7] and grad_right[1,1,3,5]
    gv[2, Cc + 0, 3, 4, 5] = np.nan             # right slab: grad_right[2,0,4,5] and grad_left[2,0,4,8]
    wl, wr = R.backward32(gv)
    assert np.isnan(wl).sum() == 2 and np.isnan(wr).sum() == 2
    gl, gr = run(lib, gv)
    for got, want, what in ((gl, wl, "grad_left"), (gr, wr, "grad_right")):
        assert np.array_equal(np.isnan(got), np.isnan(want)), what
        keep = ~np.isnan(want)
        assert np.array_equal(R.bits(got)[keep], R.bits(want)[keep]), what


# ---------------------------------------------------------------- invariance
@pytest.mark.parametrize("case", R.CASES, ids=_ids)
def test_null_forms_have_the_bits_of_the_full_call(lib, case):
    gv = reference(case, "random")[0]
    base = device_result(case)
    gl, none = run(lib, gv, need=(True, False))
    assert none is None
    _same_bits(gl, base[0], "grad_left alone")
    none, gr = run(lib, gv, need=(False, True))
    assert none is None
    _same_bits(gr, base[1], "grad_right alone")


@pytest.mark.parametrize("case", R.CASES[:7], ids=_ids)
def test_runs_addresses_and_output_contents_do_not_matter(lib, case):
    gv = reference(case, "random")[0]
    base = device_result(case)
    again = [("second run", run(lib, gv)), ("outputs holding 1.0", run(lib, gv, prefill=1.0)), ("outputs holding -inf", run(lib, gv, prefill=-np.inf))]
    for sk in (1, 2, 3):
        with G.skews(lambda name, dtype, role, sk=sk: 1 + (sk + len(name)) % 3):      # every pointer 1-3 elements past a 256-byte boundary
            again.append((f"skew pattern {sk}", run(lib, gv)))
    for what, got in again:
        _same_bits(got[0], base[0], f"grad_left, {what}")
        _same_bits(got[1], base[1], f"grad_right, {what}")


@pytest.mark.parametrize("case", [R.CASES[4], R.CASES[7]], ids=_ids)
def test_a_sample_has_the_bits_of_its_own_call(lib, case):
    """batch invariance: every output is its own sum, so sample b of a batch equals, bit for bit, the B = 1 call on it"""
    gv = reference(case, "random")[0]
    base = device_result(case)
    for b in range(case[0]):
        gl, gr = run(lib, gv[b:b + 1])
        _same_bits(gl, base[0][b:b + 1], f"grad_left of sample {b}")
        _same_bits(gr, base[1][b:b + 1], f"grad_right of sample {b}")


@pytest.mark.parametrize("what", ["both-null", "zero-width", "negative-batch", "plane-too-large"])
def test_refusals_enqueue_nothing(lib, what):
    case = R.CASES[0]
    gv = reference(case, "random")[0]
    B, Cc, D, H, W = case
    if what == "both-null":
        run(lib, gv, need=(False, False), expect=INVALID)
    else:
        dims = {"zero-width": (B, Cc, D, H, 0), "negative-batch": (-1, Cc, D, H, W), "plane-too-large": (B, Cc, D, 128, 128)}[what]
        run(lib, gv, expect=INVALID, dims=dims)


def test_batch_zero_writes_nothing(s3r, lib):
    case = R.CASES[0]
    B, Cc, D, H, W = case
    gv = reference(case, "random")[0]
    src = G.Guarded("grad_volume", gv.shape, F32, DEV, "in", data=torch.from_numpy(gv.copy()))
    out = G.Guarded("grad_left", (B, Cc, H, W), F32, DEV, "out")
    assert lib.s3r_cost_volume_backward(src.ptr, out.ptr, out.ptr, 0, Cc, D, H, W, None) == 0
    torch.cuda.synchronize()
    assert bool((G._as_bits(out.t) == POISON).all())
    gl, gr = s3r.cost_volume_backward(torch.empty(0, 2 * Cc, D, H, W, device=DEV))
    assert gl.shape == gr.shape == (0, Cc, H, W)


# ---------------------------------------------------------------- the profiler
def test_profiler_record(s3r, lib):
    case = R.CASES[6]
    B, Cc, D, H, W = case
    gv = torch.from_numpy(reference(case, "random")[0]).to(DEV)
    s3r.profile_enable(8)
    try:
        s3r.cost_volume_backward(gv)
        s3r.cost_volume_backward(gv, need_right=False)
        torch.cuda.synchronize()
        rec = s3r.profile_read(8)
    finally:
        s3r.profile_enable(0)
    assert [(r["family"], r["tag"], r["launches"]) for r in rec] == [("cost_volume", 1, 1), ("cost_volume", 1, 1)]
    assert all(r["ms"] > 0 for r in rec)
    vol, feat = 2 * Cc * D * H * W, Cc * H * W
    assert rec[0]["bytes"] == 4.0 * B * (vol + 2 * feat) == 5820416.0          # the byte model: 5.6 MB of grad_volume + 0.2 MB of gradients per sample
    assert rec[1]["bytes"] == 4.0 * B * (vol + feat)
    terms = sum(min(D, w + 1) for w in range(W))
    assert rec[0]["flops"] == 2.0 * 2 * B * Cc * H * terms and rec[1]["flops"] == 2.0 * B * Cc * H * terms


# ---------------------------------------------------------------- the autograd surface
@pytest.mark.parametrize("case", [R.CASES[0], R.CASES[4], R.CASES[6]], ids=_ids)
def test_differentiable_cost_volume(s3r, case):
    """value bit-equal to CostVolume.forward; backward bit-equal to the restated order for the output gradient autograd hands it; exactly
    the sides needs_input_grad asks for"""
    B, Cc, D, H, W = case
    g = torch.Generator().manual_seed(3)
    fl, fr = torch.randn(B, Cc, H, W, generator=g).to(DEV), torch.randn(B, Cc, H, W, generator=g).to(DEV)
    cv = s3r.CostVolume(max_disp=D)
    want = cv(fl, fr)
    gvn = reference(case, "random")[0]
    gv = torch.from_numpy(gvn).to(DEV)
    wl, wr = reference(case, "random")[1]
    for need in ((True, True), (True, False), (False, True)):
        a, b = fl.clone().requires_grad_(need[0]), fr.clone().requires_grad_(need[1])
        vol = cv.differentiable(a, b)
        assert vol.grad_fn is not None and torch.equal(vol.detach().view(torch.int32), want.view(torch.int32))
        vol.backward(gv)
        torch.cuda.synchronize()
        for t, w, n in ((a, wl, need[0]), (b, wr, need[1])):
            if n:
                _same_bits(t.grad.cpu().numpy(), w, f"needs_input_grad {need}")
            else:
                assert t.grad is None
    assert s3r.differentiable_cost_volume(fl, fr, D).grad_fn is None          # no input requires grad: no graph
    # behind torch operations: 2 on the left slab and 3 on the right one make every term -1 (left) / +1 (right): the counts n_L, n_R
    a, b = fl.clone().requires_grad_(), fr.clone().requires_grad_()
    vol = s3r.differentiable_cost_volume(a, b, D)
    (2 * vol[:, :Cc].sum() + 3 * vol[:, Cc:].sum()).backward()
    w = np.arange(W)
    assert np.array_equal(a.grad.cpu().numpy(), np.broadcast_to(-np.minimum(D, w + 1).astype(np.float32), (B, Cc, H, W)))
    assert np.array_equal(b.grad.cpu().numpy(), np.broadcast_to(np.minimum(D, W - w).astype(np.float32), (B, Cc, H, W)))


def test_surface_refusals(s3r):
    fl = torch.zeros(1, 8, 4, 4, device=DEV)
    with pytest.raises(RuntimeError, match="fp32 models only"):
        s3r.CostVolume(precision="bf16").differentiable(fl, fl)
    with pytest.raises(RuntimeError, match="must both be"):
        s3r.differentiable_cost_volume(fl, fl[:, :4], 4)
    with pytest.raises(RuntimeError, match="must be torch.float32"):
        s3r.cost_volume_backward(torch.zeros(1, 2, 2, 2, 2, device=DEV, dtype=torch.float64))
