"""s3r_stem_backward on the device, through the C-ABI in guarded, poisoned buffers: grad_shift bit for bit against the restated order,
grad_w per element within bound32(n_images m^2, sum|gs||X|) of float64 and exactly equal on integer lattices, both against
s3r_conv_backward on the converted, concatenated renders (grad_shift the same bits, grad_w within twice the bound, one planted NaN the
same pattern), run / address / scratch-content / output-subset / render-type / one-or-two-tensor invariance, the batch-composition rule,
refusals that leave poisoned outputs untouched, the Python surface and the profiler record.

Per case: ReLU and no activation, scale given and NULL, fp32 and 8-bit renders, one tensor and (n <= 5) every two-tensor split.
There is no measured tolerance in this file."""
import ctypes as C
import functools
import itertools

import numpy as np
import pytest
import torch

from tests import _convbwd64 as R
from tests import _guard as G
from tests import _stem64 as S

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32, U8 = torch.float32, torch.uint8
POISON = G._BITS[F32][2]
INVALID, WORKSPACE = -1, -3
ACT = {"none": 0, "relu": 1, "sigmoid": 2}
COMBOS = list(itertools.product(S.ACTS, (True, False), (False, True)))      # (act, scale given, 8-bit renders)
RENDERS = ("left", "right")


@pytest.fixture(scope="module")
def lib(s3r):
    return s3r.load_library()


def _same_bits(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    bad = np.argwhere(R.bits(got) != R.bits(want))
    assert bad.size == 0, f"{what}: {len(bad)} elements differ, first at {tuple(bad[0])}: got {got[tuple(bad[0])]!r} want {want[tuple(bad[0])]!r}"


def run(lib, x, y, gy, scale, act, n_left=None, need=(True, True), fill="nan", expect=0, short=0, over=None):
    """One guarded call.  x: the renders (numpy fp32 or uint8); n_left None: one tensor, else images [0, n_left) in `left` and the rest in
    `right`.  Returns (grad_w, grad_shift), None for a side not asked for (passed as NULL: it must hold nothing but poison afterwards).
    `expect` != 0: the call must be refused with that code and leave every output and the scratch untouched.  `over`: a function that
    edits the argument dict of the call (the refusals)."""
    n, in_size = x.shape[0], x.shape[2]
    need_elems = lib.s3r_stem_backward_scratch_elems(n, in_size)
    assert need_elems == S.scratch_elems(n, in_size), lib.s3r_last_error()
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a))
    rdt = U8 if x.dtype == np.uint8 else F32
    parts = [x] if n_left is None else [x[:n_left], x[n_left:]]
    rend = [G.Guarded(RENDERS[i], p.shape, rdt, DEV, "in", data=t(p), skew=0) for i, p in enumerate(parts)]      # (16-byte aligned: the contract)
    gyb = G.Guarded("grad_y", gy.shape, F32, DEV, "in", data=t(gy))
    yb = G.Guarded("y", y.shape, F32, DEV, "in", data=t(y)) if y is not None else None
    sb = G.Guarded("scale", scale.shape, F32, DEV, "in", data=t(scale)) if scale is not None else None
    ins = rend + [gyb] + [b for b in (yb, sb) if b is not None]
    outs = [G.Guarded("grad_w", (32, 3, 3, 3), F32, DEV, "out"), G.Guarded("grad_shift", (32,), F32, DEV, "out")]
    elems = need_elems - short
    scr = G.Guarded("scratch", (max(elems, 1),), F32, DEV, "scratch", fill="zero" if fill == "zero" else "nan")
    if fill == "random":
        scr.t.normal_(generator=torch.Generator(device=DEV).manual_seed(5))
    a = dict(left=rend[0].ptr, right=rend[1].ptr if len(rend) > 1 else None, n_left=n if n_left is None else n_left, u8=int(rdt == U8),
             y=yb.ptr if yb is not None else None, gy=gyb.ptr, scale=sb.ptr if sb is not None else None,
             gw=outs[0].ptr if need[0] else None, gb=outs[1].ptr if need[1] else None, n=n, in_size=in_size, act=ACT[act], scr=scr.ptr,
             elems=elems)
    if over is not None:
        over(a)
    rc = lib.s3r_stem_backward(a["left"], a["right"], a["n_left"], a["u8"], a["y"], a["gy"], a["scale"], a["gw"], a["gb"], a["n"],
                               a["in_size"], a["act"], a["scr"], a["elems"], None)
    torch.cuda.synchronize()
    G.check_all(*ins)
    where = scr.check()
    assert where is None, where
    if expect:
        assert rc == expect and lib.s3r_last_error().decode(), (rc, expect)
        need = (False, False)
        if fill == "nan":
            assert bool((G._as_bits(scr.t) == G._BITS[F32][4]).all()), "a refused call wrote to the scratch"
    else:
        assert rc == 0, f"stem backward: {lib.s3r_last_error().decode()} ({rc})"
    res = []
    for o, asked in zip(outs, need):
        if asked:
            G.check_all(o)
            res.append(o.t.cpu().numpy())
        else:
            o.role = "scratch"                                     # nothing may have been written: guards intact, every element still poison
            G.check_all(o)
            assert bool((G._as_bits(o.t) == POISON).all()), f"{o.name} was not asked for but was written"
            res.append(None)
    return tuple(res)


@functools.lru_cache(maxsize=None)
def data(case, act, scaled, u8, lattice=False):
    """inputs and references of one variant of a case, computed once and shared (left unchanged by the tests)"""
    n, s = case
    x, scale, y, gy = S.make(n, s, seed=17 * s + n + 2 * u8, act=act, u8=u8, lattice=lattice, scale=scaled)
    g = S.g32(y, gy, act)
    gs = S.gs32(g, scale)
    return dict(x=x, x32=S.render32(x), scale=scale, y=y, gy=gy, g=g, gs=gs, gb=S.grad_shift32(g), f64=S.grad_w64(S.render32(x), gs))


def _within(gw, f64, factor=1.0):
    ref, K, mag = f64
    err, lim = np.abs(gw.astype(np.float64) - ref), factor * S.bound32(K, mag)
    ratio = np.divide(err, lim, out=np.where(err > 0, np.inf, 0.0), where=lim > 0)
    print(f"grad_w max err / bound {ratio.max():.3e}, max |grad_w| {np.abs(ref).max():.3e}")
    assert (err <= lim).all(), f"worst at {np.unravel_index(ratio.argmax(), err.shape)}: {ratio.max()}"


# ---------------------------------------------------------------- values
@pytest.mark.parametrize("case", S.CASES, ids=S.case_id)
def test_random_data_bit_for_bit_and_against_float64(lib, case):
    """every variant: grad_shift bit for bit against the restated order, grad_w within bound32(n m^2, mag) of float64; with n <= 5 every
    two-tensor split returns the one-tensor call's bits"""
    n = case[0]
    for act, scaled, u8 in COMBOS:
        k = data(case, act, scaled, u8)
        gw, gb = run(lib, k["x"], k["y"], k["gy"], k["scale"], act)
        _same_bits(gb, k["gb"], f"grad_shift {act} scale {scaled} u8 {u8}")
        _within(gw, k["f64"])
        for n_left in range(1, n + 1) if n <= 5 else ():
            gw2, gb2 = run(lib, k["x"], k["y"], k["gy"], k["scale"], act, n_left=n_left)
            _same_bits(gw2, gw, f"grad_w, {n_left} of {n} images in the first tensor")
            _same_bits(gb2, gb, f"grad_shift, {n_left} of {n} images in the first tensor")


@pytest.mark.parametrize("case", S.CASES, ids=S.case_id)
def test_integer_lattice_is_exact(lib, case):
    """small integers in grad_y and scale, fp32 renders of small integers or 8-bit renders drawn from {0, 255} (X exactly 0 or 1): every
    product and partial sum is an integer below 2^24 (asserted), so both outputs must EQUAL the float64 result"""
    for act, scaled, u8 in COMBOS:
        k = data(case, act, scaled, u8, True)
        ref, K, mag = k["f64"]
        assert mag.max() < 2 ** 24 and np.abs(k["g"]).sum() < 2 ** 24
        gw, gb = run(lib, k["x"], k["y"], k["gy"], k["scale"], act, n_left=None if case[0] == 1 else 1)
        assert np.array_equal(gw.astype(np.float64), ref), (act, scaled, u8)
        assert np.array_equal(gb.astype(np.float64), k["g"].astype(np.float64).sum(axis=(0, 2, 3)))
        assert np.abs(ref).max() > 0 or case == (1, 1)


def _conv_backward(s3r, lib, c, act, x32, y, gy, scale):
    """s3r_conv_backward (grad_w and grad_shift) on the converted, concatenated renders"""
    L = s3r._lib
    d = L.ConvDesc(L.OP_CONV, 2, c.B, c.cin, c.cout, c.n, c.k, c.s, c.p, L.ACT[act], 3, -1, 0, 0, 0, 0, 0, 0, 0, 1, 0, 0.0)
    need = lib.s3r_conv_backward_scratch_elems(C.byref(d))
    assert need > 0, lib.s3r_last_error()
    dev = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    t = [dev(a) for a in (x32, y, gy, scale)]
    gw, gb = torch.empty((32, 3, 3, 3), device=DEV), torch.empty(32, device=DEV)
    scr = torch.empty(need, device=DEV)
    p = [None if a is None else a.data_ptr() for a in t]
    rc = lib.s3r_conv_backward(C.byref(d), p[0], p[1], p[2], p[3], None, gw.data_ptr(), gb.data_ptr(), scr.data_ptr(), need, None)
    torch.cuda.synchronize()
    assert rc == 0, lib.s3r_last_error()
    return gw.cpu().numpy(), gb.cpu().numpy()


@pytest.mark.parametrize("case", S.CASES, ids=S.case_id)
def test_against_conv_backward_on_the_converted_renders(s3r, lib, case):
    """8-bit renders in two tensors against s3r_conv_backward on their fp32 conversion in one: grad_shift the same bits, grad_w within
    twice the bound (each is within one bound of float64), and with ONE NaN planted in grad_y the same elements are NaN"""
    n, s = case
    c = S.conv_case(n, s)
    for act, scaled in itertools.product(S.ACTS, (True, False)):
        k = data(case, act, scaled, True)
        n_left = None if n == 1 else (n + 1) // 2
        gw, gb = run(lib, k["x"], k["y"], k["gy"], k["scale"], act, n_left=n_left)
        cw, cb = _conv_backward(s3r, lib, c, act, k["x32"], k["y"], k["gy"], k["scale"])
        _same_bits(gb, cb, "grad_shift against s3r_conv_backward")
        ref, K, mag = k["f64"]
        assert (np.abs(gw.astype(np.float64) - cw.astype(np.float64)) <= 2 * S.bound32(K, mag)).all()
    k = data(case, "relu", True, True)
    m = S.out_edge(s)
    gy = k["gy"].copy()
    y = k["y"].copy()
    place = (n - 1, 5, m - 1, m // 2)
    gy[place] = np.nan
    y[place] = 1.0                                                  # (the gate is open: the NaN is a term of the sums)
    gw, gb = run(lib, k["x"], y, gy, k["scale"], "relu")
    cw, cb = _conv_backward(s3r, lib, c, "relu", k["x32"], y, gy, k["scale"])
    assert np.array_equal(np.isnan(gw), np.isnan(cw)) and np.array_equal(np.isnan(gb), np.isnan(cb))
    assert np.isnan(gw[5]).all() and np.isnan(gb[5]) and np.isnan(gw).sum() == 27 and np.isnan(gb).sum() == 1


# ---------------------------------------------------------------- invariance
STABLE = [(3, 7), (2, 46), (1, 130), (5, 20), (70, 4), (2, 224)]


@pytest.mark.parametrize("case", STABLE, ids=S.case_id)
def test_runs_addresses_scratch_contents_output_subsets_and_render_forms_do_not_matter(lib, case):
    n = case[0]
    for act, scaled in (("relu", True), ("none", False)):
        k = data(case, act, scaled, True)
        args = (k["y"], k["gy"], k["scale"], act)
        base = run(lib, k["x"], *args)
        variants = [("second run", run(lib, k["x"], *args)), ("zero-filled scratch", run(lib, k["x"], *args, fill="zero")),
                    ("random scratch", run(lib, k["x"], *args, fill="random")),
                    ("the host conversion of the 8-bit renders", run(lib, k["x32"], *args)),
                    ("the host conversion in two tensors", run(lib, k["x32"], *args, n_left=1) if n > 1 else base)]
        for sk in (1, 2, 3):                                       # every fp32 pointer but the renders 1-3 elements past a 256-byte boundary
            with G.skews(lambda name, dtype, role, sk=sk: 1 + (sk + len(name)) % 3):
                variants.append((f"skew pattern {sk}", run(lib, k["x"], *args)))
                variants.append((f"skew pattern {sk}, fp32 renders", run(lib, k["x32"], *args)))
        for what, got in variants:
            _same_bits(got[0], base[0], f"grad_w, {what}")
            _same_bits(got[1], base[1], f"grad_shift, {what}")
        only_w, only_b = run(lib, k["x"], *args, need=(True, False)), run(lib, k["x"], *args, need=(False, True))
        assert only_w[1] is None and only_b[0] is None
        _same_bits(only_w[0], base[0], "grad_w alone")
        _same_bits(only_b[1], base[1], "grad_shift alone")


def test_a_batch_is_the_ascending_sum_of_its_images(lib):
    """(5, 20): grad_w (and grad_shift) of the batch equals, bit for bit, the ascending fp32 sum of the five single-image calls"""
    k = data((5, 20), "relu", True, True)
    gw, gb = run(lib, k["x"], k["y"], k["gy"], k["scale"], "relu", n_left=2)
    accw = accb = None
    for b in range(5):
        one = slice(b, b + 1)
        gw1, gb1 = run(lib, k["x"][one], k["y"][one], k["gy"][one], k["scale"], "relu")
        accw = gw1 if accw is None else (accw + gw1).astype(np.float32)
        accb = gb1 if accb is None else (accb + gb1).astype(np.float32)
    _same_bits(gw, accw, "grad_w")
    _same_bits(gb, accb, "grad_shift")


# ---------------------------------------------------------------- refusals
def _set(**kv):
    return lambda a: a.update(kv)


REFUSALS = {
    "both-null": dict(need=(False, False), expect=INVALID),
    "short-scratch": dict(short=1, expect=WORKSPACE),
    "null-scratch": dict(over=_set(scr=None), expect=WORKSPACE),
    "sigmoid": dict(over=_set(act=2), expect=INVALID),
    "y-null-with-relu": dict(over=_set(y=None), expect=INVALID),
    "null-grad-y": dict(over=_set(gy=None), expect=INVALID),
    "null-renders": dict(over=_set(left=None), expect=INVALID),
    "n-left-zero": dict(over=_set(n_left=0), expect=INVALID),
    "n-left-beyond": dict(over=_set(n_left=4), expect=INVALID),
    "one-tensor-n-left-short": dict(over=_set(right=None), expect=INVALID),
    "in-size-zero": dict(over=_set(in_size=0), expect=INVALID),
    "negative-images": dict(over=_set(n=-1), expect=INVALID),
    "misaligned-left": dict(over=lambda a: a.update(left=a["left"] + 4), expect=INVALID),
    "misaligned-right": dict(over=lambda a: a.update(right=a["right"] + 8), expect=INVALID),
}


@pytest.mark.parametrize("what", list(REFUSALS))
def test_refusals_enqueue_nothing(lib, what):
    """a refused call leaves the poisoned outputs and the scratch untouched"""
    k = data((3, 7), "relu", True, False)
    run(lib, k["x"], k["y"], k["gy"], k["scale"], "relu", n_left=2, **REFUSALS[what])
    if what.startswith("misaligned"):
        assert "16-byte aligned" in lib.s3r_last_error().decode()


def test_an_empty_batch_writes_nothing(lib):
    outs = torch.full((32 * 27 + 32,), float("nan"), device=DEV)
    before = outs.view(torch.int32).clone()
    x = torch.zeros(16, device=DEV)
    rc = lib.s3r_stem_backward(x.data_ptr(), None, 0, 0, None, x.data_ptr(), None, outs.data_ptr(), outs[864:].data_ptr(), 0, 7, 1, None, 0, None)
    torch.cuda.synchronize()
    assert rc == 0 and torch.equal(outs.view(torch.int32), before)


# ---------------------------------------------------------------- the Python surface and the profiler
@pytest.mark.parametrize("u8", [False, True])
def test_python_surface_has_the_abi_bits(s3r, lib, u8):
    k = data((5, 20), "relu", True, u8)
    base = run(lib, k["x"], k["y"], k["gy"], k["scale"], "relu", n_left=2)
    dev = lambda a: torch.from_numpy(a).to(DEV)
    gw, gb = s3r.stem_backward(dev(k["x"][:2]), dev(k["x"][2:]), dev(k["y"]), dev(k["gy"]), dev(k["scale"]), "relu")
    torch.cuda.synchronize()
    _same_bits(gw.cpu().numpy(), base[0], "grad_w")
    _same_bits(gb.cpu().numpy(), base[1], "grad_shift")
    gw1, gb1 = s3r.stem_backward(dev(k["x"]), None, dev(k["y"]), dev(k["gy"]), dev(k["scale"]), "relu", need_shift=False)
    assert gb1 is None
    _same_bits(gw1.cpu().numpy(), base[0], "grad_w alone, one tensor")


def test_profiler_record(s3r, lib):
    k = data((2, 46), "relu", True, True)
    dev = lambda a: torch.from_numpy(a).to(DEV)
    args = (dev(k["x"][:1]), dev(k["x"][1:]), dev(k["y"]), dev(k["gy"]), dev(k["scale"]), "relu")
    s3r._lib.profile_enable(16)
    try:
        s3r.stem_backward(*args)
        rec = s3r._lib.profile_read(16)
    finally:
        s3r._lib.profile_enable(0)
    mine = [r for r in rec if r["family"] == "stem" and r["tag"] == 1]
    assert len(mine) == 1 and len(rec) == 1, rec
    m = S.out_edge(46)
    Y = 2 * 32 * m * m
    assert mine[0]["flops"] == 2.0 * 2 * m * m * 32 * 27
    assert mine[0]["bytes"] == 4.0 * (2 * Y + 32 + 864 + 32) + 2 * 3 * 46 * 46
    assert mine[0]["launches"] == 5                                # the shift pass and its finish, the GEMM, the two finish launches
