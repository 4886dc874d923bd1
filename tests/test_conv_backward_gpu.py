"""s3r_conv_backward on the device, through the C-ABI in guarded, poisoned buffers unless stated: gs and grad_shift bit for bit against
tests/_convbwd64.py's restatement, grad_w per element within bound32(K, sum|term|) of float64 and exactly equal on integer lattices,
run / address / scratch-content / output-subset invariance, the batch-composition rule of the header, grad_x through the adjoint layer's
forward — each over the twelve original geometries and over the tiling sweep R.SHAPES (every branch of convbwd_geo and of the GEMM
kernel's masks) —, the rule that what lies beyond the tensors is replaced by 0 and not multiplied by 0 (one planted NaN), refusals that enqueue nothing, the module level (d3 + d4 under VoxelBCELoss against float64 autograd, a three-step SGD loop run
twice, trunk_features), and the profiler record.

There is no measured tolerance in this file."""
import ctypes as C
import functools
import itertools

import numpy as np
import pytest
import torch

from tests import _convbwd64 as R
from tests import _guard as G
from tests import _ref64 as R64

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32 = torch.float32
POISON = G._BITS[F32][2]
INVALID, WORKSPACE = -1, -3

RUNS = [(c, a) for i, c in enumerate(R.CASES) for a in R.acts_of(i)] + [(c, a) for c in R.D3 + R.LONG_ROWS for a in ("none", "relu")]
RUNS += [(c, a) for c in R.SHAPES for a in ("none", "relu")] + [(R.SHAPES[i], "sigmoid") for i in R.SHAPES_SIGMOID]
_ids = lambda r: f"{R.case_id(r[0])}-{r[1]}"
NAMES = ("gs", "grad_w", "grad_shift")


@pytest.fixture(scope="module")
def lib(s3r):
    return s3r.load_library()


def _rc(lib, rc, what):
    assert rc == 0, f"{what}: {lib.s3r_last_error().decode()} ({rc})"


def _same_bits(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    bad = np.argwhere(R.bits(got) != R.bits(want))
    assert bad.size == 0, f"{what}: {len(bad)} elements differ, first at {tuple(bad[0])}: got {got[tuple(bad[0])]!r} want {want[tuple(bad[0])]!r}"


def desc_of(s3r, c, act, B=None, **over):
    L = s3r._lib
    d = L.ConvDesc(L.OP_DECONV if c.op == "deconv" else L.OP_CONV, c.nd, c.B if B is None else B, c.cin, c.cout, c.n, c.k, c.s, c.p,
                   L.ACT[act], 3, -1, 0, 0, 0, 0, 0, 0, 0, 1, c.opad, 0.0)
    for k, v in over.items():
        setattr(d, k, v)
    return d


def run(s3r, lib, c, act, x, y, gy, scale, need=(True, True, True), fill="nan", expect=0, short=0, **over):
    """One guarded call on numpy fp32 inputs (y / scale may be None).  Returns (gs, grad_w, grad_shift) as numpy, None for a side not asked
    for.  EVERY output buffer is allocated, poisoned and guarded; a side that is not asked for is passed as NULL and must still hold nothing
    but poison afterwards.  `expect` != 0: the call must be refused with that code and leave every output untouched.  Skews come from an
    enclosing `with G.skews(...)`; fill "random" fills the scratch with normal noise."""
    B = x.shape[0]
    d = desc_of(s3r, c, act, B=B)
    need_elems = lib.s3r_conv_backward_scratch_elems(C.byref(d))
    assert need_elems > 0, lib.s3r_last_error()
    for k, v in over.items():
        setattr(d, k, v)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a))
    ins = [G.Guarded("x", x.shape, F32, DEV, "in", data=t(x)), G.Guarded("grad_y", gy.shape, F32, DEV, "in", data=t(gy))]
    yb = G.Guarded("y", y.shape, F32, DEV, "in", data=t(y)) if y is not None else None
    sb = G.Guarded("scale", scale.shape, F32, DEV, "in", data=t(scale)) if scale is not None else None
    ins += [b for b in (yb, sb) if b is not None]
    outs = [G.Guarded("gs", gy.shape, F32, DEV, "out"), G.Guarded("grad_w", R.weight_shape(c), F32, DEV, "out"),
            G.Guarded("grad_shift", (c.cout,), F32, DEV, "out")]
    elems = need_elems - short
    scr = G.Guarded("scratch", (max(elems, 1),), F32, DEV, "scratch", fill="zero" if fill == "zero" else "nan")
    if fill == "random":
        scr.t.normal_(generator=torch.Generator(device=DEV).manual_seed(5))
    ptrs = [o.ptr if n else None for o, n in zip(outs, need)]
    rc = lib.s3r_conv_backward(C.byref(d), ins[0].ptr, yb.ptr if yb is not None else None, ins[1].ptr, sb.ptr if sb is not None else None,
                               *ptrs, scr.ptr, elems, None)
    torch.cuda.synchronize()
    G.check_all(*ins)
    where = scr.check()
    assert where is None, where
    if expect:
        assert rc == expect and lib.s3r_last_error().decode(), (rc, expect)
        need = (False, False, False)
        if fill == "nan":
            assert bool((G._as_bits(scr.t) == G._BITS[F32][4]).all()), "a refused call wrote to the scratch"
    else:
        _rc(lib, rc, "conv backward")
    res = []
    for o, n in zip(outs, need):
        if n:
            G.check_all(o)
            res.append(o.t.cpu().numpy())
        else:
            o.role = "scratch"                                     # nothing may have been written: guards intact, every element still poison
            G.check_all(o)
            assert bool((G._as_bits(o.t) == POISON).all()), f"{o.name} was not asked for but was written"
            res.append(None)
    return tuple(res)


@functools.lru_cache(maxsize=None)
def random_case(c, act):
    """inputs and references of a (case, act), computed once and shared (left unchanged by the tests).  The sweep's x and grad_y have
    mean 1 (R.data_mean: on zero-mean data the any-order bound exceeds the gradient itself from K of about 10^5 on)"""
    x, w, scale, shift, y, gy = R.make(c, seed=31 * R.out_edge(c) + c.cin + c.B, act=act, mean=R.data_mean(c))
    if act == "none":
        y = None
    g = R.g32(y, gy, act)
    gs = R.gs32(g, scale)
    return dict(x=x, w=w, scale=scale, y=y, gy=gy, g=g, gs=gs, gb=R.grad_shift32(g), f64=R.grad_w64(c, x, gs))


# ---------------------------------------------------------------- values
@pytest.mark.parametrize("r", RUNS, ids=_ids)
def test_random_data_bit_for_bit_and_against_float64(s3r, lib, r):
    """gs and grad_shift bit for bit against the restated rule and order; grad_w per element within bound32(K, mag) of float64, K the
    number of terms whose fine position lies inside the grid (at most B Q), mag the float64 sum of |terms|"""
    c, act = r
    k = random_case(c, act)
    gs, gw, gb = run(s3r, lib, c, act, k["x"], k["y"], k["gy"], k["scale"])
    _same_bits(gs, k["gs"], "gs")
    _same_bits(gb, k["gb"], "grad_shift")
    ref, K, mag = k["f64"]
    err, lim = np.abs(gw.astype(np.float64) - ref), R.bound32(K, mag)
    ratio = np.divide(err, lim, out=np.where(err > 0, np.inf, 0.0), where=lim > 0)      # (a tap that never meets the grid has bound 0: it must be 0)
    print(f"grad_w max err / bound {ratio.max():.3e}, max |grad_w| {np.abs(ref).max():.3e}")
    assert (err <= lim).all(), f"worst at {np.unravel_index(ratio.argmax(), err.shape)}: {ratio.max()}"


@pytest.mark.parametrize("r", RUNS, ids=_ids)
def test_integer_lattice_is_exact(s3r, lib, r):
    """small integers in x, grad_y and scale: every product and every partial sum of grad_w is an integer below 2^24 (asserted: the float64
    sum of |terms| is), so fp32 arithmetic is exact in any order and grad_w must EQUAL the float64 result; so must grad_shift"""
    c, act = r
    act = "relu" if act == "sigmoid" else act
    x, _, scale, _, y, gy = R.make(c, seed=7, lattice=True)
    y = None if act == "none" else y
    g = R.g32(y, gy, act)
    gsr = R.gs32(g, scale)
    ref, K, mag = R.grad_w64(c, x, gsr)
    assert mag.max() < 2 ** 24 and np.abs(g).sum() < 2 ** 24
    gs, gw, gb = run(s3r, lib, c, act, x, y, gy, scale)
    _same_bits(gs, gsr, "gs")
    assert np.array_equal(gw.astype(np.float64), ref)
    assert np.array_equal(gb.astype(np.float64), g.astype(np.float64).sum(axis=(0,) + tuple(range(2, 2 + c.nd))))
    assert np.abs(ref).max() > 0


@pytest.mark.parametrize("c", [R.SHAPES[3], R.CASES[3]._replace(B=1, n=41)], ids=R.case_id)
def test_k_slices_are_added_in_ascending_order(s3r, lib, c):
    """grad_w[i] of a sample is (((slab 0 + slab 1) + slab 2) + ...) (csrc/s3r_conv_bwd.hip, convbwd_finish_kernel).  One coarse position in
    each of the first three K slices carries grad_y = 2^15, -2^15, 2^-10 in every channel and x is 2^15 everywhere, so every slab holds ONE
    non-zero term per element (exact whatever the order inside a slab): 2^30, -2^30 and 32.  In the defined order the sum is
    (2^30 - 2^30) + 32 = 32, the float64 value; an order that meets 32 while +-2^30 is still in the accumulator loses it (ulp(2^30) = 128)."""
    sl = R.slice_index(c)
    assert R.geo(c).nsl >= 3 and c.op == "conv" and c.B == 1
    o = R.out_edge(c)
    gy = np.zeros(R.y_shape(c), np.float32)
    for i, v in enumerate((2.0 ** 15, -2.0 ** 15, 2.0 ** -10)):
        inner = np.argwhere((sl == i) & np.pad(np.ones((o - 2,) * c.nd, bool), 1))       # (off the edge: every tap meets the grid, asserted below)
        gy[(0, slice(None)) + tuple(inner[len(inner) // 2])] = v
    x = np.full(R.x_shape(c), 2.0 ** 15, np.float32)
    ref, _, _ = R.grad_w64(c, x, gy)
    assert (ref == 32.0).all()
    _, gw, _ = run(s3r, lib, c, "none", x, None, gy, None, need=(False, True, False))
    assert np.array_equal(gw.astype(np.float64), ref), (np.unique(gw), "the K slices were not added in ascending order")


@pytest.mark.parametrize("c", [R.D3[0], R.CASES[1]], ids=R.case_id)
def test_no_activation_and_no_scale_reads_grad_y_itself(s3r, lib, c):
    """act none, scale NULL: gs IS grad_y, and with gs NULL the weight-gradient GEMM reads grad_y directly (no prep pass, nothing of gs in
    the scratch).  gs bit-equal to grad_y, grad_w within the bound, and grad_w alone / grad_w + grad_shift carry the bits of the full call"""
    x, _, _, _, _, gy = R.make(c, seed=11, act="none", scale=False)
    gs, gw, gb = run(s3r, lib, c, "none", x, None, gy, None)
    _same_bits(gs, gy, "gs")
    _same_bits(gb, R.grad_shift32(gy), "grad_shift")
    ref, K, mag = R.grad_w64(c, x, gy)
    assert (np.abs(gw.astype(np.float64) - ref) <= R.bound32(K, mag)).all()
    _same_bits(run(s3r, lib, c, "none", x, None, gy, None, need=(False, True, False))[1], gw, "grad_w alone")
    _same_bits(run(s3r, lib, c, "none", x, None, gy, None, need=(False, True, True))[1], gw, "grad_w with grad_shift")


# ---------------------------------------------------------------- invariance
STABLE = [(c, "relu") for c in R.CASES] + [(R.CASES[5], "sigmoid"), (R.D3[0], "relu"), (R.LONG_ROWS[0], "none")]
# of the sweep: the ragged last slice (k6 s2 n40), a halved run (3D k4 s4), stride-2 segments (n141), the second 64-sample block (B = 70)
STABLE += [(R.SHAPES[3], "relu"), (R.SHAPES[5], "relu"), (R.SHAPES[11], "relu"), (R.SHAPES[19], "relu")]


@pytest.mark.parametrize("r", STABLE, ids=_ids)
def test_runs_addresses_scratch_contents_and_output_subsets_do_not_matter(s3r, lib, r):
    c, act = r
    k = random_case(c, act)
    args = (s3r, lib, c, act, k["x"], k["y"], k["gy"], k["scale"])
    base = run(*args)
    for what, got in (("second run", run(*args)), ("zero-filled scratch", run(*args, fill="zero")), ("random scratch", run(*args, fill="random"))):
        for n, a, b in zip(NAMES, got, base):
            _same_bits(a, b, f"{n}, {what}")
    for sk in (1, 2, 3):
        with G.skews(lambda name, dtype, role, sk=sk: 1 + (sk + len(name)) % 3):      # every pointer 1-3 elements past a 256-byte boundary
            got = run(*args)
        for n, a, b in zip(NAMES, got, base):
            _same_bits(a, b, f"{n}, skew pattern {sk}")
    for need in itertools.product((True, False), repeat=3):
        if not any(need) or all(need):
            continue
        got = run(*args, need=need)
        for n, a, b, asked in zip(NAMES, got, base, need):
            if asked:
                _same_bits(a, b, f"{n}, outputs {need}")
            else:
                assert a is None


@pytest.mark.parametrize("c", [R.CASES[3], R.CASES[0]._replace(B=5), R.CASES[6]._replace(B=5),
                               R.SHAPES[3]._replace(B=3), R.SHAPES[0]._replace(B=3), R.SHAPES[19]], ids=R.case_id)
def test_a_batch_is_the_ascending_sum_of_its_samples(s3r, lib, c):
    """the header's order: per element, a sample's slabs in ascending slice order, then the per-sample partials in ascending b starting
    from sample 0's.  A B = 1 call returns the sample's partial, so the batch's grad_w (and grad_shift) is the ascending fp32 sum of the
    B = 1 results — which can hold only when the slicing does not depend on the batch.  Of the sweep: the ragged last slice and the two
    128-row groups at B = 3, and B = 70 (the finish kernels' second block of 64 samples), where grad_shift is the restated order's too."""
    assert c.B in (3, 5, 70)
    k = random_case(c, "relu")
    _, gw, gb = run(s3r, lib, c, "relu", k["x"], k["y"], k["gy"], k["scale"])
    _same_bits(gb, k["gb"], "grad_shift against the restated order")
    accw = accb = None
    for b in range(c.B):
        one = slice(b, b + 1)
        gs1, gw1, gb1 = run(s3r, lib, c, "relu", k["x"][one], k["y"][one], k["gy"][one], k["scale"])
        _same_bits(gs1, k["gs"][one], "gs of one sample")
        accw = gw1 if accw is None else (accw + gw1).astype(np.float32)
        accb = gb1 if accb is None else (accb + gb1).astype(np.float32)
    _same_bits(gw, accw, "grad_w")
    _same_bits(gb, accb, "grad_shift")


# ---------------------------------------------------------------- what lies beyond the tensors is replaced, not multiplied
# odd mc with a pad column (mc 33, WLP 34); a short last chunk (7 chunks of 3 rows over 20); a short last segment of a ConvTranspose
# (70 = 64 + 6); two 128-row groups with a partial f tile (Ca 130, Cf 3)
NAN_CASES = [R.SHAPES[9], R.SHAPES[3], R.SHAPES[10], R.SHAPES[0]]


@pytest.mark.parametrize("c", NAN_CASES, ids=R.case_id)
def test_nan_in_the_fine_tensor_poisons_exactly_its_own_sums(s3r, lib, c):
    """ONE NaN in F (x of a Conv, grad_y of a ConvTranspose; act none and scale NULL, so gs is grad_y itself).  By the header's formula
    grad_w[a][f][t] = sum A[b][a][q] F[b][f][q s - p + t] it is a term of grad_w[a][f*][t] for every a and exactly the taps t for which,
    on every axis, pos + p - t is a multiple of s with quotient in [0, mc) (R.nan_taps, pinned against the formula on the CPU): those
    are NaN, and EVERY other element has the bits of the clean run — the kernel reads positions, channels and taps beyond the tensors
    from clamped addresses (channel Cf - 1, position 0: the first planted place) and must replace them by 0, not multiply them by 0.
    Nothing is planted in A: what a NaN there does against the zero padding is not a stated contract."""
    x, _, _, _, _, gy = R.make(c, seed=13, act="none", scale=False)
    call = lambda x, gy: run(s3r, lib, c, "none", x, None, gy, None, need=(False, True, False))[1]
    clean = call(x, gy)
    assert np.isfinite(clean).all()
    fine = gy if c.op == "deconv" else x
    B, Cf, nf = fine.shape[0], fine.shape[1], fine.shape[2]
    places = [(0, Cf - 1) + (0,) * c.nd, (B - 1, 0) + (nf - 1,) * c.nd, (0, Cf // 2) + tuple(nf // 2 + i for i in range(c.nd))]
    hit_any = False
    for place in places:
        planted = fine.copy()
        planted[place] = np.nan
        got = call(*((x, planted) if c.op == "deconv" else (planted, gy)))
        want_nan = np.zeros(clean.shape, bool)
        want_nan[:, place[1]] = R.nan_taps(c, place[2:])
        hit_any |= bool(want_nan.any())
        is_nan = np.isnan(got)
        bad = np.argwhere(is_nan != want_nan)
        assert bad.size == 0, f"NaN at F{place}: {len(bad)} elements of grad_w are NaN / not NaN against the formula, first at {tuple(bad[0])}"
        _same_bits(np.where(want_nan, 0, got), np.where(want_nan, 0, clean), f"grad_w outside the sums of F{place}")
    assert hit_any


# ---------------------------------------------------------------- grad_x through the adjoint layer
def _adjoint_layer(s3r, c):
    op = ("conv" if c.op == "deconv" else "deconv") + f"{c.nd}d"
    return s3r.arch_spec.Layer("adj", op, c.cout, c.cin, c.k, c.s, c.p, False, "none", 1, R.adjoint_out_pad(c))


def _layer(s3r, c, act):
    return s3r.arch_spec.Layer("l", ("deconv" if c.op == "deconv" else "conv") + f"{c.nd}d", c.cin, c.cout, c.k, c.s, c.p, True, act, 1, c.opad)


@pytest.mark.parametrize("r", RUNS, ids=_ids)
def test_grad_x_through_the_adjoint_forward(s3r, r):
    """conv_backward(need_x only): grad_x = the adjoint layer's forward on gs with the layer's own weight, against torch's float64 autograd
    of sum(gs * linmap(x, w)) with respect to x (gs as the device holds it: its bits are pinned above), within tests/_ref64.py's bound for
    the adjoint layer's kernel — the tolerance tests/test_buffers_gpu.py applies to those kernels.  Also: grad_w and grad_shift through the
    Python surface carry the C-ABI's bits."""
    c, act = r
    k = random_case(c, act)
    layer, adj = _layer(s3r, c, act), _adjoint_layer(s3r, c)
    dev = lambda a: None if a is None else torch.from_numpy(a).to(DEV)
    gx, gw, gb = s3r.conv_backward(dev(k["x"]), dev(k["w"]), dev(k["y"]), dev(k["gy"]), layer, scale=dev(k["scale"]))
    torch.cuda.synchronize()
    assert gx.shape == k["x"].shape and gw.shape == k["w"].shape and gb.shape == (c.cout,)
    _same_bits(gb.cpu().numpy(), k["gb"], "grad_shift")
    xd = torch.from_numpy(k["x"]).double().requires_grad_()
    w64, gs64 = torch.from_numpy(k["w"]).double(), torch.from_numpy(k["gs"]).double()
    (ref,) = torch.autograd.grad((gs64 * R.linmap(c, xd, w64)).sum(), xd)
    assert np.allclose(ref.numpy(), R.grad_x64(c, k["w"], k["gs"]), rtol=1e-10, atol=1e-12)      # (the identity, once more, on this data)
    mag = torch.from_numpy(R.grad_x64(c, np.abs(k["w"]), np.abs(k["gs"])))
    lim = R64.bound(adj, ref, mag, "direct")
    worst, at = R64.worst(gx.cpu(), ref, lim)
    print(f"grad_x max err / bound {worst:.3e}")
    assert worst <= 1.0, (worst, at)
    only_x = s3r.conv_backward(dev(k["x"]), dev(k["w"]), dev(k["y"]), dev(k["gy"]), layer, scale=dev(k["scale"]), need_w=False, need_shift=False)
    assert only_x[1] is None and only_x[2] is None and torch.equal(only_x[0].view(torch.int32), gx.view(torch.int32))


def test_packed_weight_cache_follows_the_tensor_and_its_version(s3r):
    """the packed image belongs to a live weight TENSOR at one `_version`: a new tensor in a freed tensor's memory (the allocator hands
    the block to the next tensor of that size) is packed afresh, and an in-place update packs again"""
    c = R.CASES[5]
    layer = _layer(s3r, c, "none")
    k = random_case(c, "relu")
    x = torch.from_numpy(k["x"]).to(DEV)
    w1 = torch.from_numpy(k["w"]).to(DEV)
    y1 = s3r.conv_forward(x, w1, None, None, layer)
    addr = w1.data_ptr()
    del w1
    w2 = torch.from_numpy(-2 * k["w"]).to(DEV)                     # -2 w: exact in fp32, so the layer's output is exactly -2 y1
    reused = w2.data_ptr() == addr
    y2 = s3r.conv_forward(x, w2, None, None, layer)
    print(f"the second weight reused the first one's address: {reused}")
    assert torch.equal(y2, -2 * y1) and bool(y1.abs().max() > 0)
    w2.mul_(-0.5)                                                  # in place: the same tensor, the next version
    assert torch.equal(s3r.conv_forward(x, w2, None, None, layer), y1)
    gx_a = s3r.conv_backward(x, w2, None, y1, layer, need_w=False, need_shift=False)[0]
    w2.mul_(2.0)
    gx_b = s3r.conv_backward(x, w2, None, y1, layer, need_w=False, need_shift=False)[0]
    assert torch.equal(gx_b, 2 * gx_a) and bool(gx_a.abs().max() > 0)


# ---------------------------------------------------------------- refusals
@pytest.mark.parametrize("what", ["all-null", "short-scratch", "bf16", "dilation-2"])
def test_refusals_enqueue_nothing(s3r, lib, what):
    c = R.CASES[5]
    k = random_case(c, "relu")
    args = (s3r, lib, c, "relu", k["x"], k["y"], k["gy"], k["scale"])
    if what == "all-null":
        run(*args, need=(False, False, False), expect=INVALID)
    elif what == "short-scratch":
        run(*args, short=1, expect=WORKSPACE)
    elif what == "bf16":
        run(*args, expect=INVALID, dtype=1)
    else:
        run(*args, expect=INVALID, dilation=2)


# ---------------------------------------------------------------- the module level
@functools.lru_cache(maxsize=None)
def _decoder_state():
    import s3r
    return s3r.seeded_state_dict(s3r.Decoder(), seed=4)


def _decoder(s3r):
    dec = s3r.Decoder()
    dec.load_state_dict(_decoder_state())
    return dec.to(DEV)


@functools.lru_cache(maxsize=None)
def _d2_features(B, seed):
    """d2's output for a seeded volume, computed once and shared (left unchanged by the tests)"""
    import s3r
    vol = 0.5 * torch.randn(B, 64, 28, 28, 28, generator=torch.Generator().manual_seed(seed))
    x = _decoder(s3r).forward(vol.to(DEV), upto="d2")
    torch.cuda.synchronize()
    return vol, x


def _gt(B, seed):
    return (torch.rand(B, 32, 32, 32, generator=torch.Generator().manual_seed(seed)) < 0.3).float()


@pytest.mark.parametrize("B", [1, 2, 5])
def test_standalone_d3_forward_has_the_bits_of_the_chain(s3r, B):
    """Decoder.differentiable_features — d3 of differentiable_tail itself: a one-layer chain on d2's output, scale from folded(), shift
    built by torch under grad — against Decoder.features (the chain up to d3): both run d3's three-axis Winograd form on the same input;
    its launch forms agree bit for bit (include/s3r.h, s3r_algo), so the bits are equal.  conv_forward on folded()'s pair gives them too"""
    dec = _decoder(s3r)
    vol, x = _d2_features(B, 1)
    assert x.shape == (B, 128, 16, 16, 16)
    want = dec.features(vol.to(DEV))
    got = dec.differentiable_features(x)
    assert got.grad_fn is not None and got.shape == want.shape
    got = got.detach()
    scale, shift = dec.d3.folded()
    alone = s3r.conv_forward(x, dec.d3.conv.weight, scale, shift, s3r.arch_spec.DECODER[-2])
    torch.cuda.synchronize()
    same = torch.equal(got.view(torch.int32), want.view(torch.int32))
    print(f"B = {B}: d3 of differentiable_tail bit-identical to Decoder.features: {same}; max |d| {(got - want).abs().max().item():.3e}")
    assert same
    assert torch.equal(alone.view(torch.int32), want.view(torch.int32))


def _f64(t):
    return t.detach().cpu().double()


def test_tail_gradients_under_the_bce_loss_against_float64_autograd(s3r):
    """d3's and d4's gradients of VoxelBCELoss(Decoder.differentiable_tail(x)) at B = 2 against torch autograd in float64 of the same folded
    graph (conv_transpose3d * scale + shift, ReLU, conv3d 1x1x1 + bias, sigmoid, BCELoss) on the same d2 activation.

    The bound carries every stage's worst-case error forward and back (all quantities below are float64 reference values):
      E_a  = _ref64.bound(d3, "wino") on d3's output (its three-axis Winograd form);
      E_z  = sum_c |w4_c| E_a + bound32(65, sum |a_c w4_c| + |b4|);      E_y = E_z / 4 + (2 |z| + 6) u y        (tests/_head64.py)
      E_g4 = (E_y + gamma_8 (|y - t| + E_y)) / N                        (tests/test_head_backward_gpu.py's derivation of g = (y - t) / N)
      d4.weight: sum (|a| E_g4 + (|g4| + E_g4) E_a) + bound32(K, sum (|a| + E_a) (|g4| + E_g4)), K = B S;  d4.bias: the same with a = 1, E_a = 0
      grad of d3's output: gx = g4 w4_c, E_gx = |w4_c| E_g4 + u |w4_c| (|g4| + E_g4)
      ReLU gate: where the reference pre-activation is within E_a of 0 the device may gate the other way: E_g3 = E_gx + [|t3| <= E_a] (|gx| + E_gx)
      gs = g3 * scale: E_gs = |scale| E_g3 + u |scale| (|g3| + E_g3)
      d3.conv.weight: W(|x|, E_gs) + bound32(K, W(|x|, |gs| + E_gs)), W the weight-gradient formula, K = B Q
      grad_shift: sum E_g3 + bound32(K, sum (|g3| + E_g3)), K = B S: bn.bias.grad is grad_shift; conv.bias.grad = grad_shift * scale in
      torch (one more rounding)."""
    B = 2
    dec = _decoder(s3r)
    _, x = _d2_features(B, 1)
    gt = _gt(B, 2)
    for p in dec.parameters():
        p.grad = None
    loss = s3r.VoxelBCELoss()(dec.differentiable_tail(x), gt.to(DEV))
    loss.backward()
    torch.cuda.synchronize()
    params = dict(dec.named_parameters())
    trained = ["d3.conv.weight", "d3.conv.bias", "d3.bn.bias", "d4.conv.weight", "d4.conv.bias"]
    assert [n for n, p in params.items() if p.grad is not None] == trained
    assert params["d3.bn.weight"].grad is None
    # ---- the float64 graph (on the device in float64 where torch has the operator there; the values are reference quantities)
    ref_dev = DEV
    x64 = x.detach().double()
    try:
        probe = torch.nn.functional.conv_transpose3d(x64[:1, :, :2, :2, :2], params["d3.conv.weight"].detach().double(), None, 2, 1)
        torch.nn.functional.max_pool3d(probe, 9, 1, 4)
    except RuntimeError:
        ref_dev = "cpu"
    x64 = x64.to(ref_dev)
    P = {n: params[n].detach().double().to(ref_dev).requires_grad_() for n in trained}
    bn = dec.d3.bn
    scale = (bn.weight.detach().double() * torch.rsqrt(bn.running_var.detach().double() + bn.eps)).to(ref_dev)
    mean = bn.running_mean.detach().double().to(ref_dev)
    bc = lambda v: v.reshape(1, -1, 1, 1, 1)
    t3 = torch.nn.functional.conv_transpose3d(x64, P["d3.conv.weight"], None, 2, 1) * bc(scale) + bc(P["d3.bn.bias"] + (P["d3.conv.bias"] - mean) * scale)
    a3 = torch.relu(t3)
    z = torch.nn.functional.conv3d(a3, P["d4.conv.weight"], P["d4.conv.bias"]).squeeze(1)
    y = torch.sigmoid(z)
    t = gt.double().to(ref_dev)
    ref_loss = torch.nn.BCELoss()(y, t)
    grads = dict(zip(trained, torch.autograd.grad(ref_loss, [P[n] for n in trained])))
    with torch.no_grad():
        N, u = y.numel(), R.U32
        w3, w4, b4 = P["d3.conv.weight"].detach(), P["d4.conv.weight"].detach().reshape(-1), P["d4.conv.bias"].detach()
        shift3 = (P["d3.bn.bias"] + (P["d3.conv.bias"] - mean) * scale).detach()
        mag3 = torch.nn.functional.conv_transpose3d(x64.abs(), w3.abs(), None, 2, 1) * bc(scale.abs()) + bc(shift3.abs())
        e_a = R64.bound(s3r.arch_spec.DECODER[-2], a3, mag3, "wino")
        mag4 = torch.einsum("bcdhw,c->bdhw", a3.abs(), w4.abs()) + b4.abs()
        e_z = torch.einsum("bcdhw,c->bdhw", e_a, w4.abs()) + R.bound32(65, mag4)
        e_y = e_z / 4 + (2 * z.abs() + 6) * u * y
        assert float((y * (1 - y)).min()) > 1e-11
        g4 = (y - t) / N
        e_g4 = (e_y + R.gamma(8) * ((y - t).abs() + e_y)) / N
        K4 = N
        lim = {}
        lim["d4.conv.weight"] = (torch.einsum("bcdhw,bdhw->c", a3.abs(), e_g4) + torch.einsum("bcdhw,bdhw->c", e_a, g4.abs() + e_g4) +
                                 R.bound32(K4, torch.einsum("bcdhw,bdhw->c", a3.abs() + e_a, g4.abs() + e_g4))).reshape(1, 64, 1, 1, 1)
        lim["d4.conv.bias"] = (e_g4.sum() + R.bound32(K4, (g4.abs() + e_g4).sum())).reshape(1)
        gx = g4.unsqueeze(1) * bc(w4)
        e_gx = bc(w4.abs()) * e_g4.unsqueeze(1) + u * bc(w4.abs()) * (g4.abs() + e_g4).unsqueeze(1)
        g3 = torch.where(t3 > 0, gx, torch.zeros_like(gx))
        e_g3 = e_gx + (t3.abs() <= e_a).double() * (gx.abs() + e_gx)
        gs = g3 * bc(scale)
        e_gs = bc(scale.abs()) * e_g3 + u * bc(scale.abs()) * (g3.abs() + e_g3)

        def W(a, f):                                               # the weight-gradient formula of the transposed layer: a on the coarse grid
            w = torch.zeros_like(w3).requires_grad_()
            with torch.enable_grad():
                out = torch.nn.functional.conv_transpose3d(a, w, None, 2, 1)
                (r,) = torch.autograd.grad((out * f).sum(), w)
            return r

        K3 = B * 16 ** 3
        lim["d3.conv.weight"] = W(x64.abs(), e_gs) + R.bound32(K3, W(x64.abs(), gs.abs() + e_gs))
        KS = B * 32 ** 3
        shift_lim = e_g3.sum((0, 2, 3, 4)) + R.bound32(KS, (g3.abs() + e_g3).sum((0, 2, 3, 4)))
        lim["d3.bn.bias"] = shift_lim
        lim["d3.conv.bias"] = shift_lim * scale.abs() + u * (g3.sum((0, 2, 3, 4)).abs() + shift_lim) * scale.abs()
    print(f"loss {loss.item():.7g} vs float64 {ref_loss.item():.7g} (reference on {ref_dev})")
    for n in trained:
        got, ref, l = _f64(params[n].grad), grads[n].cpu(), lim[n].cpu()
        assert got.shape == ref.shape == l.shape, n
        err = (got - ref).abs()
        print(f"{n}: max err / bound {(err / l).max().item():.3e}; max |grad| {ref.abs().max().item():.3e}, max bound {l.max().item():.3e}")
        assert bool((err <= l).all()), n
        # the bound is a worst case over the signs of every term; for the comparison to see a mistake it must stay well below the
        # gradient: at most 5 % of the largest element (both are float64 reference quantities, not outputs of the kernels under test)
        assert l.max().item() <= 5e-2 * ref.abs().max().item() and ref.abs().max().item() > 0, n


def test_fine_tune_loop_on_d3_and_d4_is_deterministic_and_descends(s3r):
    """three SGD steps on d3 + d4 under the BCE loss, twice from the same state: identical parameter bits, and the loss after the third
    step is below the loss before the first (a small step along the negative gradient of a smooth loss)"""
    B = 2
    _, x = _d2_features(B, 1)
    gt = _gt(B, 3).to(DEV)

    def three_steps():
        dec = _decoder(s3r)
        names = ["d3.conv.weight", "d3.conv.bias", "d3.bn.bias", "d4.conv.weight", "d4.conv.bias"]
        params = dict(dec.named_parameters())
        opt = torch.optim.SGD([params[n] for n in names], lr=0.05)
        bce = s3r.VoxelBCELoss()
        losses = []
        for _ in range(3):
            opt.zero_grad()
            loss = bce(dec.differentiable_tail(x), gt)
            loss.backward()
            opt.step()
            losses.append(loss.item())
        with torch.no_grad():
            losses.append(bce(dec.differentiable_tail(x), gt).item())
        return {n: p.detach().clone() for n, p in dec.named_parameters()}, losses

    a, la = three_steps()
    b, lb = three_steps()
    print(f"losses {la}")
    assert la == lb and all(np.isfinite(la))
    assert la[3] < la[0]
    state = _decoder_state()
    for n in a:
        assert torch.equal(a[n].view(torch.int32), b[n].view(torch.int32)), n
        moved = not torch.equal(a[n].cpu(), state[n])
        assert moved == (n in ("d3.conv.weight", "d3.conv.bias", "d3.bn.bias", "d4.conv.weight", "d4.conv.bias")), f"{n}: moved = {moved}"


def test_trunk_features(s3r):
    model = s3r.Stereo2Voxel()
    s3r.seed_module(model, seed=0)
    model.to(DEV)
    left, right = s3r.synthetic_pairs(1, seed=0, device=DEV)
    d3 = model.trunk_features(left, right, upto="d3")
    assert torch.equal(d3.view(torch.int32), model.head_features(left, right).view(torch.int32))
    d2 = model.trunk_features(left, right)
    assert d2.shape == (1, 128, 16, 16, 16) and d2.grad_fn is None and not d2.requires_grad
    out = model.decoder.differentiable_tail(d2)
    assert out.shape == (1, 32, 32, 32) and out.grad_fn is not None
    with pytest.raises(RuntimeError, match="upto must be"):
        model.trunk_features(left, right, upto="d4")


def test_profiler_record(s3r, lib):
    c = R.CASES[5]
    k = random_case(c, "relu")
    layer = _layer(s3r, c, "relu")
    dev = lambda a: torch.from_numpy(a).to(DEV)
    x, w, y, gy, sc = (dev(k[n]) for n in ("x", "w", "y", "gy", "scale"))
    s3r.profile_enable(16)
    try:
        s3r.conv_backward(x, w, y, gy, layer, scale=sc, need_x=False)
        s3r.conv_backward(x, w, y, gy, layer, scale=sc, need_x=False, need_w=False)
        torch.cuda.synchronize()
        rec = s3r.profile_read(16)
    finally:
        s3r.profile_enable(0)
    tag = s3r._lib.CONV_BACKWARD_TAG
    assert [(r["family"], r["tag"]) for r in rec] == [("conv_mfma", tag), ("conv_mfma", tag)]
    assert all(r["ms"] > 0 for r in rec)
    X, Y, Wn, Q = k["x"].size, k["gy"].size, k["w"].size, c.n ** 3
    assert rec[0]["flops"] == 2.0 * c.B * Q * c.cin * c.cout * c.k ** 3 and rec[0]["bytes"] == 4.0 * (2 * Y + c.cout + X + Wn + c.cout)
    assert rec[1]["flops"] == 0.0 and rec[1]["bytes"] == 4.0 * (2 * Y + c.cout + c.cout)
    assert rec[0]["launches"] == 4 and rec[1]["launches"] == 2           # prep + shift finish + GEMM + slab finish; prep + shift finish
