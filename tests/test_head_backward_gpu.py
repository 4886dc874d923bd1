"""s3r_head_backward on the device, through the C-ABI in guarded, poisoned buffers unless stated: grad_x bit for bit (one
multiplication), grad_w and grad_shift bit for bit against the header's order as tests/_head64.py restates it AND per element within
bound32(K, sum|term|) of float64 (tests/_linear64.py's derivation), exact equality on integer lattices (tests/_lattice.py), B = 1,
scale NULL and given, every NULL form, run / address / scratch-content invariance, the autograd surface, the standalone head against
s3r_conv_forward (bit for bit) and against the fused d3 + d4 path of Decoder.forward (derived bound), d4's gradients under VoxelBCELoss
against torch autograd in float64 (derived bound), a three-step fine-tune run twice, and the profiler record.

There is no measured tolerance in this file."""
import ctypes as C
import functools
import itertools

import numpy as np
import pytest
import torch

from tests import _guard as G
from tests import _head64 as R
from tests import _lattice as LT

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32 = torch.float32
ACT = {"none": 0, "relu": 1, "sigmoid": 2}
POISON = G._BITS[F32][2]

CASES = [(s, a) for s in R.SHAPES for a in R.ACTS if s not in R.BIG or R.BIG[s] == a]
_ids = lambda c: "x".join(map(str, c[0])) + "-" + c[1]
SIDES = ("grad_x", "grad_w", "grad_shift")


@pytest.fixture(scope="module")
def lib(s3r):
    return s3r.load_library()


def _rc(lib, rc, what):
    assert rc == 0, f"{what}: {lib.s3r_last_error().decode()} ({rc})"


def _same_bits(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    gb, wb = R.bits(got), R.bits(want)
    bad = np.argwhere(gb != wb)
    assert bad.size == 0, f"{what}: {len(bad)} elements differ, first at {tuple(bad[0])}: got {got[tuple(bad[0])]!r} want {want[tuple(bad[0])]!r}"


def run(lib, x, w, scale, y, gy, act, need=(True, True, True), fill="nan", pass_y=True, pass_x=True, pass_w=True):
    """One guarded call.  x (B,C,S), w (C), y / gy (B,S): CPU fp32 tensors (y may be None); scale a float or None.  Returns (grad_x, grad_w,
    grad_shift) as numpy, None for a side not asked for.  EVERY output buffer is allocated, poisoned and guarded; a side that is not asked
    for is passed as NULL and its buffer must still hold nothing but poison afterwards.  Skews come from an enclosing `with G.skews(...)`."""
    B, ch, S = x.shape
    need_elems = lib.s3r_head_backward_scratch_elems(B, ch, S)
    assert need_elems > 0
    xb, wb = G.Guarded("x", (B, ch, S), F32, DEV, "in", data=x), G.Guarded("w", (ch,), F32, DEV, "in", data=w)
    gb = G.Guarded("grad_y", (B, S), F32, DEV, "in", data=gy)
    ins = [xb, wb, gb]
    yb = G.Guarded("y", (B, S), F32, DEV, "in", data=y) if y is not None else None
    sb = G.Guarded("scale", (1,), F32, DEV, "in", data=torch.tensor([scale], dtype=F32)) if scale is not None else None
    ins += [b for b in (yb, sb) if b is not None]
    outs = [G.Guarded("grad_x", (B, ch, S), F32, DEV, "out"), G.Guarded("grad_w", (ch,), F32, DEV, "out"), G.Guarded("grad_shift", (1,), F32, DEV, "out")]
    scr = G.Guarded("scratch", (need_elems,), F32, DEV, "scratch", fill=fill)
    ptrs = [o.ptr if n else None for o, n in zip(outs, need)]
    _rc(lib, lib.s3r_head_backward(xb.ptr if pass_x else None, wb.ptr if pass_w else None, sb.ptr if sb is not None else None,
                                   yb.ptr if (yb is not None and pass_y) else None, gb.ptr, *ptrs, B, ch, S, ACT[act], scr.ptr, need_elems,
                                   None), "head backward")
    torch.cuda.synchronize()
    G.check_all(*ins)
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
    where = scr.check()
    assert where is None, where
    if not (need[1] or need[2]) and fill == "nan":                # grad_x alone: no sum, so nothing is written to scratch
        assert bool((G._as_bits(scr.t) == G._BITS[F32][4]).all()), "scratch was written although only grad_x was asked for"
    return tuple(res)


def _scale_of(shape):
    return 0.75 if sum(shape) % 2 else None                       # (about half of the shapes carry a scale)


@functools.lru_cache(maxsize=None)
def random_case(shape, act):
    """(x, w, y, gy, scale) CPU tensors and the references, computed once per (shape, act) and shared"""
    B, ch, S = shape
    g = torch.Generator().manual_seed(B * 7919 + ch * 31 + S)
    x = torch.randn(B, ch, S, generator=g)
    w = torch.randn(ch, generator=g) / ch ** 0.5
    gy = torch.randn(B, S, generator=g)
    # y is an INPUT of the backward: any tensor of the activation's range exercises the rule (half the ReLU outputs are 0)
    y = None if act == "none" else torch.relu(torch.randn(B, S, generator=g)) if act == "relu" else torch.rand(B, S, generator=g)
    scale = _scale_of(shape)
    gg = R.g32(None if y is None else y.numpy(), gy.numpy(), act)
    gs = R.gs32(gg, scale)
    ref = dict(gx=R.grad_x32(gs, w.numpy()), gw=R.grad_w32(gs, x.numpy()), gb=R.grad_shift32(gg), f64=R.backward64(x.numpy(), gs, gg))
    return x, w, y, gy, scale, ref


@pytest.mark.parametrize("case", CASES, ids=_ids)
def test_random_data_bit_for_bit_and_against_float64(lib, case):
    shape, act = case
    x, w, y, gy, scale, ref = random_case(shape, act)
    gx, gw, gb = run(lib, x, w, scale, y, gy, act)
    _same_bits(gx, ref["gx"], "grad_x")
    _same_bits(gw, ref["gw"], "grad_w")
    _same_bits(gb, ref["gb"].reshape(1), "grad_shift")
    (gw64, K, mw), (gb64, _, mb) = ref["f64"]
    for got, want, mag, name in ((gw, gw64, mw, "grad_w"), (gb, gb64, mb, "grad_shift")):
        err, lim = np.abs(got.astype(np.float64) - want), R.bound32(K, mag)
        print(f"{shape} {act} {name}: K {K}, max err / bound {np.max(err / lim):.4f}")
        assert np.all(err <= lim), f"{name}: worst err / bound {np.max(err / lim):.3f}"


@pytest.mark.parametrize("scale", [None, 0.75, -2.0], ids=["scale-null", "scale-0.75", "scale-minus-2"])
@pytest.mark.parametrize("shape", [(2, 3, 5), (3, 4, 513), (1, 64, 256)], ids=lambda s: "x".join(map(str, s)))
def test_scale_null_and_given(lib, shape, scale):
    x, w, y, gy, _, _ = random_case(shape, "sigmoid")
    gg = R.g32(y.numpy(), gy.numpy(), "sigmoid")
    gs = R.gs32(gg, scale)
    gx, gw, gb = run(lib, x, w, scale, y, gy, "sigmoid")
    _same_bits(gx, R.grad_x32(gs, w.numpy()), "grad_x")
    _same_bits(gw, R.grad_w32(gs, x.numpy()), "grad_w")
    _same_bits(gb, R.grad_shift32(gg).reshape(1), "grad_shift (g, not gs)")


# ---------------------------------------------------------------- integer lattices: every partial sum is exact in fp32 in any order
@pytest.mark.parametrize("bn", [False, True], ids=["no-scale", "dyadic-scale"])
@pytest.mark.parametrize("act", ["none", "relu"])
@pytest.mark.parametrize("dims", [(1, 1, 1), (2, 3, 5), (1, 64, 8), (2, 64, 9), (3, 17, 10)], ids=lambda s: "x".join(map(str, s)))
def test_integer_lattice_is_exact(s3r, lib, dims, act, bn):
    B, ch, n = dims
    layer = s3r.arch_spec.Layer("h", "conv3d", ch, 1, 1, 1, 0, bn=bn, act=act)
    x, p = LT.lattice_case(layer, B, n, seed=sum(dims), xmax=2, wmax=2)
    x, w = x.reshape(B, ch, -1), p["w"].reshape(ch)
    scale = None if p["scale"] is None else float(p["scale"][0])
    z = np.einsum("bcs,c->bs", x.double().numpy(), w.double().numpy()) * (1.0 if scale is None else scale) + float(p["shift"][0])
    y64 = np.maximum(z, 0.0) if act == "relu" else z
    y = torch.from_numpy(y64.astype(np.float32))
    assert np.array_equal(y.double().numpy(), y64)                # the forward is exact on the lattice
    gy = torch.randint(-4, 5, (B, x.shape[2]), generator=torch.Generator().manual_seed(3 + sum(dims))).float()
    gg = R.g32(y.numpy(), gy.numpy(), act)
    gs = R.gs32(gg, scale)
    (gw64, _, mw), (gb64, _, mb) = R.backward64(x.numpy(), gs, gg)
    assert 4 * max(mw.max(), mb) < 2 ** 24                         # the premise (two fractional bits from a scale of 0.25)
    gx, gw, gb = run(lib, x, w, scale, y if act != "none" else None, gy, act)
    assert np.array_equal(gw.astype(np.float64), gw64), "grad_w"
    assert gb.astype(np.float64)[0] == gb64, "grad_shift"
    assert np.array_equal(gx.astype(np.float64), gs.astype(np.float64)[:, None, :] * w.double().numpy()[None, :, None]), "grad_x"
    assert np.abs(gw).max() > 0 or B * ch * n < 8


# ---------------------------------------------------------------- the NULL forms
SUBSETS = [s for s in itertools.product((True, False), repeat=3) if any(s) and not all(s)]


@pytest.mark.parametrize("case", [((2, 3, 5), "relu"), ((3, 4, 513), "sigmoid"), ((2, 64, 257), "none"), ((65, 3, 1024), "relu")], ids=_ids)
def test_null_outputs_same_bits_and_untouched(lib, case):
    shape, act = case
    x, w, y, gy, scale, _ = random_case(shape, act)
    full = run(lib, x, w, scale, y, gy, act)
    for need in SUBSETS:
        # x may be NULL when grad_w is, w when grad_x is: passed as NULL exactly then
        part = run(lib, x, w, scale, y, gy, act, need=need, pass_x=need[1], pass_w=need[0])
        for got, want, n, name in zip(part, full, need, SIDES):
            assert (got is None) == (not n)
            if n:
                _same_bits(got, want, f"{name} with need={need}")
    if act == "none":                                             # y may be NULL when act is none: the same bits
        for got, want, name in zip(run(lib, x, w, scale, torch.zeros_like(gy), gy, act, pass_y=False), full, SIDES):
            _same_bits(got, want, f"{name}, y = NULL")


# ---------------------------------------------------------------- invariances
INV = [((2, 3, 5), "sigmoid"), ((2, 64, 257), "relu"), ((3, 17, 1023), "none"), ((3, 4, 513), "sigmoid"), ((33, 2, 64), "relu"),
       ((2, 6, 1025), "sigmoid")]


@pytest.mark.parametrize("case", INV, ids=_ids)
def test_runs_addresses_and_scratch_contents_do_not_matter(lib, case):
    shape, act = case
    x, w, y, gy, scale, _ = random_case(shape, act)
    base = run(lib, x, w, scale, y, gy, act)
    g = torch.Generator().manual_seed(1)
    variants = {"second run": lambda: run(lib, x, w, scale, y, gy, act), "zero-filled scratch": lambda: run(lib, x, w, scale, y, gy, act, fill="zero")}
    for name, fn in variants.items():
        for got, want, side in zip(fn(), base, SIDES):
            _same_bits(got, want, f"{side}, {name}")
    # random scratch contents: a plain call on a scratch tensor filled with random bits
    B, ch, S = shape
    need = lib.s3r_head_backward_scratch_elems(B, ch, S)
    scr = torch.randn(need, generator=g).to(DEV)
    xd, wd, gyd = x.to(DEV), w.to(DEV), gy.to(DEV)
    yd = None if y is None else y.to(DEV)
    sd = None if scale is None else torch.tensor([scale], device=DEV)
    gxd, gwd, gbd = torch.empty(B, ch, S, device=DEV), torch.empty(ch, device=DEV), torch.empty(1, device=DEV)
    _rc(lib, lib.s3r_head_backward(xd.data_ptr(), wd.data_ptr(), None if sd is None else sd.data_ptr(), None if yd is None else yd.data_ptr(),
                                   gyd.data_ptr(), gxd.data_ptr(), gwd.data_ptr(), gbd.data_ptr(), B, ch, S, ACT[act], scr.data_ptr(), need, None),
        "head backward")
    torch.cuda.synchronize()
    for got, want, side in zip((gxd, gwd, gbd), base, SIDES):
        _same_bits(got.cpu().numpy(), want, f"{side}, random scratch")
    order = ["x", "w", "scale", "y", "grad_y", "grad_x", "grad_w", "grad_shift", "scratch"]
    for label, sk in (("every argument + 1 element", lambda name, dtype, role: 1),
                      ("arguments at 1, 2, 3, ... elements", lambda name, dtype, role: 1 + order.index(name) % 3)):
        with G.skews(sk):
            got = run(lib, x, w, scale, y, gy, act)
        for a, b, side in zip(got, base, SIDES):
            _same_bits(a, b, f"{side}, {label}")


def test_a_sample_has_the_same_partial_in_every_batch(lib):
    """the per-sample partial is a function of S only: with B = 1 the outputs ARE the partials, and the batch's outputs are their
    ascending-b sum"""
    shape, act = (3, 4, 513), "sigmoid"
    x, w, y, gy, scale, _ = random_case(shape, act)
    _, gw, gb = run(lib, x, w, scale, y, gy, act)
    pw, pb = [], []
    for b in range(3):
        _, w1, b1 = run(lib, x[b:b + 1], w, scale, y[b:b + 1], gy[b:b + 1], act)
        pw.append(w1)
        pb.append(b1)
    _same_bits(gw, R.reduce_rows(np.stack(pw)), "grad_w = ((P0 + P1) + P2)")
    _same_bits(gb, R.reduce_rows(np.stack(pb)), "grad_shift = ((P0 + P1) + P2)")


# ---------------------------------------------------------------- the Python surface and autograd
def test_autograd_function_and_needs_input_grad(s3r, lib, monkeypatch):
    B, ch, n = 2, 6, 4
    g = torch.Generator().manual_seed(3)
    x0, w0, b0 = torch.randn(B, ch, n, n, n, generator=g).to(DEV), torch.randn(1, ch, 1, 1, 1, generator=g).to(DEV), torch.randn(1, generator=g).to(DEV)
    gy = torch.randn(B, n, n, n, generator=g).to(DEV)
    seen = []
    real = lib.s3r_head_backward

    def spy(*a):
        seen.append(tuple(p is not None for p in a[5:8]))
        return real(*a)

    monkeypatch.setattr(lib, "s3r_head_backward", spy)
    for act in R.ACTS:
        y_plain = s3r.head(x0, w0, b0, act)
        assert y_plain.shape == (B, n, n, n) and y_plain.grad_fn is None
        assert s3r.head(x0.clone().requires_grad_(), w0.clone().requires_grad_(), b0, act).grad_fn is None      # records no graph
        dx, dw, db = s3r.head_backward(x0, w0, y_plain, gy, act)
        assert dx.shape == x0.shape and dw.shape == (ch,) and db.shape == (1,)
        for need in itertools.product((True, False), repeat=3):
            seen.clear()
            x, w, b = (t.clone().requires_grad_(r) for t, r in zip((x0, w0, b0), need))
            y = s3r.differentiable_head(x, w, b, act)
            assert torch.equal(y.detach().view(torch.int32), y_plain.view(torch.int32))
            if not any(need):
                assert not y.requires_grad
                continue
            y.backward(gy)
            assert seen == [need]                                 # exactly the sides needs_input_grad asks for
            for t, r, want in zip((x, w, b), need, (dx, dw.view(w0.shape), db)):
                assert (t.grad is not None) == r
                if r:
                    assert t.grad.shape == t.shape and torch.equal(t.grad.view(torch.int32), want.view(torch.int32))
    with pytest.raises(RuntimeError, match="needs the layer's output"):
        s3r.head_backward(x0, w0, None, gy, "relu")
    gx, gw, gb = s3r.head_backward(x0, w0, None, gy, "none", need_x=False, need_b=False)
    assert gx is None and gb is None and gw.shape == (ch,)
    # B = 0: zeros without a call
    seen.clear()
    x, w, b = torch.empty(0, ch, n, n, n, device=DEV, requires_grad=True), w0.clone().requires_grad_(), b0.clone().requires_grad_()
    y = s3r.differentiable_head(x, w, b, "sigmoid")
    assert y.shape == (0, n, n, n)
    y.sum().backward()
    assert seen == [] and x.grad.shape == x.shape and not w.grad.any() and not b.grad.any()


@functools.lru_cache(maxsize=None)
def _decoder_state():
    import s3r
    return s3r.seeded_state_dict(s3r.Decoder(), seed=4)


def _decoder(s3r):
    dec = s3r.Decoder()
    dec.load_state_dict(_decoder_state())
    return dec.to(DEV)


def _volume(B, seed):
    return 0.5 * torch.randn(B, 64, 28, 28, 28, generator=torch.Generator().manual_seed(seed))


@functools.lru_cache(maxsize=None)
def _features(B, seed):
    """d3's output for a seeded volume, computed once and shared (left unchanged by the tests)"""
    import s3r
    feats = _decoder(s3r).features(_volume(B, seed).to(DEV))
    torch.cuda.synchronize()
    return feats


def test_standalone_head_is_conv_forward_on_the_head_layer(s3r, lib):
    """the value of differentiable_head, bit for bit against a direct s3r_conv_forward call on d4's descriptor"""
    dec = _decoder(s3r)
    feats = _features(2, 1)
    assert feats.shape == (2, 64, 32, 32, 32) and feats.dtype == F32 and feats.grad_fn is None
    got = dec.differentiable_head(feats)
    assert got.shape == (2, 32, 32, 32) and got.grad_fn is not None
    layer = s3r.arch_spec.DECODER[-1]
    desc = s3r._lib.make_desc(layer, 2, 32)
    n = C.c_int64(0)
    _rc(lib, lib.s3r_conv_packed_elems(C.byref(desc), C.byref(n)), "packed_elems")
    pw, want = torch.empty(n.value, device=DEV), torch.empty(2, 1, 32, 32, 32, device=DEV)
    w, bias = dec.d4.conv.weight.detach().contiguous(), dec.d4.conv.bias.detach().contiguous()
    _rc(lib, lib.s3r_conv_pack_weights(C.byref(desc), w.data_ptr(), pw.data_ptr(), None), "pack")
    _rc(lib, lib.s3r_conv_forward(C.byref(desc), feats.data_ptr(), pw.data_ptr(), None, bias.data_ptr(), want.data_ptr(), None, 0, None), "conv forward")
    torch.cuda.synchronize()
    assert torch.equal(got.detach().view(torch.int32), want.squeeze(1).view(torch.int32))
    with pytest.raises(RuntimeError):
        dec.train()                                               # still the inference module


def test_standalone_head_agrees_with_the_fused_forward(s3r):
    """Stereo2Voxel.head_features + Decoder.differentiable_head against Stereo2Voxel.forward (d4 fused into d3's finish kernel), per voxel
    within tests/_head64.py's forward_bound: twice the any-order bound of the 65-term pre-activation through a slope of at most 1/4, plus
    the two sigmoid evaluations.  Measured on an MI355X: see the printed line (bit-identical or not is NOT relied upon)."""
    model = s3r.Stereo2Voxel()
    s3r.seed_module(model, seed=0)
    model.to(DEV)
    left, right = s3r.synthetic_pairs(1, seed=0, device=DEV)
    feats = model.head_features(left, right)
    assert feats.shape == (1, 64, 32, 32, 32) and feats.dtype == F32 and feats.grad_fn is None and not feats.requires_grad
    head = model.decoder.differentiable_head(feats).detach()
    fused = model(left, right)
    assert head.shape == fused.shape == (1, 32, 32, 32)
    w, bias = model.decoder.d4.conv.weight.detach().cpu().numpy().reshape(-1), model.decoder.d4.conv.bias.item()
    y64, z, mag = R.forward64(feats.cpu().numpy(), w, bias, "sigmoid")
    lim = R.forward_bound(z, mag, y64)
    err = np.abs(head.cpu().numpy().astype(np.float64) - fused.cpu().numpy().astype(np.float64))
    same = torch.equal(head.view(torch.int32), fused.view(torch.int32))
    print(f"standalone head vs fused forward: max |d| {err.max():.3e}, max err / bound {(err / lim).max():.4f}, bit-identical: {same}")
    assert (err <= lim).all()
    # ... and each is within its own half of that bound of float64
    assert (np.abs(head.cpu().numpy() - y64) <= lim).all() and (np.abs(fused.cpu().numpy() - y64) <= lim).all()


def _gt(B, seed):
    return (torch.rand(B, 32, 32, 32, generator=torch.Generator().manual_seed(seed)) < 0.3).float()


def test_head_gradients_under_the_bce_loss_against_float64_autograd(s3r):
    """d4.weight.grad and d4.bias.grad of VoxelBCELoss(Decoder.differentiable_head(features), gt) on B = 2 against torch autograd in
    float64 of the same graph (conv3d 1x1x1 + sigmoid + BCELoss) on the same features.  The bound, per gradient element: with y the fp32
    head output and y64 the real one, |y - y64| <= E_y = bound32(65, mag) / 4 + (2 |z| + 6) u y64 (tests/_head64.py, one side); the device's
    g = grad_y y (1 - y) with grad_y = (y - t) / (N y (1 - y)) is (y - t) / N through eight roundings, so
    |g - g64| <= E_g = (E_y + gamma_8 (|y64 - t| + E_y)) / N; then the sum over K = B S terms in any order:
      |grad_w[c] - ref| <= sum |x_c| E_g + bound32(K, sum |x_c| (|g64| + E_g));   grad_bias the same with x = 1.
    Premise: no voxel has y (1 - y) below the 1e-12 epsilon."""
    B = 2
    dec = _decoder(s3r)
    feats, gt = _features(B, 1), _gt(B, 2)
    for p in dec.parameters():
        p.grad = None
    loss = s3r.VoxelBCELoss()(dec.differentiable_head(feats), gt.to(DEV))
    loss.backward()
    params = dict(dec.named_parameters())
    assert [n for n, p in params.items() if p.grad is not None] == ["d4.conv.weight", "d4.conv.bias"]
    gw, gb = params["d4.conv.weight"].grad, params["d4.conv.bias"].grad
    assert gw.shape == (1, 64, 1, 1, 1) and gb.shape == (1,)
    x64 = feats.cpu().double()
    wd, bd = params["d4.conv.weight"].detach().cpu().double().requires_grad_(), params["d4.conv.bias"].detach().cpu().double().requires_grad_()
    y = torch.sigmoid(torch.nn.functional.conv3d(x64, wd, bd)).squeeze(1)
    ref = torch.nn.BCELoss()(y, gt.double())
    ref_w, ref_b = torch.autograd.grad(ref, (wd, bd))
    N = y.numel()
    y64, z, mag = R.forward64(feats.cpu().numpy(), wd.detach().numpy().reshape(-1), bd.item(), "sigmoid")
    assert (y64 * (1 - y64)).min() > 1e-11
    e_y = R.bound32(65, mag) / 4 + (2 * np.abs(z) + 6) * R.U32 * y64
    g64 = (y64 - gt.double().numpy()) / N
    e_g = (e_y + R.gamma(8) * (np.abs(y64 - gt.double().numpy()) + e_y)) / N
    ax = np.abs(x64.numpy())
    K = N
    lim_w = np.einsum("bcdhw,bdhw->c", ax, e_g) + R.bound32(K, np.einsum("bcdhw,bdhw->c", ax, np.abs(g64) + e_g))
    lim_b = e_g.sum() + R.bound32(K, (np.abs(g64) + e_g).sum())
    err_w = np.abs(gw.cpu().double().numpy().reshape(-1) - ref_w.numpy().reshape(-1))
    err_b = abs(gb.item() - ref_b.item())
    print(f"loss {loss.item():.7g} vs float64 {ref.item():.7g}; d4.weight.grad max err / bound {(err_w / lim_w).max():.3e}, "
          f"d4.bias.grad err / bound {err_b / lim_b:.3e}; |grad_w| max {ref_w.abs().max().item():.3e}, bound max {lim_w.max():.3e}")
    assert (err_w <= lim_w).all() and err_b <= lim_b
    # The bound is a worst case over the signs of 65536 terms (on an MI355X the error is 2e-5 of it).  For the comparison to see a mistake
    # at all it has to stay well below the gradient: at most 5 % of the largest element, so that a dropped sample, a missing sigmoid
    # derivative, a missing 1 / N or a wrong sign (all >= 50 %) cannot hide in it.  Both sides are float64 reference quantities, not
    # outputs of the kernels under test (measured: 1.3e-3 against 9.9e-2).  Finer mistakes — a dropped chunk is 1 / 128 of the sum — are
    # the business of the bit-for-bit tests above.
    assert lim_w.max() <= 5e-2 * ref_w.abs().max().item() and lim_b <= 5e-2 * abs(ref_b.item())
    assert ref_w.abs().max() > 0 and ref_b.abs().item() > 0


def test_fine_tune_loop_is_deterministic_and_descends(s3r):
    """three SGD steps on d4 under the BCE loss, twice from the same state.  The problem is convex in d4's 65 parameters and its
    gradient is Lipschitz with constant at most mean(|x|^2 + 1) / 4 (the sigmoid-BCE Hessian is at most x x^T / 4 per voxel), so a step
    of the inverse of that bound cannot increase the loss."""
    B = 2
    feats, gt = _features(B, 1), _gt(B, 3).to(DEV)
    lr = 4.0 / float((feats.cpu().double() ** 2).sum(1).mean() + 1.0)
    volume = _volume(1, 5).to(DEV)

    def three_steps():
        dec = _decoder(s3r)
        before = dec(volume)
        head = [dec.d4.conv.weight, dec.d4.conv.bias]
        opt = torch.optim.SGD(head, lr=lr)
        bce = s3r.VoxelBCELoss()
        losses = []
        for _ in range(3):
            opt.zero_grad()
            loss = bce(dec.differentiable_head(feats), gt)
            loss.backward()
            opt.step()
            losses.append(loss.item())
        with torch.no_grad():
            losses.append(bce(dec.differentiable_head(feats), gt).item())
        after = dec(volume)
        assert not torch.equal(after, before), "Decoder.forward still runs the packed weights from before the steps"
        return {n: p.detach().clone() for n, p in dec.named_parameters()}, losses

    a, la = three_steps()
    b, lb = three_steps()
    print(f"lr {lr:.4g}, losses {la}")
    assert la == lb and all(np.isfinite(la))
    assert la[3] < la[0]                                          # the loss after step 3 is below the loss before step 1
    state = _decoder_state()
    for n in a:
        assert torch.equal(a[n].view(torch.int32), b[n].view(torch.int32)), n
        moved = not torch.equal(a[n].cpu(), state[n])
        assert moved == n.startswith("d4.conv."), f"{n}: moved = {moved}"


def test_profiler_record(s3r, lib):
    B, ch, n = 2, 6, 8
    S = n ** 3
    x, w, y, gy = (torch.rand(s, device=DEV) for s in ((B, ch, n, n, n), (ch,), (B, n, n, n), (B, n, n, n)))
    s3r.profile_enable(16)
    try:
        s3r.head_backward(x, w, y, gy, "sigmoid")
        s3r.head_backward(x, w, None, gy, "none", need_x=False)
        s3r.head_backward(x, w, None, gy, "none", need_w=False, need_b=False)
        torch.cuda.synchronize()
        rec = s3r.profile_read(16)
    finally:
        s3r.profile_enable(0)
    assert [(r["family"], r["tag"], r["launches"]) for r in rec] == [("head", 1, 2), ("head", 1, 2), ("head", 1, 1)]
    assert all(r["ms"] > 0 for r in rec)
    assert rec[0]["flops"] == 3.0 * B * ch * S and rec[0]["bytes"] == 4.0 * (2 * B * S + 2 * (B * ch * S + ch) + 1)
    assert rec[1]["flops"] == 2.0 * B * ch * S and rec[1]["bytes"] == 4.0 * (B * S + B * ch * S + ch + 1)
    assert rec[2]["flops"] == 1.0 * B * ch * S and rec[2]["bytes"] == 4.0 * (B * S + B * ch * S + ch)
