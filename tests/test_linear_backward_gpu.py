"""s3r_linear_backward on the device, through the C-ABI unless stated: grad_bias bit for bit against the defined sequential order,
grad_w and grad_x against float64 within the derived any-order bound of tests/_linear64.py (bound32), exact equality on integer
lattices, B = 1 (where grad_bias exposes g itself), the NULL forms, run / address / scratch-content invariance in guarded buffers,
the autograd surface, the point head's six gradients against torch autograd in float64, a three-step fine-tune loop run twice, and
the profiler record.

There is no measured tolerance in this file.  Results are compared bit for bit, or per element against bound32(K, sum|term|), or —
the chain test — against a yardstick evaluated in the same test (torch's own fp32 evaluation of the same graph)."""
import functools
import itertools

import numpy as np
import pytest
import torch

from tests import _guard as G
from tests import _linear64 as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ACT = {"none": 0, "relu": 1, "sigmoid": 2}

# (B, Cin, Cout): the smallest at which each path can break — a single element, one exact tile, odd sizes below a tile, rows that are
# only 4-byte aligned, whole tiles, a batch across a 32-row tile, a K (Cout) that is no multiple of the staged chunk, split-K grad_x, and
# the point head's own p2, p3, p1
SHAPES = [(1, 1, 1), (1, 32, 32), (3, 33, 31), (2, 40, 100), (32, 128, 128), (33, 96, 160), (5, 1024, 96), (4, 64, 4096),
          (32, 1024, 1024), (2, 1024, 6144), (2, 32768, 1024)]
BIG = {(2, 1024, 6144), (2, 32768, 1024)}
CASES = [(s, a) for s in SHAPES for a in R.ACTS if not (s in BIG and a == "sigmoid")]
_ids = lambda c: "x".join(map(str, c[0])) + "-" + c[1]


@pytest.fixture(scope="module")
def lib(s3r):
    return s3r.load_library()


def _rc(lib, rc, what):
    assert rc == 0, f"{what}: {lib.s3r_last_error().decode()} ({rc})"


def _same_bits(got, want, what):
    gb, wb = R.bits(got), R.bits(want)
    bad = np.argwhere(gb != wb)
    assert bad.size == 0, f"{what}: {len(bad)} elements differ, first at {tuple(bad[0])}: got {got[tuple(bad[0])]!r} want {want[tuple(bad[0])]!r}"


def run(lib, x, w, y, gy, act, need=(True, True, True), fill="nan", pass_y=True):
    """One guarded call.  x, w, y, gy: CPU fp32 tensors (y may be None).  Returns (grad_x, grad_w, grad_bias) as numpy, None for a side
    not asked for.  EVERY output buffer is allocated, poisoned and guarded; a side that is not asked for is passed as NULL and its buffer
    must still hold nothing but poison afterwards.  Skews come from an enclosing `with G.skews(...)`."""
    B, cin, cout = x.shape[0], x.shape[1], w.shape[0]
    need_elems = lib.s3r_linear_backward_scratch_elems(B, cin, cout)
    assert need_elems > 0
    ins = [G.Guarded("x", (B, cin), torch.float32, DEV, "in", data=x), G.Guarded("w", (cout, cin), torch.float32, DEV, "in", data=w),
           G.Guarded("grad_y", (B, cout), torch.float32, DEV, "in", data=gy)]
    yb = G.Guarded("y", (B, cout), torch.float32, DEV, "in", data=y) if y is not None else None
    outs = [G.Guarded("grad_x", (B, cin), torch.float32, DEV, "out"), G.Guarded("grad_w", (cout, cin), torch.float32, DEV, "out"),
            G.Guarded("grad_bias", (cout,), torch.float32, DEV, "out")]
    scr = G.Guarded("scratch", (need_elems,), torch.float32, DEV, "scratch", fill=fill)
    ptrs = [o.ptr if n else None for o, n in zip(outs, need)]
    _rc(lib, lib.s3r_linear_backward(ins[0].ptr, ins[1].ptr, yb.ptr if (yb is not None and pass_y) else None, ins[2].ptr, *ptrs, B, cin,
                                     cout, ACT[act], scr.ptr, need_elems, None), "linear backward")
    torch.cuda.synchronize()
    G.check_all(*ins, *([yb] if yb is not None else []))
    res = []
    poison = G._BITS[torch.float32][2]
    for o, n in zip(outs, need):
        if n:
            G.check_all(o)
            res.append(o.t.cpu().numpy())
        else:
            o.role = "scratch"                                     # nothing may have been written: guards intact (check() looks at
            G.check_all(o)                                         # the guards alone for this role), every element still poison
            assert bool((G._as_bits(o.t) == poison).all()), f"{o.name} was not asked for but was written"
            res.append(None)
    where = scr.check()
    assert where is None, where
    if not (need[0] or need[1]) and fill == "nan":                # grad_bias alone: no GEMM reads g, so nothing is written to scratch
        assert bool((G._as_bits(scr.t) == G._BITS[torch.float32][4]).all()), "scratch was written although only grad_bias was asked for"
    return tuple(res)


def B_times(shape):
    return shape[0] * shape[1] * shape[2]


@functools.lru_cache(maxsize=None)
def random_case(shape, act):
    """(x, w, y, gy) CPU tensors and the references, computed once per (shape, act) and shared: g (fp32 rule), grad_bias (fp32 order),
    ((grad_w, K, mag), (grad_x, K, mag)) in float64"""
    B, cin, cout = shape
    g = torch.Generator().manual_seed(B * 7919 + cin * 31 + cout)
    x = torch.randn(B, cin, generator=g)
    w = torch.randn(cout, cin, generator=g) / cin ** 0.5
    gy = torch.randn(B, cout, generator=g)
    # y is an INPUT of the backward: any tensor of the activation's range exercises the rule (half the ReLU outputs are 0)
    y = None if act == "none" else torch.relu(torch.randn(B, cout, generator=g)) if act == "relu" else torch.rand(B, cout, generator=g)
    gg = R.g32(None if y is None else y.numpy(), gy.numpy(), act)
    return x, w, y, gy, gg, R.grad_bias32(gg), R.backward64(x.numpy(), w.numpy(), gg)


@pytest.mark.parametrize("case", CASES, ids=_ids)
def test_random_data_against_float64(lib, case):
    shape, act = case
    x, w, y, gy, gg, gb_ref, ((gw_ref, kw, mw), (gx_ref, kx, mx)) = random_case(shape, act)
    gx, gw, gb = run(lib, x, w, y, gy, act)
    _same_bits(gb, gb_ref, "grad_bias")
    for got, ref, k, mag, name in ((gw, gw_ref, kw, mw, "grad_w"), (gx, gx_ref, kx, mx, "grad_x")):
        err = np.abs(got.astype(np.float64) - ref)
        lim = R.bound32(k, mag)
        print(f"{shape} {act} {name}: K {k}, max err {err.max():.3e}, max err / bound {(err / lim).max():.4f}")
        assert (err <= lim).all(), f"{name}: {(err > lim).sum()} elements beyond the bound, worst ratio {(err / lim).max():.3f}"
        assert np.abs(got).max() > 0 or B_times(shape) < 32      # (a single ReLU output may well be 0)


# ---------------------------------------------------------------- integer lattices: every partial sum is an integer < 2^24 in any order
def device_forward(lib, x, w, bias, act):
    B, cin, cout = x.shape[0], x.shape[1], w.shape[0]
    xd, wd, bd = x.to(DEV), w.to(DEV), bias.to(DEV)
    y = torch.empty(B, cout, device=DEV)
    need = lib.s3r_linear_scratch_elems(B, cin, cout)
    scr = torch.empty(max(need, 1), device=DEV)
    _rc(lib, lib.s3r_linear_forward(xd.data_ptr(), wd.data_ptr(), bd.data_ptr(), y.data_ptr(), B, cin, cout, ACT[act], scr.data_ptr(),
                                    scr.numel(), None), "linear forward")
    torch.cuda.synchronize()
    return y.cpu()


def _lattice(shape, seed):
    B, cin, cout = shape
    g = torch.Generator().manual_seed(seed)
    x = torch.randint(-4, 5, (B, cin), generator=g).float()
    w = torch.randint(-2, 3, (cout, cin), generator=g).float()
    bias = torch.randint(-3, 4, (cout,), generator=g).float()
    gy = torch.randint(-4, 5, (B, cout), generator=g).float()
    return x, w, bias, gy


def _exact(lib, x, w, y, gy, act):
    gg = R.g32(None if y is None else y.numpy(), gy.numpy(), act)
    (gw_ref, _, mw), (gx_ref, _, mx) = R.backward64(x.numpy(), w.numpy(), gg)
    assert max(mw.max(), mx.max(), np.abs(gg).sum(0).max()) < 2 ** 24            # the premise: exact in fp32 in any order
    gx, gw, gb = run(lib, x, w, y, gy, act)
    assert np.array_equal(gw.astype(np.float64), gw_ref), "grad_w"
    assert np.array_equal(gx.astype(np.float64), gx_ref), "grad_x"
    assert np.array_equal(gb.astype(np.float64), gg.astype(np.float64).sum(0)), "grad_bias"
    return gx, gw, gb


@pytest.mark.parametrize("act", ["none", "relu"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_integer_lattice_is_exact(lib, shape, act):
    x, w, bias, gy = _lattice(shape, seed=sum(shape))
    y = device_forward(lib, x, w, bias, act)                     # the forward's own y: exact too (|sum| <= 8 Cin + 3 < 2^24)
    assert np.array_equal(y.numpy().astype(np.float64),
                          np.maximum(x.double().numpy() @ w.double().numpy().T + bias.double().numpy(), 0 if act == "relu" else -np.inf))
    gx, gw, _ = _exact(lib, x, w, y if act != "none" else None, gy, act)
    assert (np.abs(gw).max() > 0 and np.abs(gx).max() > 0) or B_times(shape) < 32


@pytest.mark.parametrize("shape", [(3, 33, 31), (33, 96, 160), (4, 64, 4096), (2, 1024, 6144), (32, 1024, 1024)],
                         ids=lambda s: "x".join(map(str, s)))
def test_planted_last_row_last_slice(lib, shape):
    """grad_y is zero except at (last batch row, last output): grad_w's last row then comes from the last batch row alone (the end of its
    K loop) and grad_x's last row from the last o alone (the end of the last K slice); everything else is exactly zero"""
    B, cin, cout = shape
    x, w, _, _ = _lattice(shape, seed=5 + sum(shape))
    x[B - 1] = torch.arange(cin).float() % 7 + 1
    w[cout - 1] = torch.arange(cin).float() % 5 + 1
    gy = torch.zeros(B, cout)
    gy[B - 1, cout - 1] = 3.0
    gx, gw, gb = _exact(lib, x, w, None, gy, "none")
    assert np.array_equal(gw[cout - 1], 3.0 * x[B - 1].numpy()) and not gw[:cout - 1].any()
    assert np.array_equal(gx[B - 1], 3.0 * w[cout - 1].numpy()) and not gx[:B - 1].any()
    assert gb[cout - 1] == 3.0 and not gb[:cout - 1].any()


# ---------------------------------------------------------------- B = 1: grad_bias is g
@pytest.mark.parametrize("act", R.ACTS)
@pytest.mark.parametrize("dims", [(1, 1), (32, 32), (33, 31), (40, 100)], ids=lambda s: "x".join(map(str, s)))
def test_batch_one_exposes_g(lib, dims, act):
    cin, cout = dims
    g = torch.Generator().manual_seed(cin + cout)
    x, w, gy = torch.randn(1, cin, generator=g), torch.randn(cout, cin, generator=g), torch.randn(1, cout, generator=g)
    y = None if act == "none" else torch.randn(1, cout, generator=g) if act == "relu" else torch.rand(1, cout, generator=g)
    if act == "relu":
        special = torch.tensor([0.0, -0.0, float("nan"), float("inf"), -float("inf")])[:cout]
        y[0, :len(special)] = special
    _, gw, gb = run(lib, x, w, y, gy, act)
    gg = R.g32(None if y is None else y.numpy(), gy.numpy(), act)
    _same_bits(gb, gg[0], "grad_bias")
    if act == "relu":
        want = [0, 0, 0, int(R.bits(gy.numpy()[0, 3:4])[0]) if cout > 3 else 0, 0][:cout]
        assert R.bits(gb[:5]).tolist() == want                    # y = 0, -0, NaN, -inf: +0.0; y = +inf: grad_y
    # K = 1: grad_w[o][i] is ONE product, correctly rounded whatever instruction made it, added to an accumulator of +0.0
    with np.errstate(all="ignore"):
        _same_bits(gw, (gg[0][:, None] * x.numpy()[0][None, :]).astype(np.float32) + np.float32(0), "grad_w")


# ---------------------------------------------------------------- the NULL forms
SUBSETS = [s for s in itertools.product((True, False), repeat=3) if any(s) and not all(s)]


@pytest.mark.parametrize("case", [((33, 96, 160), "relu"), ((4, 64, 4096), "none"), ((3, 33, 31), "sigmoid")], ids=_ids)
def test_null_outputs_same_bits_and_untouched(lib, case):
    shape, act = case
    x, w, y, gy = random_case(shape, act)[:4]
    full = run(lib, x, w, y, gy, act)
    for need in SUBSETS:
        part = run(lib, x, w, y, gy, act, need=need)
        for got, want, n, name in zip(part, full, need, ("grad_x", "grad_w", "grad_bias")):
            assert (got is None) == (not n)
            if n:
                _same_bits(got, want, f"{name} with need={need}")
    if act == "none":                                             # y may be NULL when act is none: the same bits
        for got, want in zip(run(lib, x, w, torch.zeros_like(gy), gy, act, pass_y=False), full):
            _same_bits(got, want, "y = NULL")


# ---------------------------------------------------------------- invariances
INV = [((3, 33, 31), "sigmoid"), ((2, 40, 100), "relu"), ((32, 128, 128), "none"), ((33, 96, 160), "relu"), ((4, 64, 4096), "relu"),
       ((5, 1024, 96), "sigmoid")]


@pytest.mark.parametrize("case", INV, ids=_ids)
def test_runs_addresses_and_scratch_contents_do_not_matter(lib, case):
    shape, act = case
    x, w, y, gy = random_case(shape, act)[:4]
    base = run(lib, x, w, y, gy, act)
    variants = {"second run": lambda: run(lib, x, w, y, gy, act), "zero-filled scratch": lambda: run(lib, x, w, y, gy, act, fill="zero")}
    for name, fn in variants.items():
        for got, want, side in zip(fn(), base, ("grad_x", "grad_w", "grad_bias")):
            _same_bits(got, want, f"{side}, {name}")
    order = ["x", "w", "y", "grad_y", "grad_x", "grad_w", "grad_bias", "scratch"]
    for label, sk in (("every argument + 1 element", lambda name, dtype, role: 1),
                      ("arguments at 1, 2, 3, ... elements", lambda name, dtype, role: 1 + order.index(name) % 7)):
        with G.skews(sk):
            got = run(lib, x, w, y, gy, act)
        for a, b, side in zip(got, base, ("grad_x", "grad_w", "grad_bias")):
            _same_bits(a, b, f"{side}, {label}")


# ---------------------------------------------------------------- the Python surface and autograd
def test_autograd_function(s3r, lib):
    B, cin, cout = 5, 96, 70
    g = torch.Generator().manual_seed(3)
    x0, w0, b0 = torch.randn(B, cin, generator=g).to(DEV), (torch.randn(cout, cin, generator=g) / 8).to(DEV), torch.randn(cout, generator=g).to(DEV)
    gy = torch.randn(B, cout, generator=g).to(DEV)
    for act in R.ACTS:
        y_plain = s3r.linear(x0, w0, b0, act)
        assert not y_plain.requires_grad and y_plain.grad_fn is None
        assert s3r.linear(x0.clone().requires_grad_(), w0.clone().requires_grad_(), b0, act).grad_fn is None     # records no graph
        x, w, b = x0.clone().requires_grad_(), w0.clone().requires_grad_(), b0.clone().requires_grad_()
        y = s3r.differentiable_linear(x, w, b, act)
        assert y.grad_fn is not None and torch.equal(y.detach().view(torch.int32), y_plain.view(torch.int32))
        y.backward(gy)
        dx, dw, db = s3r.linear_backward(x0, w0, y_plain, gy, act)
        for got, want in ((x.grad, dx), (w.grad, dw), (b.grad, db)):
            assert torch.equal(got.view(torch.int32), want.view(torch.int32))


def test_needs_input_grad_subsets_reach_the_kernel_as_nulls(s3r, lib, monkeypatch):
    B, cin, cout = 3, 40, 50
    x0, w0, b0, gy = (torch.randn(s, device=DEV) for s in ((B, cin), (cout, cin), (cout,), (B, cout)))
    seen = []
    real = lib.s3r_linear_backward

    def spy(*a):
        seen.append(tuple(p is not None for p in a[4:7]))
        return real(*a)

    monkeypatch.setattr(lib, "s3r_linear_backward", spy)
    for need in itertools.product((True, False), repeat=3):
        seen.clear()
        x, w, b = (t.clone().requires_grad_(n) for t, n in zip((x0, w0, b0), need))
        y = s3r.differentiable_linear(x, w, b, "relu")
        if not any(need):
            assert not y.requires_grad
            continue
        y.backward(gy)
        assert seen == [need]
        for t, n in zip((x, w, b), need):
            assert (t.grad is not None) == n
    # the functional returns None for the sides not asked for
    seen.clear()
    gx, gw, gb = s3r.linear_backward(x0, w0, None, gy, "none", need_x=False, need_b=False)
    assert gx is None and gb is None and gw.shape == (cout, cin) and seen == [(False, True, False)]
    with pytest.raises(RuntimeError, match="needs the layer's output"):
        s3r.linear_backward(x0, w0, None, gy, "relu")
    # B = 0: zeros without a call
    seen.clear()
    x, w, b = torch.empty(0, cin, device=DEV, requires_grad=True), w0.clone().requires_grad_(), b0.clone().requires_grad_()
    y = s3r.differentiable_linear(x, w, b, "relu")
    assert y.shape == (0, cout)
    y.sum().backward()
    assert seen == [] and x.grad.shape == (0, cin) and not w.grad.any() and not b.grad.any()


@functools.lru_cache(maxsize=None)
def _head_state():
    import s3r
    return s3r.seeded_state_dict(s3r.PointHead(), seed=4)


def _head(s3r):
    head = s3r.PointHead()
    head.load_state_dict(_head_state())
    return head.to(DEV)


def _latent(B, seed):
    return torch.relu(torch.randn(B, 512, 4, 4, 4, generator=torch.Generator().manual_seed(seed)))    # a post-ReLU latent, as v6 emits it


def test_point_head_differentiable_has_the_bits_of_forward(s3r):
    head = _head(s3r)
    latent = _latent(2, 1).to(DEV)
    want = head(latent)
    assert want.grad_fn is None and not want.requires_grad        # forward records no graph
    got = head.differentiable(latent)
    assert got.shape == (2, 2048, 3) and got.grad_fn is not None
    assert torch.equal(got.detach().view(torch.int32), want.view(torch.int32))
    with pytest.raises(RuntimeError):
        head.train()                                              # still the inference module: .train() raises


def test_stereo2point_latent_is_the_trunk_of_forward(s3r):
    model = s3r.Stereo2Point()
    s3r.seed_module(model, seed=0)
    model.to(DEV)
    left, right = s3r.synthetic_pairs(1, seed=0, device=DEV)
    latent = model.latent(left, right)
    assert latent.shape == (1, 512, 4, 4, 4) and latent.dtype == torch.float32 and latent.grad_fn is None
    assert torch.equal(model.point_head(latent).view(torch.int32), model(left, right).view(torch.int32))


def test_point_head_gradients_against_float64_autograd(s3r):
    """.grad of the six point-head parameters under the Chamfer loss on B = 2 against torch autograd in float64 of the same graph on the
    CPU (a plain nn.Sequential copy; the Chamfer indices are the device's, so the discrete choice is shared).  The yardstick: per
    parameter, the relative L2 error may be at most 4x that of the SAME torch graph evaluated in float32 on the CPU — two independent
    fp32 evaluations with different summation orders.  Measured on an MI355X (docs/LAB_NOTES.md): HIP 0.92e-6 … 2.2e-6, torch fp32
    3.1e-6 … 6.4e-6, ratios 0.30 … 0.34."""
    B = 2
    head = _head(s3r)
    latent = _latent(B, 2)
    target = torch.rand(B, 2048, 3, generator=torch.Generator().manual_seed(7)) - 0.5
    pts = head.differentiable(latent.to(DEV))
    loss = s3r.ChamferDistance()(pts, target.to(DEV))
    loss.backward()
    _, _, i1, i2 = s3r.chamfer_distance(pts.detach(), target.to(DEV))
    i1, i2 = i1.cpu().long(), i2.cpu().long()
    names = ["p1.conv.weight", "p1.conv.bias", "p2.conv.weight", "p2.conv.bias", "p3.conv.weight", "p3.conv.bias"]
    got = {n: dict(head.named_parameters())[n].grad.cpu() for n in names}

    def torch_grads(dtype):
        sd = {k: v.to(dtype) for k, v in _head_state().items()}
        seq = torch.nn.Sequential(torch.nn.Linear(32768, 1024), torch.nn.ReLU(), torch.nn.Linear(1024, 1024), torch.nn.ReLU(),
                                  torch.nn.Linear(1024, 6144)).to(dtype)
        seq.load_state_dict({f"{2 * i}.{leaf}": sd[f"p{i + 1}.conv.{leaf}"] for i in range(3) for leaf in ("weight", "bias")})
        p = seq(latent.to(dtype).view(B, -1)).view(B, 2048, 3)
        t = target.to(dtype)
        d1 = ((p - torch.gather(t, 1, i1[..., None].expand(-1, -1, 3))) ** 2).sum(-1)
        d2 = ((t - torch.gather(p, 1, i2[..., None].expand(-1, -1, 3))) ** 2).sum(-1)
        (d1.mean() + d2.mean()).backward()
        return {f"p{i + 1}.conv.{leaf}": getattr(seq[2 * i], leaf).grad for i in range(3) for leaf in ("weight", "bias")}, p.detach()

    ref, p64 = torch_grads(torch.float64)
    f32, _ = torch_grads(torch.float32)
    assert (pts.detach().cpu().double() - p64).norm() <= 1e-4 * p64.norm()      # (the same network: a sanity check, not the test)
    bad = []
    for n in names:
        r = ref[n]
        hip = ((got[n].double() - r).norm() / r.norm()).item()
        yard = ((f32[n].double() - r).norm() / r.norm()).item()
        print(f"{n}: HIP rel L2 error {hip:.3e}, torch fp32 rel L2 error {yard:.3e}, ratio {hip / yard:.3f} (allowed 4)")
        assert r.norm() > 0 and yard > 0
        if not hip <= 4 * yard:
            bad.append(n)
    assert not bad, bad


def test_fine_tune_loop_is_deterministic_and_invalidates_the_cache(s3r):
    B = 2
    latent = _latent(B, 3).to(DEV)
    target = (torch.rand(B, 2048, 3, generator=torch.Generator().manual_seed(8)) - 0.5).to(DEV)

    def three_steps():
        head = _head(s3r)
        before = head(latent)
        opt = torch.optim.SGD(head.parameters(), lr=0.05)
        chamfer = s3r.ChamferDistance()
        losses = []
        for _ in range(3):
            opt.zero_grad()
            loss = chamfer(head.differentiable(latent), target)
            loss.backward()
            opt.step()
            losses.append(loss.item())
            after = head(latent)
            assert not torch.equal(after, before), "PointHead.forward still runs the packed weights from before the step"
            assert torch.equal(after.view(torch.int32), head.differentiable(latent).detach().view(torch.int32))
            before = after
        return {n: p.detach().clone() for n, p in head.named_parameters()}, losses

    a, la = three_steps()
    b, lb = three_steps()
    assert len(a) == 6 and la == lb and all(np.isfinite(la))
    for n in a:
        assert torch.equal(a[n].view(torch.int32), b[n].view(torch.int32)), n
        assert not torch.equal(a[n].cpu(), _head_state()[n]), f"{n} did not move"


def test_profiler_record(s3r, lib):
    B, cin, cout = 3, 40, 50
    x, w, y, gy = (torch.rand(s, device=DEV) for s in ((B, cin), (cout, cin), (B, cout), (B, cout)))
    s3r.profile_enable(16)
    try:
        s3r.linear_backward(x, w, y, gy, "relu")
        torch.cuda.synchronize()
        full = s3r.profile_read(16)
        s3r.profile_reset()
        s3r.linear_backward(x, w, None, gy, "none", need_x=False)
        torch.cuda.synchronize()
        part = s3r.profile_read(16)
        s3r.profile_reset()
        s3r.linear_backward(x, w, None, gy, "none", need_x=False, need_w=False)
        torch.cuda.synchronize()
        bias = s3r.profile_read(16)
    finally:
        s3r.profile_enable(0)
    assert len(full) == 1 and full[0]["family"] == "linear" and full[0]["tag"] == 1 and full[0]["ms"] > 0
    assert full[0]["flops"] == 2 * 2.0 * B * cin * cout
    assert full[0]["bytes"] == 4.0 * (2 * B * cout + (B * cin + cin * cout) + (cin * cout + B * cin) + cout)
    assert len(part) == 1 and part[0]["tag"] == 1 and part[0]["flops"] == 2.0 * B * cin * cout
    assert part[0]["bytes"] == 4.0 * (B * cout + B * cin + cin * cout + cout)
    assert len(bias) == 1 and bias[0]["flops"] == 0 and bias[0]["bytes"] == 4.0 * (B * cout + cout) and bias[0]["launches"] == 1
