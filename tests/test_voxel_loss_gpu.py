"""s3r_voxel_bce_forward / s3r_voxel_bce_backward on the device, through the C-ABI in guarded, poisoned buffers unless stated.

What is compared with what (tests/_bce64.py has the restatements and the derivations):
  grad_pred   bit for bit against the fp32 restatement (elementwise, every operation rounded once), random data and the planted grid
  loss_elem   per element against float64 within elem_bound (1 - p rounded once, each logf within L = 3 ulp — the OpenCL full-profile
              limit OCML's logf is specified to; no HIP math accuracy table ships with the ROCm install, see _bce64.py —, two products,
              one add, a negation); exact values at the clamps
  loss_sum    bit for bit against the header's order applied to the DEVICE's own loss_elem (the order, separately from logf), and
              within the any-order bound of the float64 sum
There is no measured tolerance in this file."""
import functools

import numpy as np
import pytest
import torch

from tests import _bce64 as R
from tests import _guard as G

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32 = torch.float32
POISON = G._BITS[F32][2]


@pytest.fixture(scope="module")
def lib(s3r):
    return s3r.load_library()


def _rc(lib, rc, what):
    assert rc == 0, f"{what}: {lib.s3r_last_error().decode()} ({rc})"


def _same_bits(got, want, what):
    gb, wb = R.bits(got), R.bits(want)
    bad = np.argwhere(gb != wb)
    assert bad.size == 0, f"{what}: {len(bad)} elements differ, first at {tuple(bad[0])}: got {got[tuple(bad[0])]!r} want {want[tuple(bad[0])]!r}"


def _untouched(buf):
    buf.role = "scratch"                                           # guards alone, then: every element still poison
    G.check_all(buf)
    assert bool((G._as_bits(buf.t) == POISON).all()), f"{buf.name} was not asked for but was written"


def forward(lib, p, t, want_sum=True, want_elem=True):
    """one guarded call; p, t (B, V) numpy fp32.  Both outputs are allocated, poisoned and guarded; one that is not asked for is passed as
    NULL and must still hold nothing but poison.  Returns (loss_sum, loss_elem), None for the one not asked for."""
    B, V = p.shape
    ins = [G.Guarded("pred", (B, V), F32, DEV, "in", data=torch.from_numpy(p)), G.Guarded("target", (B, V), F32, DEV, "in", data=torch.from_numpy(t))]
    s, e = G.Guarded("loss_sum", (B,), F32, DEV, "out"), G.Guarded("loss_elem", (B, V), F32, DEV, "out")
    _rc(lib, lib.s3r_voxel_bce_forward(ins[0].ptr, ins[1].ptr, s.ptr if want_sum else None, e.ptr if want_elem else None, B, V, None),
        "voxel bce forward")
    torch.cuda.synchronize()
    G.check_all(*ins)
    out = []
    for buf, want in ((s, want_sum), (e, want_elem)):
        if want:
            G.check_all(buf)                                       # (a NaN the kernel computes is not the poison's bit pattern)
            out.append(buf.t.cpu().numpy())
        else:
            _untouched(buf)
            out.append(None)
    return tuple(out)


def backward(lib, p, t, scale):
    B, V = p.shape
    ins = [G.Guarded("pred", (B, V), F32, DEV, "in", data=torch.from_numpy(p)), G.Guarded("target", (B, V), F32, DEV, "in", data=torch.from_numpy(t)),
           G.Guarded("grad_scale", (B,), F32, DEV, "in", data=torch.from_numpy(np.asarray(scale, np.float32)))]
    g = G.Guarded("grad_pred", (B, V), F32, DEV, "out")
    _rc(lib, lib.s3r_voxel_bce_backward(ins[0].ptr, ins[1].ptr, ins[2].ptr, g.ptr, B, V, None), "voxel bce backward")
    torch.cuda.synchronize()
    G.check_all(*ins, g)
    return g.t.cpu().numpy()


@functools.lru_cache(maxsize=None)
def random_case(shape):
    """(p, t, scale) and the float64 references, computed once per shape and shared"""
    B, V = shape
    g = torch.Generator().manual_seed(B * 7919 + V)
    p = torch.rand(B, V, generator=g).numpy()
    t = (torch.rand(B, V, generator=g) < 0.3).float().numpy()
    t[:, ::3] = torch.rand(B, len(range(0, V, 3)), generator=g).numpy()         # soft targets among the hard ones
    scale = (torch.randn(B, generator=g) / V).numpy()
    return p, t, scale, R.loss_elem64(p, t), R.elem_bound(p, t)


_ids = lambda s: "x".join(map(str, s))


@pytest.mark.parametrize("shape", R.SHAPES, ids=_ids)
def test_forward_on_random_data(lib, shape):
    p, t, _, l64, lim = random_case(shape)
    s, e = forward(lib, p, t)
    err = np.abs(e.astype(np.float64) - l64)
    print(f"{shape}: loss_elem max err / bound {(err / lim).max():.4f}")
    assert (err <= lim).all(), f"{(err > lim).sum()} elements beyond the bound, worst ratio {(err / lim).max():.3f}"
    for b in range(shape[0]):
        assert R.bits(s[b:b + 1])[0] == R.bits(R.sum_order32(e[b]))[()], f"sample {b}: loss_sum is not the header's order of loss_elem"
        # against float64: the elements' own bounds, then any order of V - 1 additions
        assert abs(float(s[b]) - l64[b].sum()) <= lim[b].sum() + R.sum_bound(e[b])
    s_only, none = forward(lib, p, t, want_elem=False)
    assert none is None
    _same_bits(s_only, s, "loss_sum with loss_elem NULL")
    none, e_only = forward(lib, p, t, want_sum=False)
    assert none is None
    _same_bits(e_only, e, "loss_elem with loss_sum NULL")


@pytest.mark.parametrize("shape", R.SHAPES, ids=_ids)
def test_backward_on_random_data_bit_for_bit(lib, shape):
    p, t, scale, _, _ = random_case(shape)
    got = backward(lib, p, t, scale)
    _same_bits(got, R.grad32(p, t, scale), "grad_pred")
    assert np.abs(got).max() > 0


def _planted_batch():
    """sample 0 and 2: random; sample 1: the planted grid p x t at its start"""
    p, t, scale, _, _ = random_case((3, 1023))
    p, t = p.copy(), t.copy()
    pp, pt = R.planted()
    p[1, :pp.size], t[1, :pp.size] = pp, pt
    return p, t, scale


def test_planted_grid_exact_values_and_gradient(lib):
    p, t, scale = _planted_batch()
    n, nt = len(R.PLANTED_P) * len(R.PLANTED_T), len(R.PLANTED_T)
    s, e = forward(lib, p, t)
    grid = e[1, :n].reshape(-1, nt)
    assert grid[0].tolist() == [0.0, 50.0, 100.0]                 # p == 0: 0 (not 0 * -inf), exactly 100 at t = 1
    assert grid[-1].tolist() == [100.0, 50.0, 0.0]                # p == 1: exactly 100 at t = 0, 0 at t = 1
    assert grid[1].tolist() == [0.0, 50.0, 100.0]                 # p = 2^-149: the log is clamped, 1 - p rounds to 1
    assert np.isfinite(e).all() and np.isfinite(s).all()
    err = np.abs(e.astype(np.float64) - R.loss_elem64(p, t))
    assert (err <= R.elem_bound(p, t)).all()
    _same_bits(backward(lib, p, t, scale), R.grad32(p, t, scale), "grad_pred on the planted grid")


@pytest.mark.parametrize("bad", [float("nan"), -0.25, 1.5, float("inf")], ids=["nan", "negative", "above-one", "inf"])
def test_nan_or_out_of_range_pred_poisons_exactly_one_sample(lib, bad):
    p, t, scale = _planted_batch()
    clean_s, clean_e = forward(lib, p, t)
    p[1, 700] = bad
    t[1, 700] = 0.5
    s, e = forward(lib, p, t)
    assert np.isnan(s[1]) and np.isnan(e[1, 700])                 # not an error, and not swallowed by the clamp
    assert np.isnan(e).sum() == 1
    _same_bits(s[[0, 2]], clean_s[[0, 2]], "loss_sum of the other samples")
    keep = np.ones(p.shape, bool)
    keep[1, 700] = False
    assert np.array_equal(R.bits(e)[keep], R.bits(clean_e)[keep])
    g = backward(lib, p, t, scale)
    want = R.grad32(p, t, scale)
    assert np.array_equal(R.bits(g)[keep], R.bits(want)[keep])
    assert np.isnan(g[1, 700]) == np.isnan(want[1, 700])


def test_a_sample_has_the_same_bits_in_every_batch_split(lib):
    """a batch of 5, the same samples as 2 + 3, and each alone; V = 4099: odd rows, five chunks, a short last quad"""
    g = torch.Generator().manual_seed(5)
    p, t = torch.rand(5, 4099, generator=g).numpy(), torch.rand(5, 4099, generator=g).numpy()
    scale = np.array([0.5, -1.0, 2.0 ** -12, 3.0, 1e-3], np.float32)
    s, e = forward(lib, p, t)
    gr = backward(lib, p, t, scale)
    for lo, hi in ((0, 2), (2, 5), (0, 1), (1, 2), (2, 3), (3, 4), (4, 5)):
        s2, e2 = forward(lib, p[lo:hi].copy(), t[lo:hi].copy())
        _same_bits(s2, s[lo:hi], f"loss_sum of samples {lo}..{hi - 1}")
        _same_bits(e2, e[lo:hi], f"loss_elem of samples {lo}..{hi - 1}")
        _same_bits(backward(lib, p[lo:hi].copy(), t[lo:hi].copy(), scale[lo:hi]), gr[lo:hi], f"grad_pred of samples {lo}..{hi - 1}")


@pytest.mark.parametrize("shape", [(2, 5), (3, 1023), (2, 1025), (2, 4099), (2, 16385)], ids=_ids)
def test_runs_and_addresses_do_not_matter(lib, shape):
    p, t, scale, _, _ = random_case(shape)
    s, e = forward(lib, p, t)
    gr = backward(lib, p, t, scale)
    order = ["pred", "target", "loss_sum", "loss_elem", "grad_scale", "grad_pred"]
    for label, sk in (("second run", None), ("every argument + 1 element", lambda name, dtype, role: 1),
                      ("arguments at 1, 2, 3, ... elements", lambda name, dtype, role: 1 + order.index(name) % 3)):
        with G.skews(sk):
            s2, e2 = forward(lib, p, t)
            g2 = backward(lib, p, t, scale)
        _same_bits(s2, s, f"loss_sum, {label}")
        _same_bits(e2, e, f"loss_elem, {label}")
        _same_bits(g2, gr, f"grad_pred, {label}")


# ---------------------------------------------------------------- the Python surface
def test_module_value_and_gradient_against_torch_float64(s3r):
    B, shape = 3, (3, 8, 9, 10)
    g = torch.Generator().manual_seed(9)
    p0 = torch.rand(shape, generator=g) * 0.98 + 0.01
    t0 = (torch.rand(shape, generator=g) < 0.4).float()
    pp, pt = R.planted()
    p0.view(B, -1)[2, :pp.size], t0.view(B, -1)[2, :pp.size] = torch.from_numpy(pp), torch.from_numpy(pt)
    pd = p0.double().requires_grad_()
    ref = torch.nn.BCELoss()(pd, t0.double())
    (ref_grad,) = torch.autograd.grad(ref, pd)
    loss_fn = s3r.VoxelBCELoss()
    plain = loss_fn(p0.to(DEV), t0.to(DEV))
    assert plain.grad_fn is None and not plain.requires_grad      # nothing recorded without a pred that requires grad
    with torch.no_grad():
        assert loss_fn(p0.to(DEV).requires_grad_(), t0.to(DEV)).grad_fn is None
    p = p0.to(DEV).requires_grad_()
    loss = loss_fn(p, t0.to(DEV))
    assert loss.dtype == torch.float32 and loss.dim() == 0 and loss.grad_fn is not None
    assert torch.equal(loss.detach().view(torch.int32), plain.view(torch.int32))
    N = p0.numel()
    pn, tn = p0.view(B, -1).numpy(), t0.view(B, -1).numpy()
    lim = R.elem_bound(pn, tn)
    l64 = R.loss_elem64(pn, tn)
    tol = (lim.sum() + sum(R.sum_bound(l64[b] + lim[b]) for b in range(B))) / N + R.U32 * abs(ref.item())      # the final cast to fp32
    print(f"VoxelBCELoss: {loss.item():.9g} vs float64 {ref.item():.9g}, err / bound {abs(loss.item() - ref.item()) / tol:.4f}")
    assert abs(loss.item() - ref.item()) <= tol
    loss.backward()
    assert p.grad.shape == p0.shape
    # bit for bit the kernel's rule with grad_scale = float32(1 / N) ...
    want = R.grad32(pn, tn, np.full(B, np.float32(np.float64(1.0) / N), np.float32))
    _same_bits(p.grad.cpu().view(B, -1).numpy(), want, "VoxelBCELoss gradient")
    # ... which is torch's float64 gradient within five roundings and the rounding of 1 / N (gamma_6), plus the numerator's underflow
    g64 = ref_grad.view(B, -1).numpy()
    d64 = np.maximum((1.0 - pn.astype(np.float64)) * pn.astype(np.float64), 1e-12)
    assert (np.abs(want - g64) <= R.gamma(6) * np.abs(g64) + 2.0 ** -149 / d64 + 2.0 ** -149).all()
    # the functional forms
    s, e = s3r.voxel_bce(p0.to(DEV), t0.to(DEV), elements=True)
    assert s.shape == (B,) and e.shape == shape and s3r.voxel_bce(p0.to(DEV), t0.to(DEV))[1] is None
    assert torch.equal(((s.double().sum() / N).float()).view(torch.int32), plain.view(torch.int32))
    d = s3r.differentiable_voxel_bce(p0.to(DEV).requires_grad_(), t0.to(DEV).requires_grad_())
    assert d.grad_fn is not None and torch.equal(d.detach().view(torch.int32), s.view(torch.int32))
    empty = s3r.voxel_bce(torch.empty(0, 4, device=DEV), torch.empty(0, 4, device=DEV), elements=True)
    assert empty[0].shape == (0,) and empty[1].shape == (0, 4)


def test_gradient_goes_to_pred_only(s3r):
    p = torch.rand(2, 50, device=DEV).requires_grad_()
    t = torch.rand(2, 50, device=DEV).requires_grad_()
    s3r.VoxelBCELoss()(p, t).backward()
    assert p.grad is not None and t.grad is None


def test_profiler_records(s3r, lib):
    B, V = 3, 1000
    p, t, gs = torch.rand(B, V, device=DEV), torch.rand(B, V, device=DEV), torch.rand(B, device=DEV)
    s3r.profile_enable(16)
    try:
        s3r.voxel_bce(p, t)
        s3r.voxel_bce(p, t, elements=True)
        s3r.voxel_bce_backward(p, t, gs)
        torch.cuda.synchronize()
        rec = s3r.profile_read(16)
    finally:
        s3r.profile_enable(0)
    assert [(r["family"], r["tag"], r["launches"]) for r in rec] == [("iou", 1, 1), ("iou", 1, 1), ("iou", 2, 1)]      # family 6
    assert all(r["ms"] > 0 and r["flops"] == 0 for r in rec)
    assert rec[0]["bytes"] == 4.0 * (2 * B * V + B) and rec[1]["bytes"] == 4.0 * (3 * B * V + B) and rec[2]["bytes"] == 4.0 * (3 * B * V + B)
