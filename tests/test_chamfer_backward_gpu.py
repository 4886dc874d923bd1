"""s3r_chamfer_backward on the device, through the C-ABI, with the indices s3r_chamfer_forward wrote: bit equality with the defined
fp32 order (tests/_chamfer64.py (a)), the derived bound against float64 ((b)), exact equality on integer lattices, the
order-sensitive heavy-collision case, ties, the NULL forms, batch and run invariance, guarded buffers at 256-byte and at element
alignment, garbage indices, the autograd surface and the profiler record.

There is no measured tolerance in this file: results are compared bit for bit, or against
|got - fp64| <= (k + 3) 2^-24 sum|term| + 2^-149 (one rounding for the difference, one for the product, k adds each bounded by
sum|term|, +1 for second order, one subnormal), k and sum|term| computed per element by the float64 restatement."""
import functools

import numpy as np
import pytest
import torch

from tests import _chamfer64 as R
from tests import _guard as G

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def lib(s3r):
    return s3r.load_library()


def _rc(lib, rc, what):
    assert rc == 0, f"{what}: {lib.s3r_last_error().decode()} ({rc})"


def _ptr(t):
    return None if t is None else t.data_ptr()


def forward_indices(lib, p, q):
    """idx1, idx2 (device int32) as s3r_chamfer_forward writes them"""
    B, N, M = p.shape[0], p.shape[1], q.shape[1]
    d1, d2 = torch.empty(B, N, device=DEV), torch.empty(B, M, device=DEV)
    i1, i2 = torch.empty(B, N, dtype=torch.int32, device=DEV), torch.empty(B, M, dtype=torch.int32, device=DEV)
    _rc(lib, lib.s3r_chamfer_forward(p.data_ptr(), q.data_ptr(), d1.data_ptr(), d2.data_ptr(), i1.data_ptr(), i2.data_ptr(), B, N, M, None),
        "chamfer forward")
    torch.cuda.synchronize()
    return i1, i2


def backward(lib, p, q, i1, i2, g1, g2, need_p=True, need_q=True):
    """plain (unguarded) call: device tensors in, (grad_p, grad_q) numpy out (None for a side not asked for)"""
    B, N, M = p.shape[0], p.shape[1], q.shape[1]
    gp = torch.empty(B, N, 3, device=DEV) if need_p else None
    gq = torch.empty(B, M, 3, device=DEV) if need_q else None
    _rc(lib, lib.s3r_chamfer_backward(p.data_ptr(), q.data_ptr(), i1.data_ptr(), i2.data_ptr(), _ptr(g1), _ptr(g2), _ptr(gp), _ptr(gq),
                                      B, N, M, None), "chamfer backward")
    torch.cuda.synchronize()
    return tuple(None if t is None else t.cpu().numpy() for t in (gp, gq))


def _np(*ts):
    return tuple(None if t is None else t.cpu().numpy() for t in ts)


def _same_bits(got, want, what):
    gb, wb = R.bits(got), R.bits(want)
    bad = np.argwhere(gb != wb)
    assert bad.size == 0, f"{what}: {len(bad)} elements differ, first at {tuple(bad[0])}: got {got[tuple(bad[0])]!r} want {want[tuple(bad[0])]!r}"


def _clouds(B, N, M, seed):
    g = torch.Generator().manual_seed(seed)
    p, q = torch.rand(B, N, 3, generator=g), torch.rand(B, M, 3, generator=g)
    g1, g2 = torch.randn(B, N, generator=g), torch.randn(B, M, generator=g)
    return p.to(DEV), q.to(DEV), g1.to(DEV), g2.to(DEV)


# N != M, N or M = 1, sizes off 64 / 128 / 512 / 2048, multi-pass clouds, B = 1 .. 3, and the BASELINE shape
SHAPES = [(1, 1, 1), (1, 1, 37), (2, 53, 1), (1, 64, 64), (2, 100, 257), (3, 129, 130), (2, 513, 511), (3, 2049, 2047), (1, 2048, 4096),
          (1, 2500, 5000), (2, 5000, 2500), (32, 2048, 2048)]
_ids = lambda s: "x".join(map(str, s))      # noqa: E731


@functools.lru_cache(maxsize=None)
def _random_case(lib, shape):
    B, N, M = shape
    p, q, g1, g2 = _clouds(B, N, M, seed=N * 10007 + M * 3 + B)
    i1, i2 = forward_indices(lib, p, q)
    got = backward(lib, p, q, i1, i2, g1, g2)
    return _np(p, q, i1, i2, g1, g2), got


@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
def test_bits_equal_the_defined_fp32_order(lib, shape):
    args, (gp, gq) = _random_case(lib, shape)
    want_p, want_q = R.backward32(*args)
    _same_bits(gp, want_p, "grad_p")
    _same_bits(gq, want_q, "grad_q")
    assert np.abs(gp).max() > 0 and np.abs(gq).max() > 0


@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
def test_within_the_derived_bound_of_fp64(lib, shape):
    args, got = _random_case(lib, shape)
    for name, g, (ref, k, mag) in zip(("grad_p", "grad_q"), got, R.backward64(*args)):
        err = np.abs(g.astype(np.float64) - ref)
        lim = R.bound32(k, mag)
        print(f"{shape} {name}: max err {err.max():.3e}, max err / bound {(err / lim).max():.3f}, max k {k.max()}")
        assert (err <= lim).all()


@pytest.mark.parametrize("shape", [(1, 40, 300), (2, 300, 40), (3, 257, 2100)], ids=_ids)
def test_exact_on_an_integer_lattice(lib, shape):
    """integer coordinates in [-8, 8] and integer gradients in [-4, 4]: every difference, product and partial sum is an integer below
    2 * 4 * 16 * (count + 1) < 2^24, so no fp32 operation rounds in ANY order and the result equals the float64 one exactly (the
    lattice is full of ties: the gradient follows the forward's first-minimum indices)"""
    B, N, M = shape
    g = torch.Generator().manual_seed(N + M)
    p = torch.randint(-8, 9, (B, N, 3), generator=g).float().to(DEV)
    q = torch.randint(-8, 9, (B, M, 3), generator=g).float().to(DEV)
    g1 = torch.randint(-4, 5, (B, N), generator=g).float().to(DEV)
    g2 = torch.randint(-4, 5, (B, M), generator=g).float().to(DEV)
    i1, i2 = forward_indices(lib, p, q)
    got = backward(lib, p, q, i1, i2, g1, g2)
    for g_, (ref, k, mag) in zip(got, R.backward64(*_np(p, q, i1, i2, g1, g2))):
        assert mag.max() < 2 ** 24 and k.sum() > 0
        assert np.array_equal(ref, np.round(ref)) and np.array_equal(g_.astype(np.float64), ref)
        assert np.abs(ref).max() > 0


def test_heavy_collision_keeps_the_ascending_order(lib):
    """one q point inside the p cluster, every other q far away: all N terms of direction q land on ONE target, three staging passes
    deep.  This is the order-sensitive case — an atomicAdd scatter gives arrival order — and it must have the restatement's bits."""
    N, M = 5000, 9
    g = torch.Generator().manual_seed(11)
    p = (torch.rand(2, N, 3, generator=g) * 0.1).to(DEV)
    q = (100 + torch.rand(2, M, 3, generator=g))
    q[:, 4] = 0.05
    q = q.to(DEV)
    g1, g2 = torch.randn(2, N, generator=g).to(DEV), torch.randn(2, M, generator=g).to(DEV)
    i1, i2 = forward_indices(lib, p, q)
    assert bool((i1 == 4).all())
    gp, gq = backward(lib, p, q, i1, i2, g1, g2)
    args = _np(p, q, i1, i2, g1, g2)
    want_p, want_q = R.backward32(*args)
    _same_bits(gq, want_q, "grad_q")
    _same_bits(gp, want_p, "grad_p")
    (_, _, _), (ref, k, mag) = R.backward64(*args)
    assert k[:, 4].tolist() == [N, N]
    assert (np.abs(gq.astype(np.float64) - ref) <= R.bound32(k, mag)).all()
    # the order is observable here: summing the same terms in descending order gives other bits
    rev = R.backward32(args[0][:, ::-1], args[1], args[2][:, ::-1], (N - 1 - args[3]).astype(np.int32), args[4][:, ::-1], args[5])[1]
    assert not np.array_equal(R.bits(rev[:, 4]), R.bits(want_q[:, 4]))


def test_ties_follow_the_first_minimum_indices(lib):
    g = torch.Generator().manual_seed(3)
    p0, q0 = torch.rand(2, 150, 3, generator=g), torch.rand(2, 90, 3, generator=g)
    p, q = torch.cat([p0, p0, p0[:, :17]], 1).to(DEV), torch.cat([q0, q0], 1).to(DEV)       # every point has a duplicate
    g1, g2 = torch.randn(2, p.shape[1], generator=g).to(DEV), torch.randn(2, q.shape[1], generator=g).to(DEV)
    i1, i2 = forward_indices(lib, p, q)
    assert int(i1.max()) < 90 and int(i2.max()) < 150                # the first of the equal minima
    gp, gq = backward(lib, p, q, i1, i2, g1, g2)
    want_p, want_q = R.backward32(*_np(p, q, i1, i2, g1, g2))
    _same_bits(gp, want_p, "grad_p")
    _same_bits(gq, want_q, "grad_q")
    (_, kp, _), (_, kq, _) = R.backward64(*_np(p, q, i1, i2, g1, g2))
    assert kq[:, 90:].sum() == 0 and kp[:, 150:].sum() == 0          # the duplicates receive their own term only


def test_null_forms(lib):
    B, N, M = 2, 300, 2100
    p, q, g1, g2 = _clouds(B, N, M, seed=21)
    i1, i2 = forward_indices(lib, p, q)
    full_p, full_q = backward(lib, p, q, i1, i2, g1, g2)

    def guarded(gp_null=False, gq_null=False, g2_=g2):
        gp = G.Guarded("grad_p", (B, N, 3), torch.float32, DEV, "out")
        gq = G.Guarded("grad_q", (B, M, 3), torch.float32, DEV, "out")
        _rc(lib, lib.s3r_chamfer_backward(p.data_ptr(), q.data_ptr(), i1.data_ptr(), i2.data_ptr(), g1.data_ptr(), _ptr(g2_),
                                          None if gp_null else gp.ptr, None if gq_null else gq.ptr, B, N, M, None), "chamfer backward")
        torch.cuda.synchronize()
        return gp, gq

    poison = G._BITS[torch.float32][2]
    gp, gq = guarded(gq_null=True)                                   # grad_q = NULL: not computed, the buffer keeps its poison
    assert gp.check() is None and bool((G._as_bits(gq.raw)[gq.g:gq.g + gq.n] == poison).all())
    assert "leftover poison" in gq.check()
    _same_bits(gp.t.cpu().numpy(), full_p, "grad_p with grad_q = NULL")
    gp, gq = guarded(gp_null=True)                                   # ... and mirrored
    assert gq.check() is None and bool((G._as_bits(gp.raw)[gp.g:gp.g + gp.n] == poison).all())
    assert "leftover poison" in gp.check()
    _same_bits(gq.t.cpu().numpy(), full_q, "grad_q with grad_p = NULL")
    zp, zq = guarded(g2_=torch.zeros_like(g2))                       # grad_dist2 = NULL: the bits of a zero tensor
    np_, nq = guarded(g2_=None)
    G.check_all(zp, zq, np_, nq)
    assert torch.equal(G._as_bits(zp.t), G._as_bits(np_.t)) and torch.equal(G._as_bits(zq.t), G._as_bits(nq.t))
    want_p, want_q = R.backward32(*_np(p, q, i1, i2, g1, None))
    _same_bits(np_.t.cpu().numpy(), want_p, "grad_p with grad_dist2 = NULL")
    _same_bits(nq.t.cpu().numpy(), want_q, "grad_q with grad_dist2 = NULL")
    zero1 = backward(lib, p, q, i1, i2, torch.zeros_like(g1), g2)    # ... and grad_dist1 = NULL likewise
    null1 = backward(lib, p, q, i1, i2, None, g2)
    _same_bits(null1[0], zero1[0], "grad_p with grad_dist1 = NULL")
    _same_bits(null1[1], zero1[1], "grad_q with grad_dist1 = NULL")


def test_batch_and_run_invariance(lib):
    B, N, M = 3, 700, 2300
    p, q, g1, g2 = _clouds(B, N, M, seed=33)
    i1, i2 = forward_indices(lib, p, q)
    first = backward(lib, p, q, i1, i2, g1, g2)
    again = backward(lib, p, q, i1, i2, g1, g2)
    for a, b in zip(first, again):
        _same_bits(a, b, "second run")
    for b in range(B):
        s = slice(b, b + 1)
        one = backward(lib, p[s].contiguous(), q[s].contiguous(), i1[s].contiguous(), i2[s].contiguous(), g1[s].contiguous(), g2[s].contiguous())
        _same_bits(one[0][0], first[0][b], f"grad_p of sample {b} alone")
        _same_bits(one[1][0], first[1][b], f"grad_q of sample {b} alone")


def _guarded_call(lib, p, q, i1, i2, g1, g2):
    B, N, M = p.shape[0], p.shape[1], q.shape[1]
    ins = [G.Guarded(name, t.shape, t.dtype, DEV, "in", data=t) for name, t in
           (("p", p), ("q", q), ("idx1", i1), ("idx2", i2), ("grad_dist1", g1), ("grad_dist2", g2))]
    gp = G.Guarded("grad_p", (B, N, 3), torch.float32, DEV, "out")
    gq = G.Guarded("grad_q", (B, M, 3), torch.float32, DEV, "out")
    _rc(lib, lib.s3r_chamfer_backward(*[b.ptr for b in ins], gp.ptr, gq.ptr, B, N, M, None), "chamfer backward")
    torch.cuda.synchronize()
    G.check_all(*ins, gp, gq)            # inputs bitwise unchanged, outputs fully written, guards intact
    return ins + [gp, gq]


SKEWS = {"p": 1, "q": 3, "idx1": 1, "idx2": 5, "grad_dist1": 7, "grad_dist2": 1, "grad_p": 3, "grad_q": 1}


@pytest.mark.parametrize("shape", [(2, 200, 333), (1, 2100, 519)], ids=_ids)
def test_guarded_buffers_aligned_and_at_element_alignment(lib, shape):
    B, N, M = shape
    p, q, g1, g2 = _clouds(B, N, M, seed=N + M)
    i1, i2 = forward_indices(lib, p, q)
    aligned = _guarded_call(lib, p, q, i1, i2, g1, g2)
    assert all(b.ptr % 256 == 0 for b in aligned)
    with G.skews(SKEWS):
        skewed = _guarded_call(lib, p, q, i1, i2, g1, g2)
    assert all(b.ptr % 256 == 4 * SKEWS[b.name] and b.ptr % 8 == 4 for b in skewed)      # every pointer only element-aligned
    for a, s in zip(aligned[-2:], skewed[-2:]):
        assert torch.equal(G._as_bits(a.t), G._as_bits(s.t)), a.name
    want_p, want_q = R.backward32(*_np(p, q, i1, i2, g1, g2))
    _same_bits(aligned[-2].t.cpu().numpy(), want_p, "grad_p")
    _same_bits(aligned[-1].t.cpu().numpy(), want_q, "grad_q")


def test_garbage_indices_are_clamped(lib):
    """not a fault test: the kernel clamps the own-term index and an out-of-range index matches no target, so a call whose idx1 holds
    -1 and m returns S3R_OK, stays inside its buffers and equals the restatement (which clamps and skips in the same way)"""
    B, N, M = 2, 600, 250
    p, q, g1, g2 = _clouds(B, N, M, seed=8)
    i1, i2 = forward_indices(lib, p, q)
    i1 = i1.clone()
    i1[:, 5] = -1
    i1[:, 77] = M
    i1[1, 599] = 2 ** 31 - 1
    i1[0, 0] = -2 ** 31
    bufs = _guarded_call(lib, p, q, i1, i2, g1, g2)
    want_p, want_q = R.backward32(*_np(p, q, i1, i2, g1, g2))
    _same_bits(bufs[-2].t.cpu().numpy(), want_p, "grad_p")
    _same_bits(bufs[-1].t.cpu().numpy(), want_q, "grad_q")


# ---------------------------------------------------------------- autograd
def test_module_backward_is_the_functional_call(s3r, lib):
    B, N, M = 3, 500, 310
    p, q, _, _ = _clouds(B, N, M, seed=2)
    with torch.no_grad():
        plain = s3r.ChamferDistance()(p, q)
    pr = p.clone().requires_grad_()
    loss = s3r.ChamferDistance()(pr, q)
    assert loss.requires_grad and torch.equal(loss.detach().view(torch.int32), plain.view(torch.int32))
    loss.backward()
    assert q.grad is None and pr.grad is not None and pr.grad.shape == p.shape
    d1, d2, i1, i2 = s3r.chamfer_distance(p, q)
    g1 = torch.ones(B, N, device=DEV) / (B * N)                      # what mean() hands back: 1 / numel, an fp32 division
    g2 = torch.ones(B, M, device=DEV) / (B * M)
    gp, gq = s3r.chamfer_distance_backward(p, q, i1, i2, g1, g2, need_q=False)
    assert gq is None
    assert torch.equal(pr.grad.view(torch.int32), gp.view(torch.int32))
    _same_bits(gp.cpu().numpy(), R.backward32(*_np(p, q, i1, i2, g1, g2))[0], "grad_p")
    # both sides
    pr, qr = p.clone().requires_grad_(), q.clone().requires_grad_()
    s3r.ChamferDistance()(pr, qr).backward()
    gp, gq = s3r.chamfer_distance_backward(p, q, i1, i2, g1, g2)
    assert torch.equal(pr.grad.view(torch.int32), gp.view(torch.int32)) and torch.equal(qr.grad.view(torch.int32), gq.view(torch.int32))
    # only q
    qr = q.clone().requires_grad_()
    s3r.ChamferDistance()(p, qr).backward()
    assert torch.equal(qr.grad.view(torch.int32), gq.view(torch.int32))


def test_differentiable_function_surface(s3r, lib):
    B, N, M = 2, 140, 90
    p, q, g1, _ = _clouds(B, N, M, seed=4)
    pr = p.clone().requires_grad_()
    d1, d2, i1, i2 = s3r.differentiable_chamfer_distance(pr, q)
    e1, e2, j1, j2 = s3r.chamfer_distance(p, q)
    assert d1.requires_grad and d2.requires_grad and not i1.requires_grad and not i2.requires_grad
    assert torch.equal(d1.detach().view(torch.int32), e1.view(torch.int32)) and torch.equal(d2.detach().view(torch.int32), e2.view(torch.int32))
    assert torch.equal(i1, j1) and torch.equal(i2, j2) and i1.dtype == torch.int32
    (gp,) = torch.autograd.grad((d1 * g1).sum(), pr)                 # dist2 unused: its gradient arrives as None -> NULL
    want = s3r.chamfer_distance_backward(p, q, i1, i2, g1, None, need_q=False)[0]
    assert torch.equal(gp.view(torch.int32), want.view(torch.int32))
    # under no_grad, or with nothing requiring grad, nothing is recorded
    with torch.no_grad():
        out = s3r.ChamferDistance()(pr, q)
    assert not out.requires_grad and out.grad_fn is None
    out = s3r.ChamferDistance()(p, q)
    assert not out.requires_grad and out.grad_fn is None
    assert not any(t.requires_grad for t in s3r.chamfer_distance(pr, q))      # the metric itself stays no_grad


def test_gradient_steps_lower_the_loss(s3r, lib):
    p, q, _, _ = _clouds(2, 256, 256, seed=6)
    pr = p.clone().requires_grad_()
    cd = s3r.ChamferDistance()
    losses = []
    for _ in range(12):
        loss = cd(pr, q)
        losses.append(float(loss.detach()))
        (g,) = torch.autograd.grad(loss, pr)
        with torch.no_grad():
            pr -= 20.0 * g         # the loss for FIXED indices is a quadratic of curvature 2 (1 + k_i) / (B N) = (1 + k_i) / 256 per point:
                                   # a step of 20 lowers it while k_i < 24, and the true loss (a minimum over indices) is below it
    with torch.no_grad():
        losses.append(float(cd(pr, q)))
    print("losses:", " ".join(f"{v:.5f}" for v in losses))
    assert losses[-1] < 0.5 * losses[0] and all(b < a for a, b in zip(losses, losses[1:]))


def test_profiler_record(s3r, lib):
    B, N, M = 2, 300, 200
    p, q, g1, g2 = _clouds(B, N, M, seed=9)
    i1, i2 = forward_indices(lib, p, q)
    s3r.profile_enable(16)
    try:
        backward(lib, p, q, i1, i2, g1, g2)
        both = s3r.profile_read(16)
        s3r.profile_reset()
        backward(lib, p, q, i1, i2, g1, None, need_q=False)
        one = s3r.profile_read(16)
    finally:
        s3r.profile_enable(0)
    assert len(both) == 1 and both[0]["family"] == "chamfer" and both[0]["tag"] == 1 and both[0]["launches"] == 1
    assert both[0]["flops"] == B * 17.0 * (N + M) and both[0]["bytes"] == 4.0 * B * (3 * (N + M) + 2 * (N + M) + 3 * (N + M))
    assert both[0]["ms"] > 0
    assert len(one) == 1 and one[0]["flops"] == B * (7.0 * N + 10.0 * M) and one[0]["bytes"] == 4.0 * B * (3 * (N + M) + (N + M) + N + 3 * N)
