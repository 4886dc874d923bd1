"""s3r_disparity_soft_backward and the disparity loss on the device, through the C-ABI in guarded, poisoned buffers unless stated
(tests/_guard.py): every gradient per element within the derived bound of the float64 restatement (tests/_dispbwd64.py), the
equal-cost case bit for bit as values against the restated fp32 order, NULL forms, run / address / batch invariance, a NaN that stays
in its sample, the autograd surface; the loss bit for bit (elements, gradient, the sum's order on the device's own elements) with
exact counts.

There is no measured tolerance in this file."""
import functools

import numpy as np
import pytest
import torch

from tests import _dispbwd64 as R
from tests import _guard as G

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32 = torch.float32
I32 = torch.int32
INVALID = -1
TAU, SCALE = 0.7, 8.0
ALL = R.CASES + [R.NETWORK]
SAME_SIZE = R.CASES[:2]


@pytest.fixture(scope="module")
def lib(s3r):
    return s3r.load_library()


def _same_bits(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.argwhere(R.bits(got) != R.bits(want))
    assert bad.size == 0, f"{what}: {len(bad)} elements differ, first at {tuple(bad[0])}: got {got[tuple(bad[0])]!r} want {want[tuple(bad[0])]!r}"


def run(lib, case, data, grads=(True, True), need=(True, True), expect=0, tau=TAU, prefill=None, dims=None):
    """One guarded call.  data = (fl, fr, gdl, gdr) numpy fp32.  Returns (grad_left, grad_right) numpy, None for a side not asked for:
    BOTH outputs are allocated, poisoned and guarded; a side not asked for is passed as NULL and must hold what it held."""
    B, C, H, W, D, OH, OW = case
    fl, fr, gdl, gdr = data
    B = fl.shape[0]
    ins = [G.Guarded(n, a.shape, F32, DEV, "in", data=torch.from_numpy(np.array(a, np.float32)))
           for n, a in (("feat_l", fl), ("feat_r", fr), ("grad_disp_l", gdl), ("grad_disp_r", gdr))]
    outs = [G.Guarded(n, (B, C, H, W), F32, DEV, "out") for n in ("grad_left", "grad_right")]
    if prefill is not None:
        for o in outs:
            o.t.fill_(prefill)
    before = [G._as_bits(o.t).clone() for o in outs]
    gp = [i.ptr if g else None for i, g in zip(ins[2:], grads)]
    op = [o.ptr if n else None for o, n in zip(outs, need)]
    rc = lib.s3r_disparity_soft_backward(ins[0].ptr, ins[1].ptr, 0, *gp, *op, *(dims or (B, C, H, W, D)), tau, OH, OW, SCALE, None)
    torch.cuda.synchronize()
    G.check_all(*ins)
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
def reference(case, kind="random"):
    """(data, backward64's gradients and bounds) of a case, computed once and shared (left unchanged by the tests)"""
    data = (R.random_case if kind == "random" else R.equal_cost_case)(case)
    B, C, H, W, D, OH, OW = case
    return data, R.backward64(*data, D, TAU, R.out_size(case), SCALE)


@functools.lru_cache(maxsize=None)
def device_result(case, kind="random"):
    import s3r
    return run(s3r.load_library(), case, reference(case, kind)[0])


# ---------------------------------------------------------------- values
@pytest.mark.parametrize("case", ALL, ids=R.case_id)
def test_within_the_derived_bound_of_float64(lib, case):
    _, ((gl64, gr64), (bl, br)) = reference(case)
    gl, gr = device_result(case)
    worst = max((np.abs(gl - gl64) / bl).max(), (np.abs(gr - gr64) / br).max())
    print(f"{R.case_id(case)}: largest error / bound {worst:.3e}")
    assert worst <= 1.0
    if case[3] == 1:                                               # W = 1: one disparity, the read-out is the constant 0
        assert not gl.any() and not gr.any()
    else:
        assert np.abs(gl).max() > 0 and np.abs(gr).max() > 0


@pytest.mark.parametrize("case", SAME_SIZE + [R.UPSAMPLED], ids=R.case_id)
def test_equal_costs_bit_for_bit(lib, case):
    """every weight is expf(0) = 1: the whole backward is defined bit for bit; compared as values (the sign of a zero is not part of
    the contract)"""
    B, C, H, W, D, OH, OW = case
    data = reference(case, "equal")[0]
    want = R.backward32(*data, D, TAU, R.out_size(case), SCALE)
    got = device_result(case, "equal")
    for g, w, what in zip(got, want, ("grad_left", "grad_right")):
        bad = np.argwhere(g != w)
        assert bad.size == 0, f"{what}: {len(bad)} elements differ, first at {tuple(bad[0])}: {g[tuple(bad[0])]!r} != {w[tuple(bad[0])]!r}"
    assert np.abs(want[0]).max() > 0 and not got[0][:, C // 2].any()


# ---------------------------------------------------------------- invariance
@pytest.mark.parametrize("case", R.CASES, ids=R.case_id)
def test_null_forms_have_the_bits_of_the_full_call(lib, case):
    data = reference(case)[0]
    base = device_result(case)
    gl, none = run(lib, case, data, need=(True, False))
    assert none is None
    _same_bits(gl, base[0], "grad_left alone")
    none, gr = run(lib, case, data, need=(False, True))
    assert none is None
    _same_bits(gr, base[1], "grad_right alone")
    for which in (0, 1):                                           # a NULL gradient equals an explicit zero tensor
        grads = tuple(i != which for i in (0, 1))
        zeroed = list(data)
        zeroed[2 + which] = np.zeros_like(data[2 + which])
        want = run(lib, case, tuple(zeroed))
        got = run(lib, case, data, grads=grads)
        _same_bits(got[0], want[0], f"grad_left, gradient {which} NULL")
        _same_bits(got[1], want[1], f"grad_right, gradient {which} NULL")
    # each gradient alone: the two directions add up to the full call's within the bound (they share no rounding)
    _, ((gl64, gr64), (bl, br)) = reference(case)
    a, b = run(lib, case, data, grads=(True, False)), run(lib, case, data, grads=(False, True))
    assert (np.abs(a[0].astype(np.float64) + b[0] - gl64) <= 2 * bl + 2.0 ** -23 * (np.abs(a[0]) + np.abs(b[0]))).all()


@pytest.mark.parametrize("case", R.CASES[:4], ids=R.case_id)
def test_runs_addresses_and_output_contents_do_not_matter(lib, case):
    data = reference(case)[0]
    base = device_result(case)
    again = [("second run", run(lib, case, data)), ("outputs holding -inf", run(lib, case, data, prefill=-np.inf))]
    for sk in (1, 2, 3):
        with G.skews(lambda name, dtype, role, sk=sk: 1 + (sk + len(name)) % 3):      # every pointer 1-3 elements past a 256-byte boundary
            again.append((f"skew pattern {sk}", run(lib, case, data)))
    for what, got in again:
        _same_bits(got[0], base[0], f"grad_left, {what}")
        _same_bits(got[1], base[1], f"grad_right, {what}")


@pytest.mark.parametrize("case", [R.CASES[0], R.UPSAMPLED], ids=R.case_id)
def test_a_sample_has_the_bits_of_its_own_call(lib, case):
    data = reference(case)[0]
    base = device_result(case)
    for b in range(case[0]):
        gl, gr = run(lib, case, tuple(a[b:b + 1] for a in data))
        _same_bits(gl, base[0][b:b + 1], f"grad_left of sample {b}")
        _same_bits(gr, base[1][b:b + 1], f"grad_right of sample {b}")


@pytest.mark.parametrize("case", [R.CASES[0], R.UPSAMPLED], ids=R.case_id)
def test_a_nan_stays_in_its_sample(lib, case):
    data = [a.copy() for a in reference(case)[0]]
    base = device_result(case)
    data[2][1, 1, 2] = np.nan                                       # sample 1's grad_disp_l
    gl, gr = run(lib, case, tuple(data))
    _same_bits(gl[:1], base[0][:1], "grad_left of sample 0")
    _same_bits(gr[:1], base[1][:1], "grad_right of sample 0")
    assert np.isnan(gl[1]).any() and np.isnan(gr[1]).any()
    data = [a.copy() for a in reference(case)[0]]
    data[0][0, 1, 1, 2] = np.nan                                    # a feature of sample 0
    gl, gr = run(lib, case, tuple(data))
    _same_bits(gl[1:], base[0][1:], "grad_left of sample 1")
    _same_bits(gr[1:], base[1][1:], "grad_right of sample 1")
    assert np.isnan(gl[0]).any()


@pytest.mark.parametrize("what", ["both-gradients-null", "both-outputs-null", "zero-width", "negative-batch", "lds-too-large", "temperature-zero"])
def test_refusals_enqueue_nothing(lib, what):
    case = R.CASES[0]
    data = reference(case)[0]
    B, C, H, W, D, OH, OW = case
    if what == "both-gradients-null":
        run(lib, case, data, grads=(False, False), expect=INVALID)
    elif what == "both-outputs-null":
        run(lib, case, data, need=(False, False), expect=INVALID)
    elif what == "temperature-zero":
        run(lib, case, data, expect=INVALID, tau=0.0)
    else:
        dims = {"zero-width": (B, C, H, 0, D), "negative-batch": (-1, C, H, W, D), "lds-too-large": (B, 64, H, 200, 4)}[what]
        run(lib, case, data, expect=INVALID, dims=dims)


def test_profiler_record(s3r, lib):
    case = R.UPSAMPLED
    B, C, H, W, D, OH, OW = case
    fl, fr, gdl, gdr = (torch.from_numpy(a).to(DEV) for a in reference(case)[0])
    s3r.profile_enable(8)
    try:
        s3r.disparity_soft_backward(fl, fr, gdl, gdr, D, TAU, (OH, OW), SCALE)
        s3r.disparity_soft_backward(fl, fr, gdl, None, D, TAU, (OH, OW), SCALE, need_right=False)
        torch.cuda.synchronize()
        rec = s3r.profile_read(8)
    finally:
        s3r.profile_enable(0)
    assert [(r["family"], r["tag"], r["launches"]) for r in rec] == [("disparity", 4, 1), ("disparity", 4, 1)]
    feat, out = B * C * H * W, B * OH * OW
    assert rec[0]["bytes"] == 4.0 * (2 * feat + 2 * out + 2 * feat) and rec[1]["bytes"] == 4.0 * (2 * feat + out + feat)


# ---------------------------------------------------------------- the autograd surface
@pytest.mark.parametrize("case", [R.CASES[0], R.UPSAMPLED], ids=R.case_id)
def test_differentiable_disparity_soft(s3r, case):
    """values bit-equal to disparity_soft; the backward within the bound of float64 for the gradients autograd hands it (the float64
    restatement is checked against torch's float64 autograd in tests/test_disparity_backward_cpu.py); exactly the sides asked for"""
    B, C, H, W, D, OH, OW = case
    (fl, fr, gdl, gdr), ((gl64, gr64), (bl, br)) = reference(case)
    tl, tr, tgl, tgr = (torch.from_numpy(a).to(DEV) for a in (fl, fr, gdl, gdr))
    want = s3r.disparity_soft(tl, tr, D, TAU, R.out_size(case), SCALE)
    assert all(w.grad_fn is None and not w.requires_grad for w in want)
    a, b = tl.clone().requires_grad_(), tr.clone().requires_grad_()
    assert all(o.grad_fn is None for o in s3r.disparity_soft(a, b, D, TAU, R.out_size(case), SCALE))      # the plain op records no graph
    for need in ((True, True), (True, False), (False, True)):
        a, b = tl.clone().requires_grad_(need[0]), tr.clone().requires_grad_(need[1])
        dl, dr = s3r.differentiable_disparity_soft(a, b, D, TAU, R.out_size(case), SCALE)
        assert dl.grad_fn is not None and torch.equal(dl.detach().view(I32), want[0].view(I32)) and torch.equal(dr.detach().view(I32), want[1].view(I32))
        ((dl * tgl).sum() + (dr * tgr).sum()).backward()
        torch.cuda.synchronize()
        for t, ref, bound, n in ((a, gl64, bl, need[0]), (b, gr64, br, need[1])):
            if n:
                assert (np.abs(t.grad.cpu().numpy() - ref) <= bound).all()
            else:
                assert t.grad is None
    assert s3r.differentiable_disparity_soft(tl, tr, D, TAU, R.out_size(case), SCALE)[0].grad_fn is None      # no input requires grad
    with pytest.raises(RuntimeError, match="fp32 models only"):
        x = torch.zeros(1, 3, 224, 224, device=DEV)
        s3r.Stereo2Voxel(precision="bf16").to(DEV).differentiable_disparity(x, x)


# ---------------------------------------------------------------- the loss
def _loss_data(B, P, seed=0):
    rng = np.random.default_rng(seed + P)
    gt = (np.abs(rng.standard_normal((B, P))) * 20).astype(np.float32)
    pred = (gt + rng.standard_normal((B, P)) * 2).astype(np.float32)
    bad = rng.random((B, P))
    gt[bad < 0.1] = np.inf
    gt[(bad >= 0.1) & (bad < 0.15)] = -1.0
    gt[(bad >= 0.15) & (bad < 0.17)] = np.nan
    gt[(bad >= 0.17) & (bad < 0.19)] = 0.0
    k = min(P, 4)
    pred[:, :k] = gt[:, :k] + np.float32(1.0)                       # |e| == beta at beta = 1 (where the ground truth is valid)
    return pred, gt


def run_loss(lib, pred, gt, beta, elements=True, gscale=None):
    """guarded forward and backward: (loss_sum, count, loss_elem or None, grad_pred)"""
    B, P = pred.shape
    ins = [G.Guarded(n, a.shape, F32, DEV, "in", data=torch.from_numpy(np.array(a, np.float32))) for n, a in (("pred", pred), ("gt", gt))]
    gs = np.linspace(0.5, 1.5, B).astype(np.float32) if gscale is None else gscale
    gsb = G.Guarded("grad_scale", (B,), F32, DEV, "in", data=torch.from_numpy(gs))
    s, n = G.Guarded("loss_sum", (B,), F32, DEV, "out"), G.Guarded("count", (B,), I32, DEV, "out")
    e, g = G.Guarded("loss_elem", (B, P), F32, DEV, "out"), G.Guarded("grad_pred", (B, P), F32, DEV, "out")
    rc = lib.s3r_disparity_loss_forward(ins[0].ptr, ins[1].ptr, beta, s.ptr, n.ptr, e.ptr if elements else None, B, P, None)
    assert rc == 0, lib.s3r_last_error().decode()
    rc = lib.s3r_disparity_loss_backward(ins[0].ptr, ins[1].ptr, gsb.ptr, beta, g.ptr, B, P, None)
    assert rc == 0, lib.s3r_last_error().decode()
    torch.cuda.synchronize()
    if not elements:
        e.role = "scratch"
    G.check_all(*ins, gsb, s, n, e, g)
    return s.t.cpu().numpy(), n.t.cpu().numpy(), e.t.cpu().numpy() if elements else None, g.t.cpu().numpy(), gs


@pytest.mark.parametrize("beta", [1.0, 0.0, 0.37], ids=lambda b: f"beta{b}")
@pytest.mark.parametrize("P", [1, 1023, 1024, 1025, 224 * 224])
def test_loss_bit_for_bit(lib, P, beta):
    B = 3
    pred, gt = _loss_data(B, P)
    if P > 1:
        gt[1] = np.where(np.arange(P) % 3 == 0, np.inf, np.where(np.arange(P) % 3 == 1, -2.0, np.nan))      # a sample with no valid pixel
    s, n, e, g, gs = run_loss(lib, pred, gt, beta)
    want_e, ok = R.loss32(pred, gt, beta)
    _same_bits(e, want_e, "loss_elem")
    _same_bits(g, R.loss_grad32(pred, gt, gs, beta), "grad_pred")
    _same_bits(s, R.loss_sum32(e), "loss_sum in the stated order over the device's own elements")
    assert np.array_equal(n, ok.sum(1).astype(np.int32))
    assert not np.signbit(e[~ok]).any() and not e[~ok].any() and not np.signbit(g[~ok]).any() and not g[~ok].any()
    if P > 1:
        assert n[1] == 0 and s[1] == 0 and not g[1].any()
    # without loss_elem: the same sums; every batch split of B = 3: the same bits per sample
    s2, n2, _, g2, _ = run_loss(lib, pred, gt, beta, elements=False)
    _same_bits(s2, s, "loss_sum without loss_elem")
    for lo, hi in ((0, 1), (1, 3), (0, 2), (2, 3)):
        sp, np_, ep, gp, _ = run_loss(lib, pred[lo:hi], gt[lo:hi], beta, gscale=gs[lo:hi])
        _same_bits(sp, s[lo:hi], f"loss_sum of samples {lo}:{hi}")
        _same_bits(gp, g[lo:hi], f"grad_pred of samples {lo}:{hi}")
        assert np.array_equal(np_, n[lo:hi])
    # NaN or inf pred at invalid pixels changes no bit; a NaN pred at a valid pixel poisons that sample only
    p2 = pred.copy()
    p2[~ok] = np.where(np.arange((~ok).sum()) % 2 == 0, np.nan, np.inf).astype(np.float32)
    s3, n3, e3, g3, _ = run_loss(lib, p2, gt, beta)
    for got, want, what in ((s3, s, "loss_sum"), (e3, e, "loss_elem"), (g3, g, "grad_pred")):
        _same_bits(got, want, f"{what}, non-finite pred at invalid pixels")
    if ok[0].any():
        p3 = pred.copy()
        p3[0, np.argmax(ok[0])] = np.nan
        s4, n4, e4, g4, _ = run_loss(lib, p3, gt, beta)
        assert np.isnan(s4[0]) and np.array_equal(n4, n) and np.isnan(g4[0]).sum() == 1
        _same_bits(s4[1:], s[1:], "loss_sum of the other samples")
        _same_bits(g4[1:], g[1:], "grad_pred of the other samples")


def test_disparity_loss_module(s3r):
    B, P = 2, 37 * 53
    pred, gt = _loss_data(B, P, seed=3)
    tp, tg = torch.from_numpy(pred).to(DEV).view(B, 37, 53), torch.from_numpy(gt).to(DEV).view(B, 37, 53)
    for beta in (1.0, 0.0):
        crit = s3r.DisparityLoss(beta)
        plain = crit(tp, tg)
        assert plain.grad_fn is None
        e, ok = R.loss32(pred, gt, beta)
        want = np.float32(R.loss_sum32(e).astype(np.float64).sum() / max(ok.sum(), 1))
        assert plain.item() == want
        x = tp.clone().requires_grad_()
        loss = crit(x, tg)
        assert loss.grad_fn is not None and loss.item() == want
        (3 * loss).backward()
        gs = np.full(B, np.float32(np.float32(3) * np.float32(1.0 / max(ok.sum(), 1))), np.float32)
        got = x.grad.cpu().numpy().reshape(B, P)
        ref = R.loss_grad32(pred, gt, gs, beta)
        # grad_scale reaches the kernel through torch's own division and casts, at most two fp32 roundings from this one: 2 x 2^-23
        assert np.abs(got - ref).max() <= 2.0 ** -22 * np.abs(ref).max()
        assert not got[~ok].any()
        tm = torch.nn.functional.smooth_l1_loss(tp[tg.isfinite() & (tg >= 0)], tg[tg.isfinite() & (tg >= 0)], beta=beta)
        assert abs(plain.item() - tm.item()) <= int(ok.sum()) * 2.0 ** -24 * tm.item()      # torch's fp32 sum of count non-negative terms, any order
    none = torch.full_like(tg, float("inf"))
    x = tp.clone().requires_grad_()
    loss = s3r.DisparityLoss()(x, none)                              # a batch without a valid pixel: 0 and a zero gradient
    loss.backward()
    assert loss.item() == 0 and not x.grad.any()
