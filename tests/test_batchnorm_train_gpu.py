"""s3r_batchnorm_train_forward / s3r_batchnorm_train_backward on the device, through the C-ABI in guarded, poisoned buffers
(tests/_guard.py) unless stated.

Bit for bit against tests/_bn64.py's restatement of the header's order: save_mean, save_var, grad_beta, grad_gamma; y (none / ReLU) and
grad_z computed from the device's OWN save_mean and save_invstd.  save_invstd is bit for bit against float32(1) / sqrt(var + eps) of the
device's own var: the build's division and sqrtf are correctly rounded (hipcc's default without fast-math), and
test_random_data_bit_for_bit_and_against_float64 itself shows it on every case.  A sigmoid y is not restated bit for bit (the kernel's
exponential is the fast one): it is held to tests/_bn64.py's sigmoid_bound of the float64 sigmoid of the restated fp32 pre-activation,
and everything downstream is tied to the device's own y — the pattern of tests/test_voxel_loss_gpu.py for logf.

Within the derived bounds of float64 (tests/_bn64.py: forward64 for mean, var, invstd and y; backward64 for grad_z, grad_gamma and
grad_beta — a bound for grad_z IS derived there, so no measured tolerance is used for it in the C-ABI tests).  The autograd surface and
the decoder tail are compared with torch's float64 autograd under the convention of tests/test_decoder_training_gpu.py: torch's own
float32 CPU error times 8, the ReLU-gate window, the plain figures printed."""
import functools
import itertools

import numpy as np
import pytest
import torch

from tests import _bn64 as R
from tests import _guard as G

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32 = torch.float32
F = np.float32
ACT = {"none": 0, "relu": 1, "sigmoid": 2}
POISON = G._BITS[F32][2]
EPS = 1e-5
FACTOR = 8.0
_ids = lambda c: "x".join(map(str, c[0])) + "-" + c[1]
CASES = [(s, a) for s in R.SHAPES for a in R.ACTS]
BSIDES = ("grad_z", "grad_gamma", "grad_beta")


@pytest.fixture(scope="module")
def lib(s3r):
    return s3r.load_library()


def _rc(lib, rc, what):
    assert rc == 0, f"{what}: {lib.s3r_last_error().decode()} ({rc})"


def _same_bits(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.argwhere(R.bits(got) != R.bits(want))
    assert bad.size == 0, f"{what}: {len(bad)} elements differ, first at {tuple(bad[0])}: got {got[tuple(bad[0])]!r} want {want[tuple(bad[0])]!r}"


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=F))


def run_fwd(lib, z, gam, beta, act, fill="nan", eps=EPS):
    """one guarded forward call on numpy inputs z (B,C,S), gam / beta (C).  Returns (y, mean, var, invstd) as numpy"""
    B, ch, S = z.shape
    need = lib.s3r_batchnorm_train_forward_scratch_elems(B, ch, S)
    assert need > 0
    ins = [G.Guarded("z", (B, ch, S), F32, DEV, "in", data=_t(z)), G.Guarded("gamma", (ch,), F32, DEV, "in", data=_t(gam)),
           G.Guarded("beta", (ch,), F32, DEV, "in", data=_t(beta))]
    outs = [G.Guarded("y", (B, ch, S), F32, DEV, "out")] + [G.Guarded(n, (ch,), F32, DEV, "out") for n in ("save_mean", "save_var", "save_invstd")]
    scr = G.Guarded("scratch", (need,), F32, DEV, "scratch", fill=fill)
    _rc(lib, lib.s3r_batchnorm_train_forward(ins[0].ptr, ins[1].ptr, ins[2].ptr, eps, ACT[act], *[o.ptr for o in outs], B, ch, S, scr.ptr, need,
                                             None), "batchnorm forward")
    torch.cuda.synchronize()
    G.check_all(*ins, *outs)
    assert scr.check() is None, scr.check()
    return tuple(o.t.cpu().numpy() for o in outs)


def run_bwd(lib, z, y, gy, gam, mean, inv, act, need=(True, True, True), fill="nan", pass_y=True, pass_all=True):
    """one guarded backward call.  EVERY output buffer is allocated, poisoned and guarded; a side that is not asked for is passed as NULL and
    must still hold nothing but poison afterwards.  pass_all=False: the inputs the header allows to be NULL for this `need` are NULL"""
    B, ch, S = z.shape
    elems = lib.s3r_batchnorm_train_backward_scratch_elems(B, ch, S)
    assert elems > 0
    zb, gb_ = G.Guarded("z", (B, ch, S), F32, DEV, "in", data=_t(z)), G.Guarded("grad_y", (B, ch, S), F32, DEV, "in", data=_t(gy))
    yb = G.Guarded("y", (B, ch, S), F32, DEV, "in", data=_t(y)) if y is not None else None
    vec = {n: G.Guarded(n, (ch,), F32, DEV, "in", data=_t(v)) for n, v in (("gamma", gam), ("save_mean", mean), ("save_invstd", inv))}
    ins = [zb, gb_] + ([yb] if yb is not None else []) + list(vec.values())
    outs = [G.Guarded("grad_z", (B, ch, S), F32, DEV, "out"), G.Guarded("grad_gamma", (ch,), F32, DEV, "out"), G.Guarded("grad_beta", (ch,), F32, DEV, "out")]
    scr = G.Guarded("scratch", (elems,), F32, DEV, "scratch", fill=fill)
    sums = need[0] or need[1]                                     # grad_gamma or grad_z: z and the statistics are read
    p_z = zb.ptr if (pass_all or sums) else None
    p_m = vec["save_mean"].ptr if (pass_all or sums) else None
    p_i = vec["save_invstd"].ptr if (pass_all or sums) else None
    p_g = vec["gamma"].ptr if (pass_all or need[0]) else None
    p_y = yb.ptr if (yb is not None and pass_y) else None
    _rc(lib, lib.s3r_batchnorm_train_backward(p_z, p_y, gb_.ptr, p_g, p_m, p_i, ACT[act], *[o.ptr if n else None for o, n in zip(outs, need)],
                                              B, ch, S, scr.ptr, elems, None), "batchnorm backward")
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
    assert scr.check() is None, scr.check()
    return tuple(res)


@functools.lru_cache(maxsize=None)
def random_case(shape, act):
    """inputs (numpy) and the float64 forward reference, computed once per (shape, act) and shared (left unchanged)"""
    B, ch, S = shape
    rng = np.random.default_rng(B * 7919 + ch * 31 + S)
    z = (1.5 * rng.standard_normal(shape) + 0.5).astype(F)
    gam = (1.0 + 0.5 * rng.standard_normal(ch)).astype(F)
    beta = (0.3 * rng.standard_normal(ch)).astype(F)
    gy = rng.standard_normal(shape).astype(F)
    return z, gam, beta, gy, R.forward64(z, gam, beta, EPS, act)


@functools.lru_cache(maxsize=None)
def device_forward(shape, act):
    """the device's forward outputs for random_case(shape, act), computed once and shared by the backward tests"""
    import s3r
    z, gam, beta, _, _ = random_case(shape, act)
    return run_fwd(s3r.load_library(), z, gam, beta, act)


def _check_forward(z, gam, beta, act, got, f64, label):
    y, mean, var, inv = got
    rm, rv, _ = R.stats32(z, EPS)
    _same_bits(mean, rm, "save_mean")
    _same_bits(var, rv, "save_var")
    _same_bits(inv, R.invstd32(var, EPS), "save_invstd = float32(1) / sqrt(var + eps): correctly rounded division and sqrtf")
    want = R.y32(z, mean, inv, gam, beta, act)
    if act == "sigmoid":
        err, lim = np.abs(y.astype(np.float64) - want), R.sigmoid_bound(R.u32(z, mean, inv, gam, beta), want)
        print(f"{label} sigmoid y against the restated pre-activation: max err / bound {np.max(err / lim):.4f}")
        assert (err <= lim).all()
    else:
        _same_bits(y, want, "y from the device's own save_mean and save_invstd")
    for g, w, lim, name in ((mean, f64["mean"], f64["E_m"], "mean"), (var, f64["var"], f64["E_v"], "var"),
                            (inv, f64["invstd"], f64["E_i"], "invstd"), (y, f64["y"], f64["E_y"], "y")):
        err = np.abs(g.astype(np.float64) - w)
        print(f"{label} {name}: max err / bound {np.max(err / lim):.4f}")
        assert (err <= lim).all(), name


@pytest.mark.parametrize("case", CASES, ids=_ids)
def test_random_data_bit_for_bit_and_against_float64(lib, case):
    shape, act = case
    z, gam, beta, gy, f64 = random_case(shape, act)
    got = device_forward(shape, act)
    _check_forward(z, gam, beta, act, got, f64, f"{shape} {act}")
    y, mean, var, inv = got
    y_in = None if act == "none" else y
    gz, gg, gb = run_bwd(lib, z, y_in, gy, gam, mean, inv, act)
    rz, rg, rb = R.backward32(z, y_in, gy, gam, mean, inv, act)
    _same_bits(gb, rb, "grad_beta")
    _same_bits(gg, rg, "grad_gamma")
    _same_bits(gz, rz, "grad_z")
    b64 = R.backward64(z, y_in, gy, gam, mean, inv, act)
    for g, w, lim, name in ((gz, b64["grad_z"], b64["E_z"], "grad_z"), (gg, b64["grad_gamma"], b64["E_c"], "grad_gamma"), (gb, b64["grad_beta"], b64["E_b"], "grad_beta")):
        err = np.abs(g.astype(np.float64) - w)
        print(f"{shape} {act} {name}: max err / bound {np.max(err / lim):.4f}")
        assert (err <= lim).all(), name


# ---------------------------------------------------------------- integer lattices: every sum is exact in fp32 in any order
@pytest.mark.parametrize("act", ["none", "relu"])
@pytest.mark.parametrize("shape", [(2, 1, 1), (4, 3, 4), (1, 5, 512), (2, 3, 1024), (64, 2, 8)], ids=lambda s: "x".join(map(str, s)))
def test_integer_lattice_is_exact(lib, shape, act):
    """integer z with N a power of two and an integer mean: mean, var and both gradient sums are exact.  The mean is made an integer by
    mirroring: the second half of a channel's N values is 2 m - (the first half), so the sum is N m (N = 2: the pair m - k, m + k)"""
    B, ch, S = shape
    N = B * S
    assert N & (N - 1) == 0
    rng = np.random.default_rng(sum(shape))
    m = rng.integers(-3, 4, ch)
    half = rng.integers(-4, 5, (ch, N // 2))
    rows = np.concatenate([m[:, None] + half, m[:, None] - half], axis=1)                     # (C, N)
    z = rows.reshape(ch, B, S).transpose(1, 0, 2).astype(F)
    gam, beta = rng.integers(-2, 3, ch).astype(F), rng.integers(-2, 3, ch).astype(F)
    gy = rng.integers(-4, 5, shape).astype(F)
    y, mean, var, inv = run_fwd(lib, z, gam, beta, act)
    z64 = z.astype(np.float64)
    assert np.array_equal(mean.astype(np.float64), m.astype(np.float64)), "mean"
    var64 = ((z64 - m[None, :, None]) ** 2).sum(axis=(0, 2)) / N                               # integers below 2^24 over a power of two
    assert np.array_equal(var.astype(np.float64), var64), "var"
    _same_bits(inv, R.invstd32(var, EPS), "invstd")
    # the backward on exact inputs: invstd = 1 and mean = m handed in, so xhat = z - m is an integer and both sums are exact
    one = np.ones(ch, F)
    yy = R.y32(z, mean, one, gam, beta, act)
    y_in = None if act == "none" else yy
    _, gg, gb = run_bwd(lib, z, y_in, gy, gam, mean, one, act, need=(False, True, True))
    g64 = R.g32(y_in, gy, act).astype(np.float64)
    assert np.array_equal(gb.astype(np.float64), g64.sum(axis=(0, 2))), "grad_beta"
    assert np.array_equal(gg.astype(np.float64), (g64 * (z64 - m[None, :, None])).sum(axis=(0, 2))), "grad_gamma"
    assert np.abs(g64).sum() * 8 < 2 ** 24


# ---------------------------------------------------------------- the cancellation data set on the device
@pytest.mark.parametrize("shape", R.CANCEL, ids=lambda s: "x".join(map(str, s)))
def test_cancellation_data_on_the_device(lib, shape):
    z = R.cancel_data(shape, 0)
    ch = shape[1]
    _, mean, var, _ = run_fwd(lib, z, np.ones(ch, F), np.zeros(ch, F), "none")
    rm, rv, _ = R.stats32(z, EPS)
    _same_bits(mean, rm, "save_mean")
    _same_bits(var, rv, "save_var")
    var64 = z.astype(np.float64).var(axis=(0, 2))
    rel = np.abs(var - var64) / var64
    one = np.abs(R.one_pass_var32(z) - var64) / var64
    print(f"{shape}: device two-pass rel err {rel.max():.3e}; the one-pass mutant {one.min():.3e}")
    assert (rel <= 1e-5).all() and (one > 1e-2).all()


# ---------------------------------------------------------------- the NULL forms
SUBSETS = [s for s in itertools.product((True, False), repeat=3) if any(s) and not all(s)]


@pytest.mark.parametrize("case", [((2, 5, 5), "relu"), ((3, 5, 513), "sigmoid"), ((2, 3, 1029), "none"), ((65, 3, 5), "relu")], ids=_ids)
def test_null_outputs_same_bits_and_untouched(lib, case):
    shape, act = case
    z, gam, beta, gy, _ = random_case(shape, act)
    y, mean, var, inv = device_forward(shape, act)
    y_in = None if act == "none" else y
    full = run_bwd(lib, z, y_in, gy, gam, mean, inv, act)
    for need in SUBSETS:
        part = run_bwd(lib, z, y_in, gy, gam, mean, inv, act, need=need, pass_all=False)
        for got, want, n, name in zip(part, full, need, BSIDES):
            assert (got is None) == (not n)
            if n:
                _same_bits(got, want, f"{name} with need={need}")
    if act == "none":                                             # y may be NULL when act is none: the same bits
        for got, want, name in zip(run_bwd(lib, z, np.zeros_like(z), gy, gam, mean, inv, act, pass_y=False), full, BSIDES):
            _same_bits(got, want, f"{name}, y = NULL")


# ---------------------------------------------------------------- invariances
INV = [((2, 5, 5), "sigmoid"), ((3, 5, 513), "relu"), ((2, 3, 1029), "none"), ((65, 3, 5), "relu"), ((1, 5, 512), "sigmoid")]
FORDER = ["z", "gamma", "beta", "y", "save_mean", "save_var", "save_invstd", "scratch", "grad_y", "grad_z", "grad_gamma", "grad_beta"]


@pytest.mark.parametrize("case", INV, ids=_ids)
def test_runs_addresses_and_scratch_contents_do_not_matter(lib, case):
    shape, act = case
    z, gam, beta, gy, _ = random_case(shape, act)
    fbase = device_forward(shape, act)
    y, mean, var, inv = fbase
    y_in = None if act == "none" else y
    bbase = run_bwd(lib, z, y_in, gy, gam, mean, inv, act)
    fnames = ("y", "save_mean", "save_var", "save_invstd")

    def both(label, **kw):
        for a, b, n in zip(run_fwd(lib, z, gam, beta, act, **kw), fbase, fnames):
            _same_bits(a, b, f"{n}, {label}")
        for a, b, n in zip(run_bwd(lib, z, y_in, gy, gam, mean, inv, act, **kw), bbase, BSIDES):
            _same_bits(a, b, f"{n}, {label}")

    both("second run")
    both("zero-filled scratch", fill="zero")
    for label, sk in (("every argument + 1 element", lambda name, dtype, role: 1),
                      ("arguments at 1, 2, 3, ... elements", lambda name, dtype, role: 1 + FORDER.index(name) % 3)):
        with G.skews(sk):
            both(label)


# ---------------------------------------------------------------- non-finite input stays in its channel
@pytest.mark.parametrize("bad", [float("nan"), float("inf")], ids=["nan", "inf"])
def test_a_non_finite_z_poisons_its_channel_only(lib, bad):
    shape, act = (3, 5, 513), "relu"
    z, gam, beta, gy, _ = random_case(shape, act)
    y0, mean0, var0, inv0 = device_forward(shape, act)
    gz0, gg0, gb0 = run_bwd(lib, z, y0, gy, gam, mean0, inv0, act)
    zz = z.copy()
    zz[1, 2, 300] = bad
    y, mean, var, inv = run_fwd(lib, zz, gam, beta, act)
    gz, gg, gb = run_bwd(lib, zz, y, gy, gam, mean, inv, act)
    keep = [c for c in range(5) if c != 2]
    assert not np.isfinite(mean[2]) and np.isnan(var[2]) and np.isnan(inv[2]) and np.isnan(y[:, 2]).all()      # (the mean of an inf is inf)
    assert np.isnan(gg[2]) and np.isnan(gz[:, 2]).all()
    for a, b, n in ((mean, mean0, "mean"), (var, var0, "var"), (inv, inv0, "invstd"), (gg, gg0, "grad_gamma"), (gb, gb0, "grad_beta")):
        _same_bits(a[keep], b[keep], n)
    _same_bits(y[:, keep], y0[:, keep], "y")
    _same_bits(gz[:, keep], gz0[:, keep], "grad_z")


# ---------------------------------------------------------------- refused calls
def test_refused_calls_leave_outputs_and_guards_untouched(lib):
    shape, act = (2, 5, 5), "relu"
    B, ch, S = shape
    z, gam, beta, gy, _ = random_case(shape, act)
    nf, nb = lib.s3r_batchnorm_train_forward_scratch_elems(B, ch, S), lib.s3r_batchnorm_train_backward_scratch_elems(B, ch, S)
    ins = {n: G.Guarded(n, v.shape, F32, DEV, "in", data=_t(v)) for n, v in (("z", z), ("gamma", gam), ("beta", beta), ("grad_y", gy), ("y", np.abs(z)),
                                                                            ("save_mean", beta), ("save_invstd", gam))}
    outs = {n: G.Guarded(n, s, F32, DEV, "out") for n, s in (("y_out", shape), ("m", (ch,)), ("v", (ch,)), ("i", (ch,)), ("grad_z", shape),
                                                             ("grad_gamma", (ch,)), ("grad_beta", (ch,)))}
    scr = G.Guarded("scratch", (max(nf, nb),), F32, DEV, "scratch")
    I, O = {n: b.ptr for n, b in ins.items()}, {n: b.ptr for n, b in outs.items()}

    def fwd(act=1, B=B, S=S, elems=nf, y=O["y_out"], scratch=scr.ptr):
        return lib.s3r_batchnorm_train_forward(I["z"], I["gamma"], I["beta"], EPS, act, y, O["m"], O["v"], O["i"], B, ch, S, scratch, elems, None)

    def bwd(act=1, B=B, S=S, elems=nb, outs_=(O["grad_z"], O["grad_gamma"], O["grad_beta"]), y=I["y"], scratch=scr.ptr):
        return lib.s3r_batchnorm_train_backward(I["z"], y, I["grad_y"], I["gamma"], I["save_mean"], I["save_invstd"], act, *outs_, B, ch, S, scratch,
                                                elems, None)

    assert fwd(act=3) == -1 and bwd(act=5) == -1
    assert fwd(B=1, S=1) == -1 and bwd(B=1, S=1) == -1                        # N < 2
    assert fwd(elems=nf - 1) == -3 and bwd(elems=nb - 1) == -3 and fwd(scratch=None) == -3 and bwd(scratch=None) == -3
    assert fwd(y=None) == -1
    assert bwd(outs_=(None, None, None)) == -1
    assert bwd(y=None) == -1                                                   # ReLU needs y
    assert fwd(B=0) == 0 and bwd(B=0) == 0                                     # nothing launched, nothing written
    torch.cuda.synchronize()
    G.check_all(*ins.values())
    for o in outs.values():
        o.role = "scratch"
        G.check_all(o)
        assert bool((G._as_bits(o.t) == POISON).all()), f"a refused call wrote {o.name}"
    assert scr.check() is None and bool((G._as_bits(scr.t) == G._BITS[F32][4]).all()), "a refused call wrote the scratch"


def test_profiler_records(s3r, lib):
    B, ch, n = 2, 6, 8
    T = B * ch * n ** 3
    z, gy = torch.randn(B, ch, n, n, n, device=DEV), torch.randn(B, ch, n, n, n, device=DEV)
    gam, beta = torch.rand(ch, device=DEV) + 0.5, torch.rand(ch, device=DEV)
    s3r.profile_enable(16)
    try:
        y, mean, var, inv = s3r.batchnorm_train_forward(z, gam, beta, EPS, "relu")
        s3r.batchnorm_train_backward(z, y, gy, gam, mean, inv, "relu")
        s3r.batchnorm_train_backward(z, None, gy, gam, mean, inv, "none", need_z=False)
        s3r.batchnorm_train_backward(z, None, gy, gam, mean, inv, "none", need_z=False, need_gamma=False)
        torch.cuda.synchronize()
        rec = s3r.profile_read(16)
    finally:
        s3r.profile_enable(0)
    assert [(r["family"], r["tag"], r["launches"]) for r in rec] == [("head", 2, 5), ("head", 3, 3), ("head", 3, 2), ("head", 3, 2)]
    assert all(r["ms"] > 0 and r["flops"] == 0 for r in rec)
    assert rec[0]["bytes"] == 4.0 * (4 * T + 5 * ch) and rec[1]["bytes"] == 4.0 * (7 * T + 5 * ch)
    assert rec[2]["bytes"] == 4.0 * (2 * T + 4 * ch) and rec[3]["bytes"] == 4.0 * (T + ch)


# ---------------------------------------------------------------- the autograd surface
def _rel(a, ref):
    return ((a.double() - ref).norm() / ref.norm()).item()


@pytest.mark.parametrize("momentum", [0.1, None], ids=["momentum-0.1", "cumulative"])
@pytest.mark.parametrize("act", ["none", "sigmoid"])
def test_differentiable_batchnorm_against_torch_float64(s3r, lib, monkeypatch, act, momentum):
    """(3, 5, 6^3) against nn.BatchNorm3d in training mode in float64; tolerance: torch's own float32 CPU result's error times 8 (the
    convention of tests/test_decoder_training_gpu.py; act none / sigmoid have no gate).  After one call (two for the cumulative average)
    the running statistics and num_batches_tracked are torch's."""
    g = torch.Generator().manual_seed(7)
    z0 = 1.5 * torch.randn(3, 5, 6, 6, 6, generator=g) + 0.5
    gy = torch.randn(3, 5, 6, 6, 6, generator=g)
    w0, b0 = 1 + 0.5 * torch.randn(5, generator=g), 0.3 * torch.randn(5, generator=g)
    rm0, rv0 = torch.randn(5, generator=g), torch.rand(5, generator=g) + 0.5
    f = {"none": lambda t: t, "sigmoid": torch.sigmoid}[act]

    def make(dtype, dev):
        bn = torch.nn.BatchNorm3d(5, eps=EPS, momentum=momentum).to(dtype)
        with torch.no_grad():
            bn.weight.copy_(w0), bn.bias.copy_(b0), bn.running_mean.copy_(rm0), bn.running_var.copy_(rv0)
        return bn.to(dev).train()

    def torch_pass(dtype, calls):
        bn, z = make(dtype, "cpu"), z0.clone().to(dtype).requires_grad_()          # (a copy: .to(float32) of a float32 tensor is the tensor itself)
        for _ in range(calls - 1):
            bn(z.detach())
        y = f(bn(z))
        y.backward(gy.to(dtype))
        return y.detach(), z.grad, bn

    calls = 2 if momentum is None else 1
    y64, gz64, bn64 = torch_pass(torch.float64, calls)
    y32, gz32, bn32 = torch_pass(torch.float32, calls)
    seen = []
    real = lib.s3r_batchnorm_train_backward
    monkeypatch.setattr(lib, "s3r_batchnorm_train_backward", lambda *a: (seen.append(tuple(p is not None for p in a[7:10])), real(*a))[1])
    bn = make(torch.float32, DEV).eval()                           # batch statistics whatever bn.training says
    z = z0.to(DEV).requires_grad_()
    for _ in range(calls - 1):
        s3r.differentiable_batchnorm(z.detach(), bn, act)
    y = s3r.differentiable_batchnorm(z, bn, act)
    assert y.shape == z.shape and y.grad_fn is not None
    y.backward(gy.to(DEV))
    torch.cuda.synchronize()
    assert seen == [(True, True, True)]
    assert bn.weight.grad is not None and bn.bias.grad is not None and bn.weight.grad.shape == (5,)
    for name, got, r64, r32 in (("y", y.detach(), y64, y32), ("grad_z", z.grad, gz64, gz32), ("bn.weight.grad", bn.weight.grad, bn64.weight.grad, bn32.weight.grad),
                                ("bn.bias.grad", bn.bias.grad, bn64.bias.grad, bn32.bias.grad), ("running_mean", bn.running_mean, bn64.running_mean, bn32.running_mean),
                                ("running_var", bn.running_var, bn64.running_var, bn32.running_var)):
        hip, cpu = _rel(got.cpu(), r64), _rel(r32, r64)
        print(f"{act} {name}: HIP {hip:.3e}, torch float32 on the CPU {cpu:.3e}, ratio {hip / max(cpu, 1e-30):.2f}")
        assert hip <= FACTOR * max(cpu, 2.0 ** -24), name          # (floor: one fp32 rounding, where torch's float32 happens to be exact)
    assert int(bn.num_batches_tracked) == int(bn64.num_batches_tracked) == calls
    # exactly the sides needs_input_grad asks for, and the same bits as the full call
    want = (z.grad, bn.weight.grad, bn.bias.grad)
    for need in [(False, True, True), (True, False, False), (False, False, True)]:
        seen.clear()
        bn2 = make(torch.float32, DEV)
        bn2.weight.requires_grad_(need[1]), bn2.bias.requires_grad_(need[2])
        z2 = z0.to(DEV).requires_grad_(need[0])
        for _ in range(calls - 1):
            s3r.differentiable_batchnorm(z2.detach(), bn2, act)
        s3r.differentiable_batchnorm(z2, bn2, act).backward(gy.to(DEV))
        assert seen == [need]
        for t, n, w in zip((z2, bn2.weight, bn2.bias), need, want):
            assert (t.grad is not None) == n
            if n:
                assert torch.equal(t.grad.view(torch.int32), w.view(torch.int32))
    with pytest.raises(RuntimeError):
        s3r.differentiable_batchnorm(torch.zeros(1, 5, 1, 1, 1, device=DEV), bn, act)       # N < 2


# ---------------------------------------------------------------- the decoder tail with batch statistics
@functools.lru_cache(maxsize=None)
def _tail_problem():
    import s3r
    state = s3r.seeded_state_dict(s3r.Decoder(), seed=4)
    g = torch.Generator().manual_seed(9)
    x = torch.relu(torch.randn(2, 128, 16, 16, 16, generator=g))               # d3's input is a ReLU output
    gt = (torch.rand(2, 32, 32, 32, generator=g) < 0.3).float()
    return state, x, gt


def _decoder(s3r):
    dec = s3r.Decoder()
    dec.load_state_dict(_tail_problem()[0])
    return dec.to(DEV)


D3 = ["d3.conv.weight", "d3.conv.bias", "d3.bn.weight", "d3.bn.bias", "d4.conv.weight", "d4.conv.bias"]


def test_tail_with_batch_stats_against_float64_autograd(s3r, oracle):
    """Decoder.differentiable_tail(x, batch_stats=True) at B = 2 under VoxelBCELoss: every gradient, d3.bn.weight's included, against
    float64 autograd of the stock torch modules with d3's BatchNorm in training mode.  Tolerance and ReLU-gate window as
    tests/test_decoder_training_gpu.py: FACTOR = 8 times torch's float32 CPU error; a gate whose float64 pre-activation lies within
    E (per channel, 8 times the float32 pre-activation's error) of zero takes the device's side; the plain figures are printed.
    d3.conv.bias is the exception: a bias in front of a batch-statistics BatchNorm has NO gradient — the mean subtraction removes it,
    sum_{b,s} grad_z = 0 in real arithmetic whatever grad_y is; float64 gives 1e-16 — so a relative error means nothing there.  What the
    device returns is the rounding of that sum: N = B S = 65536 fp32 terms per channel added in some order, each term itself rounded a
    few times, so it is held to tests/_linear64.py's any-order bound32(N, sum |dL/dz|) with the float64 magnitudes."""
    state, x, gt = _tail_problem()
    dec = _decoder(s3r)
    xd = x.to(DEV).requires_grad_()
    feats = dec.differentiable_features(xd, batch_stats=True)
    loss = s3r.VoxelBCELoss()(dec.differentiable_head(feats), gt.to(DEV))
    loss.backward()
    torch.cuda.synchronize()
    params = dict(dec.named_parameters())
    assert sorted(n for n, p in params.items() if p.grad is not None) == sorted(D3)
    gates = (feats.detach() > 0).cpu()

    def reference(dtype, pre32=None):
        """(pre-activation, [(loss, gradients)] plain (and gate-mended when pre32 is given), E, gate counts)"""
        orc = oracle.OracleDecoder().eval()
        orc.load_state_dict(state)
        orc = orc.to(dtype)
        orc.d3.bn.train()
        a = x.to(dtype).clone().requires_grad_()
        zc = orc.d3.conv(a)
        zc.retain_grad()
        t = orc.d3.bn(zc)
        tail = lambda h: torch.nn.BCELoss()(orc.d4(h).squeeze(1), gt.to(dtype))
        own = t.detach() > 0
        heads, E, counts = [torch.relu(t)], None, None
        if pre32 is not None:
            E = FACTOR * (pre32.double() - t.detach()).abs().amax(dim=(0, 2, 3, 4), keepdim=True)
            near, differ = t.detach().abs() <= E, own != gates
            counts = (int(near.sum()), int((differ & near).sum()), int((differ & ~near).sum()), t.numel())
            heads.append(t * torch.where(near, gates, own).to(dtype))
        out = []
        for h in heads:
            orc.zero_grad()
            a.grad = None
            l = tail(h)
            l.backward(retain_graph=True)
            grads = {n: p.grad.clone() for n, p in orc.named_parameters() if n in D3}
            grads["x"] = a.grad.clone()
            grads["|dL/dz|"] = zc.grad.abs().sum(dim=(0, 2, 3, 4))
            zc.grad = None
            out.append((l.item(), grads))
        return t.detach(), out, E, counts

    pre32, [(l32, g32)], _, _ = reference(torch.float32)
    _, [(l64, g64), (_, m64)], E, (near, inside, outside, total) = reference(torch.float64, pre32)
    print(f"loss {loss.item():.7g}; float64 {l64:.7g}; float32 on the CPU {l32:.7g}")
    print(f"d3: E {E.min().item():.3e} .. {E.max().item():.3e} by channel; {near} of {total} pre-activations within E of zero, {inside} of them "
          f"gated the other way; {outside} gates differ outside")
    assert outside == 0 and near <= 1e-3 * total
    got = {n: params[n].grad for n in D3}
    got["x"] = xd.grad
    bad = []
    cb, lim = got["d3.conv.bias"].cpu().double().abs(), R.bound32(2 * 32 ** 3, m64["|dL/dz|"].numpy())
    print(f"d3.conv.bias (no gradient behind batch statistics): max |HIP| {cb.max().item():.3e}, max |HIP| / bound {(cb.numpy() / lim).max():.3e}; "
          f"float64 {g64['d3.conv.bias'].abs().max().item():.3e}, torch float32 on the CPU {g32['d3.conv.bias'].abs().max().item():.3e}; "
          f"|d3.bn.bias.grad| max {g64['d3.bn.bias'].abs().max().item():.3e}")
    assert (cb.numpy() <= lim).all()
    for n in ["x"] + [n for n in D3 if n != "d3.conv.bias"]:
        hip, cpu, raw = _rel(got[n].cpu(), m64[n]), _rel(g32[n], g64[n]), _rel(got[n].cpu(), g64[n])
        print(f"{n}: HIP {hip:.3e} (unmended float64: {raw:.3e}), torch float32 on the CPU {cpu:.3e}, ratio {hip / cpu:.2f}")
        assert g64[n].norm().item() > 0 and cpu < 1e-2, n
        if not hip <= FACTOR * cpu:
            bad.append((n, hip, cpu))
    assert not bad, bad


def test_three_sgd_steps_with_batch_stats_are_deterministic(s3r):
    _, x, gt = _tail_problem()
    xd, gtd = x.to(DEV), gt.to(DEV)

    def three_steps():
        dec = _decoder(s3r)
        params = dict(dec.named_parameters())
        opt = torch.optim.SGD([params[n] for n in D3], lr=0.05)
        bce = s3r.VoxelBCELoss()
        losses = []
        for _ in range(3):
            opt.zero_grad()
            loss = bce(dec.differentiable_tail(xd, batch_stats=True), gtd)
            loss.backward()
            opt.step()
            losses.append(loss.item())
        out = {n: p.detach().clone() for n, p in dec.named_parameters()}
        out.update({n: b.detach().clone().float() for n, b in dec.named_buffers() if n.startswith("d3.bn.")})
        return out, losses

    a, la = three_steps()
    b, lb = three_steps()
    print(f"losses {la}")
    assert la == lb and all(np.isfinite(la))
    state = _tail_problem()[0]
    for n in a:
        assert torch.equal(a[n].view(torch.int32), b[n].view(torch.int32)), n
    # (d3.conv.bias has no gradient behind batch statistics beyond the rounding of a sum that is zero: it is not asked to move)
    for n in [m for m in D3 if m != "d3.conv.bias"] + ["d3.bn.running_mean", "d3.bn.running_var"]:
        assert not torch.equal(a[n].cpu(), state[n].float()), f"{n} did not move"
    assert int(a["d3.bn.num_batches_tracked"]) == 3
    with pytest.raises(RuntimeError):
        _decoder(s3r).train()                                      # the fused inference path has no batch-statistics form


def test_tail_without_batch_stats_is_the_folded_path_bit_for_bit(s3r):
    """batch_stats=False (and the default) against the folded loop written out here as it stood before the keyword existed:
    differentiable_conv on folded()'s scale and the torch-evaluated shift, then differentiable_head"""
    _, x, gt = _tail_problem()
    gtd = gt.to(DEV)
    res = []
    for how in ("default", "false", "written out"):
        dec = _decoder(s3r)
        xd = x.to(DEV).requires_grad_()
        if how == "written out":
            blk = dec.d3
            scale, _ = blk.folded()
            shift = blk.bn.bias + (blk.conv.bias - blk.bn.running_mean.detach()) * scale
            occ = dec.differentiable_head(s3r.differentiable_conv(xd, blk.conv.weight, scale, shift, blk.layer))
        else:
            occ = dec.differentiable_tail(xd) if how == "default" else dec.differentiable_tail(xd, batch_stats=False)
        s3r.VoxelBCELoss()(occ, gtd).backward()
        torch.cuda.synchronize()
        out = {"occ": occ.detach(), "x": xd.grad}
        for n, p in dec.named_parameters():
            assert (p.grad is None) == (not n.startswith(("d3.", "d4.")) or n == "d3.bn.weight"), n
            if p.grad is not None:
                out[n] = p.grad
        assert int(dec.d3.bn.num_batches_tracked) == 0
        res.append(out)
    for other in res[1:]:
        assert set(other) == set(res[0])
        for n in res[0]:
            assert torch.equal(res[0][n].view(torch.int32), other[n].view(torch.int32)), n
