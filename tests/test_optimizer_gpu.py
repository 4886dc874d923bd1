"""s3r_optim_step on the device, bit for bit against tests/_optim64.py's fp32 restatement: five steps of every rule and flag combination
on the shared tensor list (the chunk, workgroup and ragged-tail boundaries; every pointer only 4-byte aligned, each at its own offset) in
guarded buffers — parameters, moments, all eight state dwords, the gradients unchanged, the guards intact —, the launch boundaries (63,
64, 65 and 129 tensors against a restatement that knows nothing of launches), a tensor alone against the same tensor inside a list, run,
address and scratch-content invariance, a planted NaN with and without the norm, and the Python classes (against the C-ABI's bits, the
state_dict round trip, `_version`, a parameter without a gradient, every ValueError)."""
import ctypes as C
import re
import os

import numpy as np
import pytest
import torch

from tests import _guard as G
from tests import _optim64 as R
from tests.test_optimizer_cpu import NAN_AT

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32 = torch.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib(s3r):
    return s3r.load_library()


def _tpl():
    with open(os.path.join(ROOT, "include", "s3r.h")) as f:
        return int(re.search(r"#define S3R_OPTIM_TENSORS_PER_LAUNCH (\d+)", f.read()).group(1))


def _guards_intact(b):
    bits, guard = G._as_bits(b.raw), G._BITS[b.dtype][1]
    assert bool((bits[:b.g] == guard).all()) and bool((bits[b.g + b.n:] == guard).all()), f"a guard of {b.name} was written"


def _desc(L, d):
    return L.OptimDesc(L.OPT_SGD if d.kind == "sgd" else L.OPT_ADAM, d.flags, d.beta1, d.beta2 if d.kind == "adam" else 0.0,
                       d.eps if d.kind == "adam" else 0.0, d.wd, d.clip or 0.0)


def run_device(s3r, lib, d, sizes=R.SIZES, seed=0, steps=R.STEPS, lr=R.LR, nan_at=None, fill="nan", skew_seed=1, ts0=None, gs_of=None,
               captured=False):
    """`steps` steps of the C-ABI on guarded buffers; returns [(ts, state words)] after each step, as tests/_optim64.run32 does.
    captured: the step is captured ONCE into a graph on a side stream (one torch.cuda.Stream) and every step is a replay of it"""
    L = s3r._lib
    ts0 = R.tensor_list(sizes, seed, nan_m=d.kind == "sgd") if ts0 is None else ts0
    gs_of = (lambda k: R.grads(sizes, seed, k)) if gs_of is None else gs_of
    rng = np.random.default_rng(skew_seed if skew_seed is not None else 0)
    bufs = []
    for i, t in enumerate(ts0):
        n = t["p"].size
        b = {}
        for k in ("p", "m", "v", "g"):
            skew = int(rng.integers(0, 2)) if skew_seed is not None else 0       # each of the four pointers at its own offset 0 or 1
            b[k] = G.Guarded(f"{k}{i}", n, F32, DEV, "in", data=torch.from_numpy(t[k]) if k != "g" else torch.zeros(n), skew=skew)
        bufs.append(b)
    state = G.Guarded("state", 8, F32, DEV, "out")
    scratch = G.Guarded("scratch", R.scratch_elems([t["p"].size for t in ts0]), F32, DEV, "scratch", fill=fill)
    arr = (L.OptimTensor * len(bufs))(*[L.OptimTensor(b["p"].ptr, b["g"].ptr, b["m"].ptr if d.has_m else None,
                                                      b["v"].ptr if d.has_v else None, b["p"].n) for b in bufs])
    assert lib.s3r_optim_scratch_elems(arr, len(bufs)) == scratch.n
    desc = _desc(L, d)
    assert lib.s3r_optim_state_init(state.ptr, lr, None) == 0, lib.s3r_last_error()
    out, graph = [], None
    if captured:
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=torch.cuda.Stream()):
            rc = lib.s3r_optim_step(C.byref(desc), arr, len(bufs), state.ptr, scratch.ptr if d.with_norm else None, scratch.n,
                                    torch.cuda.current_stream().cuda_stream)
        assert rc == 0, lib.s3r_last_error()
        arr = desc = None                                     # the host array and descriptor were read during the call only
    for k in range(steps):
        gs = gs_of(k)
        if nan_at is not None and nan_at[0] == k:
            gs[nan_at[1]][nan_at[2]] = np.nan
        for b, g in zip(bufs, gs):
            b["g"].t.copy_(torch.from_numpy(g))
            b["g"].snapshot = G._as_bits(b["g"].t).clone()
        if graph is not None:
            torch.cuda.synchronize()
            graph.replay()
        else:
            rc = lib.s3r_optim_step(C.byref(desc), arr, len(bufs), state.ptr, scratch.ptr if d.with_norm else None, scratch.n, None)
            assert rc == 0, lib.s3r_last_error()
        torch.cuda.synchronize()
        out.append(([{key: b[key].t.cpu().numpy() for key in "pmv"} for b in bufs], state.t.view(torch.int32).cpu().numpy()))
    for b in bufs:
        G.check_all(b["g"])                                   # grad unchanged, its guards intact
        for key in "pmv":
            _guards_intact(b[key])
        if not d.has_m:
            G.check_all(b["m"])                               # ... and a moment the rule does not own is never written
        if not d.has_v:
            G.check_all(b["v"])
    G.check_all(state)
    _guards_intact(scratch)
    return out


def _compare(got, want, d, what):
    assert len(got) == len(want)
    for k, ((gt, gw), (wt, wst)) in enumerate(zip(got, want)):
        R.assert_same(gt, gw, wt, wst, d, f"{what} step {k}:")


# ---------------------------------------------------------------- every rule and flag combination
@pytest.mark.parametrize("case", list(R.CASES))
def test_five_steps_bit_for_bit(s3r, lib, case):
    """the skip cases carry a NaN in step 2's gradient: that step changes no bit but `skipped` (and the norm it reports), and steps 3
    and 4 continue as if it never happened — the restatement does exactly that"""
    d = R.CASES[case]
    nan_at = NAN_AT if d.skip else None
    want = R.run32(d, nan_at=nan_at)
    got = run_device(s3r, lib, d, nan_at=nan_at)
    _compare(got, want, d, case)
    if d.skip:
        (t1, w1), (t2, w2) = got[1], got[2]
        assert w2[6] == w1[6] + 1 and (w2[:4] == w1[:4]).all() and np.isnan(w2[4:5].view(np.float32))[0]
        for a, b in zip(t1, t2):
            assert all((R.bits(a[k]) == R.bits(b[k])).all() for k in "pmv")
        clean = R.run32(d, steps=R.STEPS - 1, nan_at=None)     # (different gradients from step 2 on: only the counters are compared)
        assert got[-1][1][0] == clean[-1][1]["step"]


# ---------------------------------------------------------------- launch boundaries
@pytest.mark.parametrize("extra", [-1, 0, 1, None], ids=["tpl-1", "tpl", "tpl+1", "2tpl+1"])
def test_launch_boundaries(s3r, lib, extra):
    """one under, at and one over S3R_OPTIM_TENSORS_PER_LAUNCH, and two full launches and a third: the restatement knows nothing of
    launches, so the norm's bits (state dword 4) and every tensor's depend on the list only"""
    tpl = _tpl()
    n = 2 * tpl + 1 if extra is None else tpl + extra
    sizes = R.boundary_sizes(n)
    for case in ("adam-clip_skip", "sgd_momentum-plain"):
        d = R.CASES[case]
        _compare(run_device(s3r, lib, d, sizes, seed=n, steps=2), R.run32(d, sizes, seed=n, steps=2), d, f"{case} x {n} tensors")


def test_the_two_paths_of_the_ordered_total(s3r, lib):
    """the advance launch adds a tensor's chunk sums by one lane up to 128 of them and by the whole wave above (64 per load): the same
    order either way.  128 and 129 chunks, 192 (whole loads only), 200 with a ragged last chunk, beside a tensor of one chunk"""
    sizes = (65536, 3, 65537, 98304, 102395)
    assert [-(-n // 512) for n in sizes] == [128, 1, 129, 192, 200]
    for case in ("adam-clip_skip", "sgd-clip"):
        d = R.CASES[case]
        _compare(run_device(s3r, lib, d, sizes, seed=3, steps=2), R.run32(d, sizes, seed=3, steps=2), d, case)


def test_a_tensor_alone_and_inside_a_list(s3r, lib):
    """without clipping nothing couples the tensors: each of three stepped alone has the bits it has inside the list"""
    for case in ("adamw-plain", "sgd_nesterov_wd-plain"):
        d = R.CASES[case]
        ts0 = R.tensor_list(nan_m=d.kind == "sgd")
        inside = run_device(s3r, lib, d, steps=2)
        for i in (0, 5, 9):
            alone = run_device(s3r, lib, d, steps=2, ts0=[ts0[i]], gs_of=lambda k, i=i: [R.grads(step=k)[i]], skew_seed=7 + i)
            for (ta, wa), (tl, wl) in zip(alone, inside):
                assert all((R.bits(ta[0][k]) == R.bits(tl[i][k])).all() for k in "pmv"), (case, i)
                assert (wa == wl).all()


def test_run_address_and_scratch_invariance(s3r, lib):
    for case in ("adam-clip", "sgd_momentum-clip_skip"):
        d = R.CASES[case]
        base = run_device(s3r, lib, d, steps=3, skew_seed=None, fill="zero")            # every pointer 256-byte aligned, zero scratch
        for kw in (dict(skew_seed=None, fill="zero"), dict(skew_seed=11, fill="nan"), dict(skew_seed=12, fill="zero")):
            other = run_device(s3r, lib, d, steps=3, **kw)
            for (ta, wa), (tb, wb) in zip(base, other):
                assert (wa == wb).all(), (case, kw)
                for a, b in zip(ta, tb):
                    assert all((R.bits(a[k]) == R.bits(b[k])).all() for k in "pmv"), (case, kw)


@pytest.mark.parametrize("case", ["adam-plain", "sgd_momentum-plain", "sgd-plain"])
def test_a_nan_gradient_without_the_norm_poisons_its_own_element_only(s3r, lib, case):
    d = R.CASES[case]
    got = run_device(s3r, lib, d, nan_at=NAN_AT)
    _compare(got, R.run32(d, nan_at=NAN_AT), d, case)
    clean = R.run32(d)
    _, ti, ei = NAN_AT
    for (gt, gw), (ct, cst) in zip(got, clean):
        assert (gw == R.state_words(cst)).all()
        for i, (a, b) in enumerate(zip(gt, ct)):
            for k in ("p",) + (("m",) if d.has_m else ()) + (("v",) if d.has_v else ()):
                diff = np.flatnonzero(R.bits(a[k]) != R.bits(b[k]))
                assert diff.size == 0 or (i == ti and diff.tolist() == [ei]), (case, i, k, diff[:4])
    assert np.isnan(got[-1][0][ti]["p"][ei])


# ---------------------------------------------------------------- the Python classes
def _make(s3r, case, sizes, seed=0, **kw):
    d = R.CASES[case]
    ts0 = R.tensor_list(sizes, seed)
    params = [torch.nn.Parameter(torch.from_numpy(t["p"]).to(DEV)) for t in ts0]
    common = dict(lr=R.LR, weight_decay=d.wd, clip_grad_norm=d.clip, skip_nonfinite=d.skip, **kw)
    if d.kind == "sgd":
        opt = s3r.SGD(params, momentum=d.beta1, nesterov=d.nesterov, **common)
    else:
        opt = (s3r.AdamW if d.decoupled else s3r.Adam)(params, betas=(d.beta1, d.beta2), eps=d.eps, **common)
    return d, ts0, params, opt


def _read(opt, params, d):
    names = ("momentum_buffer", None) if d.kind == "sgd" else ("exp_avg", "exp_avg_sq")
    ts = []
    for p in params:
        st = opt.state[p]
        ts.append(dict(p=p.detach().cpu().numpy(), m=st[names[0]].cpu().numpy() if d.has_m else None,
                       v=st[names[1]].cpu().numpy() if d.has_v else None))
    return ts, opt.device_state(0).cpu().numpy()


def _set_grads(params, gs):
    for p, g in zip(params, gs):
        p.grad = torch.from_numpy(g).to(DEV)


PY_SIZES = (3, 513, 2049)


@pytest.mark.parametrize("case", ["sgd-plain", "sgd_nesterov_wd-clip", "adam_l2-clip_skip", "adamw-plain"])
def test_python_classes_against_the_c_abi(s3r, lib, case):
    """three steps of the class on the C-ABI's bits (both from ZERO moments), a state_dict round trip after the first step into a fresh
    optimizer on fresh parameters, and `_version` growing with every step"""
    d, ts0, params, opt = _make(s3r, case, PY_SIZES, seed=2)
    want = run_device(s3r, lib, d, PY_SIZES, seed=2, steps=3, ts0=ts0)
    versions = [p._version for p in params]
    resumed = None
    for k in range(3):
        gs = R.grads(PY_SIZES, 2, k)
        _set_grads(params, gs)
        opt.step()
        ts, words = _read(opt, params, d)
        R.assert_same(ts, words, want[k][0], _words_to_state(want[k][1]), d, f"{case} class step {k}:")
        assert all(p._version > v for p, v in zip(params, versions))
        versions = [p._version for p in params]
        if resumed is not None:
            _set_grads(resumed[0], gs)
            resumed[1].step()
            ts2, words2 = _read(resumed[1], resumed[0], d)
            R.assert_same(ts2, words2, want[k][0], _words_to_state(want[k][1]), d, f"{case} resumed step {k}:")
        if k == 0:
            sd = opt.state_dict()
            _, _, params2, opt2 = _make(s3r, case, PY_SIZES, seed=2)
            with torch.no_grad():
                for a, b in zip(params2, params):
                    a.copy_(b)
            opt2.load_state_dict(sd)
            resumed = (params2, opt2)
    assert opt.grad_norm(0).device.type == "cuda" and opt.skipped(0).dtype == torch.int32 and int(opt.skipped(0)) == 0


def _words_to_state(w):
    f = w[1:6].view(np.float32)
    return dict(step=int(w[0]), b1p=f[0], b2p=f[1], lr=f[2], norm=f[3], coef=f[4], skipped=int(w[6]), reserved=int(w[7]))


def test_a_parameter_without_a_gradient_keeps_its_bits(s3r, lib):
    d, ts0, params, opt = _make(s3r, "adam-plain", PY_SIZES, seed=4)
    gs = R.grads(PY_SIZES, 4, 0)
    _set_grads(params, gs)
    opt.step()
    before, _ = _read(opt, params, d)
    v1 = params[1]._version
    gs = R.grads(PY_SIZES, 4, 1)
    _set_grads(params, gs)
    params[1].grad = None
    opt.step()
    after, words = _read(opt, params, d)
    assert all((R.bits(before[1][k]) == R.bits(after[1][k])).all() for k in "pmv") and params[1]._version == v1
    # the other two step exactly as in a list of two: Adam couples nothing without the norm
    ts1, st1 = R.step32(d, ts0, R.grads(PY_SIZES, 4, 0), R.fresh_state(R.LR))
    ts2, st2 = R.step32(d, [ts1[0], ts1[2]], [gs[0], gs[2]], st1)
    R.assert_same([after[0], after[2]], words, ts2, st2, d, "without a gradient:")


def test_set_lr_and_a_changed_group_lr_reach_the_device(s3r, lib):
    d, ts0, params, opt = _make(s3r, "sgd_momentum-plain", PY_SIZES, seed=5)
    ts, st = ts0, R.fresh_state(R.LR)
    for k, how in enumerate(("none", "group", "set_lr")):
        if how == "group":
            opt.param_groups[0]["lr"] = 3e-3
            st["lr"] = np.float32(3e-3)
        if how == "set_lr":
            opt.set_lr(7e-4)
            st["lr"] = np.float32(7e-4)
            assert opt.param_groups[0]["lr"] == 7e-4
        gs = R.grads(PY_SIZES, 5, k)
        _set_grads(params, gs)
        opt.step()
        ts, st = R.step32(d, ts, gs, st)
        got, words = _read(opt, params, d)
        R.assert_same(got, words, ts, st, d, f"lr by {how}:")


def test_every_value_error(s3r):
    good = lambda: torch.nn.Parameter(torch.zeros(8, 4, device=DEV))      # noqa: E731
    for cls in (s3r.SGD, s3r.Adam, s3r.AdamW):
        with pytest.raises(ValueError, match="fp32"):
            cls([torch.nn.Parameter(torch.zeros(4, device=DEV, dtype=torch.bfloat16))])
        with pytest.raises(ValueError, match="contiguous"):
            cls([torch.nn.Parameter(torch.zeros(8, 4, device=DEV).t())])
        with pytest.raises(ValueError, match="GPU only"):
            cls([torch.nn.Parameter(torch.zeros(4))])
        with pytest.raises(ValueError, match="maximize"):
            cls([good()], maximize=True)
        p = good()
        opt = cls([p])
        p.grad = torch.zeros(8, 4, device=DEV).to_sparse()
        before = p.detach().clone()
        with pytest.raises(ValueError, match="sparse"):
            opt.step()
        assert torch.equal(p.detach(), before)
    with pytest.raises(ValueError, match="amsgrad"):
        s3r.Adam([good()], amsgrad=True)
    with pytest.raises(ValueError, match="amsgrad"):
        s3r.AdamW([good()], amsgrad=True)
    with pytest.raises(ValueError, match="dampening"):
        s3r.SGD([good()], momentum=0.9, dampening=0.1)
    with pytest.raises(ValueError, match="nesterov"):
        s3r.SGD([good()], nesterov=True)
