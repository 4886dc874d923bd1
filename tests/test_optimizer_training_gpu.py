"""s3r.Adam and s3r.SGD(momentum=0.9) on the two small problems of tests/test_streams_gpu.py (the point head under Chamfer, the voxel head
under BCE): three eager steps run twice have equal bits and lower the loss; the parameters stepped by tests/_optim64.py's restatement
from the device's own gradients have the same bits; forward, loss, backward and `opt.step()` captured in ONE graph, with `set_lr` halving
the rate between replays, give the bits of three eager steps under the same schedule; `step()` under capture before `init_state()`
raises and captures nothing.

The rule is elementwise without the norm, so the restatement runs on every element of a tensor up to 2^20 elements and on a sample of a
larger one (both ends — the ragged tail — and every 997th element between): the point head's first layer alone has 2^25 weights."""
import numpy as np
import pytest
import torch

from tests import _optim64 as R
from tests import test_streams_gpu as TS

pytestmark = pytest.mark.gpu
DEV = TS.DEV
OPTS = {"adam": R.Desc("adam"), "sgd_momentum": R.Desc("sgd", beta1=0.9)}
# Learning rates.  SGD: below the 0.05 tests/test_streams_gpu.py steps these problems with, since momentum 0.9 adds up to 2.71 times the
# plain step by the third.  Adam moves EVERY weight by about lr per step whatever its gradient: the voxel head has 65 parameters (1e-3,
# torch's default), the point head's first layer a fan-in of 32768, where a pre-activation moves by up to 32768 lr |x| per step — 1e-6
# keeps that at a few hundredths.
LRS = {("point-head-chamfer", "adam"): 1e-6, ("voxel-head-bce", "adam"): 1e-3,
       ("point-head-chamfer", "sgd_momentum"): 0.02, ("voxel-head-bce", "sgd_momentum"): 0.02}
PAD_STREAMS = 27       # this file takes 4 (one side stream per captured problem and rule) + 1 (the refused capture) = 5; 32 with these


def _opt(s3r, params, name, lr):
    return s3r.Adam(params, lr=lr) if name == "adam" else s3r.SGD(params, lr=lr, momentum=0.9)


def _sample(p):
    n = p.numel()
    if n <= 1 << 20:
        return torch.arange(n, device=p.device)
    return torch.unique(torch.cat([torch.arange(0, 4099), torch.arange(4099, n - 4099, 997), torch.arange(n - 4099, n)])).to(p.device)


def _run(s3r, problem, name, lrs, record=False):
    """one eager step per entry of lrs (set_lr in front of each but the first); (loss bits, parameter bits, final loss, record)"""
    params, loss_of, _ = TS._PROBLEMS[problem](s3r)
    opt = _opt(s3r, params, name, lrs[0])
    idx = [_sample(p) for p in params] if record else None
    rec = dict(p0=[p.detach().reshape(-1)[i].cpu().numpy() for p, i in zip(params, idx)], g=[], p=[]) if record else None
    losses = []
    for k, lr in enumerate(lrs):
        if k:
            opt.set_lr(lr)
        opt.zero_grad(set_to_none=True)
        loss = loss_of()
        loss.backward()
        opt.step()
        losses.append(loss.detach().clone())
        if record:
            rec["g"].append([p.grad.reshape(-1)[i].cpu().numpy() for p, i in zip(params, idx)])
            rec["p"].append([p.detach().reshape(-1)[i].cpu().numpy() for p, i in zip(params, idx)])
    with torch.no_grad():
        final = float(loss_of())
    torch.cuda.synchronize()
    return [TS._bits(l.reshape(1)).clone() for l in losses], [TS._bits(p.detach()).clone() for p in params], final, rec, opt


@pytest.mark.parametrize("name", list(OPTS))
@pytest.mark.parametrize("problem", list(TS._PROBLEMS))
def test_three_eager_steps_twice_and_against_the_restatement(s3r, problem, name):
    d, lr = OPTS[name], LRS[problem, name]
    l1, p1, final, rec, opt = _run(s3r, problem, name, [lr] * 3, record=True)
    l2, p2, _, _, _ = _run(s3r, problem, name, [lr] * 3)
    assert all(torch.equal(a, b) for a, b in zip(l1, l2)) and all(torch.equal(a, b) for a, b in zip(p1, p2)), "two runs differ"
    first = float(l1[0].view(torch.float32))
    print(f"\n{problem} {name}: loss {first:.6g} -> {final:.6g} after three steps")
    assert np.isfinite(final) and final < first
    ts = [dict(p=p, m=np.zeros_like(p), v=np.zeros_like(p)) for p in rec["p0"]]
    st = R.fresh_state(lr)
    for k in range(3):
        ts, st = R.step32(d, ts, rec["g"][k], st)
        for i, (t, got) in enumerate(zip(ts, rec["p"][k])):
            bad = np.flatnonzero(R.bits(t["p"]) != R.bits(got))
            assert not bad.size, f"step {k} tensor {i}: {bad.size} sampled elements differ from the restatement, first at {bad[0]}"
    assert (opt.device_state(0).cpu().numpy() == R.state_words(st)).all()


@pytest.mark.parametrize("name", list(OPTS))
@pytest.mark.parametrize("problem", list(TS._PROBLEMS))
def test_whole_step_in_one_graph_with_a_schedule(s3r, problem, name):
    """the learning rate lives on the device: set_lr between two replays reaches the captured step, whose bias correction advances
    on its own"""
    lr = LRS[problem, name]
    lrs = [lr, lr / 2, lr / 4]
    want_l, want_p, _, _, _ = _run(s3r, problem, name, lrs)
    params, loss_of, _ = TS._PROBLEMS[problem](s3r)                 # the same initial state again
    init = [p.detach().clone() for p in params]
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):                                  # warm-up on the side stream, with an optimizer of its own
        warm = _opt(s3r, params, name, lr)
        loss_of().backward()
        warm.step()
    side.synchronize()
    with torch.no_grad():
        for p, p0 in zip(params, init):
            p.copy_(p0)
            p.grad = None
    opt = _opt(s3r, params, name, lrs[0])                           # moments zeroed, state written: before the capture
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        loss = loss_of()
        loss.backward()
        opt.step()
    with torch.no_grad():                                          # (capture runs nothing: the state is still the initial one)
        for p, p0 in zip(params, init):
            p.copy_(p0)
    torch.cuda.synchronize()
    assert int(opt.device_state(0)[0]) == 0
    got_l = []
    for k, r in enumerate(lrs):
        if k:
            opt.set_lr(r)
        g.replay()
        torch.cuda.synchronize()
        got_l.append(TS._bits(loss.detach().reshape(1)).clone())
    for a, b in zip(got_l, want_l):
        assert torch.equal(a, b), "a replayed step's loss differs from the eager step's"
    for p, w in zip(params, want_p):
        assert torch.equal(TS._bits(p.detach()), w), "parameters after three replays differ from three eager steps"
    assert int(opt.device_state(0)[0]) == 3


def test_step_under_capture_before_init_state_raises_and_captures_nothing(s3r):
    for _ in range(PAD_STREAMS):                                   # (torch's pool of 32 streams: tests/test_optimizer_streams_gpu.py)
        with torch.cuda.stream(torch.cuda.Stream()):
            torch.zeros(1, device=DEV)
    p = torch.nn.Parameter(torch.ones(1000, device=DEV))
    q = torch.nn.Parameter(torch.ones(777, device=DEV))
    opt = s3r.Adam([p], lr=0.1)
    opt.add_param_group(dict(params=[q]))                          # a group whose moments and state nobody has initialised
    p.grad, q.grad = torch.ones_like(p), torch.ones_like(q)
    marker = torch.zeros(1, device=DEV)
    before = opt.device_state(0).clone()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=torch.cuda.Stream()):
        marker.add_(1)
        with pytest.raises(RuntimeError, match="init_state"):
            opt.step()
    g.replay()
    torch.cuda.synchronize()
    assert float(marker) == 1.0                                    # the region replays, and holds nothing of the refused step
    assert bool((p == 1).all()) and bool((q == 1).all()) and torch.equal(opt.device_state(0), before)
    opt.init_state()
    opt.step()
    torch.cuda.synchronize()
    assert bool((p != 1).all()) and bool((q != 1).all()) and int(opt.device_state(1)[0]) == 1
