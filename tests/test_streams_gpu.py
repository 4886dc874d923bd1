"""The stream contract of every entry point of include/s3r.h that takes a `void* stream` (tests/_stream_cases.py): work is enqueued
on the stream passed in and on no other, nothing is allocated or synchronised, a refused call enqueues nothing.

Instrument 1, the delayed producer (`test_delayed_producer`).  Every buffer of the call starts in a pre-state the call must not see
(inputs poison, outputs and scratch NaN, index inputs the int32 guard pattern: all documented as safe to read).  On a caller-created
non-blocking stream a gate — torch.cuda._sleep, a kernel that only takes time — is followed by the copies of the true inputs, the
poison / NaN fills, the call itself and the copies of the outputs.  The call must have RETURNED to the host while the gate was still
running (else the test fails as inconclusive), and after the stream has drained the results must be the bits of the same call made
with stream = NULL after a full synchronise, meet the entry's own reference, and leave every guard intact.  A launch, memset or copy
on any other stream runs ahead of the gate on the pre-state and is then overwritten or left unfinished.
`test_misplaced_stream_is_seen` shows that the instrument sees that: one case per family is issued on a second idle stream.

Instrument 2, capture and replay (`test_capture_and_replay`).  The call alone is captured with torch.cuda.graph in the default
`global` error mode — a hidden synchronisation, allocation or legacy-stream launch makes the capture raise — and replayed on a second
input set put into the same buffers, then on the first again: a value read on the host at enqueue time would be baked into the graph.
`test_refused_call_is_not_captured`: valid, refused, valid in one region, for the five training entries.

Module level: a training step whose forward runs on a side stream behind a gate and whose backward is called from the default
stream; a whole step (forward, loss, backward, in-place update) captured and replayed; two host threads fine-tuning the two heads.

Gate length.  torch.cuda._sleep(10^6) takes 0.43 ms on an MI355X (HIP events, the `gate` fixture, once per module).  The longest
host-side enqueue among the cases (copies, fills and the call, time.perf_counter; the library is the parent commit's) is
LONGEST_ENQUEUE_MS = 0.21 ms (conv:direct-conv3d-32to32-e8, the first case; most others 0.03 - 0.12 ms, decoder 0.17 ms).
The gate is GATE_MS = min(100, max(GATE_FLOOR_MS, GATE_FACTOR * LONGEST_ENQUEUE_MS)) ms.  GATE_FACTOR = 20 gives 4.2 ms, enough for
the C-ABI cases.  GATE_FLOOR_MS = 30 is there for what that number does not cover: the two module-level tests put a whole forward
and backward, enqueued from Python through autograd, behind the same gate (their host time is printed by the test, it was not
measured on the parent), and a host thread that loses one time slice between the gate and the event query must not turn a run
inconclusive.  30 ms is the length of every recorded run, none with an inconclusive gate; it is below the 100 ms cap and costs each
gated test 30 ms.  The event query after the call is the guarantee, the length only keeps it from tripping.

Found (docs/LAB_NOTES.md).  On the parent commit's library test_capture_and_replay fails for 9 of the 41 cases — conv:staged-tanh-
conv2d-20to33-k5-e9, conv:tclass-deconv2d-32to16-k4s2-e9, chain:handoff-b-k3-e8, encoder:{fp32,bf16}, encoder_u8:{fp32,bf16},
decoder:{fp32,bf16}.  In each the first replay (second input set) has the eager bits and the second replay (first set again) has
not: 3696 of 5346 elements of y differ (staged conv), 1647 of 10368 (tclass), 10556 of 32768 (hand-off chain), 7274 / 11490 of
50176 (encoder fp32 / bf16), 32768 of 32768 (decoder); no NaN, the same counts on every run; every eager call meets its reference.
Each of the nine enqueued a hipMemsetAsync (the staging buffer of a general layer, the workspace under ws_fresh = 1) in front of
kernels that write the same buffer.  Changed with these tests: launch_stage and s3r_chain_forward under ws_fresh = 1 zero with a
kernel of the library's own (zero_fill_kernel, s3r_general.hip) instead of hipMemsetAsync.  With that all 41 capture cases replay
bit for bit, and everything else in this file passed before and after.  Why the runtime replays a graph with such a memset node
wrongly from its second launch on is a hypothesis, not a finding: the kernel is a workaround for the observed behaviour.

Whole file on an MI355X (99 tests): about 11 s, the sum of two partial runs (6.6 s and 5.0 s); not yet timed in one run.
"""
import ctypes as C
import threading
import time

import pytest
import torch

from tests import _guard as G
from tests import _stream_cases as SC

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
LONGEST_ENQUEUE_MS = 0.21                                          # measured, see the docstring
GATE_FACTOR = 20
GATE_FLOOR_MS = 30.0
GATE_CAP_MS = 100.0
GATE_MS = min(GATE_CAP_MS, max(GATE_FLOOR_MS, GATE_FACTOR * LONGEST_ENQUEUE_MS))


@pytest.fixture(scope="module")
def lib(s3r):
    return s3r.load_library()


@pytest.fixture(scope="module")
def gate():
    """cycles of torch.cuda._sleep for GATE_MS, calibrated once against HIP events"""
    probe = 1_000_000
    torch.cuda._sleep(probe)                                       # (first launch: module load)
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    torch.cuda._sleep(probe)
    b.record()
    torch.cuda.synchronize()
    ms = a.elapsed_time(b)
    assert ms > 0
    cycles = int(probe * GATE_MS / ms)
    print(f"\ngate: _sleep({probe}) = {ms:.4f} ms; {cycles} cycles for {GATE_MS} ms")
    return cycles


def _bits(t):
    return t.view(G._BITS[t.dtype][0])


class Live:
    """a plan's buffers on the device: one guarded allocation per argument (tests/_guard.py), both input sets beside them"""

    def __init__(self, plan, copies=1):
        self.plan = plan
        self.sets = [plan.data(k) for k in (0, 1)]
        self.dev_sets = [{a.name: s[a.name].to(DEV).contiguous() for a in plan.args if a.role == "in"} for s in self.sets]
        self.bufs = {}
        for a in plan.args:
            if a.role == "in":
                b = G.Guarded(a.name, a.shape, a.dtype, DEV, "in", data=self.dev_sets[0][a.name])
            elif a.role == "out":
                b = G.Guarded(a.name, a.shape, a.dtype, DEV, "out")
            else:
                b = G.Guarded(a.name, a.shape, a.dtype, DEV, "scratch")
            self.bufs[a.name] = b
        self.results = [a for a in plan.args if a.role in ("out", "zero")]
        # further output sets for a region of several calls (same inputs and scratch)
        self.more = [{a.name: G.Guarded(a.name, a.shape, a.dtype, DEV, "out") for a in plan.args if a.role == "out"} for _ in range(copies - 1)]
        self.snap = [{n: _bits(t).clone() for n, t in s.items()} for s in self.dev_sets]
        torch.cuda.synchronize()

    def ptr(self, i=0):
        p = {n: b.ptr for n, b in self.bufs.items()}
        if i:
            p.update({n: b.ptr for n, b in self.more[i - 1].items()})
        return p

    def prestate(self):
        for a in self.plan.args:
            _bits(self.bufs[a.name].t).fill_(SC.prestate(a))

    def load(self, k):
        """the true inputs of set k (device-to-device copies on the current stream)"""
        for n, t in self.dev_sets[k].items():
            self.bufs[n].t.copy_(t)
            self.bufs[n].snapshot = self.snap[k][n]

    def fill(self):
        """poison into the outputs, NaN into scratch, zeros where the caller owes them (on the current stream)"""
        for a in self.plan.args:
            t = self.bufs[a.name].t
            if a.role == "out":
                for b in [self.bufs[a.name]] + [m[a.name] for m in self.more]:
                    _bits(b.t).fill_(G._BITS[a.dtype][2])
            elif a.role == "scr":
                _bits(t).fill_(G._BITS[a.dtype][4])
            elif a.role == "zero":
                t.zero_()

    def holders(self):
        return {a.name: torch.empty(a.shape, dtype=a.dtype, device=DEV) for a in self.results}

    def grab(self, dst, i=0):
        for a in self.results:
            src = self.more[i - 1][a.name] if i and a.role == "out" else self.bufs[a.name]
            dst[a.name].copy_(src.t)

    def check_guards(self):
        G.check_all(*self.bufs.values())
        for m in self.more:
            G.check_all(*m.values())


def _equal(a, b):
    return [n for n in a if not torch.equal(_bits(a[n]), _bits(b[n]))]


def _baseline(lib, live, k=0):
    """the call with stream = NULL after a full synchronise, on the same buffers"""
    live.load(k)
    live.fill()
    torch.cuda.synchronize()
    rc = live.plan.call(live.ptr(), None)
    assert rc == 0, lib.s3r_last_error()
    torch.cuda.synchronize()
    live.check_guards()
    base = live.holders()
    live.grab(base)
    torch.cuda.synchronize()
    return base


def _gated(lib, live, gate, call_stream=None):
    """pre-state, then gate | inputs | fills | call | result copies on one non-blocking stream; `call_stream`: the misplaced-stream
    mutant issues the call there instead.  (results, the call returned while the gate ran, host seconds of the enqueue)"""
    st = torch.cuda.Stream()
    res = live.holders()
    end = torch.cuda.Event()
    live.prestate()
    torch.cuda.synchronize()
    with torch.cuda.stream(st):
        torch.cuda._sleep(gate)
        end.record(st)
        t0 = time.perf_counter()
        live.load(0)
        live.fill()
        rc = live.plan.call(live.ptr(), (st if call_stream is None else call_stream).cuda_stream)
        if call_stream is not None:
            call_stream.synchronize()                              # the misplaced call has run: ahead of the gate, on the pre-state
        live.grab(res)
        t1 = time.perf_counter()
    ahead = not end.query()
    st.synchronize()
    torch.cuda.synchronize()
    assert rc == 0, lib.s3r_last_error()
    return res, ahead, t1 - t0


_IDS = [c.id for c in SC.CASES]


@pytest.mark.parametrize("case", SC.INSTRUMENTS["delayed_producer"], ids=_IDS)
def test_delayed_producer(s3r, lib, gate, case):
    live = Live(case.plan(lib, DEV))
    base = _baseline(lib, live)
    res, ahead, secs = _gated(lib, live, gate)
    print(f"\nenqueue {case.id}: {secs * 1e3:.3f} ms on the host")
    assert ahead, f"inconclusive: the gate ({GATE_MS} ms) had ended when the call returned after {secs * 1e3:.3f} ms"
    assert not _equal(res, base), f"not the bits of the NULL-stream call: {_equal(res, base)}"
    live.check_guards()
    live.plan.check(live.sets[0], {n: t.cpu() for n, t in res.items()})


@pytest.mark.parametrize("case", SC.MUTANTS, ids=[c.id for c in SC.MUTANTS])
def test_misplaced_stream_is_seen(s3r, lib, gate, case):
    """the call on a second idle stream while the gate, the inputs and the fills sit on the first: it reads the pre-state (documented
    as safe) and its outputs are overwritten by the poison fill — the instrument must report it"""
    live = Live(case.plan(lib, DEV))
    base = _baseline(lib, live)
    res, ahead, _ = _gated(lib, live, gate, call_stream=torch.cuda.Stream())
    assert ahead, "inconclusive: the second stream did not run ahead of the gate"
    wrong = _equal(res, base)
    left = [b.name for b in live.bufs.values() if b.role == "out" and b.check() is not None]
    print(f"\nmutant {case.id}: mismatch in {wrong}, leftover poison in {left}")
    assert wrong or left, "a call on another stream went unnoticed"


@pytest.mark.parametrize("case", SC.INSTRUMENTS["capture_replay"], ids=_IDS)
def test_capture_and_replay(s3r, lib, case):
    live = Live(case.plan(lib, DEV))
    side = torch.cuda.Stream()
    eager = []
    for k in (0, 1):                                               # warm-up and the eager bits of both sets, on the side stream
        live.load(k)
        live.fill()
        torch.cuda.synchronize()
        assert live.plan.call(live.ptr(), side.cuda_stream) == 0, lib.s3r_last_error()
        side.synchronize()
        eager.append(live.holders())
        live.grab(eager[k])
    live.load(0)
    live.fill()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):                         # capture_error_mode: the default, "global"
        rc = live.plan.call(live.ptr(), torch.cuda.current_stream().cuda_stream)
    assert rc == 0, lib.s3r_last_error()
    got = live.holders()
    for k in (1, 0):                                               # new data in the same buffers, then the first set again
        live.load(k)
        live.fill()
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        live.grab(got)
        bad = _equal(got, eager[k])
        assert not bad, f"replay on set {k} is not the eager call's bits: {bad}"
        live.check_guards()
    live.plan.check(live.sets[0], {n: t.cpu() for n, t in got.items()})


@pytest.mark.parametrize("case", SC.REFUSALS, ids=[c.id for c in SC.REFUSALS])
def test_refused_call_is_not_captured(s3r, lib, case):
    """valid, refused, valid in one captured region: the refused call returns its code and leaves nothing in the graph"""
    live = Live(case.plan(lib, DEV), copies=3)
    side = torch.cuda.Stream()
    live.load(0)
    live.fill()
    torch.cuda.synchronize()
    assert live.plan.call(live.ptr(), side.cuda_stream) == 0, lib.s3r_last_error()
    side.synchronize()
    eager = live.holders()
    live.grab(eager)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        st = torch.cuda.current_stream().cuda_stream
        rc0 = live.plan.call(live.ptr(0), st)
        rc1, want = live.plan.refuse(live.ptr(1), st)
        rc2 = live.plan.call(live.ptr(2), st)
    assert (rc0, rc1, rc2) == (0, want, 0), (rc0, rc1, rc2, lib.s3r_last_error())
    live.fill()
    torch.cuda.synchronize()
    g.replay()
    torch.cuda.synchronize()
    for i in (0, 2):
        got = live.holders()
        live.grab(got, i)
        assert not _equal(got, eager), (i, _equal(got, eager))
    for n, b in live.more[0].items():                              # the refused call's outputs: still poison, every element
        assert bool((_bits(b.t) == G._BITS[b.dtype][2]).all()), f"the refused call wrote {n}"
        guards = torch.cat([_bits(b.raw)[:b.g], _bits(b.raw)[b.g + b.n:]])
        assert bool((guards == G._BITS[b.dtype][1]).all()), f"the refused call wrote beside {n}"
    live.more[0].clear()                                           # (checked above: poison is what these must still hold)
    live.check_guards()


# ---------------------------------------------------------------- module level
_POINT = {}


def _point_problem(s3r):
    head = s3r.PointHead()
    if not _POINT:
        _POINT["state"] = s3r.seeded_state_dict(head, seed=4)
    head.load_state_dict(_POINT["state"])
    head.to(DEV)
    latent = torch.relu(torch.randn(2, 512, 4, 4, 4, generator=torch.Generator().manual_seed(3))).to(DEV)
    target = (torch.rand(2, 2048, 3, generator=torch.Generator().manual_seed(8)) - 0.5).to(DEV)
    loss_fn = s3r.ChamferDistance()
    return list(head.parameters()), (lambda: loss_fn(head.differentiable(latent), target)), 0.05


_VOXEL = {}


def _voxel_problem(s3r):
    dec = s3r.Decoder()
    if not _VOXEL:                                                 # d3's features of a seeded volume, computed once and left unchanged
        _VOXEL["state"] = s3r.seeded_state_dict(s3r.Decoder(), seed=4)
        dec.load_state_dict(_VOXEL["state"])
        dec.to(DEV)
        vol = 0.5 * torch.randn(1, 64, 28, 28, 28, generator=torch.Generator().manual_seed(1))
        _VOXEL["feats"] = dec.features(vol.to(DEV))
        _VOXEL["gt"] = (torch.rand(1, 32, 32, 32, generator=torch.Generator().manual_seed(3)) > 0.7).float().to(DEV)
        torch.cuda.synchronize()
    dec.load_state_dict(_VOXEL["state"])
    dec.to(DEV)
    feats, gt = _VOXEL["feats"], _VOXEL["gt"]
    loss_fn = s3r.VoxelBCELoss()
    return [dec.d4.conv.weight, dec.d4.conv.bias], (lambda: loss_fn(dec.differentiable_head(feats), gt)), 0.05


_PROBLEMS = {"point-head-chamfer": _point_problem, "voxel-head-bce": _voxel_problem}


def _steps(params, loss_of, lr, n, stream=None):
    """n eager SGD steps (in-place p.add_(p.grad, alpha=-lr)); (losses, parameters) as bit tensors"""
    losses = []
    ctx = torch.cuda.stream(stream) if stream is not None else torch.cuda.stream(torch.cuda.current_stream())
    with ctx:
        for _ in range(n):
            for p in params:
                p.grad = None
            loss = loss_of()
            loss.backward()
            with torch.no_grad():
                for p in params:
                    p.add_(p.grad, alpha=-lr)
            losses.append(loss.detach().clone())
    (stream or torch.cuda.current_stream()).synchronize()
    torch.cuda.synchronize()
    return [_bits(l.reshape(1)).clone() for l in losses], [_bits(p.detach()).clone() for p in params]


@pytest.mark.parametrize("name", list(_PROBLEMS))
def test_backward_from_the_default_stream_lands_behind_the_forward(s3r, gate, name):
    """forward on a side stream behind a gate, loss.backward() called outside the `with`: every gradient has the bits of the
    all-default-stream run"""
    params, loss_of, _ = _PROBLEMS[name](s3r)
    loss_of().backward()
    torch.cuda.synchronize()
    want = [_bits(p.grad).clone() for p in params]
    for p in params:
        p.grad = None
    st = torch.cuda.Stream()
    end = torch.cuda.Event()
    torch.cuda.synchronize()
    with torch.cuda.stream(st):
        torch.cuda._sleep(gate)
        end.record(st)
        t0 = time.perf_counter()
        loss = loss_of()
    loss.backward()
    ahead = not end.query()
    secs = time.perf_counter() - t0
    torch.cuda.synchronize()
    print(f"\nstep {name}: forward and backward enqueued in {secs * 1e3:.3f} ms on the host")
    assert ahead, f"inconclusive: the gate ({GATE_MS} ms) had ended when backward() returned after {secs * 1e3:.3f} ms"
    for p, w in zip(params, want):
        assert torch.equal(_bits(p.grad), w)


@pytest.mark.parametrize("name", list(_PROBLEMS))
def test_training_step_captured_as_a_graph(s3r, name):
    """forward, loss, backward and the in-place update in one graph: three replays against three eager steps from the same state"""
    params, loss_of, lr = _PROBLEMS[name](s3r)
    want_l, want_p = _steps(params, loss_of, lr, 3)
    params, loss_of, lr = _PROBLEMS[name](s3r)                      # the same initial state again
    init = [p.detach().clone() for p in params]
    side = torch.cuda.Stream()
    _steps(params, loss_of, lr, 1, stream=side)                    # warm-up on the side stream
    with torch.no_grad():
        for p, p0 in zip(params, init):
            p.copy_(p0)
            p.grad = None
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        loss = loss_of()
        loss.backward()
        with torch.no_grad():
            for p in params:
                p.add_(p.grad, alpha=-lr)
    with torch.no_grad():                                          # (capture runs nothing: the state is still the initial one)
        for p, p0 in zip(params, init):
            p.copy_(p0)
    torch.cuda.synchronize()
    got_l = []
    for _ in range(3):
        g.replay()
        torch.cuda.synchronize()
        got_l.append(_bits(loss.detach().reshape(1)).clone())
    for a, b in zip(got_l, want_l):
        assert torch.equal(a, b), "a replayed step's loss differs from the eager step's"
    for p, w in zip(params, want_p):
        assert torch.equal(_bits(p.detach()), w), "parameters after three replays differ from three eager steps"


def test_two_host_threads_fine_tune_on_two_streams(s3r):
    """one thread fine-tunes the point head, the other the voxel head, each on its own stream: the bits of the serial runs"""
    want = {n: _steps(*_PROBLEMS[n](s3r), 3) for n in _PROBLEMS}
    probs = {n: _PROBLEMS[n](s3r) for n in _PROBLEMS}
    streams = {n: torch.cuda.Stream() for n in _PROBLEMS}
    got, errors = {}, []
    start = threading.Barrier(2)

    def work(n):
        try:
            torch.cuda.set_device(0)
            start.wait(timeout=60)
            got[n] = _steps(*probs[n], 3, stream=streams[n])
        except BaseException as e:                                 # noqa: BLE001  (reported by the main thread)
            errors.append((n, repr(e)))

    threads = [threading.Thread(target=work, args=(n,)) for n in _PROBLEMS]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    for n in _PROBLEMS:
        for a, b in zip(got[n][0] + got[n][1], want[n][0] + want[n][1]):
            assert torch.equal(a, b), n
