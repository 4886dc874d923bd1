"""The stream contract of s3r_optim_state_init and s3r_optim_step, on the instruments of tests/test_streams_gpu.py (imported, used as they
are): the calls behind a delayed producer on a non-blocking stream carry the bits of the NULL-stream calls; the same calls on a second
idle stream are SEEN by the instrument; captured calls replay on new gradients in the same buffers with the eager bits; a refused call
inside a captured region returns its code and leaves nothing in the graph.  The cases are recipes in the form of tests/_stream_cases.py
(Arg / Plan / Case).  A step reads and writes its parameters and moments, which the instruments' roles do not know: in the first case
they are role "zero" (the instrument zeroes them in front of every call and collects them behind it: one Adam step with clipping from
zero parameters and moments, its state written by s3r_optim_state_init in the same call), in the refusal case role "scr" (NaN-filled,
not collected: the state dwords are the result, and the refused calls — a negative lr, beta1 = 1 — must leave their copy as poison).
What the instruments cannot show, the state ADVANCING on the device under replay, has a test of its own: the step captured once and
replayed three times on new gradients in the same buffers has the bits of three eager steps, and of the restatement."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from tests import _optim64 as R
from tests import _stream_cases as SC
from tests import test_streams_gpu as TS
from tests.test_optimizer_gpu import run_device, _compare, _desc
from tests.test_streams_gpu import gate, lib      # noqa: F401  (the instruments' fixtures)

pytestmark = pytest.mark.gpu
F32 = SC.F32
SIZES = (3, 513, 2049)
D = R.CASES["adam-clip_skip"]
LR = 1e-2


def _plan(owned):
    """owned: the role of the parameters and moments ("zero" or "scr")"""
    def make(lib, dev):
        import s3r
        L = s3r._lib
        args = [SC.Arg(f"g{i}", (n,), F32, "in") for i, n in enumerate(SIZES)]
        args += [SC.Arg(f"{k}{i}", (n,), F32, owned) for i, n in enumerate(SIZES) for k in "pmv"]
        args += [SC.Arg("state", (8,), F32, "out"), SC.Arg("scratch", (R.scratch_elems(SIZES),), F32, "scr")]

        def data(k):
            return {f"g{i}": SC._t(g) for i, g in enumerate(R.grads(SIZES, seed=20 + k))}

        def _step(ptr, st, desc):
            arr = (L.OptimTensor * len(SIZES))(*[L.OptimTensor(ptr[f"p{i}"], ptr[f"g{i}"], ptr[f"m{i}"], ptr[f"v{i}"], n)
                                                 for i, n in enumerate(SIZES)])
            return lib.s3r_optim_step(C.byref(desc), arr, len(SIZES), ptr["state"], ptr["scratch"], R.scratch_elems(SIZES), st)

        def call(ptr, st):
            rc = lib.s3r_optim_state_init(ptr["state"], LR, st)
            return rc if rc else _step(ptr, st, _desc(L, D))

        def refuse(ptr, st):
            rc = lib.s3r_optim_state_init(ptr["state"], -1.0, st)
            bad = _desc(L, D)
            bad.beta1 = 1.0
            return (rc if rc != -1 else _step(ptr, st, bad)), -1

        def check(d, res):
            zeros = [dict(p=np.zeros(n, np.float32), m=np.zeros(n, np.float32), v=np.zeros(n, np.float32)) for n in SIZES]
            ts, st = R.step32(D, zeros, [SC._np(d[f"g{i}"]) for i in range(len(SIZES))], R.fresh_state(LR))
            got = [{k: SC._np(res[f"{k}{i}"]) for k in "pmv"} for i in range(len(SIZES))]
            R.assert_same(got, SC._np(res["state"]).view(np.int32), ts, st, D, "one step from zero:")

        return SC.Plan(args, data, call, check, refuse=refuse)
    return make


ENTRIES = ("s3r_optim_state_init", "s3r_optim_step")
CASE = SC.Case("optim:adam-clip-skip", ENTRIES, "optimizer", _plan("zero"), mutant=True)
REFUSED = SC.Case("optim:refused", ENTRIES, "optimizer", _plan("scr"))
PAD_STREAMS = 25       # this file takes 1 (delayed producer) + 2 (misplaced) + 1 (capture) + 1 (refusal) + 2 (three replays) = 7; 32 with these


def test_the_pre_states_are_documented_as_safe(lib):
    """the entry's comment says what a NaN does (it propagates through the arithmetic and, in the norm, into grad_norm and clip_coef),
    so the NaN pre-state of every float buffer may be read"""
    with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "s3r.h")) as f:
        text = f.read()
    at = text.index("int s3r_optim_step(")
    comment = " ".join(re.sub(r"\n \*", " ", text[text.rfind("/* The optimizer step", 0, at):at]).split())
    assert "hip_stream" in comment and "hipStream_t" in comment and "propagates through" in comment
    assert re.search(r"int s3r_optim_state_init\(float\* state, float lr, void\* hip_stream\);", text)
    for case in (CASE, REFUSED):
        plan = case.plan(lib, None)
        assert 0 < plan.nbytes <= SC.CAP_BYTES
        for a in plan.args:
            assert SC.safe_prestate(a, comment) == "NaN (header)", a.name
        d0, d1 = plan.data(0), plan.data(1)
        assert any(not torch.equal(d0[n], d1[n]) for n in d0)


def test_delayed_producer(s3r, lib, gate):
    TS.test_delayed_producer(s3r, lib, gate, CASE)


def test_misplaced_stream_is_seen(s3r, lib, gate):
    """the instrument needs its two streams on different hardware queues, and later files must meet torch's pool of 32 streams at the
    phase they have without this file (tests/test_batchnorm_train_streams_gpu.py has the measurement): the loop below brings this
    file's streams to 32"""
    for _ in range(PAD_STREAMS):
        with torch.cuda.stream(torch.cuda.Stream()):
            torch.zeros(1, device=TS.DEV)
    torch.cuda.synchronize()
    TS.test_misplaced_stream_is_seen(s3r, lib, gate, CASE)


def test_capture_and_replay(s3r, lib):
    TS.test_capture_and_replay(s3r, lib, CASE)


def test_refused_call_is_not_captured(s3r, lib):
    TS.test_refused_call_is_not_captured(s3r, lib, REFUSED)


@pytest.mark.parametrize("case", ["adam-clip_skip", "sgd_momentum-plain"])
def test_three_replays_advance_the_state_on_the_device(s3r, lib, case):
    """the step captured once (the state initialised eagerly in front of the capture) and replayed three times on new gradients in
    the same buffers: step count, running powers and moments advance on the device — the bits of three eager steps"""
    d = R.CASES[case]
    eager = run_device(s3r, lib, d, SIZES, seed=9, steps=3)
    replayed = run_device(s3r, lib, d, SIZES, seed=9, steps=3, captured=True)
    _compare(replayed, R.run32(d, SIZES, seed=9, steps=3), d, f"{case} replayed")
    for (ta, wa), (tb, wb) in zip(eager, replayed):
        assert (wa == wb).all() and wb[0] > 0
        for a, b in zip(ta, tb):
            assert all((R.bits(a[k]) == R.bits(b[k])).all() for k in "pmv")
    assert [w[0] for _, w in replayed] == [1, 2, 3]
