"""The stream contract of s3r_batchnorm_train_forward and s3r_batchnorm_train_backward, on the instruments of tests/test_streams_gpu.py
(imported, used as they are): the call behind a delayed producer on a non-blocking stream carries the bits of the NULL-stream call; the
same call on a second idle stream is SEEN by the instrument; a captured call replays on new data in the same buffers with the eager bits;
a refused call inside a captured region returns its code and leaves nothing in the graph.  The cases are recipes in the form of
tests/_stream_cases.py (Arg / Plan / Case) at (3, 5, 1029): three chunks per row, the last one short, three samples — every launch of both
entries runs (5 forward, 3 backward).  The backward also runs with grad_z alone: both sums then live in the scratch."""
import os

import numpy as np
import pytest

from tests import _bn64 as R
from tests import _stream_cases as SC
from tests import test_streams_gpu as TS
from tests.test_streams_gpu import gate, lib      # noqa: F401  (the instruments' fixtures)

pytestmark = pytest.mark.gpu
F32 = SC.F32
F = np.float32
SHAPE, ACT, EPS = (3, 5, 1029), "relu", 1e-5
B, CH, S = SHAPE


def _inputs(k):
    rng = np.random.default_rng(60 + k)
    z = (1.5 * rng.standard_normal(SHAPE) + 0.5).astype(F)
    gam = (1.0 + 0.5 * rng.standard_normal(CH)).astype(F)
    beta = (0.3 * rng.standard_normal(CH)).astype(F)
    gy = rng.standard_normal(SHAPE).astype(F)
    return z, gam, beta, gy


def _forward():
    def make(lib, dev):
        need = lib.s3r_batchnorm_train_forward_scratch_elems(B, CH, S)
        assert need > 0
        args = [SC.Arg("z", SHAPE, F32, "in"), SC.Arg("gamma", (CH,), F32, "in"), SC.Arg("beta", (CH,), F32, "in"), SC.Arg("y", SHAPE, F32, "out"),
                SC.Arg("save_mean", (CH,), F32, "out"), SC.Arg("save_var", (CH,), F32, "out"), SC.Arg("save_invstd", (CH,), F32, "out"),
                SC.Arg("scratch", (need,), F32, "scr")]

        def data(k):
            z, gam, beta, _ = _inputs(k)
            return {"z": SC._t(z), "gamma": SC._t(gam), "beta": SC._t(beta)}

        def _call(ptr, st, elems):
            return lib.s3r_batchnorm_train_forward(ptr["z"], ptr["gamma"], ptr["beta"], EPS, 1, ptr["y"], ptr["save_mean"], ptr["save_var"],
                                                   ptr["save_invstd"], B, CH, S, ptr["scratch"], elems, st)

        def check(d, res):
            z, gam, beta = (SC._np(d[n]) for n in ("z", "gamma", "beta"))
            mean, var, inv = R.stats32(z, EPS)
            SC._same(SC._np(res["save_mean"]), mean, "save_mean")
            SC._same(SC._np(res["save_var"]), var, "save_var")
            SC._same(SC._np(res["save_invstd"]), inv, "save_invstd")
            SC._same(SC._np(res["y"]), R.y32(z, mean, inv, gam, beta, ACT), "y")

        return SC.Plan(args, data, lambda ptr, st: _call(ptr, st, need), check, refuse=lambda ptr, st: (_call(ptr, st, need - 1), -3))

    return make


def _backward(outs):
    def make(lib, dev):
        need = lib.s3r_batchnorm_train_backward_scratch_elems(B, CH, S)
        assert need > 0
        oshape = {"grad_z": SHAPE, "grad_gamma": (CH,), "grad_beta": (CH,)}
        args = [SC.Arg("z", SHAPE, F32, "in"), SC.Arg("y", SHAPE, F32, "in"), SC.Arg("grad_y", SHAPE, F32, "in"), SC.Arg("gamma", (CH,), F32, "in"),
                SC.Arg("save_mean", (CH,), F32, "in"), SC.Arg("save_invstd", (CH,), F32, "in")] + \
               [SC.Arg(o, oshape[o], F32, "out") for o in outs] + [SC.Arg("scratch", (need,), F32, "scr")]

        def data(k):
            z, gam, beta, gy = _inputs(k)
            mean, _, inv = R.stats32(z, EPS)
            y = R.y32(z, mean, inv, gam, beta, ACT)                # (ReLU: the restatement has the forward's bits)
            return {"z": SC._t(z), "y": SC._t(y), "grad_y": SC._t(gy), "gamma": SC._t(gam), "save_mean": SC._t(mean), "save_invstd": SC._t(inv)}

        def _call(ptr, st, elems):
            return lib.s3r_batchnorm_train_backward(ptr["z"], ptr["y"], ptr["grad_y"], ptr["gamma"], ptr["save_mean"], ptr["save_invstd"], 1,
                                                    ptr.get("grad_z"), ptr.get("grad_gamma"), ptr.get("grad_beta"), B, CH, S, ptr["scratch"],
                                                    elems, st)

        def check(d, res):
            z, y, gy, gam, mean, inv = (SC._np(d[n]) for n in ("z", "y", "grad_y", "gamma", "save_mean", "save_invstd"))
            want = dict(zip(("grad_z", "grad_gamma", "grad_beta"), R.backward32(z, y, gy, gam, mean, inv, ACT)))
            for n in outs:
                SC._same(SC._np(res[n]), want[n], n)

        return SC.Plan(args, data, lambda ptr, st: _call(ptr, st, need), check, refuse=lambda ptr, st: (_call(ptr, st, need - 1), -3))

    return make


ENTRIES = ("s3r_batchnorm_train_forward", "s3r_batchnorm_train_backward")
CASES = [SC.Case("batchnorm_forward", ENTRIES[:1], "batchnorm", _forward(), mutant=True),
         SC.Case("batchnorm_backward:all", ENTRIES[1:], "batchnorm", _backward(("grad_z", "grad_gamma", "grad_beta"))),
         SC.Case("batchnorm_backward:grad_z-only", ENTRIES[1:], "batchnorm", _backward(("grad_z",)))]
_IDS = [c.id for c in CASES]


def test_the_pre_states_are_documented_as_safe(lib):
    """the header comment of the entries says what a NaN does, so the NaN pre-state of every float buffer may be read"""
    with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "s3r.h")) as f:
        text = f.read()
    for case in CASES:
        at = text.index(f"int {case.entries[0]}(")
        comment = text[text[:at].rfind("/*"):at]
        assert "hip_stream" in comment and "hipStream_t" in comment
        plan = case.plan(lib, None)
        assert 0 < plan.nbytes <= SC.CAP_BYTES
        for a in plan.args:
            assert SC.safe_prestate(a, comment) == "NaN (header)", a.name


@pytest.mark.parametrize("case", CASES, ids=_IDS)
def test_delayed_producer(s3r, lib, gate, case):
    TS.test_delayed_producer(s3r, lib, gate, case)


def test_misplaced_stream_is_seen(s3r, lib, gate):
    """the instrument needs its two streams on different hardware queues: this file has few delayed-producer runs, so it uses the rest of
    torch's stream pool once first (as tests/test_conv_backward_streams_gpu.py does, which measured the need).
    The count: torch hands out its 32 pool streams round robin, and which PAIR of them an instrument of a later file gets decides whether
    its two streams share a hardware queue.  This file takes 3 (delayed producer) + 2 (this test) + 3 (capture) + 2 (refusal) = 10 streams
    beside the loop below; with 54 here that is 64, a multiple of the pool size, so every later file meets the pool at the phase it has
    without this file (measured with 40: tests/test_streams_gpu.py::test_misplaced_stream_is_seen[disparity_soft:fp32], 18 streams out
    of phase, got two streams of one queue and reported "inconclusive")"""
    import torch
    for _ in range(54):
        with torch.cuda.stream(torch.cuda.Stream()):
            torch.zeros(1, device=TS.DEV)
    torch.cuda.synchronize()
    TS.test_misplaced_stream_is_seen(s3r, lib, gate, CASES[0])


@pytest.mark.parametrize("case", CASES, ids=_IDS)
def test_capture_and_replay(s3r, lib, case):
    TS.test_capture_and_replay(s3r, lib, case)


@pytest.mark.parametrize("case", CASES[:2], ids=_IDS[:2])
def test_refused_call_is_not_captured(s3r, lib, case):
    TS.test_refused_call_is_not_captured(s3r, lib, case)
