"""The stream contract of s3r_conv_backward, on the instruments of tests/test_streams_gpu.py (used as they are): the call behind a delayed
producer on a non-blocking stream carries the bits of the NULL-stream call; the same call on a second idle stream is SEEN by the
instrument; a captured call replays on new data in the same buffers with the eager bits; a refused call inside a captured region
returns its code and leaves nothing in the graph.  The cases are recipes in the form of tests/_stream_cases.py (Arg / Plan / Case):
Conv3d 5 -> 7, k3 s1 p1 over an edge of 5 at B = 3 — three K slices per sample, so the prep pass, the grad_shift finish, the
weight-gradient GEMM and the slab finish all launch — with every output, and with grad_w alone (gs then lives in the scratch)."""
import ctypes as C

import numpy as np
import pytest

from tests import _convbwd64 as CB64
from tests import _stream_cases as SC
from tests import test_streams_gpu as TS
from tests.test_streams_gpu import gate, lib      # noqa: F401  (the instruments' fixtures)

pytestmark = pytest.mark.gpu
F32 = SC.F32


def _conv_backward(outs):
    c, act = CB64.CASES[0], "relu"

    def make(lib, dev):
        import s3r
        LB = s3r._lib
        desc = LB.ConvDesc(LB.OP_CONV, c.nd, c.B, c.cin, c.cout, c.n, c.k, c.s, c.p, LB.ACT[act], 0, -1, 0, 0, 0, 0, 0, 0, 0, 1, c.opad, 0.0)
        need = lib.s3r_conv_backward_scratch_elems(C.byref(desc))
        assert need > 0
        oshape = {"gs": CB64.y_shape(c), "grad_w": CB64.weight_shape(c), "grad_shift": (c.cout,)}
        args = [SC.Arg("x", CB64.x_shape(c), F32, "in"), SC.Arg("y", CB64.y_shape(c), F32, "in"), SC.Arg("grad_y", CB64.y_shape(c), F32, "in"),
                SC.Arg("scale", (c.cout,), F32, "in")] + [SC.Arg(o, oshape[o], F32, "out") for o in outs] + [SC.Arg("scratch", (need,), F32, "scr")]

        def data(k):
            x, _, scale, _, y, gy = CB64.make(c, seed=40 + k, act=act)
            return {"x": SC._t(x), "y": SC._t(y), "grad_y": SC._t(gy), "scale": SC._t(scale)}

        def _call(ptr, st, elems):
            return lib.s3r_conv_backward(C.byref(desc), ptr["x"], ptr["y"], ptr["grad_y"], ptr["scale"], ptr.get("gs"), ptr.get("grad_w"),
                                         ptr.get("grad_shift"), ptr["scratch"], elems, st)

        def check(d, res):
            x, y, gy, scale = (SC._np(d[n]) for n in ("x", "y", "grad_y", "scale"))
            g = CB64.g32(y, gy, act)
            gs = CB64.gs32(g, scale)
            if "gs" in res:
                SC._same(SC._np(res["gs"]), gs, "gs")
            if "grad_shift" in res:
                SC._same(SC._np(res["grad_shift"]), np.asarray(CB64.grad_shift32(g), np.float32), "grad_shift")
            if "grad_w" in res:
                ref, K, mag = CB64.grad_w64(c, x, gs)
                SC._within_np(SC._np(res["grad_w"]), ref, CB64.bound32(K, mag), "grad_w")

        return SC.Plan(args, data, lambda ptr, st: _call(ptr, st, need), check, refuse=lambda ptr, st: (_call(ptr, st, need - 1), -3))

    return make


CASES = [SC.Case("conv_backward:all", ("s3r_conv_backward",), "conv_backward", _conv_backward(("gs", "grad_w", "grad_shift")), mutant=True),
         SC.Case("conv_backward:grad_w-only", ("s3r_conv_backward",), "conv_backward", _conv_backward(("grad_w",)))]
_IDS = [c.id for c in CASES]


def test_the_pre_states_are_documented_as_safe(lib):
    """the header comment of the entry says what a NaN does, so the NaN pre-state of every float buffer may be read"""
    import os
    with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "s3r.h")) as f:
        text = f.read()
    at = text.index("int s3r_conv_backward(")
    comment = text[text[:at].rfind("/*"):at]
    for case in CASES:
        plan = case.plan(lib, None)
        assert 0 < plan.nbytes <= SC.CAP_BYTES
        for a in plan.args:
            assert SC.safe_prestate(a, comment) == "NaN (header)", a.name


@pytest.mark.parametrize("case", CASES, ids=_IDS)
def test_delayed_producer(s3r, lib, gate, case):
    TS.test_delayed_producer(s3r, lib, gate, case)


def test_misplaced_stream_is_seen(s3r, lib, gate):
    """the instrument needs its two streams on different hardware queues.  tests/test_streams_gpu.py reaches its own mutants after 41
    delayed-producer runs, each on a stream of its own: by then every stream of torch's pool has been used once.  This file has two such
    runs, so it uses the rest of the pool once first (measured here without that: the second stream waited behind the gate, and the
    instrument said "inconclusive")"""
    import torch
    for _ in range(40):
        with torch.cuda.stream(torch.cuda.Stream()):
            torch.zeros(1, device=TS.DEV)
    torch.cuda.synchronize()
    TS.test_misplaced_stream_is_seen(s3r, lib, gate, CASES[0])


@pytest.mark.parametrize("case", CASES, ids=_IDS)
def test_capture_and_replay(s3r, lib, case):
    TS.test_capture_and_replay(s3r, lib, case)


def test_refused_call_is_not_captured(s3r, lib):
    TS.test_refused_call_is_not_captured(s3r, lib, CASES[0])
