"""The stream contract of s3r_cost_volume_backward, on the instruments of tests/test_streams_gpu.py (used as they are): the call behind a
delayed producer on a non-blocking stream carries the bits of the NULL-stream call; the same call on a second idle stream is SEEN by
the instrument; a captured call replays on new data in the same buffers with the eager bits; a refused call inside a captured region
returns its code and leaves nothing in the graph.  The cases are recipes in the form of tests/_stream_cases.py (Arg / Plan / Case): one
small shape, (3, 2, 6, 5, 13) — 390 outputs per side: a full and a partial workgroup, rows that wrap inside a wavefront —, with both
gradients and with grad_right alone."""
import os

import pytest

from tests import _costvol64 as R
from tests import _stream_cases as SC
from tests import test_streams_gpu as TS
from tests.test_streams_gpu import gate, lib      # noqa: F401  (the instruments' fixtures)

pytestmark = pytest.mark.gpu
F32 = SC.F32
CASE = R.CASES[4]


def _cost_volume_backward(outs):
    B, Cc, D, H, W = CASE

    def make(lib, dev):
        args = [SC.Arg("grad_volume", (B, 2 * Cc, D, H, W), F32, "in")] + [SC.Arg(o, (B, Cc, H, W), F32, "out") for o in outs]

        def data(k):
            return {"grad_volume": SC._t(R.random_gv(CASE, seed=40 + k))}

        def _call(ptr, st, max_disp):
            return lib.s3r_cost_volume_backward(ptr["grad_volume"], ptr.get("grad_left"), ptr.get("grad_right"), B, Cc, max_disp, H, W, st)

        def check(d, res):
            gl, gr = R.backward32(SC._np(d["grad_volume"]))
            if "grad_left" in res:
                SC._same(SC._np(res["grad_left"]), gl, "grad_left")
            if "grad_right" in res:
                SC._same(SC._np(res["grad_right"]), gr, "grad_right")

        # the refused form: max_disp = 0 with every pointer valid (S3R_ERR_INVALID, "dims must be positive")
        return SC.Plan(args, data, lambda ptr, st: _call(ptr, st, D), check, refuse=lambda ptr, st: (_call(ptr, st, 0), -1))

    return make


CASES = [SC.Case("cost_volume_backward:both", ("s3r_cost_volume_backward",), "cost_volume_backward",
                 _cost_volume_backward(("grad_left", "grad_right")), mutant=True),
         SC.Case("cost_volume_backward:grad_right-only", ("s3r_cost_volume_backward",), "cost_volume_backward",
                 _cost_volume_backward(("grad_right",)))]
_IDS = [c.id for c in CASES]


def test_the_pre_states_are_documented_as_safe(lib):
    """the header comment of the entry says what a NaN does, so the NaN pre-state of every float buffer may be read"""
    with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "s3r.h")) as f:
        text = f.read()
    at = text.index("int s3r_cost_volume_backward(")
    comment = text[text[:at].rfind("/*"):at]
    assert "hip_stream" in comment and "hipStream_t" in comment
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
    runs, so it uses the rest of the pool once first (as tests/test_conv_backward_streams_gpu.py does, for the reason measured there)"""
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
