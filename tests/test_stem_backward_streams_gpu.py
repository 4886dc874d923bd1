"""The stream contract of s3r_stem_backward, on the instruments of tests/test_streams_gpu.py (imported, used as they are): the call
behind a delayed producer on a non-blocking stream carries the bits of the NULL-stream call; the same call on a second idle stream is
SEEN by the instrument; a captured call replays on new data in the same buffers with the eager bits; a refused call inside a captured
region returns its code and leaves nothing in the graph.  The cases are recipes in the form of tests/_stream_cases.py (Arg / Plan / Case)
at three renders of 46^2 (m = 23: 529 positions, two chunks with a short one, 23 slices per image): 8-bit renders in two tensors with
both outputs — all five launches run — and fp32 renders in one tensor with grad_w alone."""
import os

import numpy as np
import pytest

from tests import _stem64 as S
from tests import _stream_cases as SC
from tests import test_streams_gpu as TS
from tests.test_streams_gpu import gate, lib      # noqa: F401  (the instruments' fixtures)

pytestmark = pytest.mark.gpu
F32, U8 = SC.F32, SC.U8
N, EDGE, ACT = 3, 46, "relu"
M = S.out_edge(EDGE)


def _stem(u8, n_left, outs):
    def make(lib, dev):
        need = lib.s3r_stem_backward_scratch_elems(N, EDGE)
        assert need == S.scratch_elems(N, EDGE) > 0
        rdt = U8 if u8 else F32
        rend = [SC.Arg("left", (n_left, 3, EDGE, EDGE), rdt, "in")]
        if n_left < N:
            rend.append(SC.Arg("right", (N - n_left, 3, EDGE, EDGE), rdt, "in"))
        oshape = {"grad_w": (32, 3, 3, 3), "grad_shift": (32,)}
        args = rend + [SC.Arg("y", (N, 32, M, M), F32, "in"), SC.Arg("grad_y", (N, 32, M, M), F32, "in"), SC.Arg("scale", (32,), F32, "in")] + \
               [SC.Arg(o, oshape[o], F32, "out") for o in outs] + [SC.Arg("scratch", (need,), F32, "scr")]

        def data(k):
            x, scale, y, gy = S.make(N, EDGE, seed=70 + k, act=ACT, u8=u8)
            d = {"left": SC._t(x[:n_left]), "y": SC._t(y), "grad_y": SC._t(gy), "scale": SC._t(scale)}
            if n_left < N:
                d["right"] = SC._t(x[n_left:])
            return d

        def _call(ptr, st, elems):
            return lib.s3r_stem_backward(ptr["left"], ptr.get("right"), n_left, int(u8), ptr["y"], ptr["grad_y"], ptr["scale"],
                                         ptr.get("grad_w"), ptr.get("grad_shift"), N, EDGE, 1, ptr["scratch"], elems, st)

        def check(d, res):
            x = np.concatenate([SC._np(d[n]) for n in ("left", "right") if n in d])
            y, gy, scale = (SC._np(d[n]) for n in ("y", "grad_y", "scale"))
            g = S.g32(y, gy, ACT)
            if "grad_shift" in outs:
                SC._same(SC._np(res["grad_shift"]), S.grad_shift32(g), "grad_shift")
            ref, K, mag = S.grad_w64(S.render32(x), S.gs32(g, scale))
            SC._within_np(SC._np(res["grad_w"]), ref, S.bound32(K, mag), "grad_w")

        return SC.Plan(args, data, lambda ptr, st: _call(ptr, st, need), check, refuse=lambda ptr, st: (_call(ptr, st, need - 1), -3))

    return make


ENTRY = ("s3r_stem_backward",)
CASES = [SC.Case("stem_backward:u8-two-tensors", ENTRY, "stem_backward", _stem(True, 1, ("grad_w", "grad_shift")), mutant=True),
         SC.Case("stem_backward:fp32-grad_w-only", ENTRY, "stem_backward", _stem(False, N, ("grad_w",)))]
_IDS = [c.id for c in CASES]


def test_the_pre_states_are_documented_as_safe(lib):
    """the header comment of the entry says what a NaN does, so the NaN pre-state of every float buffer may be read; every byte of an
    8-bit render is a sample"""
    with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "s3r.h")) as f:
        text = f.read()
    at = text.index("int s3r_stem_backward(")
    comment = text[text[:at].rfind("/*"):at]
    assert "hip_stream" in comment and "hipStream_t" in comment
    for case in CASES:
        plan = case.plan(lib, None)
        assert 0 < plan.nbytes <= SC.CAP_BYTES
        for a in plan.args:
            assert SC.safe_prestate(a, comment) == ("any byte is a render sample" if a.dtype == U8 else "NaN (header)"), a.name


@pytest.mark.parametrize("case", CASES, ids=_IDS)
def test_delayed_producer(s3r, lib, gate, case):
    TS.test_delayed_producer(s3r, lib, gate, case)


def test_misplaced_stream_is_seen(s3r, lib, gate):
    """the instrument needs its two streams on different hardware queues, and later files must meet torch's pool of 32 streams at the
    phase they have without this file (tests/test_batchnorm_train_streams_gpu.py has the measurement): this file takes 2 (delayed
    producer) + 2 (this test) + 2 (capture) + 2 (refusal) = 8 streams beside the loop below; with 56 here that is 64, a multiple of
    the pool size"""
    import torch
    for _ in range(56):
        with torch.cuda.stream(torch.cuda.Stream()):
            torch.zeros(1, device=TS.DEV)
    torch.cuda.synchronize()
    TS.test_misplaced_stream_is_seen(s3r, lib, gate, CASES[0])


@pytest.mark.parametrize("case", CASES, ids=_IDS)
def test_capture_and_replay(s3r, lib, case):
    TS.test_capture_and_replay(s3r, lib, case)


@pytest.mark.parametrize("case", CASES, ids=_IDS)
def test_refused_call_is_not_captured(s3r, lib, case):
    TS.test_refused_call_is_not_captured(s3r, lib, case)
