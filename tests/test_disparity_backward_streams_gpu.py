"""The stream contract of s3r_disparity_soft_backward, s3r_disparity_loss_forward and s3r_disparity_loss_backward, on the instruments of
tests/test_streams_gpu.py (imported, used as they are): the call behind a delayed producer on a non-blocking stream carries the bits of
the NULL-stream call; the same call on a second idle stream is SEEN by the instrument; a captured call replays on new data in the same
buffers with the eager bits; a refused call inside a captured region returns its code and leaves nothing in the graph.  The cases are
recipes in the form of tests/_stream_cases.py (Arg / Plan / Case), one per entry: the backward at the ragged upsampled shape of
tests/_dispbwd64.py (refused by a shape whose LDS is too large), the two loss entries at (3, 2500) (refused by a negative beta)."""
import os

import numpy as np
import pytest

from tests import _dispbwd64 as R
from tests import _stream_cases as SC
from tests import test_streams_gpu as TS
from tests.test_streams_gpu import gate, lib      # noqa: F401  (the instruments' fixtures)

pytestmark = pytest.mark.gpu
F32, I32 = SC.F32, SC.I32
CASE = R.UPSAMPLED
TAU, SCALE, BETA = 0.7, 8.0, 1.0
LOSS = (3, 2500)


def _soft_backward(lib, dev):
    B, C, H, W, D, OH, OW = CASE
    names = ("feat_l", "feat_r", "grad_disp_l", "grad_disp_r")
    args = [SC.Arg("feat_l", (B, C, H, W), F32, "in"), SC.Arg("feat_r", (B, C, H, W), F32, "in"),
            SC.Arg("grad_disp_l", (B, OH, OW), F32, "in"), SC.Arg("grad_disp_r", (B, OH, OW), F32, "in"),
            SC.Arg("grad_left", (B, C, H, W), F32, "out"), SC.Arg("grad_right", (B, C, H, W), F32, "out")]

    def data(k):
        return {n: SC._t(a) for n, a in zip(names, R.random_case(CASE, seed=30 + k))}

    def _call(ptr, st, c, w, d):
        return lib.s3r_disparity_soft_backward(ptr["feat_l"], ptr["feat_r"], 0, ptr["grad_disp_l"], ptr["grad_disp_r"], ptr["grad_left"],
                                               ptr["grad_right"], B, c, H, w, d, TAU, OH, OW, SCALE, st)

    def check(d, res):
        (gl, gr), (bl, br) = R.backward64(*(SC._np(d[n]) for n in names), D, TAU, (OH, OW), SCALE)
        SC._within_np(SC._np(res["grad_left"]), gl, bl, "grad_left")
        SC._within_np(SC._np(res["grad_right"]), gr, br, "grad_right")

    # the refused form: a shape whose LDS is too large (C 64, W 200: S3R_ERR_INVALID before anything is enqueued), every pointer valid
    return SC.Plan(args, data, lambda ptr, st: _call(ptr, st, C, W, D), check, refuse=lambda ptr, st: (_call(ptr, st, 64, 200, 4), -1))


def _loss_data(k):
    B, P = LOSS
    rng = np.random.default_rng(P + 13 * k)
    gt = (np.abs(rng.standard_normal((B, P))) * 20).astype(np.float32)
    pred = (gt + rng.standard_normal((B, P)) * 2).astype(np.float32)
    u = rng.random((B, P))
    gt[u < 0.2] = np.inf
    gt[(u >= 0.2) & (u < 0.25)] = -1.0
    return pred, gt


def _loss_forward(lib, dev):
    B, P = LOSS
    args = [SC.Arg("pred", (B, P), F32, "in"), SC.Arg("gt", (B, P), F32, "in"), SC.Arg("loss_sum", (B,), F32, "out"),
            SC.Arg("count", (B,), I32, "out"), SC.Arg("loss_elem", (B, P), F32, "out")]

    def data(k):
        p, t = _loss_data(k)
        return {"pred": SC._t(p), "gt": SC._t(t)}

    def _call(ptr, st, beta):
        return lib.s3r_disparity_loss_forward(ptr["pred"], ptr["gt"], beta, ptr["loss_sum"], ptr["count"], ptr["loss_elem"], B, P, st)

    def check(d, res):
        want, ok = R.loss32(SC._np(d["pred"]), SC._np(d["gt"]), BETA)
        SC._same(SC._np(res["loss_elem"]), want, "loss_elem")
        SC._same(SC._np(res["loss_sum"]), R.loss_sum32(want), "loss_sum")
        SC._same(SC._np(res["count"]), ok.sum(1).astype(np.int32), "count")

    return SC.Plan(args, data, lambda ptr, st: _call(ptr, st, BETA), check, refuse=lambda ptr, st: (_call(ptr, st, -1.0), -1))


def _loss_backward(lib, dev):
    B, P = LOSS
    args = [SC.Arg("pred", (B, P), F32, "in"), SC.Arg("gt", (B, P), F32, "in"), SC.Arg("grad_scale", (B,), F32, "in"),
            SC.Arg("grad_pred", (B, P), F32, "out")]

    def data(k):
        p, t = _loss_data(k)
        return {"pred": SC._t(p), "gt": SC._t(t), "grad_scale": SC._t(np.linspace(0.5, 1.5, B).astype(np.float32) / P)}

    def _call(ptr, st, beta):
        return lib.s3r_disparity_loss_backward(ptr["pred"], ptr["gt"], ptr["grad_scale"], beta, ptr["grad_pred"], B, P, st)

    return SC.Plan(args, data, lambda ptr, st: _call(ptr, st, BETA),
                   lambda d, res: SC._same(SC._np(res["grad_pred"]),
                                           R.loss_grad32(SC._np(d["pred"]), SC._np(d["gt"]), SC._np(d["grad_scale"]), BETA), "grad_pred"),
                   refuse=lambda ptr, st: (_call(ptr, st, -1.0), -1))


CASES = [SC.Case("disparity_soft_backward:upsampled", ("s3r_disparity_soft_backward",), "disparity_backward", _soft_backward, mutant=True),
         SC.Case("disparity_loss_forward", ("s3r_disparity_loss_forward",), "disparity_backward", _loss_forward),
         SC.Case("disparity_loss_backward", ("s3r_disparity_loss_backward",), "disparity_backward", _loss_backward)]
_IDS = [c.id for c in CASES]


def test_the_pre_states_are_documented_as_safe(lib):
    """the header comment of each entry says that a NaN propagates through its arithmetic, so the NaN pre-state of every float buffer
    may be read; an int32 output is never read"""
    with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "s3r.h")) as f:
        text = f.read()
    for case in CASES:
        at = text.index(f"int {case.entries[0]}(")
        comment = text[text[:at].rfind("/*"):at]
        assert "hip_stream" in comment and "hipStream_t" in comment and "propagates through" in comment
        plan = case.plan(lib, None)
        assert 0 < plan.nbytes <= SC.CAP_BYTES
        for a in plan.args:
            assert SC.safe_prestate(a, comment) == ("never read" if a.dtype == I32 else "NaN (header)"), a.name


@pytest.mark.parametrize("case", CASES, ids=_IDS)
def test_delayed_producer(s3r, lib, gate, case):
    TS.test_delayed_producer(s3r, lib, gate, case)


def test_misplaced_stream_is_seen(s3r, lib, gate):
    """the instrument needs its two streams on different hardware queues, and later files must meet torch's pool of 32 streams at the
    phase they have without this file (tests/test_batchnorm_train_streams_gpu.py has the measurement): this file takes 3 (delayed
    producer) + 2 (this test) + 3 (capture) + 3 (refusal) = 11 streams beside the loop below; with 53 here that is 64, a multiple of
    the pool size"""
    import torch
    for _ in range(53):
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
