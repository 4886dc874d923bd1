"""What the Python layer (modules.py, ops.py) enqueues, as tests/golden/module_trace_golden.json pins it: every C-ABI entry point opens
a profiler scope, so the ordered profiler records (s3r_profile_detail(1)) of one module call are the trace of that call.

Shared by tests/golden/make_module_trace_golden.py (which writes the file, and with --hashes the sha256 of every result) and
tests/test_module_trace_gpu.py (which compares with it).  Models are seeded with `s3r.seed_module(model, seed=0)`, renders come from
`s3r.synthetic_pairs`; every case runs on a model of its own (a copy of a seeded one that never ran), so its records hold the weight
packing and the arena's first use and do not depend on the cases before it.
"""
from __future__ import annotations

import copy
import dataclasses
import functools
import hashlib
from typing import Callable

import s3r
from s3r import arch_spec as spec

from tests import _dispatch_cases as DC

FIELDS = DC.REC_INTS + DC.REC_DOUBLES      # the golden holds a record as one row of these, a case as one line of rows
CAP = 1024                         # profiler records per case: the largest (a whole training step with batch statistics) takes a fraction


@dataclasses.dataclass(frozen=True)
class Case:
    id: str
    make: Callable                 # (torch) -> state: models and inputs on the device; nothing of it is traced
    run: Callable                  # (state) -> the tensors the call returns (a training case: after .backward())
    max_chunk: int = 0             # s3r.modules.MAX_CHUNK while `run` runs (0: as it is)
    model: Callable = None         # (state) -> the module whose gradients (and buffers) a training case leaves behind


@functools.lru_cache(maxsize=None)
def _seeded(kind, precision, winograd):
    cls = {"voxel": s3r.Stereo2Voxel, "point": s3r.Stereo2Point}[kind]
    return s3r.seed_module(cls(precision, winograd), seed=0).to("cuda:0")


def _model(kind, precision="fp32", winograd=None):
    return copy.deepcopy(_seeded(kind, precision, winograd))


def _pairs(B, u8=False):
    left, right = s3r.synthetic_pairs(B, seed=0, device="cuda:0")
    if u8:
        import torch
        return tuple((t * 255).round().to(torch.uint8) for t in (left, right))
    return left, right


def _rand(torch, shape, seed):
    return torch.rand(shape, generator=torch.Generator(device="cpu").manual_seed(seed)).to("cuda:0")


def _tup(y):
    return tuple(y) if isinstance(y, (tuple, list)) else (y,)


def _net(cid, kind, B, call, precision="fp32", winograd=None, u8=False, max_chunk=0):
    """`call(model, left, right)` on a fresh network"""
    return Case(cid, lambda torch: (_model(kind, precision, winograd),) + _pairs(B, u8), lambda s: _tup(call(*s)), max_chunk)


def _second_call():
    def make(torch):
        s = (_model("voxel"),) + _pairs(2)
        s[0](*s[1:])
        torch.cuda.synchronize()
        return s
    return Case("voxel-fp32-B2-second-call", make, lambda s: _tup(s[0](*s[1:])))


def _decoder_upto():
    def make(torch):
        m = _model("voxel")
        return m.decoder, _rand(torch, (1, 2 * spec.FEAT_C, spec.MAX_DISP, spec.FEAT_HW, spec.FEAT_HW), 3)
    return Case("decoder-upto-v3-B1", make, lambda s: _tup(s[0](s[1], upto="v3")))


def _train(cid, kind, B, step, target, **kw):
    """forward + loss + .backward() on a fresh network: `step(model, left, right, *target(torch))` returns (outputs..., loss)"""
    def make(torch):
        return (_model(kind),) + _pairs(B) + tuple(target(torch))

    def run(s):
        out = _tup(step(*s, **kw))
        out[-1].backward()
        return out
    return Case(cid, make, run, model=lambda s: s[0])


def _voxel_step(m, l, r, gt, batch_stats):
    y = m.differentiable(l, r, batch_stats=batch_stats)
    return y, s3r.VoxelBCELoss()(y, gt)


def _point_step(m, l, r, target):
    y = m.differentiable(l, r)
    return y, s3r.ChamferDistance()(y, target)


def _disparity_step(m, l, r, gt_l, gt_r):
    dl, dr = m.differentiable_disparity(l, r, full_resolution=True)
    return dl, dr, s3r.DisparityLoss()(dl, gt_l) + s3r.DisparityLoss()(dr, gt_r)


def _tail_step(m, l, r, gt):
    y = m.decoder.differentiable_tail(m.trunk_features(l, r, upto="d2"))
    return y, s3r.VoxelBCELoss()(y, gt)


def _occupancy(B):
    return lambda torch: ((_rand(torch, (B, spec.VOX, spec.VOX, spec.VOX), 7) > 0.5).float(),)


def _disparity_gt(torch):
    # disparities in render pixels; about a tenth of the pixels invalid (negative), as the background of an EXR map
    return tuple(_rand(torch, (1, spec.IMG_HW, spec.IMG_HW), seed) * 70.0 - 7.0 for seed in (11, 12))


CASES = [
    _net("voxel-fp32-B1", "voxel", 1, lambda m, l, r: m(l, r)),
    _net("voxel-fp32-B3-u8", "voxel", 3, lambda m, l, r: m(l, r), u8=True),
    _net("voxel-direct-B1", "voxel", 1, lambda m, l, r: m(l, r), winograd=False),
    _net("voxel-bf16-B2", "voxel", 2, lambda m, l, r: m(l, r), precision="bf16"),
    _second_call(),
    _net("point-fp32-B2", "point", 2, lambda m, l, r: m(l, r)),
    _net("point-bf16-B1", "point", 1, lambda m, l, r: m(l, r), precision="bf16"),
    _net("disparity-wta-B2", "voxel", 2, lambda m, l, r: m.disparity(l, r, readout="wta")),
    _net("disparity-soft-full-confidence-B2", "voxel", 2,
         lambda m, l, r: m.disparity(l, r, readout="soft", full_resolution=True, confidence=True)),
    _net("disparity-soft-bf16-B1", "voxel", 1, lambda m, l, r: m.disparity(l, r, readout="soft"), precision="bf16"),
    _net("encoder-upto-e3-B1", "voxel", 1, lambda m, l, r: m.encoder(l, upto="e3")),
    _decoder_upto(),
    _net("trunk-features-d2-B1", "voxel", 1, lambda m, l, r: m.trunk_features(l, r, upto="d2")),
    _net("head-features-B1", "voxel", 1, lambda m, l, r: m.head_features(l, r)),
    _net("point-latent-B1", "point", 1, lambda m, l, r: m.latent(l, r)),
    _net("stereo-features-B1", "voxel", 1, lambda m, l, r: m.stereo_features(l, r)),
    _net("chunks-2-2-1-voxel", "voxel", 5, lambda m, l, r: m(l, r), max_chunk=2),
    _net("chunks-2-2-1-point", "point", 5, lambda m, l, r: m(l, r), max_chunk=2),
    _net("chunks-2-2-1-disparity-soft", "voxel", 5, lambda m, l, r: m.disparity(l, r, readout="soft"), max_chunk=2),
    _train("train-voxel-B2", "voxel", 2, _voxel_step, _occupancy(2), batch_stats=False),
    _train("train-voxel-B2-batch-stats", "voxel", 2, _voxel_step, _occupancy(2), batch_stats=True),
    _train("train-point-B1", "point", 1, _point_step, lambda torch: (_rand(torch, (1, spec.N_POINTS, 3), 9),)),
    _train("train-disparity-full-B1", "voxel", 1, _disparity_step, _disparity_gt),
    _train("train-tail-from-d2-B1", "voxel", 1, _tail_step, _occupancy(1)),
]
IDS = [c.id for c in CASES]
assert len(set(IDS)) == len(IDS)
BY_ID = {c.id: c for c in CASES}


def trace(lib, case, patch_chunk):
    """(records, state, outputs) of one case.  `patch_chunk(n)` sets s3r.modules.MAX_CHUNK for the caller's lifetime of choice
    (monkeypatch in the test, a try / finally in the generator)."""
    import torch
    state = case.make(torch)
    torch.cuda.synchronize()
    if case.max_chunk:
        patch_chunk(case.max_chunk)
    assert lib.s3r_profile_enable(CAP) == 0 and lib.s3r_profile_detail(1) == 0
    try:
        out = case.run(state)
        torch.cuda.synchronize()
        records = DC._read_records(lib, CAP)          # (asserts that fewer than CAP came back: nothing was dropped)
    finally:
        lib.s3r_profile_detail(0)
        lib.s3r_profile_enable(0)
    return records, state, out


def rows(records):
    return [[r[k] for k in FIELDS] for r in records]


def dump_golden(doc, f):
    """the golden's text: the header keys, then one line per case (a case's rows side by side: the file is data, not prose)"""
    import json
    head = {k: v for k, v in doc.items() if k != "cases"}
    f.write(json.dumps(head, sort_keys=True)[:-1] + ', "cases": {\n')
    f.write(",\n".join(f"{json.dumps(cid)}: {json.dumps(doc['cases'][cid])}" for cid in sorted(doc["cases"])))
    f.write("\n}}\n")


def _sha(t):
    if t is None:
        return "none"
    import torch
    t = t.detach().contiguous().cpu()
    return f"{t.dtype}{tuple(t.shape)}:" + hashlib.sha256(t.reshape(-1).view(torch.uint8).numpy().tobytes()).hexdigest()


def hashes(case, state, out):
    """sha256 of every tensor the case returned; a training case: of every parameter's .grad and of every buffer afterwards too"""
    doc = {"out": [_sha(t) for t in out]}
    if case.model is not None:
        m = case.model(state)
        doc["grad"] = {k: _sha(p.grad) for k, p in m.named_parameters()}
        doc["buffers"] = {k: _sha(b) for k, b in m.named_buffers()}
    return doc
