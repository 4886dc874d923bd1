"""s3r_augment_pair on the device, bit for bit against tests/_augment64.py's restatement, in guarded buffers (tests/_guard.py): every
op alone and all together, 3 and 4 channels, with and without disparity maps, over shapes that cross every path of the order; the
identity against the host conversion; a sample's bits alone, at any position of any batch, at element-aligned pointers and for any
scratch contents; what the two views share; and the stream contract on the instruments of tests/test_streams_gpu.py (imported, used
as they are): behind a delayed producer, captured and replayed on new ids and renders, a refused call inside a captured region."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from tests import _augment64 as R
from tests import _guard as G
from tests import _stream_cases as SC
from tests import test_streams_gpu as TS
from tests.test_streams_gpu import gate, lib      # noqa: F401  (the instruments' fixtures)

pytestmark = pytest.mark.gpu
DEV = TS.DEV
F32, I32, U8 = torch.float32, torch.int32, torch.uint8


def _ids32(ids):
    """(B,) int64 ids as the (2 B,) int32 words the guarded buffers hold (tests/_guard.py has no 64-bit pattern)"""
    return torch.from_numpy(np.asarray(ids, np.int64).view(np.int32).copy())


def _bits(a):
    return np.ascontiguousarray(a).view(np.int32)


def device_call(s3r, lib, cfg, left, right, ids, dl=None, dr=None, skew=0, scratch_fill="nan"):
    """the call on guarded buffers; returns the outputs as numpy arrays after every guard has been checked"""
    L = s3r._lib
    B, ch, H, W = left.shape
    desc = R.to_cfg(s3r, cfg).desc(ch)
    need = lib.s3r_augment_scratch_elems(C.byref(desc), B, H, W)
    assert need >= 0, lib.s3r_last_error()
    with G.skews(lambda name, dtype, role: skew):
        bufs = {"left": G.Guarded("left", left.shape, U8, DEV, "in", data=torch.from_numpy(left).to(DEV)),
                "right": G.Guarded("right", right.shape, U8, DEV, "in", data=torch.from_numpy(right).to(DEV)),
                "ids": G.Guarded("ids", (2 * B,), I32, DEV, "in", data=_ids32(ids).to(DEV), skew=2 * skew),
                "ol": G.Guarded("ol", (B, 3, H, W), F32, DEV, "out"), "or": G.Guarded("or", (B, 3, H, W), F32, DEV, "out"),
                "scratch": G.Guarded("scratch", (max(need, 1),), F32, DEV, "scratch", fill=scratch_fill)}
        if dl is not None:
            bufs["dl"] = G.Guarded("dl", dl.shape, F32, DEV, "in", data=torch.from_numpy(dl).to(DEV))
            bufs["dr"] = G.Guarded("dr", dr.shape, F32, DEV, "in", data=torch.from_numpy(dr).to(DEV))
            bufs["odl"] = G.Guarded("odl", dl.shape, F32, DEV, "out")
            bufs["odr"] = G.Guarded("odr", dr.shape, F32, DEV, "out")
    p = {n: b.ptr for n, b in bufs.items()}
    torch.cuda.synchronize()
    rc = lib.s3r_augment_pair(C.byref(desc), p["left"], p["right"], p["ids"], p.get("dl"), p.get("dr"), p["ol"], p["or"], p.get("odl"),
                              p.get("odr"), B, H, W, p["scratch"] if need else None, need, None)
    assert rc == 0, lib.s3r_last_error()
    torch.cuda.synchronize()
    G.check_all(*bufs.values())
    names = ["ol", "or"] + (["odl", "odr"] if dl is not None else [])
    return [bufs[n].t.cpu().numpy() for n in names]


def _same(got, want, what):
    assert len(got) == len(want)
    for i, (g, w) in enumerate(zip(got, want)):
        bad = np.argwhere(_bits(g) != _bits(w))
        assert not bad.size, f"{what}: output {i}: first of {len(bad)} differing elements at {tuple(bad[0])}: " \
                             f"got {g[tuple(bad[0])]!r}, want {w[tuple(bad[0])]!r}"


# ---------------------------------------------------------------- bit for bit against the restatement
@pytest.mark.parametrize("ch", [3, 4])
@pytest.mark.parametrize("name", list(R.CONFIGS))
def test_bits_of_the_restatement(s3r, lib, name, ch):
    cfg = R.CONFIGS[name]
    for n, (H, W) in enumerate(R.SHAPES):
        B = 3
        ids = [R.COVERAGE_IDS[(7 * n + 5 * i + ch) % 64] for i in range(B)]
        left, right = R.renders(B, ch, H, W, 100 * n + ch)
        for with_disp in (False, True):
            dl, dr = R.disparities(B, H, W, n) if with_disp else (None, None)
            got = device_call(s3r, lib, cfg, left, right, ids, dl, dr)
            _same(got, R.augment32(cfg, left, right, ids, dl, dr), f"{name} ch={ch} {H}x{W} disp={with_disp}")


def test_network_size_once(s3r, lib):
    """224 x 224 at B = 2, RGBA, every op on, with disparity maps"""
    cfg, (H, W) = R.CONFIGS["all"], R.BIG
    left, right = R.renders(2, 4, H, W, 224)
    dl, dr = R.disparities(2, H, W, 224)
    ids = [2 ** 40 + 3, -5]                                              # both words of an id enter the counter
    _same(device_call(s3r, lib, cfg, left, right, ids, dl, dr), R.augment32(cfg, left, right, ids, dl, dr), "224 x 224")


def test_identity_is_the_host_conversion(s3r, lib):
    left, right = R.renders(2, 3, 17, 31, 1)
    got = device_call(s3r, lib, R.IDENTITY, left, right, [1, 2])
    _same(got, [s3r.data.renders_to_float(left), s3r.data.renders_to_float(right)], "identity, RGB")
    left, right = R.renders(2, 4, 17, 31, 2)
    got = device_call(s3r, lib, R.IDENTITY, left, right, [1, 2])
    want = [s3r.data.renders_to_float(np.stack([s3r.data.composite_over_white_u8(s.transpose(1, 2, 0)).transpose(2, 0, 1) for s in x]))
            for x in (left, right)]
    _same(got, want, "identity, RGBA")
    # ... and through the package: ops.augment_pair / StereoAugment on torch tensors, the kept buffers at the same addresses
    tl, tr = torch.from_numpy(left).to(DEV), torch.from_numpy(right).to(DEV)
    ids = torch.tensor([1, 2], dtype=torch.int64, device=DEV)
    ol, orr = s3r.ops.augment_pair(tl, tr, ids, s3r.AugmentConfig.identity())
    _same([ol.cpu().numpy(), orr.cpu().numpy()], want, "ops.augment_pair")
    aug = s3r.StereoAugment(R.to_cfg(s3r, R.CONFIGS["all"]))
    dl, dr = (torch.from_numpy(d).to(DEV) for d in R.disparities(2, 17, 31, 3))
    first = aug(tl, tr, ids, dl, dr)
    ptrs = [t.data_ptr() for t in first]
    want = R.augment32(R.CONFIGS["all"], left, right, [1, 2], dl.cpu().numpy(), dr.cpu().numpy())
    _same([t.cpu().numpy() for t in first], want, "StereoAugment")
    again = aug(tl, tr, ids + 7, dl, dr)
    assert [t.data_ptr() for t in again] == ptrs
    _same([t.cpu().numpy() for t in again], R.augment32(R.CONFIGS["all"], left, right, [8, 9], dl.cpu().numpy(), dr.cpu().numpy()),
          "StereoAugment, new ids")


# ---------------------------------------------------------------- a sample's bits do not depend on where it is computed
@functools.lru_cache(maxsize=None)
def _batch65():
    H, W = 17, 31
    ids = R.COVERAGE_IDS + [64]
    left, right = R.renders(65, 4, H, W, 65)
    dl, dr = R.disparities(65, H, W, 65)
    return ids, left, right, dl, dr, R.augment32(R.CONFIGS["all"], left, right, ids, dl, dr)


def test_whole_coverage_batch(s3r, lib):
    """B = 65 (a second round of the per-pair wave's lanes would start at 64): ids 0..63 draw every permutation and shift sign"""
    ids, left, right, dl, dr, want = _batch65()
    _same(device_call(s3r, lib, R.CONFIGS["all"], left, right, ids, dl, dr), want, "B = 65")


@pytest.mark.parametrize("rows", [(0,), (17,), (64,), (40, 5, 64), (64, 0, 33)])
@pytest.mark.parametrize("skew,fill", [(0, "nan"), (1, "nan"), (3, "zero")])
def test_a_sample_alone_or_elsewhere_has_the_same_bits(s3r, lib, rows, skew, fill):
    """samples of the B = 65 batch alone (B = 1) and at other positions of a B = 3 batch, at pointers one and three elements past an
    aligned address (bytes for the renders), NaN- and zero-filled scratch"""
    ids, left, right, dl, dr, want = _batch65()
    rows = list(rows)
    got = device_call(s3r, lib, R.CONFIGS["all"], left[rows], right[rows], [ids[r] for r in rows], dl[rows], dr[rows], skew=skew,
                      scratch_fill=fill)
    _same(got, [w[rows] for w in want], f"rows {rows} skew {skew} scratch {fill}")


def test_views_share_everything_but_the_noise(s3r, lib):
    left, _ = R.renders(3, 4, 16, 32, 9)
    quiet = R.CONFIGS["all"]._replace(noise_sigma=0.0)
    a, b = device_call(s3r, lib, quiet, left, left, [3, 4, 5])
    assert np.array_equal(_bits(a), _bits(b))
    a, b = device_call(s3r, lib, R.CONFIGS["all"], left, left, [3, 4, 5])
    assert not np.array_equal(_bits(a), _bits(b))


# ---------------------------------------------------------------- stream contract
B_S, H_S, W_S = 3, 33, 31
CFG_S = R.CONFIGS["all"]


def _plan(lib, dev):
    import s3r
    desc = R.to_cfg(s3r, CFG_S).desc(4)
    need = lib.s3r_augment_scratch_elems(C.byref(desc), B_S, H_S, W_S)
    args = [SC.Arg("left", (B_S, 4, H_S, W_S), U8, "in"), SC.Arg("right", (B_S, 4, H_S, W_S), U8, "in"), SC.Arg("ids", (2 * B_S,), I32, "in"),
            SC.Arg("dl", (B_S, H_S, W_S), F32, "in"), SC.Arg("dr", (B_S, H_S, W_S), F32, "in"),
            SC.Arg("ol", (B_S, 3, H_S, W_S), F32, "out"), SC.Arg("or", (B_S, 3, H_S, W_S), F32, "out"),
            SC.Arg("odl", (B_S, H_S, W_S), F32, "out"), SC.Arg("odr", (B_S, H_S, W_S), F32, "out"), SC.Arg("scratch", (need,), F32, "scr")]

    def data(k):
        left, right = R.renders(B_S, 4, H_S, W_S, 50 + k)
        dl, dr = R.disparities(B_S, H_S, W_S, 50 + k)
        ids = [11 + 20 * k, 2 + 20 * k, 2 ** 33 + k]
        return {"left": SC._t(left), "right": SC._t(right), "ids": _ids32(ids), "dl": SC._t(dl), "dr": SC._t(dr), "_ref": ids}

    def _call(ptr, st, d):
        return lib.s3r_augment_pair(C.byref(d), ptr["left"], ptr["right"], ptr["ids"], ptr["dl"], ptr["dr"], ptr["ol"], ptr["or"], ptr["odl"],
                                    ptr["odr"], B_S, H_S, W_S, ptr["scratch"], need, st)

    def call(ptr, st):
        return _call(ptr, st, desc)

    def refuse(ptr, st):
        bad = R.to_cfg(s3r, CFG_S).desc(4)
        bad.flags = 3                                                    # an unknown flag bit
        return _call(ptr, st, bad), -1

    def check(d, res):
        want = R.augment32(CFG_S, SC._np(d["left"]), SC._np(d["right"]), d["_ref"], SC._np(d["dl"]), SC._np(d["dr"]))
        _same([SC._np(res[n]) for n in ("ol", "or", "odl", "odr")], want, "stream case")

    return SC.Plan(args, data, call, check, refuse=refuse)


CASE = SC.Case("augment:all-rgba-disp", ("s3r_augment_scratch_elems", "s3r_augment_pair"), "augment", _plan)
PAD_STREAMS = 29       # this file takes 1 (delayed producer) + 1 (capture) + 1 (refusal) = 3 of torch's pool of 32; 32 with these


def test_delayed_producer(s3r, lib, gate):
    TS.test_delayed_producer(s3r, lib, gate, CASE)


def test_capture_and_replay(s3r, lib):
    """captured once, replayed on new ids, renders and maps in the same buffers: fresh draws, the eager bits"""
    TS.test_capture_and_replay(s3r, lib, CASE)


def test_refused_call_is_not_captured(s3r, lib):
    TS.test_refused_call_is_not_captured(s3r, lib, CASE)
    # later files meet torch's round-robin pool of 32 streams at the phase they have without this file (the measurement:
    # tests/test_batchnorm_train_streams_gpu.py)
    for _ in range(PAD_STREAMS):
        with torch.cuda.stream(torch.cuda.Stream()):
            torch.zeros(1, device=DEV)
    torch.cuda.synchronize()
