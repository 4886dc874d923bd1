"""s3r_voxel_surface_points on the device, bit for bit against tests/_surface64.py's restatement (points and n_faces), through the
C-ABI in guarded, poisoned buffers (tests/_guard.py): every grid kind over shapes that cross every path (one lane, ragged chunks, chunks
without a face, 256 voxels in a row, the prefix above the staged size), every point count around a wave, an empty sample in the middle
of the batch; a sample's bits alone, elsewhere in a batch, at element-aligned pointers, for any scratch contents, without n_faces and
twice; the dependence on seed, id and n_points; the stream contract on the instruments of tests/test_streams_gpu.py (imported, used as
they are); and the Python surface: the op and its module, test_point_net on grids, fit(variant="point") on grids, runner.py."""
import ctypes as C
import functools
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import _guard as G
from tests import _stream_cases as SC
from tests import _surface64 as R
from tests import test_streams_gpu as TS
from tests.test_streams_gpu import gate, lib      # noqa: F401  (the instruments' fixtures)

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = TS.DEV
F32, I32 = torch.float32, torch.int32


def _ids32(ids):
    """(B,) int64 ids as the (2 B,) int32 words the guarded buffers hold (tests/_guard.py has no 64-bit pattern)"""
    return torch.from_numpy(np.asarray(ids, np.int64).view(np.int32).copy())


def _bits(a):
    return np.ascontiguousarray(a).view(np.int32)


def device_call(lib, grids, ids, n_points, seed=R.SEED, threshold=0.5, skew=0, scratch_fill="nan", counts=True):
    """the call on guarded buffers; (points, n_faces or None) as numpy arrays after every guard has been checked"""
    grids = np.ascontiguousarray(grids, np.float32)
    B, D, H, W = grids.shape
    need = lib.s3r_voxel_surface_points_scratch_elems(B, D, H, W)
    assert need > 0, lib.s3r_last_error()
    with G.skews(lambda name, dtype, role: skew):
        bufs = {"occ": G.Guarded("occ", grids.shape, F32, DEV, "in", data=torch.from_numpy(grids).to(DEV)),
                "ids": G.Guarded("ids", (2 * B,), I32, DEV, "in", data=_ids32(ids).to(DEV), skew=2 * skew),
                "points": G.Guarded("points", (B, n_points, 3), F32, DEV, "out"),
                "scratch": G.Guarded("scratch", (need,), F32, DEV, "scratch", fill=scratch_fill)}
        if counts:
            bufs["n_faces"] = G.Guarded("n_faces", (B,), I32, DEV, "out")
    p = {n: b.ptr for n, b in bufs.items()}
    torch.cuda.synchronize()
    rc = lib.s3r_voxel_surface_points(p["occ"], threshold, p["ids"], seed, p["points"], p.get("n_faces"), B, D, H, W, n_points,
                                      p["scratch"], need, None)
    assert rc == 0, lib.s3r_last_error()
    torch.cuda.synchronize()
    G.check_all(*bufs.values())
    return bufs["points"].t.cpu().numpy(), bufs["n_faces"].t.cpu().numpy() if counts else None


def _same(got, want, what):
    for name, g, w in zip(("points", "n_faces"), got, want):
        if g is None:
            continue
        bad = np.argwhere(_bits(g) != _bits(w))
        assert not bad.size, f"{what}: {name}: first of {len(bad)} differing elements at {tuple(bad[0])}: " \
                             f"got {g[tuple(bad[0])]!r}, want {w[tuple(bad[0])]!r}"


# ---------------------------------------------------------------- bit for bit against the restatement
@pytest.mark.parametrize("kind,shape", R.CASES, ids=lambda v: str(v).replace(" ", ""))
def test_bits_of_the_restatement(lib, kind, shape):
    """B = 3 with an empty sample in the middle, every point count"""
    grids = R.batch(kind, shape)
    for n in R.N_POINTS:
        _same(device_call(lib, grids, R.IDS, n), R.surface32(grids, R.IDS, n), f"{kind} {shape} n_points={n}")


@functools.lru_cache(maxsize=None)
def _network_size():
    grids = np.stack([R.grid("ball", R.BIG), R.grid("checkerboard", R.BIG)])
    ids = [2 ** 40 + 3, -5]                                              # both words of an id enter the counter
    return grids, ids, R.surface32(grids, ids, 2048)


def test_network_size_once(lib):
    grids, ids, want = _network_size()
    assert want[1].tolist() == [2688, 98304]
    _same(device_call(lib, grids, ids, 2048), want, "32^3, 2048 points")


def test_prefix_above_the_staged_size(lib):
    """8 x 256 x 256: 8192 chunks, where the draw kernel bisects the prefix in global memory"""
    grids = R.grid("half", R.ABOVE_LDS)[None]
    _same(device_call(lib, grids, [R.IDS[2]], 257), R.surface32(grids, [R.IDS[2]], 257), "8 x 256 x 256")


# ---------------------------------------------------------------- a sample's bits do not depend on where it is computed
@functools.lru_cache(maxsize=None)
def _batch9():
    shape = (5, 7, 9)
    kinds = ["half", "specials", "empty", "checkerboard", "corner", "full", "gap", "half", "specials"]
    grids = np.stack([R.grid(k, shape, seed=i) for i, k in enumerate(kinds)])
    ids = [1, 0, 7, 2 ** 32 + 5, 3, -1, 10, 33, 2 ** 63 - 1]
    return grids, ids, R.surface32(grids, ids, 257)


def test_whole_batch(lib):
    grids, ids, want = _batch9()
    _same(device_call(lib, grids, ids, 257), want, "B = 9")


@pytest.mark.parametrize("rows", [(0,), (3,), (8,), (6, 2, 1), (8, 0, 3)])
@pytest.mark.parametrize("skew,fill,counts", [(0, "nan", True), (1, "nan", True), (3, "zero", True), (1, "nan", False)])
def test_a_sample_alone_or_elsewhere_has_the_same_bits(lib, rows, skew, fill, counts):
    """samples of the B = 9 batch alone and at other positions of a B = 3 batch, at pointers one and three elements past an aligned
    address, NaN- and zero-filled scratch, with and without n_faces"""
    grids, ids, want = _batch9()
    rows = list(rows)
    got = device_call(lib, grids[rows], [ids[r] for r in rows], 257, skew=skew, scratch_fill=fill, counts=counts)
    _same(got, [w[rows] for w in want], f"rows {rows} skew {skew} scratch {fill} counts {counts}")


def test_scratch_of_all_ones_bytes_and_two_runs(lib, s3r):
    grids, ids, want = _batch9()
    t = torch.from_numpy(grids).to(DEV)
    i = torch.tensor(ids, dtype=torch.int64, device=DEV)
    need = lib.s3r_voxel_surface_points_scratch_elems(*grids.shape)
    scratch = torch.full((need,), -1, dtype=torch.int32, device=DEV).view(F32)                  # 0xFF bytes
    out = (torch.empty(9, 257, 3, device=DEV), torch.empty(9, dtype=I32, device=DEV))
    for _ in range(2):                                                   # the second run meets the first one's scratch
        p, n = s3r.voxel_surface_points(t, i, 257, R.SEED, return_counts=True, out=out, scratch=scratch)
        _same((p.cpu().numpy(), n.cpu().numpy()), want, "0xFF scratch / second run")


# ---------------------------------------------------------------- dependence on the inputs
def test_seed_id_and_n_points(lib):
    grids, ids, want = _batch9()
    g, i = grids[:1], ids[:1]
    base = device_call(lib, g, i, 257)[0]
    other_seed = device_call(lib, g, i, 257, seed=R.SEED + 2 ** 32)[0]
    other_id = device_call(lib, g, [i[0] + 2 ** 32], 257)[0]
    assert not np.array_equal(_bits(base), _bits(other_seed)) and not np.array_equal(_bits(base), _bits(other_id))
    _same((other_seed, None), R.surface32(g, i, 257, seed=R.SEED + 2 ** 32), "seed high word")
    _same((other_id, None), R.surface32(g, [i[0] + 2 ** 32], 257), "id high word")
    for n in (1, 64, 300):                                               # the counter holds j, not n_points: a common prefix
        got = device_call(lib, g, i, n)[0]
        m = min(n, 257)
        assert np.array_equal(_bits(got[:, :m]), _bits(base[:, :m])), n


# ---------------------------------------------------------------- stream contract
B_S, SHAPE_S, N_S = 3, (5, 7, 9), 257


def _plan(lib, dev):
    need = lib.s3r_voxel_surface_points_scratch_elems(B_S, *SHAPE_S)
    args = [SC.Arg("occ", (B_S,) + SHAPE_S, F32, "in"), SC.Arg("ids", (2 * B_S,), I32, "in"), SC.Arg("points", (B_S, N_S, 3), F32, "out"),
            SC.Arg("n_faces", (B_S,), I32, "out"), SC.Arg("scratch", (need,), F32, "scr")]

    def data(k):
        grids = np.stack([R.grid(kind, SHAPE_S, seed=10 * k + i) for i, kind in enumerate(("half", "empty", "specials"))])
        ids = [1 + 20 * k, 2 + 20 * k, 2 ** 33 + k]
        return {"occ": SC._t(grids), "ids": _ids32(ids), "_ref": ids}

    def _call(ptr, st, n_points):
        return lib.s3r_voxel_surface_points(ptr["occ"], 0.5, ptr["ids"], R.SEED, ptr["points"], ptr["n_faces"], B_S, *SHAPE_S, n_points,
                                            ptr["scratch"], need, st)

    def call(ptr, st):
        return _call(ptr, st, N_S)

    def refuse(ptr, st):
        return _call(ptr, st, 0), -1                                     # n_points = 0

    def check(d, res):
        _same([SC._np(res["points"]), SC._np(res["n_faces"])], R.surface32(SC._np(d["occ"]), d["_ref"], N_S), "stream case")

    return SC.Plan(args, data, call, check, refuse=refuse)


CASE = SC.Case("surface_points:5x7x9", ("s3r_voxel_surface_points_scratch_elems", "s3r_voxel_surface_points"), "surface_points", _plan)
PAD_STREAMS = 29       # this file takes 1 (delayed producer) + 1 (capture) + 1 (refusal) = 3 of torch's pool of 32; 32 with these


def test_delayed_producer(s3r, lib, gate):
    TS.test_delayed_producer(s3r, lib, gate, CASE)


def test_capture_and_replay(s3r, lib):
    """captured once, replayed on new grids and ids in the same buffers: fresh clouds, the eager bits"""
    TS.test_capture_and_replay(s3r, lib, CASE)


def test_refused_call_is_not_captured(s3r, lib):
    TS.test_refused_call_is_not_captured(s3r, lib, CASE)
    # later files meet torch's round-robin pool of 32 streams at the phase they have without this file (the measurement:
    # tests/test_batchnorm_train_streams_gpu.py)
    for _ in range(PAD_STREAMS):
        with torch.cuda.stream(torch.cuda.Stream()):
            torch.zeros(1, device=DEV)
    torch.cuda.synchronize()


# ---------------------------------------------------------------- Python surface
def test_the_op_and_the_module(s3r):
    grids, ids, want = _batch9()
    t = torch.from_numpy(grids).to(DEV)
    i = torch.tensor(ids, dtype=torch.int64, device=DEV)
    p, n = s3r.voxel_surface_points(t, i, 257, seed=R.SEED, return_counts=True)
    _same((p.cpu().numpy(), n.cpu().numpy()), want, "voxel_surface_points")
    assert not p.requires_grad and p.shape == (9, 257, 3) and n.dtype == I32
    p = s3r.voxel_surface_points(t, i, 65, seed=R.SEED, threshold=0.25)
    _same((p.cpu().numpy(), None), R.surface32(grids, ids, 65, threshold=0.25), "threshold 0.25")
    mod = s3r.SurfacePoints(257, seed=R.SEED)
    first = mod(t, i)
    _same((first.cpu().numpy(), None), want, "SurfacePoints")
    again = mod(t.flip(0).contiguous(), i)
    assert again.data_ptr() == first.data_ptr()                            # the kept buffer
    _same((again.cpu().numpy(), None), R.surface32(grids[::-1], ids, 257), "SurfacePoints, other grids")
    assert s3r.voxel_surface_points(t[:0], i[:0], 8).shape == (0, 8, 3)
    with pytest.raises(RuntimeError, match="int64"):
        s3r.voxel_surface_points(t, i.int(), 8)


N, B = 6, 2
_CACHE = {}


def _sets(s3r):
    if "ds" not in _CACHE:
        _CACHE["ds"] = torch.utils.data.TensorDataset(*s3r.evaluate.synthetic_eval_set(N, 3, "uint8"))
    return _CACHE["ds"]


def _model(s3r):
    model = s3r.Stereo2Point()
    s3r.seed_module(model, seed=0)
    return model.to(DEV)


def _cfg(s3r, **kw):
    base = dict(variant="point", epochs=1, batch=B, lr=1e-2, optimizer="sgd", clip_grad_norm=1.0, augment=s3r.AugmentConfig.default(seed=9),
                seed=4, val_every=0, save_every=0, cloud_points=512, cloud_seed=11)
    base.update(kw)
    return s3r.TrainConfig(**base)


def _digest(model):
    h = hashlib.sha256()
    for n, p in sorted(model.state_dict().items()):
        h.update(n.encode())
        h.update(p.detach().cpu().contiguous().reshape(-1).numpy().tobytes())
    return h.hexdigest()


def _reference_run(s3r):
    if "ref" not in _CACHE:
        model = _model(s3r)
        res = s3r.fit(model, _sets(s3r), None, _cfg(s3r))
        torch.cuda.synchronize()
        _CACHE["ref"] = (res["losses"], _digest(model))
    return _CACHE["ref"]


def test_point_net_on_grids_equals_point_net_on_the_sampled_clouds(s3r):
    left, right, gt = _sets(s3r).tensors
    model = _model(s3r)
    ids = torch.arange(N, dtype=torch.int64, device=DEV)
    clouds = s3r.voxel_surface_points(gt.to(DEV), ids, 512, seed=11).cpu()
    want = s3r.evaluate.test_point_net(model, left, right, clouds, batch=B, device=DEV)
    got = s3r.evaluate.test_point_net(model, left, right, gt, batch=B, device=DEV, cloud_points=512, cloud_seed=11)
    assert torch.equal(got["per_sample"].view(I32), want["per_sample"].view(I32)) and got["mean_chamfer"] == want["mean_chamfer"]
    other = s3r.evaluate.test_point_net(model, left, right, gt, batch=B, device=DEV, cloud_points=512, cloud_seed=12)
    assert not torch.equal(other["per_sample"], want["per_sample"])


def test_fit_on_grids_twice_is_bit_identical(s3r):
    losses, digest = _reference_run(s3r)
    assert len(losses) == 3 and all(l == l and abs(l) < float("inf") for l in losses)
    model = _model(s3r)
    start = _digest(model)
    assert s3r.fit(model, _sets(s3r), None, _cfg(s3r))["losses"] == losses and _digest(model) == digest != start
    other = s3r.fit(_model(s3r), _sets(s3r), None, _cfg(s3r, cloud_seed=12, max_steps=1))        # the clouds enter the loss
    assert other["losses"][0] != losses[0]


def test_fit_on_grids_stopped_and_resumed_continues_with_the_same_bits(s3r, tmp_path):
    losses, digest = _reference_run(s3r)
    first = s3r.fit(_model(s3r), _sets(s3r), None, _cfg(s3r, max_steps=2, out_dir=str(tmp_path)))
    assert first["losses"] == losses[:2]
    ck = s3r.checkpoint.load_training_checkpoint(first["checkpoint"])
    assert (ck["config"]["cloud_points"], ck["config"]["cloud_seed"]) == (512, 11)
    fresh = s3r.Stereo2Point()
    s3r.seed_module(fresh, seed=123)
    fresh.to(DEV)
    second = s3r.fit(fresh, _sets(s3r), None, _cfg(s3r, resume=first["checkpoint"]))
    assert second["losses"] == losses[2:] and _digest(fresh) == digest


def test_fit_on_grids_equals_a_hand_written_loop_that_samples_the_same_clouds(s3r):
    losses, digest = _reference_run(s3r)
    cfg = _cfg(s3r)
    model = _model(s3r)
    opt = s3r.SGD([p for p in model.parameters() if p.requires_grad], lr=cfg.lr, momentum=0.9, clip_grad_norm=cfg.clip_grad_norm)
    chamfer = s3r.ChamferDistance()
    order = s3r.train.epoch_order(N, cfg.seed, 0)
    left, right, gt = _sets(s3r).tensors
    got = []
    for k in range(0, N, B):
        idx = order[k:k + B]
        ids = torch.tensor(idx, dtype=torch.int64, device=DEV) + 0 * N
        l, r = s3r.ops.augment_pair(left[idx].to(DEV), right[idx].to(DEV), ids, cfg.augment)
        target = s3r.voxel_surface_points(gt[idx].to(DEV), ids, cfg.cloud_points, cfg.cloud_seed)
        opt.zero_grad()
        loss = chamfer(model.differentiable(l, r), target)
        loss.backward()
        opt.step()
        got.append(loss.item())
    assert got == losses and _digest(model) == digest


def test_fit_validates_on_grids(s3r):
    ds = _sets(s3r)
    lines = []
    model = _model(s3r)
    s3r.fit(model, ds, ds.tensors, _cfg(s3r, val_every=1), log=lines.append)
    want = s3r.evaluate.test_point_net(model, *ds.tensors, batch=B, device=DEV, cloud_points=512, cloud_seed=11)
    assert lines[0]["val"]["samples"] == N and lines[0]["val"]["mean_chamfer"] == want["mean_chamfer"]


# ---------------------------------------------------------------- runner.py
def _runner(*args, timeout=400):
    return subprocess.run([sys.executable, os.path.join(ROOT, "runner.py"), *args], capture_output=True, text=True, timeout=timeout, cwd=ROOT)


def test_runner_trains_on_an_npz_with_volume_only_and_evaluates(s3r, tmp_path):
    left, right, gt = s3r.evaluate.synthetic_eval_set(4, 2, "uint8")
    data = tmp_path / "set.npz"
    np.savez(data, left=left.numpy(), right=right.numpy(), volume=gt.numpy())
    out = tmp_path / "run"
    r = _runner("--train", "--variant", "point", "--data", str(data), "--epochs", "1", "--batch", "2", "--cloud-points", "512", "--out", str(out))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    lines = [json.loads(l) for l in r.stdout.strip().splitlines() if l.startswith("{")]
    assert lines[0]["step"] == 1 and "mean_chamfer" in lines[0]["val"] and lines[-1]["done"] and lines[-1]["train_samples"] == 2
    last = out / "last.pth"
    r = _runner("--test", "--variant", "point", "--weights", str(last), "--data", str(data), "--batch", "2", "--cloud-points", "512",
                "--cloud-seed", "3")
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    res = json.loads(r.stdout.strip().splitlines()[-1])
    assert res["samples"] == 4 and res["weights"] == str(last) and res["mean_chamfer"] > 0 and res["data"] == str(data)


def test_runner_evaluates_the_point_variant_on_a_dataset_tree(tmp_path):
    from tests.test_data_cpu import _make_tree
    _make_tree(str(tmp_path), n_models=2, views=(0,), size=224)
    r = _runner("--test", "--variant", "point", "--dataset-root", str(tmp_path), "--batch", "2", "--seed", "3")
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert out["samples"] == 2 and out["mean_chamfer"] > 0 and out["data"] == str(tmp_path)
    assert out["per_taxonomy"] and sum(v["samples"] for v in out["per_taxonomy"].values()) == 2
    assert all(v["mean_chamfer"] > 0 for v in out["per_taxonomy"].values())
