"""The kernels that take a discrete decision, on the device, on the inputs where such a kernel can be wrong without a large error:
equal minima on both sides of every block, slice and pass boundary of chamfer_kernel, NaN and infinities on each of its code paths,
voxels exactly on, one ulp above and one ulp below the IoU threshold, counts above 2^24, minima shared by some disparities of a
pixel, and the edge values of the stereo metrics.

Everything is compared bit for bit with the plain sequential references of tests/_select_ref.py (or, for the soft read-out, with
tests/_disp64.py at the tolerance tests/test_disparity_soft_gpu.py::test_feature_resolution_matches_fp64 uses).  There is no
tolerance of its own in this file.  The cases and the coverage conditions they must meet are tests/_selection_cases.py's;
tests/test_selection_cpu.py shows, with mutants of the references, that these cases see the bugs they are there for.  A failure
names the case and the first differing element: `planted pass0-slice3|pass1-slice0 idx1: ... first at (0, 17): got 2100, want 1600`.
"""
import numpy as np
import pytest
import torch

from tests import _chamfer64 as R64
from tests import _disp64 as D64
from tests import _guard as G
from tests import _select_ref as SR
from tests import _selection_cases as C

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
VARIANTS = [(n, s) for n in list(C.LATTICE) + list(C.SHUFFLED) for s in (False, True)]
VID = [n + ("+shift" if s else "") for n, s in VARIANTS]
_sid = lambda s: "x".join(map(str, s))      # noqa: E731


@pytest.fixture(scope="module")
def lib(s3r):
    return s3r.load_library()


def _rc(lib, rc, what):
    assert rc == 0, f"{what}: {lib.s3r_last_error().decode()} ({rc})"


def chamfer_forward(lib, p, q):
    """s3r_chamfer_forward on guarded buffers: numpy (B,N,3), (B,M,3) in, (dist1, dist2, idx1, idx2) numpy out"""
    B, N, M = p.shape[0], p.shape[1], q.shape[1]
    pb = G.Guarded("p", p.shape, torch.float32, DEV, "in", data=torch.from_numpy(p).to(DEV))
    qb = G.Guarded("q", q.shape, torch.float32, DEV, "in", data=torch.from_numpy(q).to(DEV))
    outs = [G.Guarded("dist1", (B, N), torch.float32, DEV, "out"), G.Guarded("dist2", (B, M), torch.float32, DEV, "out"),
            G.Guarded("idx1", (B, N), torch.int32, DEV, "out"), G.Guarded("idx2", (B, M), torch.int32, DEV, "out")]
    _rc(lib, lib.s3r_chamfer_forward(pb.ptr, qb.ptr, *[o.ptr for o in outs], B, N, M, None), "chamfer forward")
    torch.cuda.synchronize()
    G.check_all(pb, qb, *outs)
    return tuple(o.t.cpu().numpy() for o in outs)


def _check_forward(got, want, case):
    for g, w, what in zip(got, want, ("dist1", "dist2", "idx1", "idx2")):
        SR.assert_same(g, w, what, case)


# ---------------------------------------------------------------- Chamfer: lattice clouds and shuffled copies
@pytest.mark.parametrize("case", VARIANTS, ids=VID)
def test_chamfer_tie_dense_clouds_and_their_backward(lib, case):
    """dist1, dist2, idx1, idx2 equal the sequential scan bit for bit; then the hand-off: s3r_chamfer_backward with the indices the
    forward wrote equals the defined fp32 order (tests/_chamfer64.py) bit for bit"""
    name, shifted = case
    cid = VID[VARIANTS.index(case)]
    print(cid, C.check_chamfer_coverage(name, shifted))             # the case still covers its boundaries
    p, q = C.chamfer_case(name, shifted)
    got = chamfer_forward(lib, p, q)
    _check_forward(got, C.chamfer_want(name, shifted), cid)
    B, N, M = p.shape[0], p.shape[1], q.shape[1]
    g = torch.Generator().manual_seed(N + M)
    g1 = torch.randint(-4, 5, (B, N), generator=g).float()
    g2 = torch.randint(-4, 5, (B, M), generator=g).float()
    dev = [torch.from_numpy(np.ascontiguousarray(a)).to(DEV) for a in (p, q, got[2], got[3])] + [g1.to(DEV), g2.to(DEV)]
    gp, gq = torch.empty(B, N, 3, device=DEV), torch.empty(B, M, 3, device=DEV)
    _rc(lib, lib.s3r_chamfer_backward(*[t.data_ptr() for t in dev], gp.data_ptr(), gq.data_ptr(), B, N, M, None), "chamfer backward")
    torch.cuda.synchronize()
    want_p, want_q = R64.backward32(p, q, got[2], got[3], g1.numpy(), g2.numpy())
    SR.assert_same(gp.cpu().numpy(), want_p, "grad_p", cid)
    SR.assert_same(gq.cpu().numpy(), want_q, "grad_q", cid)
    if shifted:           # (unshifted, most or all nearest distances are zero and so are the gradients: a check of the zeros' signs)
        assert np.abs(want_p).max() > 0 and np.abs(want_q).max() > 0


# ---------------------------------------------------------------- Chamfer: planted indices
@pytest.mark.parametrize("name", list(C.PLANTED))
def test_chamfer_planted_minima(lib, name):
    queries, cands = C.planted_case(name)
    first = min(C.PLANTED[name])
    for swapped in (False, True):                                  # both directions of the kernel see the planted cloud as candidates
        p, q = (cands, queries) if swapped else (queries, cands)
        cid = f"planted {name}{' swapped' if swapped else ''}"
        got = chamfer_forward(lib, p, q)
        _check_forward(got, SR.chamfer_scan(p, q), cid)
        idx = got[3] if swapped else got[2]
        bad = np.argwhere(idx != first)
        assert bad.size == 0, f"{cid}: query {tuple(bad[0])}: got idx {idx[tuple(bad[0])]}, want {first}"


# ---------------------------------------------------------------- Chamfer: non-finite input
@pytest.mark.parametrize("kind", C.NONFINITE)
def test_chamfer_nonfinite_input(lib, kind):
    """NaN, +-inf and inf - inf on the block path, the tail path, every slice and a later pass: the minimum is taken over the
    distances that are not NaN, a query with no distance below +inf gets (+inf, 0); and the answer does not depend on where in
    the staging the special values sit: the clouds rotated along the point axis give the rotated distances"""
    p, q = C.nonfinite_case(kind)
    got = chamfer_forward(lib, p, q)
    want = SR.chamfer_scan(p, q)
    _check_forward(got, want, f"non-finite {kind}")
    assert np.isinf(got[0][:, list(C.NF_P_AT)]).all() and (got[2][:, list(C.NF_P_AT)] == 0).all()      # a non-finite point's own answer
    assert np.isinf(got[1][:, list(C.NF_Q_AT)]).all() and (got[3][:, list(C.NF_Q_AT)] == 0).all()
    assert not np.isnan(got[0]).any() and not np.isnan(got[1]).any()
    rp, rq = 41, 777
    p2, q2 = np.roll(p, rp, 1), np.roll(q, rq, 1)
    rot = chamfer_forward(lib, p2, q2)
    _check_forward(rot, SR.chamfer_scan(p2, q2), f"non-finite {kind} rotated")
    SR.assert_same(rot[0], np.roll(got[0], rp, 1), "dist1 against the unrotated answer", f"non-finite {kind} rotated")
    SR.assert_same(rot[1], np.roll(got[1], rq, 1), "dist2 against the unrotated answer", f"non-finite {kind} rotated")


@pytest.mark.parametrize("where", ["p", "q"])
@pytest.mark.parametrize("value", ["nan", "inf", "-inf"])
def test_a_nonfinite_coordinate_makes_the_loss_nonfinite(s3r, where, value):
    """through s3r.ChamferDistance: the point's own distance is +inf, so corrupt data cannot yield a finite loss"""
    g = torch.Generator().manual_seed(5)
    p, q = torch.rand(2, 300, 3, generator=g), torch.rand(2, 2100, 3, generator=g)
    clean = s3r.ChamferDistance()(p.to(DEV), q.to(DEV))
    assert bool(torch.isfinite(clean))
    for at in (0, 77, 299) if where == "p" else (3, 1027, 2048 + 10, 2099):
        bad_p, bad_q = p.clone(), q.clone()
        (bad_p if where == "p" else bad_q)[1, at, at % 3] = float(value)
        loss = s3r.ChamferDistance()(bad_p.to(DEV), bad_q.to(DEV))
        assert not bool(torch.isfinite(loss)), f"{value} in {where}[1, {at}]: loss {loss.item()}"
        d1, d2, i1, i2 = s3r.chamfer_distance(bad_p.to(DEV), bad_q.to(DEV))
        own_d, own_i = (d1, i1) if where == "p" else (d2, i2)
        assert own_d[1, at].item() == float("inf") and own_i[1, at].item() == 0
        assert bool(torch.isfinite(d1[0]).all()) and bool(torch.isfinite(d2[0]).all())      # the other sample is untouched


# ---------------------------------------------------------------- WTA and soft read-out
def wta_forward(lib, fl, fr, D):
    B, Cc, H, W = fl.shape
    a = G.Guarded("left", fl.shape, torch.float32, DEV, "in", data=torch.from_numpy(fl).to(DEV))
    b = G.Guarded("right", fr.shape, torch.float32, DEV, "in", data=torch.from_numpy(fr).to(DEV))
    dl, dr = G.Guarded("disp_l", (B, H, W), torch.float32, DEV, "out"), G.Guarded("disp_r", (B, H, W), torch.float32, DEV, "out")
    _rc(lib, lib.s3r_disparity_wta(a.ptr, b.ptr, dl.ptr, dr.ptr, B, Cc, H, W, D, None), "wta")
    torch.cuda.synchronize()
    G.check_all(a, b, dl, dr)
    return dl.t.cpu().numpy(), dr.t.cpu().numpy()


@pytest.mark.parametrize("shape", C.READOUT_SHAPES, ids=_sid)
def test_wta_takes_the_first_of_a_partly_shared_minimum(lib, oracle, shape):
    print(shape, f"{C.check_readout_coverage(shape):.1%}")
    fl, fr = C.readout_feats(shape)
    want = oracle.disparity_wta(torch.from_numpy(fl), torch.from_numpy(fr), shape[4])
    for g, w, what in zip(wta_forward(lib, fl, fr, shape[4]), want, ("disp_l", "disp_r")):
        SR.assert_same(g, w.numpy(), what, f"wta {_sid(shape)}")


def _soft_against_fp64(s3r, fl, fr, D, tau, size, cid):
    """the assertions of test_disparity_soft_gpu.py::test_feature_resolution_matches_fp64, same constants; `size` upsamples both"""
    got = [t.cpu().double().numpy() for t in
           s3r.disparity_soft(torch.from_numpy(fl).to(DEV), torch.from_numpy(fr).to(DEV), D, tau, out_size=size, confidence=True)]
    disp, conf = D64.soft(fl, fr, D, tau)
    want = list(disp) + list(conf)
    if size is not None:
        want = [D64.bilinear(w, *size) for w in want]
    for k, (g, w) in enumerate(zip(got, want)):
        err = np.abs(g - w) if k < 2 else np.abs(g - w) / w
        lim = 2e-5 * D if k < 2 else 1e-5
        print(f"{cid} {('disp_l', 'disp_r', 'conf_l', 'conf_r')[k]}: max err {err.max():.3e} (limit {lim:.1e})")
        at = np.unravel_index(err.argmax(), err.shape)
        assert err.max() <= lim, f"{cid} output {k} at {at}: got {g[at]!r}, want {w[at]!r}"
    return got


@pytest.mark.parametrize("upsampled", [False, True], ids=["feature", "upsampled"])
@pytest.mark.parametrize("tau", [0.05, 1.0])
@pytest.mark.parametrize("shape", C.READOUT_SHAPES, ids=_sid)
def test_soft_readout_on_partly_shared_minima(s3r, shape, tau, upsampled):
    C.check_readout_coverage(shape)
    fl, fr = C.readout_feats(shape)
    cid = f"soft {_sid(shape)} tau {tau}{' upsampled' if upsampled else ''}"
    got = _soft_against_fp64(s3r, fl, fr, shape[4], tau, C.READOUT_UP[shape] if upsampled else None, cid)
    if tau == 0.05 and not upsampled:
        # cold: integer costs one apart weigh e^-20; a pixel whose minimum is shared by the set T reads mean(T)
        for g, (_, marked, mean) in zip(got[:2], C.readout_ties(shape)):
            assert marked.sum() > 0
            err = np.abs(g - mean)[marked]
            assert err.max() <= 2e-5 * shape[4], f"{cid}: a shared minimum reads {g[marked][err.argmax()]!r}, its set's mean is {mean[marked][err.argmax()]!r}"


@pytest.mark.parametrize("shape", C.READOUT_SHAPES[1:], ids=_sid)
def test_readouts_with_a_nan_feature(s3r, lib, oracle, shape):
    """the header's arithmetic as written: a NaN cost never wins a strict `<`, so the WTA skips it (and answers 0 where every cost
    of a pixel is NaN: nothing beats the initial +inf); the soft read-out's weights sum to NaN wherever one cost is NaN"""
    B, Cc, H, W, D = shape
    fl, fr = (a.copy() for a in C.readout_feats(shape))
    b0, c0, h0, w0 = 1, Cc - 2, H // 2, W // 2
    fl[b0, c0, h0, w0] = np.nan
    wl, wr = wta_forward(lib, fl, fr, D)
    want = oracle.disparity_wta(torch.from_numpy(fl), torch.from_numpy(fr), D)
    SR.assert_same(wl, want[0].numpy(), "disp_l", f"wta with NaN {_sid(shape)}")
    SR.assert_same(wr, want[1].numpy(), "disp_r", f"wta with NaN {_sid(shape)}")
    assert wl[b0, h0, w0] == 0                                     # every cost of the left pixel (h0, w0) holds the NaN
    clean = wta_forward(lib, *C.readout_feats(shape), D)
    own = np.zeros((B, H, W), bool)
    own[b0, h0, w0] = True                                         # left: only the pixel itself reads L(h0, w0)
    touched = np.zeros((B, H, W), bool)
    touched[b0, h0, max(0, w0 - D + 1):w0 + 1] = True              # right: the pixels one of whose partners w + d is (h0, w0)
    assert np.array_equal(wl[~own], clean[0][~own]) and np.array_equal(wr[~touched], clean[1][~touched])
    for tau in (0.05, 1.0):
        sl, sr = (t.cpu().numpy() for t in s3r.disparity_soft(torch.from_numpy(fl).to(DEV), torch.from_numpy(fr).to(DEV), D, tau))
        (rl, rr), _ = D64.soft(fl, fr, D, tau)
        assert np.array_equal(np.isnan(sl), own) and np.array_equal(np.isnan(rl), own)
        assert np.array_equal(np.isnan(sr), touched) and np.array_equal(np.isnan(rr), touched)
        assert np.abs(sl[~own] - rl[~own]).max() <= 2e-5 * D and np.abs(sr[~touched] - rr[~touched]).max() <= 2e-5 * D


# ---------------------------------------------------------------- IoU
def iou_forward(lib, pred, gt, th):
    B, V = pred.shape
    a = G.Guarded("pred", pred.shape, torch.float32, DEV, "in", data=torch.from_numpy(pred).to(DEV))
    b = G.Guarded("gt", gt.shape, torch.float32, DEV, "in", data=torch.from_numpy(gt).to(DEV))
    out = G.Guarded("iou", B, torch.float32, DEV, "out")
    _rc(lib, lib.s3r_voxel_iou(a.ptr, b.ptr, th, out.ptr, B, V, None), "iou")
    torch.cuda.synchronize()
    G.check_all(a, b, out)
    return out.t.cpu().numpy()


@pytest.mark.parametrize("V", C.IOU_V)
def test_iou_on_the_threshold_and_special_values(s3r, lib, V):
    assert len(s3r.evaluate.THRESHOLDS) >= 4
    for th in s3r.evaluate.THRESHOLDS:
        pred, gt = C.iou_case(V, th)
        want = SR.iou_ref(pred, gt, th)
        SR.assert_same(iou_forward(lib, pred, gt, th), want, "iou (C entry)", f"V={V} th={th}")
        mod = s3r.voxel_iou(torch.from_numpy(pred).to(DEV), torch.from_numpy(gt).to(DEV), th)
        SR.assert_same(mod.cpu().numpy(), want, "iou (s3r.voxel_iou)", f"V={V} th={th}")
        assert want[3] == 1 and (V < 255 or 0 < want[0] < 1)


def test_iou_counts_above_2_to_24(s3r, lib):
    pred, gt = C.iou_big_case()
    want = SR.iou_ref(pred, gt, 0.5)
    assert 0 < want[0] < 1
    SR.assert_same(iou_forward(lib, pred, gt, 0.5), want, "iou (C entry)", f"V={C.IOU_BIG_V}")
    mod = s3r.voxel_iou(torch.from_numpy(pred).to(DEV), torch.from_numpy(gt).to(DEV), 0.5)
    SR.assert_same(mod.cpu().numpy(), want, "iou (s3r.voxel_iou)", f"V={C.IOU_BIG_V}")


# ---------------------------------------------------------------- metrics and EPE
def test_metrics_on_signed_zero_subnormal_and_overflowing_values(s3r, lib):
    pred, gt = C.metrics_case()
    B, P = pred.shape
    pb = G.Guarded("pred", pred.shape, torch.float32, DEV, "in", data=torch.from_numpy(pred).to(DEV))
    gb = G.Guarded("gt", gt.shape, torch.float32, DEV, "in", data=torch.from_numpy(gt).to(DEV))
    e, c = G.Guarded("epe", B, torch.float32, DEV, "out"), G.Guarded("counts", (B, 4), torch.int32, DEV, "out")
    _rc(lib, lib.s3r_disparity_metrics(pb.ptr, gb.ptr, e.ptr, c.ptr, B, P, None), "metrics")
    torch.cuda.synchronize()
    G.check_all(pb, gb, e, c)
    with np.errstate(over="ignore"):
        want_e, want_c = D64.metrics(pred, gt)
    got_e, got_c = e.t.cpu().double().numpy(), c.t.cpu().numpy()
    print("epe", got_e, "want", want_e, "counts", got_c.tolist())
    SR.assert_same(got_c.astype(np.int64), want_c.astype(np.int64), "counts", "metrics")
    inf = np.isinf(want_e)
    assert inf.tolist() == [False, False, True, False, False] and np.array_equal(got_e[inf], want_e[inf])      # inf included
    assert (np.abs(got_e[~inf] - want_e[~inf]) <= 1e-6 * want_e[~inf].max()).all()      # (the bound of test_metrics_match_numpy)
    assert got_e[1] <= 2.0 ** -126                                 # every error of that sample is at most the smallest normal number
    epe, cnt = s3r.disparity_epe(torch.from_numpy(pred).to(DEV), torch.from_numpy(gt).to(DEV))
    SR.assert_same(epe.cpu().numpy(), e.t.cpu().numpy(), "epe of s3r_disparity_epe against s3r_disparity_metrics", "metrics")
    SR.assert_same(cnt.cpu().numpy().astype(np.int64), want_c[:, 0].astype(np.int64), "valid count of s3r_disparity_epe", "metrics")
