"""The harness of tests/test_selection_gpu.py, without a GPU: the sequential references (tests/_select_ref.py) against the oracle, the
coverage conditions of tests/_selection_cases.py, and MUTANTS — wrong variants of each rule, written in Python, each of which at
least one case of its family must reject.  That is the evidence that the cases can see the bug they are there for.

The Chamfer mutants live in `kernel_model`, which mirrors the structure of chamfer_kernel (passes of 2048, four slices of
ceil(count / 4) per pass whose running bests persist across passes, blocks of 8 with a minimum tree and a search for the first
element at the minimum, a tail, the final merge with its index comparison).  Unmutated, the model must equal the sequential scan
on every case: the structure is one way of computing the rule, the scan is the rule."""
import functools
import os

import numpy as np
import pytest
import torch

from tests import _disp64 as D64
from tests import _select_ref as SR
from tests import _selection_cases as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VARIANTS = [(n, s) for n in list(C.LATTICE) + list(C.SHUFFLED) for s in (False, True)]
VID = [n + ("+shift" if s else "") for n, s in VARIANTS]


# ---------------------------------------------------------------- the structural model of chamfer_kernel and its mutants
def _model_one_way(a, c, mutant):
    B, Q, K = a.shape[0], a.shape[1], c.shape[1]
    ax, ay, az = a[:, :, None, 0], a[:, :, None, 1], a[:, :, None, 2]
    inf = np.float32(np.inf)
    best = np.full((SR.SLICES, B, Q), inf, np.float32)
    besti = np.zeros((SR.SLICES, B, Q), np.int32)
    less = (lambda x, y: x <= y) if mutant == "le" else (lambda x, y: x < y)

    def dists(lo, hi):
        cc = c[:, None, lo:hi]
        return SR.dist3(ax, ay, az, cc[..., 0], cc[..., 1], cc[..., 2])          # (B, Q, hi - lo)

    for j0 in range(0, K, SR.CH_TILE):
        cnt = min(SR.CH_TILE, K - j0)
        per = (cnt + SR.SLICES - 1) // SR.SLICES
        if mutant == "reset-per-pass":
            best[:], besti[:] = inf, 0
        for s in range(SR.SLICES):
            t, t_end = min(cnt, s * per), min(cnt, min(cnt, s * per) + per)
            while t + SR.CBLK <= t_end:
                d = dists(j0 + t, j0 + t + SR.CBLK)
                if mutant == "nan-propagates":
                    m = d[..., 0]
                    for e in range(1, SR.CBLK):
                        m = np.minimum(m, d[..., e])                # NaN if any is
                elif mutant == "nan-smallest":
                    m = np.where(np.isnan(d).any(-1), -inf, np.fmin.reduce(np.where(np.isnan(d), inf, d), -1)).astype(np.float32)
                    d = np.where(np.isnan(d), -inf, d)
                else:
                    m = d[..., 0]
                    for e in range(1, SR.CBLK):
                        m = np.fmin(m, d[..., e])                   # IEEE minNum, as v_min_f32
                upd = less(m, best[s])
                at = d == m[..., None]
                e_min = np.full(m.shape, SR.CBLK - 1, np.int32)
                order = range(SR.CBLK - 1) if mutant == "last-in-block" else range(SR.CBLK - 2, -1, -1)
                for e in order:
                    e_min = np.where(at[..., e], e, e_min)
                best[s] = np.where(upd, m, best[s])
                besti[s] = np.where(upd, j0 + t + e_min, besti[s])
                t += SR.CBLK
            if t < t_end:
                d = dists(j0 + t, j0 + t_end)
                for e in range(t_end - t):
                    dd = d[..., e]
                    if mutant == "nan-smallest":
                        dd = np.where(np.isnan(dd), -inf, dd)
                    upd = less(dd, best[s])
                    if mutant == "nan-propagates":
                        upd = upd | np.isnan(dd)
                    best[s] = np.where(upd, dd, best[s])
                    besti[s] = np.where(upd, j0 + t + e, besti[s])
    d, bi = best[0].copy(), besti[0].copy()
    for s in range(1, SR.SLICES):
        take = best[s] <= d if mutant == "merge-takes-ties" else best[s] < d
        if mutant not in ("merge-without-index", "merge-takes-ties"):
            take |= (best[s] == d) & (besti[s] < bi)
        d, bi = np.where(take, best[s], d), np.where(take, besti[s], bi)
    return d.astype(np.float32), bi.astype(np.int32)


def kernel_model(p, q, mutant=None):
    p, q = np.ascontiguousarray(p, np.float32), np.ascontiguousarray(q, np.float32)
    with np.errstate(all="ignore"):
        d1, i1 = _model_one_way(p, q, mutant)
        d2, i2 = _model_one_way(q, p, mutant)
    return d1, d2, i1, i2


def _same(a, b):
    return all(np.array_equal(SR.bits(x), SR.bits(y)) for x, y in zip(a, b))


def _planted_both(name):
    queries, cands = C.planted_case(name)
    return [(queries, cands), (cands, queries)]


# the cases a Chamfer mutant is run on, cheapest first; the rule mutants see the tie cases, the NaN mutants the non-finite ones
TIE_FAMILY = [f"planted {n}" for n in C.PLANTED] + ["lat-300x2100", "shuf-4100"]
NONFINITE_FAMILY = [f"non-finite {k}" for k in C.NONFINITE]
CHAMFER_MUTANTS = {"le": TIE_FAMILY, "last-in-block": TIE_FAMILY, "merge-without-index": TIE_FAMILY, "merge-takes-ties": TIE_FAMILY,
                   "reset-per-pass": TIE_FAMILY, "nan-propagates": NONFINITE_FAMILY, "nan-smallest": NONFINITE_FAMILY}


@functools.lru_cache(maxsize=None)
def _family_case(name):
    """(p, q, the scan's answer); the unmutated model must give that answer"""
    kind, _, row = name.partition(" ")
    p, q = C.planted_case(row) if kind == "planted" else C.nonfinite_case(row) if kind == "non-finite" else C.chamfer_case(name)
    want = SR.chamfer_scan(p, q)
    assert _same(kernel_model(p, q), want), f"{name}: the unmutated model departs from the scan"
    return p, q, want


def _sees(name, mutant):
    p, q, want = _family_case(name)
    return not _same(kernel_model(p, q, mutant), want)


@pytest.mark.parametrize("mutant", list(CHAMFER_MUTANTS))
def test_chamfer_mutant_is_rejected(mutant):
    rejected = next((name for name in CHAMFER_MUTANTS[mutant] if _sees(name, mutant)), None)
    print(f"{mutant}: rejected by {rejected}")
    assert rejected, f"no case of its family sees the mutant {mutant}"


def test_each_planted_boundary_kills_the_mutant_it_is_there_for():
    """the table's rows are not interchangeable.  `<=` in the scan is seen by two minima in ONE slice (in different blocks, in a
    block and its tail, in two passes); two minima in different slices are put right by the merge, so those rows are what sees a
    wrong merge: one without the index comparison (an earlier index in a later slice), one that takes ties (a later index in a
    later slice); last-in-block needs two minima in one block"""
    def sees(row, mutant):
        return _sees(f"planted {row}", mutant)
    for row in ("block-7|8", "pass1|pass2-same-slice", "last-pass-block|tail", "last-block|last-tail"):
        assert sees(row, "le"), row
    for row in ("slice-511|512", "first|last", "last-pass-slices"):
        assert sees(row, "merge-takes-ties") and not sees(row, "le"), row
    for row in ("pass-2047|2048", "pass0-slice3|pass1-slice0", "every-pass"):
        assert sees(row, "merge-without-index"), row
    assert sees("same-block", "last-in-block") and not sees("block-7|8", "last-in-block")
    assert sees("pass1|pass2-same-slice", "reset-per-pass") and sees("pass-2047|2048", "reset-per-pass")
    assert not sees("last", "le")                                  # a single minimum: nothing to get wrong


@pytest.mark.parametrize("name", list(C.PLANTED))
def test_planted_index_is_the_lowest_of_the_set(name):
    queries, cands = C.planted_case(name)
    d1, d2, i1, i2 = SR.chamfer_scan(queries, cands)
    assert (i1 == min(C.PLANTED[name])).all() and np.isfinite(d1).all() and d1.max() < 3
    assert len(np.unique(cands.reshape(-1, 3), axis=0)) == cands.shape[0] * cands.shape[1] - 2 * len(C.PLANTED[name]) + 2
    assert all(0 <= j < C.PLANT_M for j in C.PLANTED[name])


# ---------------------------------------------------------------- the scan against the oracle
@pytest.mark.parametrize("case", VARIANTS, ids=VID)
def test_scan_equals_the_oracle_and_the_model(oracle, case):
    name, shifted = case
    p, q = C.chamfer_case(name, shifted)
    want = C.chamfer_want(name, shifted)
    for b in range(p.shape[0]):                                    # (one sample at a time: the oracle's (N, M, 3) difference tensor)
        got = oracle.chamfer_distance(torch.from_numpy(p[b:b + 1]), torch.from_numpy(q[b:b + 1]))
        for g, w, what in zip(got, want, ("dist1", "dist2", "idx1", "idx2")):
            SR.assert_same(g.numpy(), w[b:b + 1], what, f"{VID[VARIANTS.index(case)]} sample {b}")
    if name in ("lat-300x2100", "lat-37x4097", "lat-4097x37", "shuf-2049"):
        assert _same(kernel_model(p, q), want)


@pytest.mark.parametrize("name", list(C.PLANTED))
def test_scan_equals_the_oracle_on_the_planted_cases(oracle, name):
    for p, q in _planted_both(name):
        got = oracle.chamfer_distance(torch.from_numpy(p), torch.from_numpy(q))
        for g, w, what in zip(got, SR.chamfer_scan(p, q), ("dist1", "dist2", "idx1", "idx2")):
            SR.assert_same(g.numpy(), w, what, f"planted {name}")


@pytest.mark.parametrize("kind", C.NONFINITE)
def test_scan_departs_from_the_oracle_exactly_where_the_contract_says(oracle, kind):
    """torch.min propagates NaN; the contract takes the minimum over the distances that are not NaN.  So: a query with no NaN
    distance agrees with the oracle bit for bit; a query with one has the oracle answering NaN and the scan answering the minimum of
    the others, or (+inf, 0) when none of them is below +inf."""
    p, q = C.nonfinite_case(kind)
    assert not np.isfinite(p).all() and not np.isfinite(q).all()
    got = SR.chamfer_scan(p, q)
    ora = [t.numpy() for t in oracle.chamfer_distance(torch.from_numpy(p), torch.from_numpy(q))]
    with np.errstate(all="ignore"):
        dense = SR.dist3(p[:, :, None, 0], p[:, :, None, 1], p[:, :, None, 2], q[:, None, :, 0], q[:, None, :, 1], q[:, None, :, 2])
    seen = 0
    for d, i, od, oi, axis in ((got[0], got[2], ora[0], ora[2], 2), (got[1], got[3], ora[1], ora[3], 1)):
        has_nan = np.isnan(dense).any(axis)
        rest = np.where(np.isnan(dense), np.inf, dense)            # the distances that are not NaN
        assert np.array_equal(SR.bits(d[~has_nan]), SR.bits(od[~has_nan])) and np.array_equal(i[~has_nan], oi[~has_nan])
        assert np.isnan(od[has_nan]).all() and not np.isnan(d).any()
        assert np.array_equal(d, rest.min(axis))                   # (a check of the answer, not the rule: the scan took the decision)
        first = np.where(np.isinf(rest.min(axis)), 0, (rest == np.expand_dims(rest.min(axis), axis)).argmax(axis))
        assert np.array_equal(i, first)
        none_finite = np.isinf(d)
        assert (i[none_finite] == 0).all()
        seen += int(has_nan.sum()) + int(none_finite.sum())
    assert seen > 0
    if kind in ("+inf", "-inf"):                                   # no NaN distance anywhere: the oracle and the scan agree throughout
        assert not np.isnan(dense).any()


def test_nonfinite_positions_cover_every_path():
    """block path and tail path of every slice, a full pass and a later partial pass (q); blocks and tails of a one-pass cloud (p)"""
    _, N, M = C.NF_SHAPE
    def place(j, K):
        j0 = j // SR.CH_TILE * SR.CH_TILE
        cnt = min(SR.CH_TILE, K - j0)
        per = (cnt + 3) // 4
        s, t = (j - j0) // per, (j - j0) % per
        length = min(cnt, (s + 1) * per) - s * per
        return j0 // SR.CH_TILE, s, "block" if t < length // SR.CBLK * SR.CBLK else "tail"
    q_at = {place(j, M) for j in C.NF_Q_AT}
    assert {(0, s, "block") for s in range(4)} <= q_at and {(1, s, "tail") for s in range(4)} <= q_at and (1, 0, "block") in q_at
    p_at = {place(i, N) for i in C.NF_P_AT}
    assert {s for _, s, _ in p_at} == {0, 1, 2, 3} and {k for _, _, k in p_at} == {"block", "tail"}


# ---------------------------------------------------------------- coverage conditions
@pytest.mark.parametrize("case", VARIANTS, ids=VID)
def test_chamfer_coverage_conditions(case):
    print(C.check_chamfer_coverage(*case))


def test_the_conditions_and_exemptions_are_what_the_shapes_allow():
    asked = {(n, d, c) for n in list(C.LATTICE) + list(C.SHUFFLED) for d, c in C.chamfer_conditions(n)}
    assert not asked & set(C.EXEMPT)
    # C3 is met by the lattice-of-8 case and the two larger shuffled-copies cases, in every direction that is asked of them
    assert {("lat-5000x4500", 0, "C3"), ("lat-5000x4500", 1, "C3"), ("shuf-4100", 0, "C3"), ("shuf-6151", 0, "C3")} <= asked
    assert {n for n, _, c in asked if c == "C1"} == set(C.LATTICE)
    for (name, direction, cond) in C.EXEMPT:                      # an exemption names a direction the rule would otherwise ask
        p, q = C.chamfer_case(name)
        assert (q, p)[direction].shape[1] > SR.CH_TILE and cond in ("C2", "C3")
    src = open(os.path.join(ROOT, "stereo-3d-reconstruction_amd", "csrc", "s3r_chamfer.hip")).read()
    assert f"constexpr int CH_TILE = {SR.CH_TILE};" in src and f"constexpr int CBLK = {SR.CBLK};" in src and "(cnt + 3) >> 2" in src


@pytest.mark.parametrize("shape", C.READOUT_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_readout_coverage_condition(shape):
    print(f"{C.check_readout_coverage(shape):.1%}")
    fl, fr = C.readout_feats(shape)
    assert set(np.unique(fl)) <= {-2, -1, 0, 1, 2} and set(np.unique(fr)) <= {-2, -1, 0, 1, 2}


# ---------------------------------------------------------------- WTA
def _wta_last_minimum(fl, fr, D):
    out = []
    for right in (False, True):
        c = D64.costs(fl, fr, D, right)
        best, arg = np.full(c.shape[:-1], np.inf, np.float32), np.zeros(c.shape[:-1], np.float32)
        for d in range(c.shape[-1]):
            upd = c[..., d] <= best
            upd &= np.isfinite(c[..., d])                          # (outside a pixel's range nothing is scanned)
            best, arg = np.where(upd, c[..., d], best), np.where(upd, np.float32(d), arg)
        out.append(arg)
    return out


@pytest.mark.parametrize("shape", C.READOUT_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_wta_oracle_takes_the_first_of_the_marked_minima_and_rejects_the_last(oracle, shape):
    fl, fr = C.readout_feats(shape)
    want = [t.numpy() for t in oracle.disparity_wta(torch.from_numpy(fl), torch.from_numpy(fr), shape[4])]
    last = _wta_last_minimum(fl, fr, shape[4])
    for w, l, (c, marked, _) in zip(want, last, C.readout_ties(shape)):
        first = (c == np.take_along_axis(c, w.astype(np.int64)[..., None], -1)).argmax(-1)
        assert np.array_equal(first, w)                            # the oracle's index is the first at its own cost ...
        assert (np.take_along_axis(c, w.astype(np.int64)[..., None], -1)[..., 0] <= c.min(-1)).all()      # ... which is the minimum
        assert not np.array_equal(l, w) and (l[marked] > w[marked]).all()


# ---------------------------------------------------------------- IoU
def _iou_mutant(pred, gt, th, mutant):
    t = np.float64(th) if mutant == "fp64-threshold" else np.float32(th)
    pr, g = (pred.astype(np.float64), gt.astype(np.float64)) if mutant == "fp64-threshold" else (pred, gt)
    with np.errstate(invalid="ignore"):
        a, b = (pr >= t, g >= t) if mutant == "ge" else (pr > t, g > t)
    inter, union = np.count_nonzero(a & b, axis=1), np.count_nonzero(a | b, axis=1)

    def conv(n):
        f = np.float32(int(n))
        if mutant == "truncated-counts" and int(f) > int(n):
            f = np.nextafter(f, np.float32(0))
        return f
    return np.array([conv(i) / conv(u) if u else np.float32(1) for i, u in zip(inter, union)], np.float32)


def _iou_cases(th_list):
    for th in th_list:
        for V in C.IOU_V:
            yield f"V={V} th={th}", C.iou_case(V, th), th
    yield "big", C.iou_big_case(), 0.5


@pytest.mark.parametrize("mutant", ["ge", "fp64-threshold", "truncated-counts"])
def test_iou_mutant_is_rejected(s3r, mutant):
    rejected = []
    for name, (pred, gt), th in _iou_cases(s3r.evaluate.THRESHOLDS):
        want = SR.iou_ref(pred, gt, th)
        assert np.array_equal(SR.bits(_iou_mutant(pred, gt, th, None)), SR.bits(want))
        if not np.array_equal(SR.bits(_iou_mutant(pred, gt, th, mutant)), SR.bits(want)):
            rejected.append(name)
    print(f"{mutant}: rejected by {rejected}")
    assert rejected
    if mutant == "truncated-counts":
        assert rejected == ["big"]
    if mutant == "fp64-threshold":                                 # every threshold that is not an fp32 number sees it
        assert {n.split("th=")[1] for n in rejected} == {str(t) for t in s3r.evaluate.THRESHOLDS if float(np.float32(t)) != t}


def test_iou_reference_on_hand_cases(s3r, oracle):
    t = np.float32(0.3)
    lo, hi = np.nextafter(t, np.float32(0)), np.nextafter(t, np.float32(1))
    nan, inf = np.float32("nan"), np.float32("inf")
    pred = np.array([[t, hi, hi, nan, inf, -0.0], [t, lo, 0, nan, -inf, -0.0]], np.float32)
    gt = np.array([[hi, hi, lo, hi, hi, 0.0], [lo, t, nan, nan, -0.0, 0.0]], np.float32)
    # sample 0: pred occupied at 1, 2, 4; gt at 0, 1, 3, 4: intersection 2, union 5.  sample 1: nothing occupied: 1
    got = SR.iou_ref(pred, gt, 0.3)
    assert got.tolist() == [float(np.float32(2) / np.float32(5)), 1.0]
    assert float(np.float32(0.3)) > 0.3 and sorted(s3r.evaluate.THRESHOLDS) == [0.2, 0.3, 0.4, 0.5]
    # the big case: both counts pass 2^24 and neither is an fp32 number
    pred, gt = C.iou_big_case()
    u, i = C.IOU_BIG_V, C.IOU_BIG_V - C.IOU_BIG_UNSET
    assert u > 2 ** 24 and i > 2 ** 24 and int(np.float32(u)) == u + 1 and int(np.float32(i)) == i - 1      # ties to even, up and down
    assert SR.iou_ref(pred, gt, 0.5)[0] == np.float32(i - 1) / np.float32(u + 1) != np.float32(i - 1) / np.float32(u - 1)
    # on data without special values the oracle agrees (its threshold is a Python float: on float32 tensors torch compares in fp32)
    for V in (255, 32768):
        g = torch.Generator().manual_seed(V)
        a, b = torch.rand(3, V, generator=g), torch.rand(3, V, generator=g)
        SR.assert_same(SR.iou_ref(a.numpy(), b.numpy(), 0.4), oracle.voxel_iou(a, b, 0.4).numpy(), "iou", f"random V={V}")


# ---------------------------------------------------------------- metrics
def test_metrics_case_holds_what_it_is_there_for():
    pred, gt = C.metrics_case()
    with np.errstate(over="ignore"):
        epe, counts = D64.metrics(pred, gt)
    P = pred.shape[1]
    assert counts[0, 0] == P and np.signbit(gt[0]).all()                        # -0.0 is valid
    assert P // 4 <= counts[0, 1] < P - P // 4 and counts[0, 2] < counts[0, 1]      # errors of exactly 1 and 3 are not above them
    assert counts[1, 0] == P and (gt[1] > 0).all() and (gt[1] < np.finfo(np.float32).tiny).all()      # subnormal ground truth is valid
    assert np.isinf(epe[2]) and counts[2, 0] == P and np.isfinite(gt[2]).all() and np.isfinite(pred[2]).all()
    assert np.isfinite(np.delete(epe, 2)).all()
    assert D64.metrics(pred[3:4, :3], gt[3:4, :3])[1].tolist() == [[3, 2, 1, 0]]
    assert counts[4, 0] == 2 * (P // 5) + 1 and epe[4] < 8       # -0.0, +subnormal and FLT_MAX valid; inf, NaN, -subnormal not


# ---------------------------------------------------------------- the written contract
def test_the_contract_sentences_are_written_down(s3r, oracle):
    header = " ".join(open(os.path.join(ROOT, "include", "s3r.h")).read().split())
    for words in ("((dx*dx + dy*dy) + dz*dz)", "lowest index", "minNum", "dist = +inf, idx = 0", "non-finite loss",
                  "NaN is not occupied", "rounded to fp32", "round-to-nearest-even"):
        assert words in header, words
    for fn, words in ((s3r.chamfer_distance, ("lowest index", "minNum", "+inf, idx = 0")), (s3r.voxel_iou, ("NaN is not occupied", "strict")),
                      (oracle.chamfer_distance, ("torch.min", "NaN"))):
        doc = " ".join(fn.__doc__.split())
        for w in words:
            assert w in doc, (fn.__name__, w)
    design = " ".join(open(os.path.join(ROOT, "DESIGN.md")).read().split())
    assert "tests/_select_ref.py" in design and "first minimum" in design
