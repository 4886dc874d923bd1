"""The linear forward's launch plan (tests/_linear_cases.py) against the library's own, and the branch coverage of the shapes the
GPU files run — host only: s3r_linear_scratch_elems launches nothing."""
import os
import random

import pytest

from tests import _exact_cases as X
from tests import _linear_cases as LC


@pytest.fixture(scope="module")
def lib(s3r):
    import __graft_entry__ as g
    if not os.path.exists(s3r.LIB_PATH):
        g.build()
    return s3r.load_library()


def _suite_shapes():
    """every (B, cin, cout) tests/test_exact_gpu.py::test_linear runs"""
    return sorted({(c.B, c.layer.cin, c.layer.cout) for c in X.LINEAR_CASES})


def _draw(n=400, seed=20):
    """shapes around the plan's thresholds: Cin on and off the 32 / 128 grids and either side of 4096, couts either side of a tile
    edge and of the 128-workgroup rule, batches either side of a batch tile"""
    r = random.Random(seed)
    out = []
    for _ in range(n):
        cin = r.choice([r.randint(1, 300), 32 * r.randint(1, 140), 128 * r.randint(1, 40), 2 ** r.randint(5, 17), 4096 + 128 * r.randint(-2, 2)])
        cout = r.choice([r.randint(1, 40), 32 * r.randint(1, 140) + r.randint(-1, 1), 128 * r.randint(1, 40) + r.randint(-1, 1), r.randint(4000, 4200)])
        B = r.choice([1, 2, 3, 31, 32, 33, 64, 65, r.randint(1, 130)])
        if cin * cout <= 1 << 27:
            out.append((B, cin, cout))
    return out


def test_the_draw_reaches_every_kernel():
    kinds = {LC.plan(*s).kernel for s in _draw()}
    assert kinds == {"wgk", "stream", "naive"} and len(_draw()) >= 300


def test_plan_matches_the_library(lib):
    """the scratch is 1 float for the one-launch kernel and ks x B x Cout otherwise: equal scratch pins the kernel choice and ks"""
    wrong = []
    for B, cin, cout in LC.SWEEP + _suite_shapes() + _draw():
        p = LC.plan(B, cin, cout)
        assert p.scratch == (1 if p.kernel == "wgk" else p.ks * B * cout)
        got = lib.s3r_linear_scratch_elems(B, cin, cout)
        if got != p.scratch:
            wrong.append(((B, cin, cout), p, got))
    assert not wrong, (len(wrong), wrong[:6])


def test_plan_of_the_two_gib_rule(lib):
    """a weight tensor of 2 GiB or more leaves the 32-bit byte offsets of the two ring kernels: the naive kernel, ks = 1 (host only:
    nothing that size is allocated)"""
    for B, cin, cout in ((2, 4096, 131072), (2, 32768, 16384), (2, 4096, 131071)):
        p = LC.plan(B, cin, cout)
        assert (p.kernel == "naive") == (cin * cout * 4 >= LC.TWO31), p
        assert lib.s3r_linear_scratch_elems(B, cin, cout) == p.scratch


def test_shapes_cover_the_plan():
    """the sweep and the shapes the suite already had reach every branch label; the sweep alone the ones it was written for"""
    have = set()
    for s in LC.SWEEP + _suite_shapes():
        have |= LC.labels(*s)
    assert have >= LC.ALL_LABELS, sorted(LC.ALL_LABELS - have)
    assert have <= LC.ALL_LABELS, sorted(have - LC.ALL_LABELS)
    sweep = set()
    for s in LC.SWEEP:
        sweep |= LC.labels(*s)
    new = {"wgk-nblk-1", "wgk-nblk-2", "wgk-nblk-3", "wgk-ragged-cout", "wgk-batch-tiles", "wgk-cin-limit", "stream-nblk-1",
           "ks-4", "ks-16", "ks->=128", "finish4-q-4", "finish4-q->=32", "naive-workgroups"}
    assert sweep >= new, sorted(new - sweep)
    before = set()
    for B, cin, cout in X.LIN_SHAPES + [(B, l.cin, l.cout) for l in X.spec.POINT_HEAD for B in (1, 3)]:
        before |= LC.labels(B, cin, cout)
    assert not (before & new), ("no longer new", sorted(before & new))


def test_sweep_rows_are_what_their_comments_say():
    want = {
        (1, 128, 4096): ("wgk", 1, 1, 128, 1, False), (33, 256, 2049): ("wgk", 1, 2, 65, 2, True), (2, 384, 4099): ("wgk", 1, 3, 129, 1, True),
        (3, 4096, 4065): ("wgk", 1, 32, 128, 1, True), (65, 512, 2017): ("wgk", 1, 4, 64, 3, True),
        (3, 32, 5): ("stream", 1, 1, 1, 1, True), (2, 160, 130): ("stream", 1, 5, 2, 1, True), (40, 512, 200): ("stream", 4, 4, 2, 2, True),
        (3, 2048, 33): ("stream", 16, 4, 1, 1, True), (2, 4096, 129): ("stream", 32, 4, 2, 1, True), (1, 16384, 3): ("stream", 128, 4, 1, 1, True),
        (2, 65536, 2): ("stream", 512, 4, 1, 1, True), (9, 33, 100): ("naive", 1, 0, 4, 1, True), (5, 1056, 70): ("stream", 1, 33, 1, 1, True),
    }
    assert set(want) == set(LC.SWEEP)
    for s, w in want.items():
        p = LC.plan(*s)
        assert (p.kernel, p.ks, p.nblk, p.otiles, p.btiles, p.ragged) == w, (s, p)
    for name, s in LC.PER_KERNEL.items():
        p = LC.plan(*s)
        assert s in LC.SWEEP and name == p.kernel + ("" if p.finish is None else "-" + p.finish), (name, p)
    # linear_finish_kernel only ever sees ks <= 8: its eight-at-a-time loop (z + 8 <= ks from z = 1) needs ks >= 9
    assert all(LC.plan(*s).ks <= 8 for s in LC.SWEEP + _suite_shapes() + _draw() if LC.plan(*s).finish == "finish")
