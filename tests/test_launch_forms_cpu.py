"""tests/_launch_cases.py without a GPU: computed from the restatement alone at 256 compute units, every row of the table takes the
launch form it is in the table for and the rows reach, between them, every edge of the cut's arithmetic; every case is exact
(tests/_lattice.py); and its data can see a mistake in that arithmetic — a remainder that starts one tile off, a dropped ragged tile,
two cout tiles of the remainder swapped all differ from the float64 reference.  What the library does on a device is
tests/test_launch_forms_gpu.py's half."""
import pytest
import torch

from tests import _launch_cases as LC
from tests import _lattice as LT

CUS = 256
PLANS = {c.id: LC.plan(c, CUS) for c in LC.CASES}
CUT = [c for c in LC.CASES if PLANS[c.id].n_cut is not None]


@pytest.mark.parametrize("c", LC.CASES, ids=[c.id for c in LC.CASES])
def test_row_takes_the_form_the_table_names(c):
    row, q = LC.ROW_OF[c.id], PLANS[c.id]
    assert LC.kind(q.bits, c) == row.want, (c.id, q)
    assert (q.n_cut or 0) == row.n_cut, (c.id, q.n_cut, row.n_cut)
    assert LC.form(c, CUS) == {"one-launch": (3, 1), "two-launch": (5, 2), "two-stage": (0, 1), "ring": (4, 1)}[row.want]
    if row.tile >= 0:
        assert q.cfg == row.tile
    if q.n_cut is not None:
        bm, bn = LC.TILE_DIMS[q.cfg]
        assert q.cfg != 3 and q.n_cut % bn == 0 and 0 < q.tail < q.g.Ntotal
        # the bulk's workgroups end within one position tile's worth of a whole number of rounds
        per_tile = LC.cdiv(q.g.cout, bm) * (8 if q.g.transposed else 1)
        bulk = per_tile * (q.n_cut // bn)
        rounds = LC.cdiv(bulk, CUS)
        assert rounds >= 1 and bulk <= rounds * CUS < bulk + per_tile


def test_no_row_matches_a_tuned_shape():
    """a kTuned row would pick the tile of the AUTO case from the table, not from the rules restated here"""
    for c in LC.CASES:
        assert not LC.matches_ktuned(LC.geometry(c.layer, c.n_in, c.B)), c.id
    assert len(LC.KTUNED) == 16 and len(set(LC.KTUNED)) == 16


def test_rows_reach_every_edge_of_the_cut():
    have = set()
    for c in CUT:
        q = PLANS[c.id]
        g = q.g
        have.add("one-launch" if q.bits & LC.FORM_ONE_LAUNCH else "two-launch")
        have.add("cut inside a row" if q.n_cut % g.Nw else "cut on a row boundary")
        if q.n_cut % g.S:
            have.add("cut inside a sample")
        else:
            have.add("cut on a sample boundary")
        have.add("ragged last tile" if q.tail % 64 else "whole last tile")
        if q.tail <= 64:
            have.add("one-tile remainder")
        if q.tail < 64:
            have.add("one partial tile")
        have.add(f"vec{q.vec}")
        if g.stride == 2:
            have.add("stride 2")
        have.add("couts fill their tiles" if g.cout % 64 == 0 and g.cout % LC.TILE_DIMS[q.cfg][0] == 0 else "ragged cout tile")
        if LC.cdiv(g.cout, 64) != LC.cdiv(g.cout, LC.TILE_DIMS[q.cfg][0]):
            have.add("other cout tiling in the remainder")
        if g.transposed:
            have.add("transposed")
        if q.cfg not in LC.DUAL_TILES:
            have.add("tile without a dual kernel")
        if c.tile < 0:
            have.add("auto pick")
        if q.launches == 2 and q.bits & LC.FORM_RING:
            have.add("ring on a sub-range")
        if c.layer.act == "leaky_relu":
            have.add("leaky")
        if not c.layer.bn:
            have.add("no batchnorm")
        have.add(f"out_halo {c.out_halo}")
        have.add(f"tile {q.cfg}")
    want = {"one-launch", "two-launch", "cut inside a row", "cut inside a sample", "cut on a sample boundary", "ragged last tile",
            "whole last tile", "one-tile remainder", "one partial tile", "vec1", "vec4", "stride 2", "couts fill their tiles",
            "ragged cout tile", "other cout tiling in the remainder", "transposed", "tile without a dual kernel", "auto pick",
            "ring on a sub-range", "leaky", "no batchnorm", "out_halo 0", "out_halo 1", "out_halo 2", "out_halo 3",
            "tile 0", "tile 1", "tile 2", "tile 4", "tile 6", "tile 7"}
    assert want <= have, sorted(want - have)
    # the uncut 64 x 64 tile on both sides of the ring's threshold, as close to it as whole cout tiles allow
    wgs = {LC.ROW_OF[c.id].want: LC.cdiv(c.layer.cout, 64) * LC.cdiv(PLANS[c.id].g.Ntotal, 64) for c in LC.CASES if c.tile == 3}
    assert wgs == {"two-stage": 392, "ring": 368} and wgs["ring"] <= LC.RING_MAX_WGS < wgs["two-stage"]


def test_one_launch_rows_cut_under_the_two_launch_model_too():
    """S3R_NO_DUAL: the same rows as two launches (tests/test_launch_forms_gpu.py runs them so in a child process)"""
    for c in LC.ONE_LAUNCH:
        assert LC.form(c, CUS, dual_built=False) == (LC.FORM_CUT | LC.FORM_RING, 2), c.id
        assert LC.plan(c, CUS, dual_built=False).n_cut == PLANS[c.id].n_cut


def test_restatement_follows_the_compute_units():
    """the plan is a function of the device: at 304 compute units most rows fit their rounds and go out uncut; the restatement
    answers for any count (the GPU test asks it for the device's own)"""
    kinds = [LC.kind(LC.form(c, 304)[0], c) for c in LC.CASES]
    assert kinds.count(None) >= 10 and "two-stage" in kinds and "ring" in kinds
    assert LC.tail_cut(70, 33712, 1, False, True, 256) == 32768 and LC.tail_cut(70, 33712, 1, False, True, 33712) is None
    assert LC.tail_cut(32, 33712, 2, False, True, 256) is None and LC.tail_cut(70, 33712, 3, False, True, 256) is None
    assert LC.tail_cut(70, 256 * 256, 1, False, True, 256) is None                 # whole rounds: nothing to cut
    assert LC.pick_tile(130, 65600, False) == 7 and LC.pick_tile(130, 65600 // 2, False) == 3 and LC.pick_tile(32, 65600, False) == 2


_REF = {}


def _made(d):
    if d not in _REF:
        x, p = d.make()
        _REF[d] = (x, p, LT.expected(d.layer, x, p))
    return _REF[d]


DATA = []
for _c in LC.CASES:
    if _c.data not in DATA:
        DATA.append(_c.data)


@pytest.mark.parametrize("d", DATA, ids=[d.id for d in DATA])
def test_case_is_admissible(d):
    x, p, _ = _made(d)
    rec = LT.exactness(d.layer, x, p, d.form, d.dtype)
    print(f"\n{d.id}: " + " ".join(f"{k}={v:.4g}" if isinstance(v, float) else f"{k}={v}" for k, v in rec.items()))
    assert LT.admissible(rec) is None, (LT.admissible(rec), rec)


@pytest.mark.parametrize("c", CUT, ids=[c.id for c in CUT])
def test_data_sees_a_mistake_in_the_cut(c):
    q = PLANS[c.id]
    _, _, want = _made(c.data)
    ref, mutants = LC.cut_mutants(want, q)
    assert ref.shape == (q.g.cout, 8 if q.g.transposed else 1, q.g.Ntotal)
    expect = {"shifted-back"} | ({"shifted-on"} if q.tail >= 128 else set()) | ({"ragged-zeroed"} if q.tail % 64 else set()) | \
        ({"halves-swapped"} if q.g.cout > 64 else set())
    assert set(mutants) == expect
    for name, m in mutants.items():
        assert not torch.equal(m.view(torch.int32), ref.view(torch.int32)), (c.id, name, "goes unseen")


def test_position_view_is_the_launchers():
    """by_position: position n of a convolution is (b, flat spatial); of a transposed layer, class (rd, rh, rw) at input position n
    is output (2 pd + rd, 2 ph + rh, 2 pw + rw) — make_params' decode"""
    g = LC.geometry(LC.c2(48), 5, 2)
    y = torch.arange(2 * 48 * 25, dtype=torch.float32).reshape(2, 48, 5, 5)
    v = LC.by_position(y, g)
    assert v.shape == (48, 1, 50) and float(v[7, 0, 25 + 13]) == float(y[1, 7, 2, 3])
    g = LC.geometry(LC.dc(48), 3, 2)
    y = torch.arange(2 * 48 * 216, dtype=torch.float32).reshape(2, 48, 6, 6, 6)
    v = LC.by_position(y, g)
    assert v.shape == (48, 8, 54) and float(v[5, 0b101, 27 + (2 * 3 + 1) * 3 + 2]) == float(y[1, 5, 2 * 2 + 1, 2 * 1 + 0, 2 * 2 + 1])
