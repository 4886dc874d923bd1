"""Host-side half of tests/test_exact_gpu.py: the lattice harness proves itself without a GPU.

For the data of every case of the GPU file: the case is admissible (tests/_lattice.py::exactness, conditions computed from the
reference alone), and the comparison it allows — bit equality with `expected` — catches, on the CPU restatement of the layer in
fp32, ONE (channel, tap) weight zeroed, one doubled, one output shifted by a position, and on bf16 outputs a conversion that
truncates or rounds halves away from zero.  For the deep layers (K >= 16384: p1, v6, the 32768-wide linear shape) the two
single-term mutants are also shown to be INVISIBLE to tests/_ref64.py's bound — the reason this file exists.  Which
configurations the library refuses is checked against its planner (host only).
"""
import ctypes as C
import dataclasses
import os

import pytest
import torch

from tests import _buffer_cases as BC
from tests import _exact_cases as X
from tests import _lattice as LT
from tests import _ref64 as R

torch.set_num_threads(min(16, torch.get_num_threads()))
DATA = X.unique_data()


@pytest.fixture(scope="module")
def lib(s3r):
    import __graft_entry__ as g
    if not os.path.exists(s3r.LIB_PATH):
        g.build()
    return s3r.load_library()


# ---------------------------------------------------------------- admissibility
@pytest.mark.parametrize("d", DATA, ids=[d.id for d in DATA])
def test_case_is_admissible(d):
    x, p = d.make()
    rec = LT.exactness(d.layer, x, p, d.form, d.dtype)
    print(f"\n{d.id}: " + " ".join(f"{k}={v:.4g}" if isinstance(v, float) else f"{k}={v}" for k, v in rec.items()))
    assert LT.admissible(rec, d.bf16_out) is None, (LT.admissible(rec, d.bf16_out), rec)


AUTO_SWEEP = [c for c in X.WINO_SHAPE_CASES if c.algo == 0]


@pytest.mark.parametrize("c", AUTO_SWEEP, ids=[c.id for c in AUTO_SWEEP])
def test_auto_case_is_admissible_under_the_form_it_resolves_to(s3r, lib, c):
    """a sweep case under algo = AUTO runs whatever the policy picks: its data must be on THAT form's lattice with that form's flow
    below 2^24 (two-axis data is one-axis data too — multiples of 576 are multiples of 24, one tap per joint fibre is at most one per
    H fibre — but not the other way round, and the flow differs), and the planner must resolve it to a Winograd form at all"""
    form = X.auto_form(c)
    x, p = c.data.make()
    rec = LT.exactness(c.layer, x, p, form)
    assert LT.admissible(rec) is None, (form, LT.admissible(rec), rec)
    assert c.data.form == form or (c.data.form, form) == ("f43x2", "f43-h"), (c.data.form, form)
    # (host only: AUTO plans a transformed input for this descriptor exactly when it resolves to a Winograd form over an edge % 4 == 0;
    # at other edges the scratch of the forced algorithm is what AUTO asks for too)
    auto, forced = _desc(s3r, c), _desc(s3r, dataclasses.replace(c, algo=X.WINO, tile=3 if form != "f43-h" else -1))
    need = lib.s3r_conv_scratch_elems(C.byref(auto))
    assert need > 0 and need == lib.s3r_conv_scratch_elems(C.byref(forced)), (need, lib.s3r_last_error())


# ---------------------------------------------------------------- mutation self-test
def _one_channel(layer, p, o):
    w = p["w"]
    w = w[:, o:o + 1] if layer.op.startswith("deconv") else w[o:o + 1]
    return dataclasses.replace(layer, cout=1), {"w": w.clone(), "scale": None if p["scale"] is None else p["scale"][o:o + 1],
                                                 "shift": None if p["shift"] is None else p["shift"][o:o + 1]}


def _term_with_effect(layer, x, p, active):
    """flat index into w of ONE (channel, tap) term whose own contribution reaches an output that is non-zero after the activation"""
    w = p["w"]
    nz = w.reshape(-1).nonzero().reshape(-1)
    order = nz[torch.randperm(nz.numel(), generator=torch.Generator().manual_seed(1))]
    for t in order[:64].tolist():
        single = torch.zeros_like(w)
        single.reshape(-1)[t] = w.reshape(-1)[t]
        if bool(((R.linmap(layer, x.double(), single.double()) != 0) & active).any()):
            return t
    raise AssertionError("no single term reaches an active output: the case cannot see a dropped term")


def _rhaz_bf16(v):
    """fp32 -> bf16 rounding halves AWAY from zero (add half a bf16 ulp to the magnitude, truncate)"""
    b = v.contiguous().view(torch.int32)
    return (((b & 0x7FFFFFFF) + 0x8000) & ~0xFFFF | (b & -2 ** 31)).view(torch.float32)


def _trunc_bf16(v):
    return (v.contiguous().view(torch.int32) & ~0xFFFF).view(torch.float32)


@pytest.mark.parametrize("d", DATA, ids=[d.id for d in DATA])
def test_bit_equality_catches_every_mutant(d):
    _mutants_caught(d, *d.make())


def _vector_mutants_caught(d, xs, p):
    """a given scale taken as 1, a given shift taken as 0: each must change an output bit (on an active channel with scale != 1 /
    shift != 0, or the case could not tell a kernel that ignores the vector)"""
    want = LT.expected(d.layer, xs, p, "bf16" if d.bf16_out else "fp32")
    bits = (lambda t: t.view(torch.int16)) if d.bf16_out else (lambda t: t.view(torch.int32))
    for k, name in (("scale", "scale taken as 1"), ("shift", "shift taken as 0")):
        if p[k] is not None:
            got = LT.fp32_layer(d.layer, xs, dict(p, **{k: None}))
            got = got.to(torch.bfloat16) if d.bf16_out else got
            assert not torch.equal(bits(got), bits(want)), (name, "not caught")


def test_null_forms_hold_the_vectors_they_say():
    for site, forms in X.EP_GROUPS:
        for d in forms:
            _, p = d.make()
            assert (p["scale"] is None) == (d.ep[0] == "0") and (p["shift"] is None) == (d.ep[1] == "0"), (site, d.ep)
    for c in X.LINEAR_NULL_BIAS:
        _, p = c.data.make()
        assert p["scale"] is None and p["shift"] is None


@pytest.mark.parametrize("site,forms", X.EP_GROUPS, ids=[g[0] for g in X.EP_GROUPS])
def test_epilogue_forms_differ_pairwise_and_see_their_vectors(site, forms):
    """the four forms of a site share x and w; their expected outputs differ pairwise (a NULL form that reused a sibling's vector would
    show), and for each given vector the mutants `scale taken as 1` and `shift taken as 0` change an output bit"""
    assert [d.ep for d in forms] == list(LT.EP_FORMS)
    made = [d.make() for d in forms]
    assert all(torch.equal(m[0], made[0][0]) and torch.equal(m[1]["w"], made[0][1]["w"]) for m in made)
    sc, sh = made[0][1]["scale"], made[0][1]["shift"]
    assert torch.equal(made[2][1]["scale"], sc) and bool((made[1][1]["shift"] == sh.floor()).all())
    outs = [LT.expected(d.layer, x, p, "bf16" if d.bf16_out else "fp32") for d, (x, p) in zip(forms, made)]
    act = outs[0].float().transpose(0, 1).reshape(forms[0].layer.cout, -1) if forms[0].layer.op != "linear" else outs[0].float().t()
    live = (act != 0).any(1)
    assert bool((live & (sc != 1) & (sh != 0)).any()), "no active channel with scale != 1 and shift != 0"
    for i in range(4):
        for j in range(i):
            assert not torch.equal(outs[i], outs[j]), (site, forms[i].ep, forms[j].ep)
    for d, (x, p) in zip(forms, made):
        _vector_mutants_caught(d, x, p)


def _mutants_caught(d, xs, p):
    """d: the Data whose layer / form / dtype apply; (xs, p): the layer's actual input and parameters"""
    x = xs[:1]
    for o in range(d.layer.cout // 2, d.layer.cout):            # (the first channel from the middle on that has an output above the ReLU)
        l1, p1 = _one_channel(d.layer, p, o)
        if bool((R.ref64(l1, x, p1)[0] != 0).any()):
            break
    want = LT.expected(l1, x, p1, "bf16" if d.bf16_out else "fp32")
    bits = (lambda t: t.view(torch.int16)) if d.bf16_out else (lambda t: t.view(torch.int32))
    to_out = (lambda t: t.to(torch.bfloat16)) if d.bf16_out else (lambda t: t)
    clean = LT.fp32_layer(l1, x, p1)
    assert torch.equal(bits(to_out(clean)), bits(want)), "the fp32 restatement itself differs from the reference"
    ref, mag = R.ref64(l1, x, p1)
    active = ref != 0
    assert bool(active.any()), "no channel with an active output"
    t = _term_with_effect(l1, x, p1, active)
    deep = R.k_terms(d.layer) >= 16384 and d.form == "direct"      # (dense data: a Winograd case keeps one tap in 9 or 16)
    bnd = R.bound(l1, ref, mag, "bf16" if d.bf16_out else ("direct" if d.form == "direct" else "wino"))
    for name, f in (("zeroed", 0.0), ("doubled", 2.0)):
        q = dict(p1, w=p1["w"].clone())
        q["w"].reshape(-1)[t] *= f
        m = LT.fp32_layer(l1, x, q)
        assert not torch.equal(bits(to_out(m)), bits(want)), (name, "one term: not caught")
        if deep and not d.bf16_out:
            r, _ = R.worst(m, ref, bnd)
            assert r <= 1.0, (name, "the fp64 bound was expected NOT to see one term at this K", r)
    flat = clean.reshape(-1)
    if flat.numel() > 1:
        i = int((flat[1:] - flat[:-1]).abs().argmax())
        s = flat.clone()
        s[i] = flat[i + 1]
        assert not torch.equal(bits(to_out(s.reshape(clean.shape))), bits(want)), "a shifted output: not caught"
    if d.bf16_out:
        full = LT.expected(d.layer, xs, p, "fp32")               # (the whole case: its share of ties is a condition on all of it)
        for name, conv in (("truncation", _trunc_bf16), ("round-half-away", _rhaz_bf16)):
            assert not torch.equal(conv(full).to(torch.bfloat16).view(torch.int16), full.to(torch.bfloat16).view(torch.int16)), \
                (name, "not caught")


# ---------------------------------------------------------------- producers: the cost volume in v1's layouts, two-layer chains
@pytest.mark.parametrize("c", X.CV_CASES, ids=[c.id for c in X.CV_CASES])
def test_cost_volume_case(c):
    vol, p = c.make()
    assert float(vol.abs().max()) <= 2 and bool((vol == vol.round()).all())
    rec = LT.exactness(c.data.layer, vol, p, c.data.form)
    print(f"\n{c.id}: {rec}")
    assert LT.admissible(rec) is None, (LT.admissible(rec), rec)
    _mutants_caught(c.data, vol, p)


_FIRST = {}


def _first_layer(c, x, p0):
    """(exactness record, intermediate) of a chain's first layer: the same for every case over one (first Data, producer form)"""
    key = (c.first, c.pep, c.dtype)
    if key not in _FIRST:
        _FIRST.clear()
        _FIRST[key] = (LT.exactness(c.first.layer, x, p0, c.first.form, c.dtype), c.intermediate(x, p0))
    return _FIRST[key]


@pytest.mark.parametrize("c", X.ALL_CHAIN_CASES, ids=[c.id for c in X.ALL_CHAIN_CASES])
def test_chain_case(c):
    x, (p0, p1) = c.make()
    assert c.first.layer.act == "relu"
    if c.pep == "unit":
        assert (p0["scale"] is None or bool((p0["scale"] == 1).all())) and bool((p0["shift"] == 0).all())
    elif c.pep == "null":
        assert p0["scale"] is None and p0["shift"] is None
    else:         # integers: the intermediate stays on the integer lattice, and the producer's scale is not the identity
        sc, sh = p0["scale"], p0["shift"]
        assert bool(((sc == 1) | (sc == 2)).all()) and bool((sc == 2).any()) and bool((sh == sh.round()).all()) and bool((sh != 0).any())
    r0, h = _first_layer(c, x, p0)
    assert bool((h == h.round()).all()), "the intermediate left the integer lattice"
    r1 = LT.exactness(c.second.layer, h, p1, c.second.form, c.dtype)
    print(f"\n{c.id}: {r0}\n{r1}")
    # (the intermediate of the bf16 chain is never stored as bf16 data the test reads: no share of ties is asked of it, but it must
    # be exact in bf16, so that rounding it or not is the same number)
    assert LT.admissible(r0) is None and LT.admissible(r1) is None, (LT.admissible(r0), LT.admissible(r1))
    if c.dtype == "bf16":
        assert float(h.abs().max()) <= 256 and torch.equal(h, LT.expected(c.first.layer, x, p0))
    _mutants_caught(dataclasses.replace(c.second, dtype="fp32"), h, p1)
    _vector_mutants_caught(dataclasses.replace(c.second, dtype="fp32"), h, p1)
    if c.pep == "int":        # the PRODUCER's vectors inside the fused epilogue: scale taken as 1, shift taken as 0
        want = LT.expected(c.second.layer, h, p1)
        for name, q in (("producer scale as 1", dict(p0, scale=None)), ("producer shift as 0", dict(p0, shift=None))):
            assert not torch.equal(LT.expected(c.second.layer, c.intermediate(x[:2], q), p1), want[:2]), (name, "not caught")


def _head_routes():
    routes = {}
    for c in X.HEAD_CHAIN_CASES:
        routes.setdefault((c.first, c.pep, c.algo, c.tile), []).append(c)
    return list(routes.values())


@pytest.mark.parametrize("group", _head_routes(), ids=lambda g: g[0].id.rsplit("-h", 1)[0])
def test_head_forms_of_a_route_differ_pairwise(group):
    """a NULL head vector that silently took a sibling's values would give that sibling's output"""
    assert [c.second.ep for c in group] == list(LT.EP_FORMS)
    x, (p0, _) = group[0].make()
    h = group[0].intermediate(x[:2], p0)
    outs = [LT.expected(c.second.layer, h, c.make()[1][1]) for c in group]
    for i in range(4):
        for j in range(i):
            assert not torch.equal(outs[i], outs[j]), (group[i].id, group[j].id)


@pytest.mark.parametrize("group", _head_routes()[::2], ids=lambda g: g[0].id.rsplit("+head", 1)[0])
def test_head_weighs_its_first_and_last_channel_and_dropping_either_is_a_mismatch(group):
    """a fused head that skipped its last (or first) input channel passes wherever that channel's weight is 0 (tests/mutants/table.py:
    dwino3_head_last_channel did, on the head data this suite had before)"""
    c = group[0]
    x, (p0, p1) = c.make()
    w = p1["w"].reshape(-1)
    assert w[0] != 0 and w[-1] != 0, (c.id, w[0], w[-1])
    h = c.intermediate(x[:2], p0)
    want = LT.expected(c.second.layer, h, p1)
    for drop in (0, -1):
        wd = p1["w"].clone() if hasattr(p1["w"], "clone") else p1["w"].copy()
        wd.reshape(-1)[drop] = 0
        assert not torch.equal(LT.expected(c.second.layer, h, dict(p1, w=wd)), want), (c.id, drop)


def test_head_chain_routes_are_the_issues(s3r, lib):
    """one row per route of conv_head_fused, eight cases each; every pair plans as a chain (that the head rode in the first layer's
    launch is asserted on the device: no head record); the tile-1 batch is the smallest with 2000 workgroups of 256 positions"""
    B = X.tile1_batch(8)
    assert -(-(B * 512) // 256) >= 2000 > -(-((B - 1) * 512) // 256)
    ids = {c.id.split("+head")[0] for c in X.HEAD_CHAIN_CASES}
    assert ids == {"direct-c24-tile2", "direct-c40-tile7", f"direct-c40-tile1-B{B}", "transposed-direct", "dwino2-tile0", "dwino2-tile1",
                   "dwino2-tile2", "dwino3-tile6", "dwino3-tile7", "dwino3-tile8", "d3+d4"} and len(X.HEAD_CHAIN_CASES) == 11 * 8
    for c in X.HEAD_CHAIN_CASES[::8]:
        arr = (s3r._lib.Layer * 2)()
        arr[0].desc = s3r._lib.make_desc(c.first.layer, c.first.B, c.first.n_in, tag=0, algo=c.algo, tile=c.tile)
        arr[1].desc = s3r._lib.make_desc(c.second.layer, c.first.B, c.second.n_in, tag=1)
        assert lib.s3r_chain_workspace_elems(arr, 2) >= 0, (c.id, lib.s3r_last_error())      # (0: a fused 1 x 1 x 1 pair needs nothing)
        assert 33 <= c.first.layer.cout <= 64 or c.first.layer.cout == 24, c.id


def test_rounding_mutants_are_what_they_say():
    v = torch.tensor([257.0, 259.0, 258.5, -257.0, -259.0, 1.0, 300.25])           # 257: tie, even below; 259: tie, even above
    assert _trunc_bf16(v).tolist() == [256.0, 258.0, 258.0, -256.0, -258.0, 1.0, 300.0]
    assert _rhaz_bf16(v).tolist() == [258.0, 260.0, 258.0, -258.0, -260.0, 1.0, 300.0]
    assert v.to(torch.bfloat16).float().tolist() == [256.0, 260.0, 258.0, -256.0, -260.0, 1.0, 300.0]
    assert LT.bf16_shares(v) == (4 / 7, 2 / 7)


def test_lattice_steps_come_from_the_matrices():
    """F(4, 3) with the points 0, +-1, +-2, inf: 24; F(2, 4) with 0, +-1, 2, inf: 6 (computed, tools/wino_matrices.py's construction)"""
    assert LT.wino_step("f43") == 24 and LT.wino_step("f24") == 6 and LT.wino_step("f22") == 1
    for kind in ("f43", "f24"):
        AT, G, BT = LT.wino_matrices(kind)
        assert all(v.denominator == 1 for row in AT + BT for v in row), "B^T and A^T are integer matrices"


# ---------------------------------------------------------------- refusals (host only: the planner)
def _desc(s3r, c):
    ih = c.in_halo if c.in_halo >= 0 else BC.need_halo(c.layer, c.n_in, c.dtype)
    return s3r._lib.make_desc(c.layer, c.B, c.n_in, tile=c.tile, in_halo=ih, out_halo=c.out_halo, ksplit=c.ksplit,
                              dtype=s3r._lib.DTYPE[c.dtype], algo=c.algo)


CONV = [c for c in X.ALL_CASES if c.layer.op != "linear" and c.dtype == "fp32"]


def _plans(s3r, lib, l, n, tile, oh):
    d = s3r._lib.make_desc(l, 1, n, tile=tile, in_halo=1, out_halo=oh, algo=X.WINO)
    r = lib.s3r_conv_scratch_elems(C.byref(d))
    return r >= 0, r, lib.s3r_last_error()


def test_two_axis_lds_rule_is_the_planners(s3r, lib):
    """include/s3r.h, s3r_algo: the two-axis Conv2d form (tile 3, 4, 5) serves an edge n <= 124 with n + 2 out_halo <= 128, the
    semi-fused Conv3d form (tile 5) n <= 60 with n + 2 out_halo <= 64; the class-parallel Conv3d form (tile 4) has no such bound and
    the library's pick (tile 3) takes it outside the semi-fused form's.  The scratch query plans a descriptor if and only if that
    rule holds — restated here from the header, not from the planner: before this test the planner knew the edge bounds only, and
    the launcher refused the rest behind an enqueued input transform (177 of the 756 descriptors here disagreed)."""
    wrong = []
    for n in range(112, 126):
        for oh in range(9):
            for tile in (3, 4, 5):
                ok, r, msg = _plans(s3r, lib, X.L("t", "conv2d", 32, 2, 3, 1, 1), n, tile, oh)
                want = n <= 124 and n + 2 * oh <= 128
                if ok != want or (not ok and n <= 124 and b"128" not in msg):
                    wrong.append(("conv2d", n, oh, tile, want, r, msg))
    for n in range(48, 62):
        for oh in range(9):
            for tile in (3, 4, 5):
                ok, r, msg = _plans(s3r, lib, X.L("t", "conv3d", 32, 2, 3, 1, 1), n, tile, oh)
                want = tile != 5 or (n <= 60 and n + 2 * oh <= 64)
                if ok != want or (not ok and b"64" not in msg):
                    wrong.append(("conv3d", n, oh, tile, want, r, msg))
    assert not wrong, (len(wrong), wrong[:8])


def test_library_pick_sizes_its_scratch_for_the_form_it_can_launch(s3r, lib):
    """Conv3d 32 -> 2 over edge 60 with out_halo 3 under algo = WINOGRAD, tile = 3 (the two-axis algorithm in the library's launch
    form) at batches where the library would take the semi-fused form: four 66^2 slices do not fit, so the plan is the
    class-parallel form's — for ANY batch the scratch is that of tile 4.  (tile = -1 resolves this edge, above 28, to the one-axis
    kernel, which has no such bound.)"""
    l = X.L("t", "conv3d", 32, 2, 3, 1, 1)
    for B in (1, 2, 8):
        need = {}
        for tile in (-1, 3, 4):
            d = s3r._lib.make_desc(l, B, 60, tile=tile, in_halo=1, out_halo=3, algo=X.WINO)
            need[tile] = lib.s3r_conv_scratch_elems(C.byref(d))
        one = s3r._lib.make_desc(l, B, 60, tile=1, in_halo=1, out_halo=3, algo=X.WINO)      # (the library's pick is sized class-parallel)
        assert need[3] == need[4] > 0 and need[-1] == lib.s3r_conv_scratch_elems(C.byref(one)) > 0, (B, need, lib.s3r_last_error())


def test_refusals_match_the_planner(s3r, lib):
    """fp32: a forced tile without its gather is refused by the scratch query, everything else plans (the bf16 path refuses a forced
    tile when it resolves the launch: the GPU file asserts those)"""
    wrong = []
    for c in CONV:
        d = _desc(s3r, c)
        if (lib.s3r_conv_scratch_elems(C.byref(d)) < 0) != c.refused:
            wrong.append((c.id, c.refused, lib.s3r_last_error()))
    assert not wrong, wrong
