"""Identities between the planner's size answers (csrc/s3r_plan_algo.hip, s3r_plan_geometry.hip, s3r_plan_chain.hip): each rule is
stated once in the library, and what two queries say about the same tensor must agree.  Host only, no GPU."""
import ctypes as C
import os

import pytest


@pytest.fixture(scope="module")
def lib(s3r):
    return s3r.load_library()


def _align(n):
    return -(-n // 256) * 256


def _scratch(lib, d):
    n = lib.s3r_conv_scratch_elems(C.byref(d))
    assert n >= 0, lib.s3r_last_error()
    return n


def _consumers(s3r):
    """(id, layer, edge, in_halo, the layout its producer may write, desc keywords, explicit per-sample count or None = ask the query)"""
    L, Ly = s3r._lib, s3r.arch_spec.Layer
    W = L.ALGO_WINOGRAD
    c2 = lambda ci, co: Ly("c", "conv2d", ci, co, 3, 1, 1)
    c3 = lambda ci, co, k=3, p=1: Ly("c", "conv3d", ci, co, k, 1, p)
    return [("wino-h-conv2d-32to48-e40", c2(32, 48), 40, 1, L.LAYOUT_WINO_H, dict(algo=W, tile=0), None),
            ("wino-h-conv3d-64to64-e12", c3(64, 64), 12, 1, L.LAYOUT_WINO_H, dict(algo=W, tile=0), None),
            ("wino-dh-conv3d-32to64-e12", c3(32, 64), 12, 1, L.LAYOUT_WINO_DH, {}, None),
            ("wino-hw-conv2d-64to96-e20", c2(64, 96), 20, 1, L.LAYOUT_WINO_HW, dict(algo=W, tile=3), None),
            ("wino-hw-conv2d-64to96-e124", c2(64, 96), 124, 1, L.LAYOUT_WINO_HW, dict(algo=W, tile=3), None),
            # (no query names WINO_3D: the explicit count — 36 sets of 2 x 2 groups x 9 padded columns; 25 sets of 3 x 3 groups x 8 columns)
            ("wino-3d-conv3d-32to32-e7-k3p1", c3(32, 32), 7, 1, L.LAYOUT_WINO_3D, {}, 36 * 32 * 2 * 2 * 9),
            ("wino-3d-conv3d-32to32-e8-k4p0", c3(32, 32, 4, 0), 8, 0, L.LAYOUT_WINO_3D, {}, 25 * 32 * 3 * 3 * 8)]


@pytest.mark.parametrize("B", [1, 3])
def test_operand_size_is_what_a_written_operand_saves(s3r, lib, B):
    """A consumer fed with its transformed operand needs exactly that operand less scratch: scratch(plain input) - scratch(layout
    input) == s3r_conv_wino_input_elems rounded up to 256 — the element count of an operand, said by two queries"""
    L = s3r._lib
    for cid, layer, n, halo, layout, kw, per_sample in _consumers(s3r):
        plain = L.make_desc(layer, B, n, in_halo=halo, **kw)
        fed = L.make_desc(layer, B, n, in_halo=halo, in_layout=layout, **kw)
        if per_sample is None:
            assert lib.s3r_conv_wino_input_layout(C.byref(plain)) == layout, cid
            elems = lib.s3r_conv_wino_input_elems(C.byref(plain))
            assert elems > 0, cid
        else:
            elems = B * per_sample
        assert _scratch(lib, plain) - _scratch(lib, fed) == _align(elems), (cid, B)


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("pair", ["v4", "v5"])
def test_handoff_region_is_the_consumers_operand(s3r, lib, pair, B):
    """The region of a 3D hand-off pair is sized from the PRODUCER's descriptor (out_layout), the operand it may hold from the
    CONSUMER's (in_layout): the two must be one size.  Observed as tests/test_handoff3d_cpu.py observes the arena: workspace of the
    two-layer chain == the larger of the plain activation and the consumer-side operand + the scratch both layers share."""
    if os.environ.get("S3R_WINO") not in (None, "1") or os.environ.get("S3R_WINO_HANDOFF") not in (None, "1"):
        pytest.skip("the library's own plan is under test (the switches are read once, at load)")
    L = s3r._lib
    rows = s3r.arch_spec.stage_table("decoder")
    i = next(i for i, (l, _, _) in enumerate(rows) if l.name == pair)
    (a, na, ma), (b, nb, _) = rows[i], rows[i + 1]
    hb = b.p                                                          # the halo the consumer reads: v5 k3 p1, v6 k4 p0
    arr = (L.Layer * 2)()
    arr[0].desc, arr[1].desc = L.make_desc(a, B, na, tag=0, in_halo=1), L.make_desc(b, B, nb, tag=1)
    need = lib.s3r_chain_workspace_elems(arr, 2)
    assert need > 0, lib.s3r_last_error()
    cons = L.make_desc(b, B, nb, in_halo=hb)
    fed = L.make_desc(b, B, nb, in_halo=hb, in_layout=L.LAYOUT_WINO_3D)
    operand = _scratch(lib, cons) - _scratch(lib, fed)                # (already rounded up to 256)
    assert operand > 0
    plain = B * a.cout * (ma + 2 * hb) ** 3
    scratch = max(_scratch(lib, L.make_desc(a, B, na, in_halo=1, out_halo=hb)), _scratch(lib, cons))
    assert need == max(_align(plain), operand) + _align(scratch), (pair, B, need, plain, operand, scratch)


def test_fits_one_call_edge(s3r, lib):
    """One call's plane sets stay under 2 GiB: the v1-shaped layer's 36 sets are 36 x 64 x 7 x 7 x 30 floats a sample, so the first
    batch a producer cannot write them for follows on the CPU; there, and one below, the layout and the size answer flip together"""
    L = s3r._lib
    layer = s3r.arch_spec.Layer("c", "conv3d", 64, 64, 3, 1, 1)
    per_sample = 36 * 64 * (28 // 4) ** 2 * (28 + 2)
    first_plain = (2 ** 31 - 1) // (4 * per_sample) + 1
    assert first_plain == 159
    for B, layout in ((first_plain - 1, L.LAYOUT_WINO_DH), (first_plain, L.LAYOUT_PLAIN)):
        d = L.make_desc(layer, B, 28, in_halo=1)
        assert lib.s3r_conv_wino_input_layout(C.byref(d)) == layout, B
        assert lib.s3r_conv_wino_input_elems(C.byref(d)) == (B * per_sample if layout else 0), B


def test_refusals_stated_on_both_paths_keep_their_texts(s3r, lib):
    """resolve_algo refuses a Conv2d whose padded output plane does not fit the two-axis finish kernel's LDS under WINOGRAD and under
    AUTO, and a two-axis layout under a direct kernel: each text once in the library, each prefix / suffix as it was"""
    L = s3r._lib
    layer = s3r.arch_spec.Layer("c", "conv2d", 32, 2, 3, 1, 1)
    plane = "the two-axis form of a Conv2d stages one padded output plane in 64 KiB of LDS: edge + 2 out_halo <= 128 (got 124 + 2 x 3)"
    for d, msg in ((L.make_desc(layer, 1, 124, in_halo=1, out_halo=3, algo=L.ALGO_WINOGRAD, tile=3), "algo = WINOGRAD: " + plane),
                   (L.make_desc(layer, 1, 124, in_halo=1, out_halo=3, in_layout=L.LAYOUT_WINO_HW), plane),
                   (L.make_desc(layer, 1, 124, in_halo=1, in_layout=L.LAYOUT_WINO_HW, algo=L.ALGO_DIRECT),
                    "a two-axis transformed input / output runs the two-axis kernel only: algo AUTO / WINOGRAD, no direct tile / split-K override")):
        assert lib.s3r_conv_scratch_elems(C.byref(d)) == -1
        assert lib.s3r_last_error().decode() == msg
