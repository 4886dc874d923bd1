"""Host-only planning of the 3D hand-off pairs (tests/test_handoff3d_gpu.py runs them): the decoder's arena at small, benchmark and
very large batches, and the chains earlier rounds had to repair must still plan."""
import ctypes as C
import os

import pytest


@pytest.fixture(scope="module")
def lib(s3r):
    return s3r.load_library()


def _align(n):
    return -(-n // 256) * 256


@pytest.mark.parametrize("B", [1, 32, 256, 300])
def test_decoder_arena_with_handoff_regions(s3r, lib, B):
    """Every intermediate of the decoder has a region of its own, stored with its consumer's halo.  The regions of v4, v5, v6 and d1 hold
    EITHER the plain activation OR the consumer's operand — v5's 36 and v6's 25 plane sets, [x | Dh | Dd | Ddh] of d1 and d2 —
    whichever the launch forms pick on the device at hand, so they are sized for the larger: the size of an arena must not depend on
    the device it is asked on.  What depends on the batch alone decides the layout itself: d1 / d2 materialise their depth
    differences only while four tensors fit the cache (B <= 113 / 49), so at B = 256 and 300 those two regions are plain again while
    v4's and v5's still hold either form.  d3's output does not exist (fused head); the scratch is sized for the two-pass routes."""
    if os.environ.get("S3R_WINO") not in (None, "1") or os.environ.get("S3R_WINO_HANDOFF") not in (None, "1") or "S3R_DWINO_MAT" in os.environ:
        pytest.skip("the library's own plan is under test (the switches are read once, at load)")
    L = s3r._lib
    rows = s3r.arch_spec.stage_table("decoder")
    arr = (L.Layer * len(rows))()
    for i, (l, n, m) in enumerate(rows):
        arr[i].desc = L.make_desc(l, B, n, tag=i, in_halo=1 if i == 0 else 0)
    need = lib.s3r_chain_workspace_elems(arr, len(rows))
    assert need > 0, lib.s3r_last_error()
    halo = lambda l: 1 if l.op == "deconv3d" else l.p
    want, scratch = 0, 0
    for i, (l, n, m) in enumerate(rows):
        d = L.make_desc(l, B, n, in_halo=halo(l))
        scratch = max(scratch, lib.s3r_conv_scratch_elems(C.byref(d)))
        if l.name in ("d3", "d4"):
            continue
        nxt = rows[i + 1][0]
        op = m + 2 * halo(nxt)
        plain = B * l.cout * op ** 3
        operand = 0
        if l.name == "v4":
            operand = 36 * B * l.cout * 2 * 2 * op                   # v5: two groups of four for 7 per axis
        elif l.name == "v5":
            operand = 25 * B * l.cout * 2 * 2 * op                   # v6: F(2,4), 4 outputs per axis
        elif l.name in ("v6", "d1") and 16 * B * l.cout * op ** 3 <= 192 << 20:
            operand = 4 * plain
        want += _align(max(plain, operand))
    assert need == want + _align(scratch), (B, need, want, scratch)


def test_chains_earlier_rounds_repaired_still_plan(s3r, lib):
    """Linear -> ConvTranspose2d and a reshaping Conv -> ConvTranspose2d go past the new pairing untouched"""
    Ly = s3r.arch_spec.Layer
    for chain in (((Ly("a", "linear", 32, 256, 1, 1, 0, False), 1), (Ly("b", "deconv2d", 16, 8, 4, 2, 1), 4)),
                  ((Ly("a", "conv2d", 16, 64, 3, 1, 1), 4), (Ly("b", "deconv2d", 16, 8, 4, 2, 1), 8))):
        arr = (s3r._lib.Layer * 2)()
        for i, (l, n) in enumerate(chain):
            arr[i].desc = s3r._lib.make_desc(l, 2, n)
        assert lib.s3r_chain_workspace_elems(arr, 2) > 0, lib.s3r_last_error()


def test_new_layouts_are_checked(s3r, lib):
    """S3R_LAYOUT_WINO_3D / S3R_LAYOUT_DIFF on layers that cannot read or write them are refused with a message, never run"""
    L, Ly = s3r._lib, s3r.arch_spec.Layer
    conv, dcv = Ly("a", "conv3d", 32, 32, 3, 1, 1), Ly("t", "deconv3d", 32, 32, 4, 2, 1)
    ok = L.make_desc(conv, 2, 7, in_halo=1, in_layout=L.LAYOUT_WINO_3D)
    assert lib.s3r_conv_scratch_elems(C.byref(ok)) > 0, lib.s3r_last_error()
    plain = L.make_desc(conv, 2, 7, in_halo=1)
    assert lib.s3r_conv_scratch_elems(C.byref(plain)) - lib.s3r_conv_scratch_elems(C.byref(ok)) == _align(36 * 2 * 32 * 2 * 2 * 9)
    okd = L.make_desc(dcv, 2, 4, in_halo=1, in_layout=L.LAYOUT_DIFF)
    assert lib.s3r_conv_scratch_elems(C.byref(okd)) >= 0, lib.s3r_last_error()
    for bad in (L.make_desc(conv, 2, 7, in_halo=1, in_layout=L.LAYOUT_DIFF),               # a convolution reads no difference tensors
                L.make_desc(dcv, 2, 4, in_halo=1, in_layout=L.LAYOUT_WINO_3D),             # nor a transposed layer plane sets
                L.make_desc(dcv, 2, 6, in_halo=1, in_layout=L.LAYOUT_DIFF),                # edge % 4 != 0: no Winograd form
                L.make_desc(dcv, 2, 4, in_halo=1, in_layout=L.LAYOUT_DIFF, algo=L.ALGO_DIRECT),
                L.make_desc(conv, 2, 7, in_halo=1, out_halo=1, out_layout=L.LAYOUT_DIFF),  # output edge 7: not the edge of a transposed Winograd layer
                L.make_desc(conv, 2, 8, in_halo=1, out_halo=0, out_layout=L.LAYOUT_DIFF),
                L.make_desc(conv, 2, 7, in_halo=1, out_halo=2, out_layout=L.LAYOUT_WINO_3D),
                L.make_desc(Ly("s", "conv3d", 32, 32, 3, 1, 1, True, "sigmoid"), 2, 8, in_halo=1, out_halo=1, out_layout=L.LAYOUT_WINO_3D)):
        assert lib.s3r_conv_scratch_elems(C.byref(bad)) == -1 and lib.s3r_last_error(), bad
