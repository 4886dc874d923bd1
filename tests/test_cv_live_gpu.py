"""v1 reading the cost volume's S3R_LAYOUT_WINO_DH plane sets (column outside the row group) and leaving out the K tiles that hold only
structural zeros (csrc/s3r_cv_live.h): the output is, bit for bit, the same layer's over the plain halo-padded volume through its own
input transform — in the class-parallel and the semi-fused launch form — and stays so after every plane-set element that only dead
K tiles would read is overwritten with NaN: a dead tile is never fetched."""
import ctypes as C

import pytest
import torch

from tests import _cv_live as CV
from tests._abi_calls import DEV, rc_ok, sync

pytestmark = pytest.mark.gpu

B = 3
# (edge, feature channels, cout).  Edge 16: one tile is a whole depth group, nothing is dead.  Feature channels 16: one 32-channel chunk
# holds both halves (dead when both are); 32: a chunk per half, as in the network.  cout 70: a partial second cout tile
SHAPES = [(n, 16, cout) for n in (16, 20, 28) for cout in (64, 70)] + [(20, 32, 64), (28, 32, 64)]
FORMS = {"class-parallel": 4, "semi-fused": 5}      # the two-axis tile codes (include/s3r.h)


@pytest.fixture(scope="module")
def lib(s3r):
    return s3r.load_library()


def _forward(s3r, lib, layer, params, pk_desc, x, n, what):
    need = lib.s3r_conv_scratch_elems(C.byref(pk_desc))
    assert need >= 0, (what, lib.s3r_last_error())
    npk = C.c_int64(0)
    rc_ok(lib, lib.s3r_conv_packed_elems(C.byref(pk_desc), C.byref(npk)), "packed_elems")
    pk = torch.full((npk.value,), float("nan"), device=DEV)
    rc_ok(lib, lib.s3r_conv_pack_weights(C.byref(pk_desc), params["w"].data_ptr(), pk.data_ptr(), None), "pack_weights")
    y = torch.full((B, layer.cout, n, n, n), float("nan"), device=DEV)
    scr = torch.full((max(need, 1),), float("nan"), device=DEV)
    rc_ok(lib, lib.s3r_conv_forward(C.byref(pk_desc), x.data_ptr(), pk.data_ptr(), params["scale"].data_ptr(), params["shift"].data_ptr(),
                                    y.data_ptr(), scr.data_ptr(), need, None), what)
    sync()
    return y


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "e%d-c%d-cout%d" % s)
def test_v1_on_cost_volume_planes(s3r, lib, shape, form):
    from tests import _ref64 as R
    n, Cc, cout = shape
    tile = FORMS[form]
    layer = s3r.arch_spec.Layer("v1", "conv3d", 2 * Cc, cout, 3, 1, 1)
    params = {k: v.to(DEV).contiguous() for k, v in R.make_params(layer, 7 * n + cout).items()}
    g = torch.Generator().manual_seed(n + Cc)
    fl = torch.randn(B, Cc, n, n, generator=g).to(DEV)
    fr = torch.randn(B, Cc, n, n, generator=g).to(DEV)
    L = s3r._lib

    # the reference: the plain halo-1 volume through the layer's own input transform, the same launch form
    vol = torch.zeros(B, 2 * Cc, n + 2, n + 2, n + 2, device=DEV)
    rc_ok(lib, lib.s3r_cost_volume_forward(fl.data_ptr(), fr.data_ptr(), vol.data_ptr(), B, Cc, n, n, n, 1, None), "cost_volume")
    plain = L.make_desc(layer, B, n, tile=tile, in_halo=1, algo=L.ALGO_WINOGRAD)
    want = _forward(s3r, lib, layer, params, plain, vol, n, "plain input")
    assert torch.isfinite(want).all()

    sg = n // 4
    planes = torch.zeros(36, B, 2 * Cc, sg, n + 2, sg, device=DEV)
    rc_ok(lib, lib.s3r_cost_volume_forward_wino2(fl.data_ptr(), fr.data_ptr(), planes.data_ptr(), B, Cc, n, n, n, None), "cost_volume_wino2")
    pre = L.make_desc(layer, B, n, tile=tile, in_halo=1, algo=L.ALGO_WINOGRAD, in_layout=L.LAYOUT_WINO_DH)
    got = _forward(s3r, lib, layer, params, pre, planes, n, "plane sets")
    assert torch.equal(got.view(torch.int32), want.view(torch.int32)), "the plane-set input changes the bits"

    # NaN wherever only dead K tiles read: still the same bits
    only_dead = torch.from_numpy(CV.dead_only_elements(n, B, Cc)).to(DEV)      # [B, 2C, sd, wp, sh]
    count = int(only_dead.sum())
    print(f"edge {n}, {2 * Cc} channels: {count} of {only_dead.numel()} elements per plane set are read by dead K tiles only")
    if n == 16:
        assert count == 0
    if n == 28:
        assert count > 0
    assert not bool((planes != 0)[:, only_dead].any()), "an element only dead tiles read is not a structural zero"
    planes[:, only_dead] = float("nan")
    got = _forward(s3r, lib, layer, params, pre, planes, n, "poisoned plane sets")
    assert torch.equal(got.view(torch.int32), want.view(torch.int32)), "a dead K tile was fetched"
