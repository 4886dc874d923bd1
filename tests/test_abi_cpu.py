"""The C-ABI library: loads, exports every symbol include/s3r.h declares, and its host-only entry
points (geometry, packing sizes, argument validation) behave — no GPU compute is called here."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib(s3r):
    import __graft_entry__ as g
    if not os.path.exists(s3r.LIB_PATH):
        g.build()
    return s3r.load_library()


def test_header_symbols_all_exported(s3r, lib):
    header = open(os.path.join(ROOT, "include", "s3r.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    declared = set(re.findall(r"\b(s3r_[a-z0-9_]+)\s*\(", header))
    assert len(declared) >= 20
    bound = set(s3r._lib.SIGNATURES)
    assert declared == bound, declared ^ bound
    for name in declared:
        assert hasattr(lib, name), name
    assert lib.s3r_abi_version() == 8


def test_struct_layouts_match_header(s3r):
    assert C.sizeof(s3r._lib.ConvDesc) == 22 * 4     # ABI 7: + algo; ABI 8: + dilation, out_pad, act_param
    assert C.sizeof(s3r._lib.Layer) == 22 * 4 + 3 * 8
    assert C.sizeof(s3r._lib.ProfRecord) == 48      # 4 x 4 bytes + 3 doubles + algo + launch_form
    header = open(os.path.join(ROOT, "include", "s3r.h")).read()
    body = header[header.index("typedef struct s3r_conv_desc {"):header.index("} s3r_conv_desc;")]
    fields = re.findall(r"(?:int32_t|float)\s+([a-z_, ]+);", re.sub(r"/\*.*?\*/", "", body, flags=re.S))
    names = [n.strip() for f in fields for n in f.split(",")]
    assert names == [n for n, _ in s3r._lib.ConvDesc._fields_]


def _desc(s3r, layer, batch, n):
    return s3r._lib.make_desc(layer, batch, n)


def test_out_size_and_packed_elems(s3r, lib):
    spec = s3r.arch_spec
    for stage in ("encoder", "decoder", "point_head"):
        for l, n, m in spec.stage_table(stage):
            d = _desc(s3r, l, 2, n)
            assert lib.s3r_conv_out_size(C.byref(d)) == m
            e = C.c_int64(0)
            assert lib.s3r_conv_packed_elems(C.byref(d), C.byref(e)) == 0, lib.s3r_last_error()
            nd = spec.ndim(l)
            if l.name == "e1":
                assert e.value == 27 * 32
            elif l.name == "d4":
                assert e.value == l.cin
            elif l.op == "linear":
                assert e.value == l.cin * l.cout
            else:
                pad = (l.cout + 127) // 128 * 128
                # a 3 x 3 [x 3] stride-1 pad-1 convolution packs its six Winograd F(4,3)-along-H class slabs behind the direct one
                wino = 6 * 3 ** (nd - 1) * l.cin * pad if (l.op != "deconv3d" and l.k == 3 and l.s == 1 and l.p == 1) else 0
                if l.op == "deconv3d":            # ... and a transposed convolution its 72 F(2,2)^2 (parity class, class) slabs of 2 taps
                    wino = 72 * 2 * l.cin * pad
                    if n in (8, 16, 32):          # ... + the 8 x 27 slabs of the three-axis form (64-cout tiles)
                        wino += 8 * 27 * l.cin * ((l.cout + 63) // 64 * 64)
                if l.op == "conv3d" and l.s == 1 and l.k == 3 and l.p == 1:      # ... a 3D one also the 36 two-axis F(4,3)^2 slabs
                    wino += 36 * 3 * l.cin * pad
                if l.op == "conv3d" and l.s == 1 and l.k == 4 and l.p == 0:      # (v6: 25 F(2,4)^2 slabs of 4 taps)
                    wino += 25 * 4 * l.cin * pad
                if l.op == "conv2d" and l.s == 1 and l.k == 3 and l.p == 1:      # a 2D one the 36 (H, W) slabs of a single tap
                    wino += 36 * l.cin * pad
                assert e.value == l.k ** nd * l.cin * pad + wino


def test_workspace_query(s3r, lib, monkeypatch):
    if os.environ.get("S3R_WINO") not in (None, "1"):
        pytest.skip("the library's own kernel policy is under test (S3R_WINO is read once, at load)")
    spec = s3r.arch_spec
    rows = spec.stage_table("encoder")
    arr = (s3r._lib.Layer * len(rows))()
    for i, (l, n, m) in enumerate(rows):
        arr[i].desc = _desc(s3r, l, 4, n)
    need = lib.s3r_chain_workspace_elems(arr, len(rows))
    # every intermediate has its own region, stored with the zero halo its consumer's gather reads
    # (3x3 pad-1 consumers: halo 1; the 1x1 e8: none), each region rounded up to 256 floats — but the stem's, which
    # holds the six F(4,3) plane sets its consumer e2 reads (the stem writes them itself: 6 x 4 x 32 x 28 groups x 114)
    want = -(-(6 * 4 * 32 * (112 // 4) * 114) // 256) * 256
    for i, (l, n, m) in enumerate(rows[:-1]):
        if i == 0:
            continue
        if l.name == "e6":      # ... and e6's, which holds the 36 two-axis plane sets of e7 (written by e6's finish kernel):
            want += 36 * l.cout * (-(-(4 * 7 * 7) // 64) * 64)      # positions of the 4 images flat, rounded up to a GEMM tile
            continue
        halo = rows[i + 1][0].p
        want += -(-(4 * l.cout * (m + 2 * halo) ** 2) // 256) * 256
    # ... plus ONE split-K scratch region sized for the hungriest layer
    scratch = 0
    for i, (l, n, m) in enumerate(rows):
        d = _desc(s3r, l, 4, n)
        d.in_halo = l.p
        if i == 1:
            d.in_layout = s3r._lib.LAYOUT_WINO_H                  # (e2's planes come from the stem: not in its scratch)
        if l.name == "e7":
            d.in_layout = s3r._lib.LAYOUT_WINO_HW                 # (e7's from e6)
        if l.name == "e6":
            d.out_layout = s3r._lib.LAYOUT_WINO_HW
        scratch = max(scratch, lib.s3r_conv_scratch_elems(C.byref(d)))
    assert need == want + -(-scratch // 256) * 256
    # a chain whose first layer gathers with padding pads an unpadded input itself: one more region
    sub = (s3r._lib.Layer * 2)()
    sub[0].desc, sub[1].desc = _desc(s3r, rows[1][0], 4, rows[1][1]), _desc(s3r, rows[2][0], 4, rows[2][1])
    need2 = lib.s3r_chain_workspace_elems(sub, 2)
    # (e2, e3 do not split K; e2's Winograd scratch is the chain's: its F(4,3) input planes — 6 x 4 x 32 x 28 groups x 114
    # columns — followed by the class-parallel slabs of the launch form the library plans for 4 images)
    d2 = _desc(s3r, rows[1][0], 4, rows[1][1])
    d2.in_halo = 1
    planes = -(-(6 * 4 * 32 * (112 // 4) * 114) // 256) * 256
    assert lib.s3r_conv_scratch_elems(C.byref(d2)) >= planes
    wino = -(-lib.s3r_conv_scratch_elems(C.byref(d2)) // 256) * 256
    assert need2 == -(-(4 * 32 * 114 * 114) // 256) * 256 + -(-(4 * 64 * 114 * 114) // 256) * 256 + wino
    sub[0].desc.in_halo = 1                       # caller hands a padded input: no pad region
    assert lib.s3r_chain_workspace_elems(sub, 2) == -(-(4 * 64 * 114 * 114) // 256) * 256 + wino


def test_split_k_choice_is_batch_invariant(s3r, lib):
    """Split-K changes a sample's summation order, so the library must pick it from per-sample geometry
    only: the scratch it asks for scales exactly with the batch (never switches on or off with it)."""
    spec = s3r.arch_spec
    split = {}
    for l, n, m in spec.stage_table("decoder"):
        per_batch = []
        for b in (1, 2, 32, 64):
            d = _desc(s3r, l, b, n)
            d.in_halo = 1
            d.tile = 3                                   # fixed 64x64 tile: scratch = cls*ks*cout*ceil64(b*S)
            per_batch.append(lib.s3r_conv_scratch_elems(C.byref(d)))
        assert all((x > 0) == (per_batch[0] > 0) for x in per_batch), (l.name, per_batch)
        split[l.name] = per_batch[0] > 0
    assert split["v6"] and not split["v1"] and not split["d3"]


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("null", ["scale", "shift", "both"])
def test_stem_refuses_a_null_scale_or_shift(s3r, lib, dtype, null):
    """include/s3r.h makes scale and shift optional (NULL = 1 / 0) and every kernel guards its read — except the three stem kernels,
    which index both vectors unconditionally: s3r_conv_forward (fp32 and bf16 stem) and s3r_chain_forward (a chain of the stem alone,
    and stem -> e2, where the stem writes e2's Winograd planes: a third kernel) refuse a NULL host-side with S3R_ERR_INVALID before
    anything is enqueued.  Argument validation only: the pointers are never dereferenced"""
    spec = s3r.arch_spec
    (e1, n1, _), (e2, n2, _) = spec.stage_table("encoder")[:2]
    ok = C.c_void_p(64)
    sc, sh = (None if null in ("scale", "both") else ok), (None if null in ("shift", "both") else ok)
    d = s3r._lib.make_desc(e1, 2, n1, dtype=s3r._lib.DTYPE[dtype])
    assert lib.s3r_conv_forward(C.byref(d), ok, ok, sc, sh, ok, None, 0, None) == -1
    assert b"stem needs scale and shift" in lib.s3r_last_error(), lib.s3r_last_error()
    chains = [[(e1, n1)]] + ([[(e1, n1), (e2, n2)]] if dtype == "fp32" else [])
    for rows in chains:
        arr = (s3r._lib.Layer * len(rows))()
        for i, (l, n) in enumerate(rows):
            arr[i].desc = s3r._lib.make_desc(l, 2, n, tag=i, dtype=s3r._lib.DTYPE[dtype])
            arr[i].packed_w, arr[i].scale, arr[i].shift = ok.value, ok.value, ok.value
        arr[0].scale, arr[0].shift = (sc.value if sc else None), (sh.value if sh else None)
        assert lib.s3r_chain_workspace_elems(arr, len(rows)) >= 0, lib.s3r_last_error()
        # (ws_fresh = 0: no zero fill is enqueued in front of the check)
        assert lib.s3r_chain_forward(arr, len(rows), ok, ok, ok, 1 << 40, 0, None) == -1, (len(rows), lib.s3r_last_error())
        assert b"stem needs" in lib.s3r_last_error(), lib.s3r_last_error()


def test_halo_contract(s3r, lib):
    """The MFMA conv kernels read zero padding from memory: single-layer calls must state a halo."""
    spec = s3r.arch_spec
    l, n, _ = spec.stage_table("decoder")[0]                   # v1: conv3d k3 p1
    d = _desc(s3r, l, 1, n)
    one = C.c_void_p(16)                                       # non-null dummies: validation fails first
    assert lib.s3r_conv_forward(C.byref(d), one, one, None, None, one, None, 0, None) == -1
    assert b"halo" in lib.s3r_last_error()
    d.in_halo = 9
    e = C.c_int64(0)
    assert lib.s3r_conv_packed_elems(C.byref(d), C.byref(e)) == -1


def test_invalid_arguments_are_reported_not_crashed(s3r, lib):
    spec = s3r.arch_spec
    e = C.c_int64(0)
    bad = _desc(s3r, spec.Layer("x", "conv2d", 5, 8, 3, 1, 1), 1, 8)       # cin % 16 != 0: fp32 stages it (ABI 8), bf16 cannot
    # (cin <= 8: staged UNFOLDED — K rows = cin k^2 = 45 -> 48 — whatever the batch: the weights are packed once for every batch)
    assert lib.s3r_conv_packed_elems(C.byref(bad), C.byref(e)) == 0 and e.value == 48 * 128
    bad.batch = 100000
    assert lib.s3r_conv_packed_elems(C.byref(bad), C.byref(e)) == 0 and e.value == 48 * 128
    assert lib.s3r_conv_scratch_elems(C.byref(bad)) == (2 ** 28 // (48 * 64)) * 48 * 64      # sub-batches of <= 2^28 floats (1 GiB) per pass
    bad.batch = 1
    bad.dtype = 1
    assert lib.s3r_conv_packed_elems(C.byref(bad), C.byref(e)) == -1
    assert b"cin" in lib.s3r_last_error()
    bad = _desc(s3r, spec.Layer("x", "deconv3d", 16, 8, 3, 1, 3), 1, 8)    # a transposed layer that crops more than its kernel reaches
    assert lib.s3r_conv_packed_elems(C.byref(bad), C.byref(e)) == -1
    bad = _desc(s3r, spec.Layer("x", "conv3d", 16, 8, 3, 1, 1), 0, 8)      # empty batch at the ABI
    assert lib.s3r_conv_packed_elems(C.byref(bad), C.byref(e)) == -1
    huge = _desc(s3r, spec.Layer("x", "conv3d", 64, 64, 3, 1, 1), 4096, 28)
    assert lib.s3r_conv_packed_elems(C.byref(huge), C.byref(e)) == -1
    assert b"split the batch" in lib.s3r_last_error()
    assert lib.s3r_cost_volume_forward(None, None, None, 1, 1, 1, 1, 1, 0, None) == -1
    assert lib.s3r_chamfer_forward(None, None, None, None, None, None, 1, 1, 1, None) == -1
    assert lib.s3r_chain_forward(None, 0, None, None, None, 0, 0, None) == -1
    assert lib.s3r_disparity_wta(None, None, None, None, 1, 1, 1, 1, 1, None) == -1
    one = C.c_void_p(16)                                       # non-null dummies: validation fails first
    assert lib.s3r_disparity_wta(one, one, one, one, 1, 64, 2, 200, 4, None) == -1
    assert b"64 KiB" in lib.s3r_last_error()
    assert lib.s3r_disparity_wta(one, one, one, one, 1, 8, 2, 8, 0, None) == -1
    assert lib.s3r_disparity_epe(None, None, None, None, 1, 1, None) == -1
    assert lib.s3r_disparity_epe(one, one, one, one, 0, 16, None) == -1


def test_out_size_validates_instead_of_dividing_by_zero(s3r, lib):
    """s3r_conv_out_size on a descriptor with stride 0 used to die with SIGFPE: every entry point
    returns a negative status instead."""
    spec = s3r.arch_spec
    d = _desc(s3r, spec.Layer("x", "conv2d", 16, 8, 3, 1, 1), 1, 8)
    assert lib.s3r_conv_out_size(C.byref(d)) == 8
    for field, value in (("stride", 0), ("k", 0), ("in_size", 0), ("pad", -1), ("op", 7)):
        bad = _desc(s3r, spec.Layer("x", "conv2d", 16, 8, 3, 1, 1), 1, 8)
        setattr(bad, field, value)
        assert lib.s3r_conv_out_size(C.byref(bad)) == -1, field
    assert lib.s3r_conv_out_size(None) == -1
    tiny = _desc(s3r, spec.Layer("x", "conv2d", 16, 8, 5, 1, 0), 1, 3)        # kernel larger than the input
    assert lib.s3r_conv_out_size(C.byref(tiny)) == -1


def test_encoder_entry_takes_a_left_right_pair(s3r, lib):
    """ABI v3: s3r_encoder_forward(layers, n, images_left, images_right, ...) — argument validation only (no GPU)."""
    spec = s3r.arch_spec
    rows = spec.stage_table("encoder")
    arr = (s3r._lib.Layer * len(rows))()
    for i, (l, n, m) in enumerate(rows):
        arr[i].desc = _desc(s3r, l, 3, n)                     # odd image count with two tensors: refused
    one = C.c_void_p(16)
    assert lib.s3r_encoder_forward(arr, len(rows), one, one, one, one, 1 << 40, 0, None) == -1
    assert b"even image count" in lib.s3r_last_error()
    dec = spec.stage_table("decoder")
    arr2 = (s3r._lib.Layer * 1)()
    arr2[0].desc = _desc(s3r, dec[0][0], 2, dec[0][1])
    assert lib.s3r_encoder_forward(arr2, 1, one, one, one, one, 1 << 40, 0, None) == -1     # not an encoder chain


def test_every_entry_that_reaches_a_stem_checks_render_alignment(s3r, lib):
    """The stems read render rows with 16-byte loads from base + row * width.  The check lives in the chain implementation, so
    s3r_chain_forward over a tower prefix (what Encoder.forward(upto=...) calls) refuses an unaligned pointer exactly like
    s3r_encoder_forward[_u8] — argument validation only, nothing is launched."""
    spec = s3r.arch_spec
    rows = spec.stage_table("encoder")[:2]
    arr = (s3r._lib.Layer * len(rows))()
    for i, (l, n, m) in enumerate(rows):
        arr[i].desc = _desc(s3r, l, 2, n)
    ok, odd = C.c_void_p(64), C.c_void_p(68)
    for fn, args in ((lib.s3r_chain_forward, (odd, ok)), (lib.s3r_encoder_forward, (odd, ok, ok)), (lib.s3r_encoder_forward, (ok, odd, ok)),
                     (lib.s3r_encoder_forward_u8, (ok, C.c_void_p(65), ok))):
        assert fn(arr, len(rows), *args, ok, 1 << 40, 0, None) == -1
        assert b"16-byte aligned" in lib.s3r_last_error(), lib.s3r_last_error()


def _bf16_refusal_calls(s3r, lib):
    """(id, call(ptrs) -> rc, names of the bf16 pointers, names of the fp32 pointers, the message of the LATER host check every call
    here is built to run into — a workspace of 0 floats, a shape the entry refuses — so that nothing is ever launched)"""
    spec, Ld = s3r.arch_spec, s3r._lib
    BF = Ld.DTYPE["bf16"]
    net = dict((l.name, (l, n)) for stage in ("encoder", "decoder") for l, n, _ in spec.stage_table(stage))
    # one layer, forced split-K, scratch_elems = 0: S3R_ERR_WORKSPACE after every alignment check
    conv = Ld.make_desc(spec.Layer("t", "conv3d", 64, 40, 4, 1, 0), 2, 7, ksplit=2, dtype=BF)
    head = Ld.make_desc(spec.Layer("t", "conv3d", 64, 40, 4, 1, 0), 2, 7, ksplit=2, dtype=0)

    def layers(rows, batch, dtype):
        arr = (Ld.Layer * len(rows))()
        for i, (l, n, _) in enumerate(rows):
            arr[i].desc = Ld.make_desc(l, batch, n, dtype=dtype)
        return arr, len(rows)

    enc, dec = layers(spec.stage_table("encoder"), 2, BF), layers(spec.stage_table("decoder"), 1, BF)
    two = layers(spec.stage_table("decoder")[:2], 1, BF)
    return [
        ("conv_forward-bf16", lambda p, d=conv: lib.s3r_conv_forward(C.byref(d), p["x"], p["packed"], p["scale"], p["shift"], p["y"],
                                                                     p["scratch"], 0, None),
         ("x", "y", "scratch"), ("packed", "scale", "shift"), b"needs"),
        ("conv_forward-fp32", lambda p, d=head: lib.s3r_conv_forward(C.byref(d), p["x"], p["packed"], p["scale"], p["shift"], p["y"],
                                                                     p["scratch"], 0, None),
         (), ("x", "y", "scratch", "packed", "scale", "shift"), b"needs"),
        ("chain_forward", lambda p: lib.s3r_chain_forward(*two, p["x"], p["y"], p["ws"], 0, 1, None), ("x", "y", "ws"), (), b"workspace"),
        ("encoder_forward", lambda p: lib.s3r_encoder_forward(*enc, p["left"], p["right"], p["features"], p["ws"], 0, 1, None),
         ("features", "ws"), (), b"workspace"),
        ("encoder_forward_u8", lambda p: lib.s3r_encoder_forward_u8(*enc, p["left"], p["right"], p["features"], p["ws"], 0, 1, None),
         ("features", "ws"), (), b"workspace"),
        # (the occupancy comes out of the fused head: fp32)
        ("decoder_forward", lambda p: lib.s3r_decoder_forward(*dec, p["volume"], p["occupancy"], p["ws"], 0, 1, None),
         ("volume", "ws"), ("occupancy",), b"workspace"),
        ("cost_volume_forward_bf16", lambda p: lib.s3r_cost_volume_forward_bf16(p["left"], p["right"], p["volume"], 1, 4, 4, 4, 4, 0, None),
         ("left", "right", "volume"), (), b"channels % 8"),
        ("channels_last_to_f32", lambda p: lib.s3r_channels_last_to_f32(p["x"], p["y"], 70000, 8, 4, None), ("x",), ("y",), b"too large"),
        ("disparity_soft-bf16", lambda p: lib.s3r_disparity_soft(p["left"], p["right"], BF, p["disp_l"], p["disp_r"], p["conf_l"], p["conf_r"],
                                                                 1, 64, 4, 4096, 64, 1.0, 4, 4096, 1.0, None),
         ("left", "right"), ("disp_l", "disp_r", "conf_l", "conf_r"), b"64 KiB"),
        ("disparity_soft-fp32", lambda p: lib.s3r_disparity_soft(p["left"], p["right"], 0, p["disp_l"], p["disp_r"], p["conf_l"], p["conf_r"],
                                                                 1, 64, 4, 4096, 64, 1.0, 4, 4096, 1.0, None),
         (), ("left", "right", "disp_l", "disp_r", "conf_l", "conf_r"), b"64 KiB"),
    ]


ALL_POINTERS = ("x", "y", "scratch", "packed", "scale", "shift", "ws", "left", "right", "features", "volume", "occupancy", "disp_l",
                "disp_r", "conf_l", "conf_r")


def test_every_entry_that_takes_a_bf16_tensor_checks_its_alignment(s3r, lib):
    """include/s3r.h, Conventions: a bf16 tensor (and the scratch / workspace of S3R_BF16 layers, which holds bf16 intermediates)
    must be 16-byte aligned; fp32 / int32 tensors need 4 bytes.  Fake pointers, argument validation only: at addresses = 2, 4, 8
    (mod 16) every bf16 pointer is refused with S3R_ERR_INVALID and "16-byte aligned" before the later host check the call is built
    to fail (so nothing is launched, on any machine); at = 0 the call gets past the alignment check and meets that later one; an
    fp32 pointer of the same entries at the same addresses is never refused for its alignment"""
    base = 1 << 20
    for name, call, bf16_ptrs, f32_ptrs, later in _bf16_refusal_calls(s3r, lib):
        aligned = {k: C.c_void_p(base + 4096 * i) for i, k in enumerate(ALL_POINTERS)}
        rc = call(aligned)
        assert rc < 0 and later in lib.s3r_last_error() and b"16-byte aligned" not in lib.s3r_last_error(), (name, rc, lib.s3r_last_error())
        for off in (2, 4, 8):
            for k in bf16_ptrs:
                p = dict(aligned)
                p[k] = C.c_void_p(aligned[k].value + off)
                assert call(p) == -1, (name, k, off)
                assert b"16-byte aligned" in lib.s3r_last_error(), (name, k, off, lib.s3r_last_error())
            for k in f32_ptrs:
                if off == 2:
                    continue                                     # (not an address an fp32 tensor can have)
                p = dict(aligned)
                p[k] = C.c_void_p(aligned[k].value + off)
                rc = call(p)
                assert rc < 0 and later in lib.s3r_last_error() and b"16-byte aligned" not in lib.s3r_last_error(), \
                    (name, k, off, rc, lib.s3r_last_error())


def test_alignment_exceptions_are_the_header_s_sentences(s3r):
    """the (entry, argument) pairs whose fp32 / int32 / 8-bit pointer needs more than its element size: ONE table
    (tests/_alignment_cases.py), every row quoting the sentence of include/s3r.h that documents it"""
    from tests import _alignment_cases as AC
    header = " ".join(re.sub(r"[/*]+", " ", open(os.path.join(ROOT, "include", "s3r.h")).read()).split())
    assert AC.EXCEPTIONS
    for entry, arg, name, nbytes, sentence, reason in AC.EXCEPTIONS:
        assert " ".join(sentence.split()) in header, (entry, arg, sentence)
        assert reason and name and nbytes == 16
        assert entry in s3r._lib.SIGNATURES, entry


def test_render_pointers_are_refused_at_every_entry_that_reaches_a_stem(s3r, lib):
    """the exception list's rows, asserted: s3r_conv_forward on the stem descriptor (both precisions) refuses a render pointer that
    is 4- or 8-byte aligned, like the chain and encoder entries above; its fp32 arguments are not refused for alignment"""
    spec = s3r.arch_spec
    l, n, _ = spec.stage_table("encoder")[0]
    for dtype in (0, 1):
        d = s3r._lib.make_desc(l, 2, n, dtype=dtype)
        ok = C.c_void_p(1 << 20)
        for off in (4, 8) + ((2,) if dtype else ()):
            assert lib.s3r_conv_forward(C.byref(d), C.c_void_p(ok.value + off), ok, ok, ok, ok, None, 0, None) == -1
            assert b"render tensors must be 16-byte aligned" in lib.s3r_last_error()
        if dtype:
            assert lib.s3r_conv_forward(C.byref(d), ok, ok, ok, ok, C.c_void_p(ok.value + 8), None, 0, None) == -1
            assert b"16-byte aligned" in lib.s3r_last_error() and b"render" not in lib.s3r_last_error()
        # (scale = NULL: "stem needs scale and shift" is the later host check)
        assert lib.s3r_conv_forward(C.byref(d), ok, C.c_void_p(ok.value + 4), None, C.c_void_p(ok.value + 4), ok, None, 0, None) == -1
        assert b"16-byte aligned" not in lib.s3r_last_error() and b"scale and shift" in lib.s3r_last_error()


def test_missing_library_fails_loudly(s3r, monkeypatch, tmp_path):
    monkeypatch.setattr(s3r._lib, "_lib", None)
    monkeypatch.setattr(s3r._lib, "LIB_PATH", str(tmp_path / "nope.so"))
    with pytest.raises(s3r.S3RError, match="no CPU fallback"):
        s3r._lib.load()


def test_algo_field_selects_the_kernel_and_scratch_is_never_a_selector(s3r, lib):
    """ABI 7: which convolution algorithm runs is the descriptor's `algo` — AUTO resolves from per-sample geometry only — and
    a scratch buffer smaller than the resolved algorithm needs is S3R_ERR_WORKSPACE, not a silent switch to the other kernel
    (whose bits differ)."""
    if os.environ.get("S3R_WINO") not in (None, "1"):
        pytest.skip("the library's own kernel policy is under test")
    spec = s3r.arch_spec
    enc = {l.name: (l, n) for l, n, _ in spec.stage_table("encoder")}
    dec = {l.name: (l, n) for l, n, _ in spec.stage_table("decoder")}
    L = s3r._lib

    def scratch(name, algo, batch=4, **kw):
        l, n = (enc if name in enc else dec)[name]
        d = L.make_desc(l, batch, n, in_halo=1, algo=algo, **kw)
        return lib.s3r_conv_scratch_elems(C.byref(d)), d

    planes_e2 = 6 * 4 * 32 * 28 * 114
    auto, d_auto = scratch("e2", L.ALGO_AUTO)
    assert auto >= planes_e2                                   # the policy takes e2 (edge 112 = 4 x 28) on the Winograd kernel
    assert scratch("e2", L.ALGO_WINOGRAD)[0] == auto
    assert scratch("e2", L.ALGO_DIRECT)[0] == 0                # the direct kernel does not split e2's K
    assert scratch("e2", L.ALGO_AUTO, tile=3)[0] == 0          # a direct-kernel tile override is a direct-kernel request
    assert scratch("v5", L.ALGO_DIRECT)[0] > 0                 # (the direct kernel splits v5's K)
    assert scratch("v5", L.ALGO_AUTO)[0] == scratch("v5", L.ALGO_WINOGRAD)[0] > 0
    # v5 (edge 7) resolves to the TWO-AXIS form: 36 plane sets of 2 x 2 groups x 9 columns per channel, then 36 class slabs
    v5_two = -(-(36 * 4 * 256 * 2 * 2 * 9) // 256) * 256 + 36 * 256 * -(-(4 * 2 * 2 * 7) // 64) * 64
    assert scratch("v5", L.ALGO_AUTO)[0] == v5_two == scratch("v5", L.ALGO_WINOGRAD, tile=3)[0]
    assert scratch("v5", L.ALGO_WINOGRAD, tile=0)[0] != v5_two                 # the one-axis kernel stays selectable
    l6, n6 = dec["v6"]
    d6 = L.make_desc(l6, 4, n6, in_halo=0, algo=L.ALGO_AUTO)                   # v6: k4 p0 — F(2,4) x F(2,4), 25 classes
    assert lib.s3r_conv_scratch_elems(C.byref(d6)) == -(-(25 * 4 * 256 * 2 * 2 * 7) // 256) * 256 + 25 * 512 * 64
    d6.algo = L.ALGO_WINOGRAD; d6.tile = 0
    assert lib.s3r_conv_scratch_elems(C.byref(d6)) == -1                       # no one-axis form for a 4-tap kernel
    # AUTO never depends on the batch: the same choice at 1 and at 64 samples (the scratch follows the batch, the kernel not)
    for name in ("e2", "e7", "v1", "v3", "v5", "d1", "d3"):      # (v3, v5: the two-axis form, v1 and the rest the one-axis one)
        assert all(scratch(name, L.ALGO_AUTO, b)[0] > 0 for b in (1, 2, 64)), name
    assert scratch("e3", L.ALGO_WINOGRAD)[0] == -1             # stride 2: no Winograd form
    assert b"WINOGRAD" in lib.s3r_last_error()
    assert scratch("e2", 7)[0] == -1 and b"algo" in lib.s3r_last_error()
    assert scratch("e2", L.ALGO_WINOGRAD, ksplit=2)[0] == -1
    # every launch form of the Winograd kernel can be forced (tile = form code), and only the class-parallel ones add slabs
    serial = scratch("e2", L.ALGO_WINOGRAD, tile=0)[0]
    assert serial == -(-planes_e2 // 256) * 256
    assert scratch("e2", L.ALGO_WINOGRAD, tile=1)[0] == serial + 6 * 64 * 12544      # 4 images x 28 groups x 112 columns
    # too little scratch: an error, before anything is launched (dummy pointers)
    one = C.c_void_p(1 << 20)
    assert lib.s3r_conv_forward(C.byref(d_auto), one, one, None, None, one, one, auto - 1, None) == -3
    assert b"scratch" in lib.s3r_last_error()
    assert lib.s3r_conv_forward(C.byref(d_auto), one, one, None, None, one, None, 0, None) == -3
    dv6 = L.make_desc(dec["v6"][0], 4, dec["v6"][1], algo=L.ALGO_DIRECT)
    need = lib.s3r_conv_scratch_elems(C.byref(dv6))
    assert need > 0                                            # the direct kernel splits v6's K
    assert lib.s3r_conv_forward(C.byref(dv6), one, one, None, None, one, None, 0, None) == -3      # (ABI 6 ran it unsplit)
    dd = L.make_desc(dec["d2"][0], 4, dec["d2"][1], in_halo=1)
    assert lib.s3r_conv_forward(C.byref(dd), one, one, None, None, one, one, 16, None) == -3


def test_policy_override_is_read_once_at_load(s3r):
    """S3R_WINO is a PROCESS-level override of what AUTO resolves to, read when the library is loaded."""
    import subprocess
    import sys
    code = (
        "import os, sys, ctypes as C\n"
        "sys.path.insert(0, %r)\n"
        "import s3r\n"
        "lib = s3r.load_library(); spec = s3r.arch_spec\n"
        "l, n, _ = spec.stage_table('encoder')[1]\n"
        "d = s3r._lib.make_desc(l, 4, n, in_halo=1)\n"
        "a = lib.s3r_conv_scratch_elems(C.byref(d))\n"
        "os.environ['S3R_WINO'] = '1'\n"
        "b = lib.s3r_conv_scratch_elems(C.byref(d))\n"
        "d.algo = 2\n"
        "print('RES', a, b, lib.s3r_conv_scratch_elems(C.byref(d)))\n" % ROOT)
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=dict(os.environ, S3R_WINO="0"), cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    a, b, c = [int(v) for v in r.stdout.split("RES")[1].split()]
    assert a == 0 and b == 0 and c > 0          # AUTO -> direct under S3R_WINO=0, also after the variable changed; WINOGRAD still runs


def test_two_axis_forms_know_their_lds_limits(s3r, lib):
    """The finish kernels of the two-axis forms stage whole padded planes (2D) / four padded slices (3D, semi-fused form) in
    64 KiB of LDS: a layer too large for that has no such form — forcing it is S3R_ERR_INVALID at the scratch query already,
    AUTO resolves to another algorithm, and a forced two-axis call on a large 3D layer plans its class-parallel form."""
    L = s3r._lib
    Layer = s3r.arch_spec.Layer
    big2d = L.make_desc(Layer("b2", "conv2d", 32, 32), 1, 128, in_halo=1, algo=L.ALGO_WINOGRAD, tile=3)
    assert lib.s3r_conv_scratch_elems(C.byref(big2d)) == -1
    big2d.tile = -1                                                  # the one-axis form remains
    assert lib.s3r_conv_scratch_elems(C.byref(big2d)) > 0
    ok2d = L.make_desc(Layer("o2", "conv2d", 32, 32), 1, 124, in_halo=1, algo=L.ALGO_WINOGRAD, tile=3)
    assert lib.s3r_conv_scratch_elems(C.byref(ok2d)) > 0
    big3d = L.make_desc(Layer("b3", "conv3d", 32, 32), 1, 64, in_halo=1, algo=L.ALGO_WINOGRAD, tile=5)
    assert lib.s3r_conv_scratch_elems(C.byref(big3d)) == -1
    big3d.tile = 3                                                   # planned: class-parallel (36 slabs), not semi-fused (24)
    n = 16 * 16 * 64
    assert lib.s3r_conv_scratch_elems(C.byref(big3d)) == -(-(36 * 32 * 16 * 16 * 66) // 256) * 256 + 36 * 32 * n


def test_wino_hw_layout_rules(s3r, lib):
    """S3R_LAYOUT_WINO_HW (the two-axis 2D kernel's plane sets, flat positions): accepted as the input of a Conv2d k3 s1 p1 over
    an edge % 4 == 0 and as the output of a two-axis Conv2d in front of one; the descriptor must resolve to the two-axis
    algorithm (never the direct kernel, never the one-axis form), and the consumer's scratch shrinks by the planes it no longer
    makes itself."""
    L = s3r._lib
    enc = {l.name: (l, n) for l, n, _ in s3r.arch_spec.trace(s3r.arch_spec.ENCODER, s3r.arch_spec.IMG_HW)}
    e6, n6 = enc["e6"]
    e7, n7 = enc["e7"]
    plain = L.make_desc(e7, 4, n7, in_halo=1)
    pre = L.make_desc(e7, 4, n7, in_halo=1, in_layout=L.LAYOUT_WINO_HW)
    assert lib.s3r_conv_wino_input_layout(C.byref(plain)) == L.LAYOUT_WINO_HW
    planes = 36 * e7.cin * (-(-(4 * 7 * 7) // 64) * 64)
    assert lib.s3r_conv_wino_input_elems(C.byref(plain)) == planes
    assert lib.s3r_conv_scratch_elems(C.byref(plain)) - lib.s3r_conv_scratch_elems(C.byref(pre)) == -(-planes // 256) * 256
    pre.algo = L.ALGO_DIRECT                                         # the direct kernel cannot read plane sets
    assert lib.s3r_conv_scratch_elems(C.byref(pre)) == -1
    pre.algo, pre.tile = L.ALGO_WINOGRAD, 0                          # ... nor can the one-axis form
    assert lib.s3r_conv_scratch_elems(C.byref(pre)) == -1
    out = L.make_desc(e6, 4, n6, in_halo=1)
    out.out_layout = L.LAYOUT_WINO_HW
    assert lib.s3r_conv_scratch_elems(C.byref(out)) > 0
    out.algo = L.ALGO_DIRECT
    assert lib.s3r_conv_scratch_elems(C.byref(out)) == -1
    e4, n4 = enc["e4"]                                               # edge 56: AUTO alone picks the one-axis form there, but the
    big = L.make_desc(e4, 4, n4, in_halo=1)                          # layout is a request for the two-axis algorithm, which the
    big.out_layout = L.LAYOUT_WINO_HW                                # layer has (the chain never plans this hand-off itself)
    assert lib.s3r_conv_scratch_elems(C.byref(big)) > 0
    v5 = [l for l in s3r.arch_spec.DECODER if l.name == "v5"][0]     # a 3D layer has no such layout at all
    d3 = L.make_desc(v5, 2, 7, in_halo=1)
    d3.out_layout = L.LAYOUT_WINO_HW
    assert lib.s3r_conv_scratch_elems(C.byref(d3)) == -1


def test_winograd_switch_asks_the_library_which_layers_have_the_form(s3r, lib):
    """`_HipChain(winograd=True)` runs the Winograd kernel wherever the layer has one — and the DIRECT kernel elsewhere, instead
    of handing the library a descriptor it must refuse (the Python mirror of the rules knew k / s / p / cin only;
    the library also wants edge >= 4, a transposed layer's edge % 4 == 0 and no sigmoid)."""
    L = s3r._lib
    Layer = s3r.arch_spec.Layer
    cases = [  # (layer, edge, has a Winograd form)
        (Layer("a", "conv2d", 32, 32), 8, True),
        (Layer("a", "conv2d", 32, 32), 2, False),                    # edge < 4
        (Layer("a", "conv3d", 32, 32), 3, False),
        (Layer("a", "conv3d", 32, 32, 4, 1, 0), 7, True),            # F(2,4) x F(2,4)
        (Layer("a", "deconv3d", 32, 32, 4, 2, 1), 8, True),
        (Layer("a", "deconv3d", 32, 32, 4, 2, 1), 6, False),         # edge % 4 != 0
        (Layer("a", "conv2d", 32, 32, 3, 1, 1, True, "sigmoid"), 8, False),
        (Layer("a", "conv2d", 16, 32), 8, False),                    # cin % 32 != 0
        (Layer("a", "conv2d", 32, 32, 3, 2, 1), 8, False),           # stride 2
    ]
    for l, edge, has in cases:
        ch = s3r.modules._HipChain([l], edge, precision="fp32", winograd=True)
        assert ch._has_winograd_form(l) == has, (l, edge)
        assert ch._algo_of(l) == (L.ALGO_WINOGRAD if has else L.ALGO_DIRECT), (l, edge)
        assert s3r.modules._HipChain([l], edge, precision="fp32", winograd=False)._algo_of(l) == L.ALGO_DIRECT
        assert s3r.modules._HipChain([l], edge, precision="fp32")._algo_of(l) == L.ALGO_AUTO
    assert not s3r.modules._HipChain([cases[0][0]], 8, precision="bf16", winograd=True)._has_winograd_form(cases[0][0])


def test_env_switch_table_matches_the_sources():
    """tools/README.md lists EVERY environment switch the library reads (one table, checked against `grep getenv`): a
    switch added to a kernel source without a row — or a row whose switch is gone — fails here."""
    import glob, re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    found = set()
    for f in glob.glob(os.path.join(root, "stereo-3d-reconstruction_amd", "csrc", "*.hip")) + \
            glob.glob(os.path.join(root, "stereo-3d-reconstruction_amd", "csrc", "*.h")):
        found |= set(re.findall(r'getenv\("(S3R_[A-Z0-9_]+)"\)', open(f).read()))
    readme = open(os.path.join(root, "tools", "README.md")).read()
    table = set(re.findall(r"^\| `(S3R_[A-Z0-9_]+)` \|", readme, re.M))
    assert found == table, (sorted(found - table), sorted(table - found))
    assert len(found) <= 13                      # (18 in r04: new switches replace old ones, they do not pile up)
    bench = open(os.path.join(root, "bench.py")).read()
    for name in found:                           # ... and a bench run under any of them is marked as not the plain configuration
        assert f'"{name}"' in bench, name


def test_parameter_general_descriptors_plan_without_a_gpu(s3r, lib):
    """ABI 8: sizes of the parameter-general layers (host-side planning only): output edges follow torch's formulas with dilation and
    output padding; a layer the tuned kernels do not serve packs K rows for its channel count rounded up to 16 and asks for the scratch
    of its staged copy; nonsense is refused, not planned."""
    L = s3r._lib
    Layer = s3r.arch_spec.Layer
    import torch
    for layer, n in ((Layer("a", "conv2d", 3, 8, 7, 2, 3), 33), (Layer("a", "conv3d", 16, 16, 3, 1, 3, True, "none", 3), 9),
                     (Layer("a", "deconv2d", 12, 20, 3, 2, 1, True, "relu", 1, 1), 6), (Layer("a", "deconv3d", 16, 8, 5, 3, 2, True, "tanh", 1, 2), 4),
                     (Layer("a", "deconv2d", 16, 16, 3, 2, 2, True, "none", 2, 1), 6)):
        d = L.make_desc(layer, 2, n)
        blk = s3r.modules._Block(layer)
        nd = s3r.arch_spec.ndim(layer)
        want = blk.conv(torch.zeros((1, layer.cin) + (n,) * nd)).shape[-1]
        assert lib.s3r_conv_out_size(C.byref(d)) == want == s3r.arch_spec.out_size(layer, n), (layer, want)
    staged = L.make_desc(Layer("a", "conv2d", 20, 40, 3, 2, 1), 2, 15)
    e = C.c_int64(0)
    assert lib.s3r_conv_packed_elems(C.byref(staged), C.byref(e)) == 0 and e.value == 9 * 32 * 128
    assert lib.s3r_conv_scratch_elems(C.byref(staged)) == -(-(2 * 32 * 17 * 17) // 256) * 256       # (B, 32, 15 + 2, 15 + 2)
    # a ConvTranspose with dilation 1 runs as stride^ndim residue classes over the halo-padded (NOT zero-stuffed) input: k4 s2 p1 reads
    # one element beyond each side (halo 1) and packs its 2 x 2 classes of 2 x 2 taps; k2 s3 p0 has a class WITHOUT a tap (one zero tap)
    up = L.make_desc(Layer("a", "deconv2d", 16, 8, 4, 2, 1), 1, 7)
    assert lib.s3r_conv_scratch_elems(C.byref(up)) == -(-(16 * 9 * 9) // 256) * 256
    assert lib.s3r_conv_packed_elems(C.byref(up), C.byref(e)) == 0 and e.value == 16 * 16 * 128
    gap = L.make_desc(Layer("a", "deconv2d", 8, 8, 2, 3, 0), 1, 5)
    assert lib.s3r_conv_packed_elems(C.byref(gap), C.byref(e)) == 0 and e.value == 9 * 16 * 128
    dil = L.make_desc(Layer("a", "deconv2d", 16, 8, 3, 2, 2, True, "none", 2, 1), 1, 7)             # dilation 2: still stuffed (edge 14, halo 2)
    assert lib.s3r_conv_scratch_elems(C.byref(dil)) == -(-(16 * 18 * 18) // 256) * 256
    for bad in (Layer("a", "deconv2d", 16, 8, 3, 2, 3), Layer("a", "deconv2d", 16, 8, 3, 2, 1, True, "relu", 1, 2)):
        assert lib.s3r_conv_scratch_elems(C.byref(L.make_desc(bad, 1, 7))) == -1                    # pad > k - 1; out_pad >= stride
    wino = L.make_desc(Layer("a", "conv3d", 32, 32, 3, 1, 1, True, "elu"), 1, 8, in_halo=1, algo=L.ALGO_WINOGRAD)
    assert lib.s3r_conv_scratch_elems(C.byref(wino)) == -1 and b"no Winograd form" in lib.s3r_last_error()
    bf = L.make_desc(Layer("a", "conv2d", 32, 32, 3, 1, 2, True, "relu", 2), 1, 8, in_halo=2, dtype=1)
    assert lib.s3r_conv_scratch_elems(C.byref(bf)) == -1 and b"bf16" in lib.s3r_last_error()


def test_release_path_reads_no_kernel_policy_from_the_environment(s3r, monkeypatch):
    """descriptor fields come from the model, its tuning tables or an explicit s3r.debug_overrides(...)
    context — never from os.environ (r05 read S3R_TILE_ / S3R_KSPLIT_ / S3R_ALGO_<layer> on every forward)."""
    import re
    # every file of the package that builds a descriptor, as one text (modules.py first: the one use is in it)
    src = "\n".join(open(os.path.join(ROOT, "stereo-3d-reconstruction_amd", f)).read() for f in ("modules.py", "ops.py", "_tensors.py"))
    uses = [l.strip() for l in src.split("\n") if "os.environ" in l and not l.strip().startswith("#")]
    assert len(uses) == 1 and "S3R_BF16_MFMA" in uses[0] and "_cache_key" in src[:src.index(uses[0])].rsplit("def ", 1)[1]
    for name in ("S3R_TILE_v2", "S3R_KSPLIT_v2", "S3R_ALGO_v2"):
        monkeypatch.setenv(name, "3")
    dec = s3r.Decoder()
    v2 = dec._layers[1]
    assert dec._tile_ksplit_of(v2) == (-1, 0) and dec._algo_of(v2) == s3r.ALGO_AUTO
    dec.tile_override["v2"] = 1
    with s3r.debug_overrides(tile={"v2": 2}, algo={"v2": s3r.ALGO_DIRECT}):
        assert dec._tile_ksplit_of(v2) == (2, 0) and dec._algo_of(v2) == s3r.ALGO_DIRECT
        with s3r.debug_overrides(ksplit={"v2": 4}):
            assert dec._tile_ksplit_of(v2) == (2, 4)
            assert s3r.debug_overrides.active() == {"tile": {"v2": 2}, "ksplit": {"v2": 4}, "algo": {"v2": 1}}
        assert dec._tile_ksplit_of(v2) == (2, 0)
    assert dec._tile_ksplit_of(v2) == (1, 0) and s3r.debug_overrides.active() == {}
    with pytest.raises(TypeError):
        s3r.debug_overrides(tile={"v2": "2"})


def test_scratch_queries_do_not_depend_on_the_launch_form_the_device_would_pick(s3r, lib):
    """launch forms (bit-identical among themselves) are planned against the current device's compute-unit count and have
    different scratch footprints; a size query made on another device — or on none — than the forward's would then disagree with it.
    Whenever the LIBRARY picks the form the query is sized for the largest one, so it covers every form a device may pick."""
    L = s3r._lib
    dec = {l.name: (l, n) for l, n, _ in s3r.arch_spec.stage_table("decoder")}
    enc = {l.name: (l, n) for l, n, _ in s3r.arch_spec.stage_table("encoder")}
    for name, table, forms in (("e2", enc, (0, 1, 2)), ("e4", enc, (0, 1, 2)), ("v1", dec, (3, 4, 5)), ("e6", enc, (3, 4, 5)), ("v5", dec, (3, 4, 5)),
                               ("d2", dec, (0, 1, 2)), ("d3", dec, (6, 7, 8))):
        layer, n = table[name]
        for batch in (1, 2, 8, 32, 64):
            auto = lib.s3r_conv_scratch_elems(C.byref(L.make_desc(layer, batch, n, in_halo=1, algo=L.ALGO_AUTO)))
            assert auto > 0, (name, batch, lib.s3r_last_error())
            for tile in forms:
                forced = lib.s3r_conv_scratch_elems(C.byref(L.make_desc(layer, batch, n, in_halo=1, algo=L.ALGO_WINOGRAD, tile=tile)))
                if forced >= 0:            # (a form the layer does not have at this batch is refused, not sized)
                    assert auto >= forced, (name, batch, tile, auto, forced)
