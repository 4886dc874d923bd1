"""s3r_augment_pair without a device: the Philox known answers, the restatement (tests/_augment64.py) against the host conversions, the
coverage the device test's ids must have, the mutants the bit-for-bit comparison of tests/test_augment_gpu.py must catch (on that
file's inputs), the header and bindings, every refusal (host-side: nothing is enqueued), the scratch query's formula and
`render_channels=4`."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from tests import _augment64 as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32


@pytest.fixture(scope="module")
def lib(s3r):
    return s3r.load_library()


@pytest.fixture(autouse=True)
def _the_entry_exists(s3r, lib):
    """every test of this file is about s3r_augment_pair: a restatement pins nothing without the entry point it restates"""
    assert hasattr(lib, "s3r_augment_pair") and hasattr(s3r, "AugmentConfig")


@pytest.fixture(scope="module")
def header():
    with open(os.path.join(ROOT, "include", "s3r.h")) as f:
        return f.read()


# ---------------------------------------------------------------- random numbers
def _hex(words):
    return " ".join("%08x" % int(w) for w in words)


def test_philox_known_answers():
    assert _hex(R.philox((0, 0, 0, 0), (0, 0))) == "6627e8d5 e169c58d bc57ac4c 9b00dbd8"
    ones = 0xFFFFFFFF
    assert _hex(R.philox((ones,) * 4, (ones,) * 2)) == "408f276d 41c83b0e a20bc7c6 6d5451fd"
    assert _hex(R.philox((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0))) == "d16cfe09 94fdcceb 5001e420 24126ea1"
    # vectorised over the index, as the noise draws use it
    idx = np.arange(5, dtype=np.uint32)
    many = R.philox((7, 9, 3, idx), (11, 13))
    for i in range(5):
        assert [int(w[i]) for w in many] == [int(w) for w in R.philox((7, 9, 3, i), (11, 13))]


def test_unit_is_exact():
    from fractions import Fraction
    w = np.array([0, 1, 255, 256, 0x12345678, 0x80000000, 0xFFFFFF00, 0xFFFFFFFF], np.uint32)
    u = R.unit(w)
    assert u.dtype == F
    for wi, ui in zip(w, u):
        assert Fraction(float(ui)) == Fraction(int(wi) >> 8, 2 ** 24)
    assert u.max() < 1.0 and u.min() == 0.0


# ---------------------------------------------------------------- the restatement against the host conversions
def test_identity_is_the_host_conversion(s3r):
    left, right = R.renders(3, 3, 9, 13, 1)
    ids = [5, 6, 7]
    ol, orr = R.augment32(R.IDENTITY, left, right, ids)
    assert np.array_equal(ol.view(np.int32), s3r.data.renders_to_float(left).view(np.int32))
    assert np.array_equal(orr.view(np.int32), s3r.data.renders_to_float(right).view(np.int32))
    left, right = R.renders(3, 4, 9, 13, 2)
    ol, orr = R.augment32(R.IDENTITY, left, right, ids)
    for got, x in ((ol, left), (orr, right)):
        comp = np.stack([s3r.data.composite_over_white_u8(s.transpose(1, 2, 0)).transpose(2, 0, 1) for s in x])
        assert np.array_equal(got.view(np.int32), s3r.data.renders_to_float(comp).view(np.int32))
    # all 256 codes against every alpha
    c, a = np.meshgrid(np.arange(256, dtype=np.uint8), np.arange(256, dtype=np.uint8))
    x = np.stack([c, c, c, a])[None]
    ol, _ = R.augment32(R.IDENTITY, x, x, [0])
    comp = s3r.data.composite_over_white_u8(x[0].transpose(1, 2, 0)).transpose(2, 0, 1)
    assert np.array_equal(ol[0].view(np.int32), s3r.data.renders_to_float(comp).view(np.int32))
    assert s3r.AugmentConfig.identity() == R.to_cfg(s3r, R.IDENTITY)


def test_identity_leaves_the_disparity_maps_alone():
    left, right = R.renders(2, 3, 5, 7, 3)
    dl, dr = R.disparities(2, 5, 7, 3)
    _, _, ol, orr = R.augment32(R.IDENTITY, left, right, [1, 2], dl, dr)
    assert np.array_equal(ol.view(np.int32), dl.view(np.int32)) and np.array_equal(orr.view(np.int32), dr.view(np.int32))
    bits = set(np.concatenate([dl.view(np.uint32).ravel(), dr.view(np.uint32).ravel()]).tolist())
    assert {0x7FC00001, 0xFFC12345, 0x7F800001, 0x7F800000, 0xFF800000, 0x80000000} <= bits


# ---------------------------------------------------------------- coverage of the device test's ids
def test_the_device_tests_ids_cover_every_draw():
    cfg = R.CONFIGS["all"]
    assert cfg.seed == R.SEED == 0 and cfg.max_shift == R.MAX_SHIFT == 3 and R.COVERAGE_IDS == list(range(64))
    d = [R.draws(cfg, i) for i in R.COVERAGE_IDS]
    assert {x.perm for x in d} == set(range(6))
    for axis in ("dy", "dx"):
        v = [getattr(x, axis) for x in d]
        assert min(v) < 0 and max(v) > 0 and 0 in v and set(v) <= set(range(-3, 4))
    # a window that leaves the image on each side: rows uncovered at the top (dy > 0) and bottom (dy < 0), columns at the left and right
    assert any(x.dy > 0 for x in d) and any(x.dy < 0 for x in d) and any(x.dx > 0 for x in d) and any(x.dx < 0 for x in d)
    assert len({x.bg[0] for x in d}) > 8 and all(0 <= c <= 255 for x in d for c in x.bg)
    for name in ("brightness", "contrast"):
        v = [float(getattr(x, name)) for x in d]
        assert min(v) < 1.0 < max(v) and 0.5 <= min(v) and max(v) <= 1.5
    # switching one op on never changes another op's draw
    alone = [R.draws(R.CONFIGS["shift"], i) for i in R.COVERAGE_IDS]
    assert [(x.dy, x.dx, x.perm, x.bg) for x in alone] == [(x.dy, x.dx, x.perm, x.bg) for x in d]


def test_mutants_of_the_restatement_change_the_device_tests_result():
    """each wrong version differs from the right one on inputs the device test compares bit for bit (the 'all' configuration)"""
    cfg = R.CONFIGS["all"]
    hit = {m: False for m in R.MUTANTS}
    for (H, W), ch in (((33, 31), 4), ((25, 41), 4), ((17, 31), 3)):
        ids = R.COVERAGE_IDS[:3]
        left, right = R.renders(3, ch, H, W, H * W)
        want = R.augment32(cfg, left, right, ids)
        for m in R.MUTANTS:
            got = R.augment32(cfg, left, right, ids, mutant=m)
            if any(not np.array_equal(g.view(np.int32), w.view(np.int32)) for g, w in zip(got, want)):
                hit[m] = True
    assert all(hit.values()), hit
    assert (33, 31) in R.SHAPES and (25, 41) in R.SHAPES and (17, 31) in R.SHAPES


def test_views_share_everything_but_the_noise():
    left, _ = R.renders(2, 3, 6, 10, 4)
    quiet = R.CONFIGS["all"]._replace(noise_sigma=0.0)
    a, b = R.augment32(quiet, left, left, [3, 4])
    assert np.array_equal(a.view(np.int32), b.view(np.int32))
    a, b = R.augment32(R.CONFIGS["all"], left, left, [3, 4])
    assert not np.array_equal(a, b)
    assert a.min() >= 0.0 and a.max() <= 1.0


def test_table_shapes_cross_every_path_of_the_order():
    sizes = {h * w for h, w in R.SHAPES}
    assert min(sizes) < 4 and 4 in sizes and 256 in sizes and 512 in sizes and 1024 in sizes         # a short quad, a lane row, one and two chunks
    assert any(s % 4 and s > 512 for s in sizes) and any(512 < s < 1024 for s in sizes) and any(s > 1024 for s in sizes)
    assert any(w % 4 for _, w in R.SHAPES)
    assert R.BIG == (224, 224)


# ---------------------------------------------------------------- header, bindings
def _proto(header, ret, name):
    plain = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    m = re.search(r"\b%s\s+%s\s*\(([^)]*)\)\s*;" % (ret, name), plain)
    assert m, f"{name} is not declared in include/s3r.h"
    return [" ".join(a.split()) for a in m.group(1).split(",")]


def test_header_prototypes_match_the_bindings(s3r, lib, header):
    L = s3r._lib
    assert _proto(header, "int64_t", "s3r_augment_scratch_elems") == ["const s3r_augment_desc* d", "int batch", "int height", "int width"]
    assert _proto(header, "int", "s3r_augment_pair") == [
        "const s3r_augment_desc* d", "const uint8_t* left", "const uint8_t* right", "const int64_t* sample_ids", "const float* disp_left",
        "const float* disp_right", "float* out_left", "float* out_right", "float* out_disp_left", "float* out_disp_right", "int batch",
        "int height", "int width", "float* scratch", "int64_t scratch_elems", "void* hip_stream"]
    assert L.SIGNATURES["s3r_augment_scratch_elems"] == (C.c_int64, [C.POINTER(L.AugmentDesc), C.c_int, C.c_int, C.c_int])
    res, args = L.SIGNATURES["s3r_augment_pair"]
    assert res == C.c_int and args == [C.POINTER(L.AugmentDesc)] + [C.c_void_p] * 9 + [C.c_int] * 3 + [C.c_void_p, C.c_int64, C.c_void_p]
    assert lib.s3r_augment_pair.argtypes == args and hasattr(lib, "s3r_augment_scratch_elems")
    body = header[header.index("typedef struct s3r_augment_desc {"):header.index("} s3r_augment_desc;")]
    fields = re.findall(r"(?:uint64_t|int32_t|float)\s+([a-z_, ]+);", re.sub(r"/\*.*?\*/", "", body, flags=re.S))
    assert [n.strip() for f in fields for n in f.split(",")] == [n for n, _ in L.AugmentDesc._fields_]
    assert C.sizeof(L.AugmentDesc) == 56
    assert re.search(r"#define S3R_AUG_PERMUTE_RGB %d\b" % L.AUG_PERMUTE_RGB, header)
    assert re.search(r"#define S3R_AUG_MAX_SHIFT %d\b" % L.AUG_MAX_SHIFT, header)
    assert lib.s3r_abi_version() == 8 and "#define S3R_ABI_VERSION 8" in header
    assert {"AugmentConfig", "StereoAugment", "augment_pair"} <= set(s3r.__all__) and s3r.ops.augment_pair is s3r.augment_pair


def test_the_header_states_the_order(header):
    at = header.index("#define S3R_AUG_PERMUTE_RGB")
    comment = " ".join(re.sub(r"\n \*", " ", header[header[:at].rfind("/* Training-time augmentation"):at]).split())
    for wording in ("Philox4x32-10", "0xD2511F53", "0xBB67AE85", "(float)(w >> 8) * 2^-24", "t = hi - lo; t = u * t; lo + t",
                    "whether or not its op is enabled", "dy = w0 % (2 max_shift + 1) - max_shift", "perm = w2 % 6", "bias",
                    "purpose 1 + 3 side + c", "only the noise is per view", "(src[c] * a + bg[c] * (255 - a) + 127) / 255",
                    "v = (float)code / 255.f", "a = contrast * v; t = 1.f - contrast; b = t * m; v = a + b",
                    "l = (0.299f * v0 + 0.587f * v1) + 0.114f * v2", "s = s * 1.7320508f", "out[c'] = v[perm[c']]", "+inf",
                    "ONE value per pair", "chunks of 512 consecutive positions", "m = total / (float)(2 S)", "2 B ceil(S / 512) + B",
                    "before anything is enqueued", "Every node is a kernel", "hip_stream", "hipStream_t", "INVENTED by this build"):
        assert wording in comment, wording


# ---------------------------------------------------------------- refusals and the scratch query (host-only)
A = 0x100000      # non-NULL addresses far apart: every case is refused before anything could dereference them


def _desc(L, **kw):
    f = dict(seed=0, channels=3, max_shift=2, flags=1, bg_lo=0, bg_hi=255, brightness_lo=0.8, brightness_hi=1.2, contrast_lo=0.8,
             contrast_hi=1.2, saturation_lo=0.8, saturation_hi=1.2, noise_sigma=0.02)
    f.update(kw)
    return L.AugmentDesc(*[f[n] for n, _ in L.AugmentDesc._fields_])


def _call(lib, d, B=2, H=8, W=8, **kw):
    p = dict(left=A * 1, right=A * 2, ids=A * 3, dl=None, dr=None, ol=A * 6, orr=A * 7, odl=None, odr=None, scratch=A * 10, n=1 << 20)
    p.update(kw)
    return lib.s3r_augment_pair(C.byref(d) if d is not None else None, p["left"], p["right"], p["ids"], p["dl"], p["dr"], p["ol"], p["orr"],
                                p["odl"], p["odr"], B, H, W, p["scratch"], p["n"], None)


def _refused(lib, rc, *words):
    assert rc == -1, rc
    msg = lib.s3r_last_error().decode()
    assert msg.startswith("augment")
    for w in words:
        assert w in msg, (w, msg)


def test_null_and_partial_pointers_are_refused(s3r, lib):
    L = s3r._lib
    _refused(lib, _call(lib, None), "null descriptor")
    for k in ("left", "right", "ids", "ol", "orr"):
        _refused(lib, _call(lib, _desc(L), **{k: None}), "null")
    maps = dict(dl=A * 4, dr=A * 5, odl=A * 8, odr=A * 9)
    for k in maps:
        _refused(lib, _call(lib, _desc(L), **dict(maps, **{k: None})), "all NULL or all given")
        _refused(lib, _call(lib, _desc(L), **{k: maps[k]}), "all NULL or all given")


def test_bad_descriptors_and_shapes_are_refused(s3r, lib):
    L = s3r._lib
    inf, nan = float("inf"), float("nan")
    for kw, word in ((dict(channels=2), "channels"), (dict(channels=5), "channels"), (dict(max_shift=-1), "max_shift"),
                     (dict(max_shift=4097), "max_shift"), (dict(flags=2), "flag"), (dict(flags=3), "flag"), (dict(bg_lo=-1), "background"),
                     (dict(bg_hi=256), "background"), (dict(bg_lo=9, bg_hi=8), "background"), (dict(noise_sigma=-0.1), "noise_sigma"),
                     (dict(noise_sigma=inf), "noise_sigma"), (dict(noise_sigma=nan), "noise_sigma")):
        _refused(lib, _call(lib, _desc(L, **kw)), word)
        assert lib.s3r_augment_scratch_elems(C.byref(_desc(L, **kw)), 2, 8, 8) == -1
    for name in ("brightness", "contrast", "saturation"):
        for lo, hi in ((1.2, 0.8), (-0.1, 1.0), (0.5, inf), (nan, 1.0), (0.5, nan)):
            _refused(lib, _call(lib, _desc(L, **{name + "_lo": lo, name + "_hi": hi})), name)
    for shape in (dict(B=0), dict(B=-1), dict(H=0), dict(W=0), dict(W=-3)):
        _refused(lib, _call(lib, _desc(L), **shape), "positive")
    _refused(lib, _call(lib, _desc(L), H=65536, W=32768), "2^31")
    _refused(lib, _call(lib, _desc(L), B=1024, H=1024, W=1024), "2^31")
    assert lib.s3r_augment_scratch_elems(None, 2, 8, 8) == -1
    assert lib.s3r_augment_scratch_elems(C.byref(_desc(L)), 2, 65536, 32768) == -1
    assert _call(lib, _desc(L, max_shift=4096), ol=None) == -1                 # 4096 itself gets past the descriptor's checks


def test_scratch_and_overlap_are_refused(s3r, lib):
    L = s3r._lib
    d = _desc(L)
    need = lib.s3r_augment_scratch_elems(C.byref(d), 2, 8, 8)
    assert need == 2 * 2 * 1 + 2
    _refused(lib, _call(lib, d, scratch=None), "scratch")
    _refused(lib, _call(lib, d, n=need - 1), "scratch", str(need))
    px = 2 * 8 * 8
    # an output that overlaps an input, another output, the ids or the scratch (first and last byte of the range)
    _refused(lib, _call(lib, d, ol=A * 1), "overlap")
    _refused(lib, _call(lib, d, orr=A * 2 + 3 * px - 1), "overlap")
    _refused(lib, _call(lib, d, orr=A * 6 + 12 * px - 4), "overlap")
    _refused(lib, _call(lib, d, ol=A * 3 + 12), "overlap")
    _refused(lib, _call(lib, d, scratch=A * 7 + 4), "overlap")
    maps = dict(dl=A * 4, dr=A * 5, odl=A * 8, odr=A * 9)
    _refused(lib, _call(lib, d, **dict(maps, odl=A * 4)), "overlap")
    _refused(lib, _call(lib, d, **dict(maps, odr=A * 8 + 4 * px - 4)), "overlap")
    _refused(lib, _call(lib, d, **dict(maps, odl=A * 7 - 4)), "overlap")
    # without contrast no scratch is looked at: the call gets past every check but the first later one (a NULL output)
    quiet = _desc(L, contrast_lo=1.0, contrast_hi=1.0)
    assert lib.s3r_augment_scratch_elems(C.byref(quiet), 2, 8, 8) == 0
    _refused(lib, _call(lib, quiet, scratch=None, n=0, ol=None), "null out")


def test_scratch_query_formula(s3r, lib):
    L = s3r._lib
    for B, H, W in ((1, 1, 1), (1, 16, 32), (2, 17, 31), (3, 33, 31), (32, 224, 224), (65, 25, 41)):
        for ch in (3, 4):
            assert lib.s3r_augment_scratch_elems(C.byref(_desc(L, channels=ch)), B, H, W) == 2 * B * -(-(H * W) // 512) + B
            assert lib.s3r_augment_scratch_elems(C.byref(_desc(L, channels=ch, contrast_lo=1.0, contrast_hi=1.0)), B, H, W) == 0


def test_config_validates_and_builds_the_descriptor(s3r):
    cfg = s3r.AugmentConfig.default(seed=2 ** 40 + 5)
    d = cfg.desc(4)
    assert (d.seed, d.channels, d.max_shift, d.flags, d.bg_lo, d.bg_hi) == (2 ** 40 + 5, 4, 8, 1, 255, 255)
    assert (d.brightness_lo, d.noise_sigma) == (F(0.8), F(0.02)) and cfg.needs_scratch and not s3r.AugmentConfig.identity().needs_scratch
    i = s3r.AugmentConfig.identity().desc(3)
    assert (i.max_shift, i.flags, i.contrast_lo, i.contrast_hi, i.noise_sigma) == (0, 0, 1.0, 1.0, 0.0)
    for kw in (dict(seed=-1), dict(max_shift=4097), dict(background=(3, 2)), dict(brightness=(1.2, 0.8)), dict(noise_sigma=-1.0),
               dict(contrast=(0.0, float("inf")))):
        with pytest.raises(ValueError):
            s3r.AugmentConfig(**kw)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        s3r.augment_pair(torch.zeros(1, 3, 4, 4, dtype=torch.uint8), torch.zeros(1, 3, 4, 4, dtype=torch.uint8),
                         torch.zeros(1, dtype=torch.int64), cfg)


# ---------------------------------------------------------------- render_channels=4
def test_render_channels_4_yields_uncomposited_rgba(s3r, tmp_path):
    from tests.test_data_cpu import _make_tree
    _make_tree(str(tmp_path), n_models=1, views=(0,), size=224)
    rgb = s3r.data.StereoShapeNet(str(tmp_path))
    rgba = s3r.data.StereoShapeNet(str(tmp_path), render_channels=4)
    assert len(rgb) == len(rgba) == 1
    l3, r3, v3 = rgb[0]
    l4, r4, v4 = rgba[0]
    assert l4.shape == (4, 224, 224) and l4.dtype == torch.uint8 and torch.equal(v3, v4)
    assert torch.all(l4[3, :112] == 0) and not torch.all(l4[:3, :112] == 255)      # the transparent half keeps its own colour codes
    for x4, x3 in ((l4, l3), (r4, r3)):
        comp = s3r.data.composite_over_white_u8(x4.numpy().transpose(1, 2, 0)).transpose(2, 0, 1)
        assert np.array_equal(comp, x3.numpy())
        # ... which is what the identity augmentation computes from the RGBA codes
        got, _ = R.augment32(R.IDENTITY, x4.numpy()[None], x4.numpy()[None], [0])
        assert np.array_equal(got[0].view(np.int32), s3r.data.renders_to_float(x3.numpy()).view(np.int32))
    with pytest.raises(ValueError):
        s3r.data.StereoShapeNet(str(tmp_path), render_channels=2)
    with pytest.raises(ValueError):
        s3r.data.StereoShapeNet(str(tmp_path), render_channels=4, render_dtype="float32")
