"""Host-side half of tests/test_buffers_gpu.py: the guard helper's own unit test, the fp64 checker's mutation self-test for every
case of the GPU file, and the producer x consumer planning matrix of s3r_chain_forward (no GPU: planning entries only)."""
import ctypes as C
import dataclasses
import math
import os

import pytest
import torch

from tests import _alignment_cases as AC
from tests import _buffer_cases as BC
from tests import _guard as G
from tests import _linear_cases as LC
from tests import _ref64 as R


@pytest.fixture(scope="module")
def lib(s3r):
    import __graft_entry__ as g
    if not os.path.exists(s3r.LIB_PATH):
        g.build()
    return s3r.load_library()


# ---------------------------------------------------------------- the guard helper
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.int32])
def test_guard_reports_each_region(dtype):
    def out():
        return G.Guarded("y", (2, 3, 6, 6), dtype, "cpu", "out", halo=1, spatial=(2, 3))

    b = out()
    assert b.t.data_ptr() % 256 == 0 and b.g * b.t.element_size() == G.GUARD_BYTES
    assert b.check() == "leftover poison in y +7 (index (0, 0, 1, 1))"
    b.t[:, :, 1:5, 1:5] = 1
    assert b.check() is None
    b.t[0, 1, 4, 2] = 3                                          # another interior value: fine
    assert b.check() is None
    b.t[0, 0, 2, 3] = G._BITS[dtype][2] if dtype == torch.int32 else float("nan")
    if dtype == torch.int32:
        assert b.check() == "leftover poison in y +15 (index (0, 0, 2, 3))"
    b = out()
    b.t[:, :, 1:5, 1:5] = 1
    b.t[1, 2, 5, 0] = 0                                          # a zero written into the halo
    assert b.check() == f"write into the halo of y +{36 * 5 + 30} (index (1, 2, 5, 0))"
    b = out()
    b.t[:, :, 1:5, 1:5] = 1
    b.raw[b.g - 1] = 0                                           # one element in front of the payload
    assert b.check() == f"front guard of y +{b.g - 1}"
    b = out()
    b.t[:, :, 1:5, 1:5] = 1
    b.raw[b.g + b.n + 1344] = 0
    assert b.check() == "back guard of y +1344"


def test_guard_inputs_and_scratch():
    x = torch.arange(24, dtype=torch.float32).reshape(2, 12)
    b = G.Guarded("x", x.shape, torch.float32, "cpu", "in", data=x)
    assert b.check() is None
    b.t[0, 0] = -0.0                                             # equal to +0.0 as a value, not as bits
    assert b.check() == "change of the input x +0 (index (0, 0))"
    s = G.Guarded("scratch", 100, torch.float32, "cpu", "scratch")
    assert torch.isnan(s.t).all() and s.check() is None
    s.t.zero_()
    assert s.check() is None                                     # contents are the kernel's
    s.raw[-1] = 1.0
    assert s.check() == f"back guard of scratch +{s.g - 1}"
    z = G.Guarded("ws", 0, torch.float32, "cpu", "scratch", fill="zero")
    assert z.check() is None and z.t.numel() == 0


@pytest.mark.parametrize("skew", [1, 33])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.int32])
def test_guard_at_a_skewed_payload(dtype, skew):
    """a payload `skew` elements past a 256-byte boundary: guards, poison, sentinel and first-offender reporting as at skew 0"""
    def out():
        return G.Guarded("y", (2, 3, 6, 6), dtype, "cpu", "out", halo=1, spatial=(2, 3), skew=skew)

    b = out()
    esz = b.t.element_size()
    assert b.skew == skew and b.t.data_ptr() % 256 == skew * esz % 256 and b.ptr == b.t.data_ptr()
    assert b.t.data_ptr() - b.raw.data_ptr() == G.GUARD_BYTES and b.raw.numel() == 2 * b.g + b.n      # guards contiguous around it
    assert b.check() == "leftover poison in y +7 (index (0, 0, 1, 1))"
    b.t[:, :, 1:5, 1:5] = 1
    assert b.check() is None
    b.t[1, 2, 5, 0] = 0
    assert b.check() == f"write into the halo of y +{36 * 5 + 30} (index (1, 2, 5, 0))"
    b = out()
    b.t[:, :, 1:5, 1:5] = 1
    b.raw[b.g - 1] = 0                                           # a 16-byte store that starts one element early
    assert b.check() == f"front guard of y +{b.g - 1}"
    b = out()
    b.t[:, :, 1:5, 1:5] = 1
    b.raw[b.g + b.n] = 0                                         # ... or runs one element past the payload
    assert b.check() == "back guard of y +0"
    x = torch.arange(24, dtype=torch.float32).to(dtype).reshape(2, 12)
    i = G.Guarded("x", x.shape, dtype, "cpu", "in", data=x, skew=skew)
    assert i.check() is None and torch.equal(i.t, x)
    i.t[1, 3] = 0
    assert i.check() == "change of the input x +15 (index (1, 3))"
    s = G.Guarded("scratch", 100, dtype, "cpu", "scratch", skew=skew) if dtype != torch.int32 else None
    if s is not None:
        assert torch.isnan(s.t.float()).all() and s.check() is None
        s.raw[0] = 1.0
        assert s.check() == "front guard of scratch +0"


def test_skews_by_argument_name():
    """`with G.skews(...)`: by dict or by callable; an explicit skew= wins; outside the block everything is aligned again"""
    with G.skews({"x": 1, "ws": 33}):
        x = G.Guarded("x", 8, torch.float32, "cpu", "scratch")
        y = G.Guarded("y", 8, torch.float32, "cpu", "scratch")
        ws = G.Guarded("ws", 8, torch.float32, "cpu", "scratch")
        z = G.Guarded("x", 8, torch.float32, "cpu", "scratch", skew=0)
        with G.skews(lambda name, dtype, role: 8 if dtype == torch.bfloat16 else 3):
            h = G.Guarded("x", 8, torch.bfloat16, "cpu", "scratch")
            f = G.Guarded("q", 8, torch.float32, "cpu", "scratch")
        again = G.Guarded("x", 8, torch.float32, "cpu", "scratch")
    after = G.Guarded("x", 8, torch.float32, "cpu", "scratch")
    assert [b.ptr % 256 for b in (x, y, ws, z, h, f, again, after)] == [4, 0, 132, 0, 16, 12, 4, 0]
    assert all(b.check() is None for b in (x, y, ws, z, h, f, again, after))


def test_patterns_move_what_they_say():
    """the pattern table of tests/test_alignment_gpu.py (tests/_alignment_cases.py): fp32 skews in elements, bf16 / render / bf16-workspace arguments at 16 or 144 bytes"""
    f32, bf, u8 = torch.float32, torch.bfloat16, torch.uint8
    p = AC.Pattern("mixed")
    assert [p(n, f32, r) for n, r in (("x", "in"), ("w", "in"), ("packed", "out"), ("y", "out"), ("scratch", "scratch"), ("x", "in"))] == \
        [1, 2, 3, 4, 33, 1]
    for pid, want in (("all1", (1, 1, 1)), ("all3", (3, 3, 3)), ("in1", (1, 0, 0)), ("out1", (0, 1, 0)), ("out4", (0, 4, 0)), ("ws1", (0, 0, 1))):
        p = AC.Pattern(pid)
        assert tuple(p(n, f32, r) for n, r in (("x", "in"), ("y", "out"), ("ws", "scratch"))) == want, pid
    p = AC.Pattern("all1", sixteen={"left"}, bf16_call=True)
    assert (p("left", f32, "in"), p("left", u8, "in"), p("features", bf, "out"), p("ws", f32, "scratch"), p("packed0", f32, "out"),
            p("shift", f32, "in")) == (4, 16, 8, 4, 1, 1)
    p = AC.Pattern("all3", sixteen={"left"}, bf16_call=True)
    assert (p("left", f32, "in"), p("left", u8, "in"), p("features", bf, "out"), p("ws", f32, "scratch")) == (36, 144, 72, 36)
    with G.skews(AC.Pattern("all3", bf16_call=True)):
        b = [G.Guarded(n, 8, dt, "cpu", role) for n, dt, role in (("x", bf, "scratch"), ("scratch", f32, "scratch"), ("shift", f32, "scratch"))]
    assert [t.ptr % 256 for t in b] == [144, 144, 12] and [t.ptr % 16 for t in b[:2]] == [0, 0]


# ---------------------------------------------------------------- the checker's mutation self-test
def _one_channel(layer, p, o):
    """the layer restricted to output channel o"""
    w = p["w"]
    w = w[:, o:o + 1] if layer.op.startswith("deconv") else w[o:o + 1]
    return dataclasses.replace(layer, cout=1), {"w": w.clone(), "scale": None if p["scale"] is None else p["scale"][o:o + 1],
                                                 "shift": p["shift"][o:o + 1]}


def _fp32(layer, x, p):
    """the layer computed in fp32 (torch's CPU fp32 reduction standing in for a kernel's)"""
    return R.activate(layer, R.epilogue(layer, R.linmap(layer, x.float(), p["w"].float()), p["scale"], p["shift"]))


def _tap_view(layer, w):
    """the one output channel's weights as a (cin, taps) view"""
    w1 = w[:, 0] if layer.op.startswith("deconv") else w[0]
    return w1.reshape(w1.shape[0], -1)


def _mutants(layer, x, p, clean):
    """(name, fp32 output) of: one tap of the channel dropped, one tap counted twice, one output element shifted by one position"""
    out = []
    for name, f in (("drop", 0.0), ("twice", 2.0)):
        q = dict(p, w=p["w"].clone())
        if layer.op == "linear":                                 # (the term of largest |w x|: a dropped zero input changes nothing)
            t = int((q["w"][0] * x.reshape(-1)).abs().argmax())
            q["w"][0, t] *= f
        else:
            taps = _tap_view(layer, q["w"])
            taps[:, taps.shape[1] // 2] *= f
        out.append((name, _fp32(layer, x, q)))
    flat = clean.reshape(-1)
    if flat.numel() > 1:
        d = (flat[1:] - flat[:-1]).abs()
        i = int(d.argmax())
        s = flat.clone()
        s[i] = flat[i + 1]
        out.append(("shift", s.reshape(clean.shape)))
    return out


def _selftest(layer, n_in, form, seed, bf16=False):
    nd = R.ndim(layer)
    p = R.make_params(layer, seed)
    x = torch.randn((1, layer.cin) + (n_in,) * nd, generator=torch.Generator().manual_seed(seed))
    if bf16:
        x = x.to(torch.bfloat16).float()
        p["w"] = p["w"].to(torch.bfloat16).float()
    o = layer.cout // 2
    l1, p1 = _one_channel(layer, p, o)
    ref, mag = R.ref64(l1, x, p1)
    bnd = R.bound(l1, ref, mag, form)
    clean = _fp32(l1, x, p1)
    if bf16:
        clean = clean.to(torch.bfloat16).float()
    ok, _ = R.worst(clean, ref, bnd)
    assert ok <= 1.0, ("an fp32 computation breaks the bound", ok)
    for name, m in _mutants(l1, x, p1, clean):
        if bf16:
            m = m.to(torch.bfloat16).float()
        r, _ = R.worst(m, ref, bnd)
        assert r > 1.0, (name, "not flagged", r)


SELF_CONV = [c for c in BC.CONV_CASES if not c.id.startswith("unfolded-subbatch")]      # (its single-batch twin: unfolded-conv2d-*)


@pytest.mark.parametrize("case", SELF_CONV, ids=[c.id for c in SELF_CONV])
def test_checker_flags_mutations_conv(case):
    _selftest(case.layer, case.n_in, case.form, 7, bf16=case.dtype == "bf16" and not BC._stem(case.layer) and not BC._head(case.layer, case.n_in))


@pytest.mark.parametrize("shape", [(3, 50, 7), (33, 96, 40), (2, 64, 7), (7, 7, 7), (1, 256, 1), (4, 1, 9), (3, 7, 1), (5, 1024, 6144),
                                   (70, 4096, 100), (32, 8192, 1024)] + [s for s in LC.SWEEP if s[1] <= 8192],
                         ids=lambda s: "x".join(map(str, s)))
def test_checker_flags_mutations_linear(s3r, shape):
    """(the sweep's K = 16384 and 65536 are not here: one term in that many is inside the bound, which grows with K — the reason those
    shapes are held bit for bit by tests/test_exact_gpu.py; tests/test_exact_cpu.py asserts exactly that for K >= 16384)"""
    B, cin, cout = shape
    _selftest(s3r.arch_spec.Layer("t", "linear", cin, min(cout, 8), 1, 1, 0, False, "none"), 1, "direct", cin)


@pytest.mark.parametrize("pair", BC.CHAIN_PAIRS, ids=[n for n, _, _, _ in BC.CHAIN_PAIRS])
def test_checker_flags_mutations_chain(pair):
    """a dropped / doubled tap of the consumer and a shifted output element stand out of the CHAIN's bound (the producer's error
    carried through the consumer included)"""
    name, p, c, _ = pair
    forms = ["wino" if BC.has_wino(BC.ConvCase("", q.layer, q.n_in, 1, algo=q.algo, tile=q.tile)) else "direct" for q in (p, c)]
    params = [R.make_params(q.layer, 31 + i) for i, q in enumerate((p, c))]
    x = torch.randn((1, p.layer.cin) + (p.n_in,) * R.ndim(p.layer), generator=torch.Generator().manual_seed(5))
    o = c.layer.cout // 2
    l1, p1 = _one_channel(c.layer, params[1], o)
    ref, bnd = R.chain_ref64([p.layer, l1], forms, x, [params[0], p1])
    h = _fp32(p.layer, x, params[0])
    if l1.op != "linear":
        h = h.reshape((1, l1.cin) + (c.n_in,) * R.ndim(l1))
    clean = _fp32(l1, h, p1)
    ok, _ = R.worst(clean, ref, bnd)
    assert ok <= 1.0, ("an fp32 computation breaks the bound", ok)
    for mname, m in _mutants(l1, h, p1, clean):
        r, _ = R.worst(m, ref, bnd)
        assert r > 1.0, (mname, "not flagged", r)


def test_bound_constants():
    """c_K = 1.01 (K + 3) from the docstring's derivation, K the non-zero products of one output"""
    L = BC.L
    assert R.k_terms(L("a", "conv3d", 256, 256, 3, 1, 1)) == 256 * 27
    assert R.k_terms(L("a", "deconv3d", 512, 256, 4, 2, 1)) == 512 * 8           # parity classes: 2 taps per axis
    assert R.k_terms(L("a", "deconv2d", 16, 16, 2, 3, 0)) == 16                  # k < s: one tap per class at most
    assert R.k_terms(L("a", "deconv2d", 16, 16, 3, 2, 2, True, "none", 2, 1)) == 16 * 9    # dilated: zero-stuffed, every tap
    assert R.k_terms(L("a", "linear", 96, 40, 1, 1, 0)) == 96
    assert (1.01 * (2 ** 16 + 3) * R.U) < 0.0041 and math.isclose(R.lipschitz(L("a", "conv2d", 4, 4, act="sigmoid")), 0.25)


# ---------------------------------------------------------------- chain planning matrix (host only)
@pytest.mark.parametrize("pair", BC.CHAIN_PAIRS, ids=[n for n, _, _, _ in BC.CHAIN_PAIRS])
def test_chain_planning_matrix(s3r, lib, pair):
    """every producer -> consumer pair plans, except a consumer that reads its zero padding from the producer's halo behind a
    reshaping producer (a linear layer, or a conv whose output the consumer reads in another geometry): refused with
    S3R_ERR_INVALID and a message, as include/s3r.h documents"""
    name, p, c, refused = pair
    arr = (s3r._lib.Layer * 2)()
    arr[0].desc = s3r._lib.make_desc(p.layer, 2, p.n_in, algo=p.algo, tile=p.tile)
    arr[1].desc = s3r._lib.make_desc(c.layer, 2, c.n_in, algo=c.algo, tile=c.tile, out_halo=1 if c.layer.op != "linear" and
                                     not BC._head(c.layer, c.n_in) else 0)
    r = lib.s3r_chain_workspace_elems(arr, 2)
    if refused:
        assert r == -1 and lib.s3r_last_error(), (name, r)
    else:
        assert r > 0, (name, r, lib.s3r_last_error())


def test_reshaping_producers_feed_residue_class_consumers(s3r, lib):
    """Linear -> ConvTranspose2d(16 -> 8, k4 s2 p1) and a reshaping Conv -> ConvTranspose2d were refused since
    r06 gave residue-class consumers the wider halo (want_halo) even where the producer cannot carry one; they stage their own copy"""
    L = s3r.arch_spec.Layer
    for chain in (((L("a", "linear", 32, 256, 1, 1, 0, False), 1), (L("b", "deconv2d", 16, 8, 4, 2, 1), 4)),
                  ((L("a", "linear", 32, 192, 1, 1, 0, False), 1), (L("b", "deconv2d", 12, 8, 4, 2, 1), 4)),
                  ((L("a", "conv2d", 16, 64, 3, 1, 1), 4), (L("b", "deconv2d", 16, 8, 4, 2, 1), 8))):
        arr = (s3r._lib.Layer * 2)()
        for i, (l, n) in enumerate(chain):
            arr[i].desc = s3r._lib.make_desc(l, 2, n)
        assert lib.s3r_chain_workspace_elems(arr, 2) > 0, lib.s3r_last_error()


def test_forced_tile_without_its_gather_is_refused(s3r, lib):
    """tile 5 (64 x 512) exists for the 16-byte gather only: forced on rows of 9 positions it was a launch error (S3R_ERR_HIP, 'invalid
    argument'); now the descriptor is refused up front, and the same tile over rows of 12 positions plans"""
    L = s3r.arch_spec.Layer("t", "conv3d", 64, 70, 3, 1, 1)
    d = s3r._lib.make_desc(L, 2, 9, tile=5, in_halo=1)
    assert lib.s3r_conv_scratch_elems(C.byref(d)) == -1 and b"16-byte gather" in lib.s3r_last_error()
    d = s3r._lib.make_desc(L, 2, 12, tile=5, in_halo=1)
    assert lib.s3r_conv_scratch_elems(C.byref(d)) >= 0
