"""Every C-ABI entry point at pointers that are only element-aligned: "at which address", after tests/test_buffers_gpu.py ("which
bytes") and tests/test_exact_gpu.py ("which bits"), and built from both.

The contract (include/s3r.h, Conventions): fp32 / int32 tensors need 4-byte alignment at every entry and the result bits do not
depend on the address; bf16 tensors, the scratch / workspace of S3R_BF16 layers and renders need 16 bytes (refused on the host
otherwise: tests/test_abi_cpu.py).  Every case runs its entry once with all payloads 256-byte aligned and once per skew pattern of
tests/_alignment_cases.py (all1, all3, mixed, in1, out1, out4, ws1), and every run asserts

  1. the reference the aligned test of that entry asserts: bit equality with the fp64 lattice result (the convolution cases of
     tests/_exact_cases.py), bit equality with the oracle (cost volume, Chamfer, IoU, WTA, EPE counts, channels-last), or the
     per-element fp64 bound of tests/_ref64.py at HALF (transcendental activations, chains, linear) - no tolerance is new here;
  2. address invariance: the output bits equal those of the aligned run of the same test;
  3. the guards: tests/_guard.py::check_all over every argument (inputs unchanged bit for bit, no poison left, sentinels and guards
     intact: a 16-byte store that starts before or runs past a skewed payload lands in a guard and is reported with its offset).

The bodies are tests/_abi_bodies.py's, shared with tests/test_buffers_gpu.py; assertions 1 and 3 live there.  The second half drives
the modules with torch views at storage offset 1.  test_a_shifted_input_is_a_mismatch is the harness's self-check: an input moved by
one element against its reference (the "neighbour's data" a truncated address would fetch) fails assertion 1.

Measured on an MI355X, in one visit: tests/test_buffers_gpu.py 7.4 - 7.8 s (420 tests), this file 14 - 16 s (131 tests: each case runs 8
times - aligned + 7 patterns - and the convolution, chain and linear bodies twice or four times per run).  Every case passes: every
entry point gives the same bits at 4-byte (bf16: 16-byte) alignment as at 256 bytes, so the tests found no kernel bug; the three
16-byte accesses that were typed as 16-byte aligned on caller-derived addresses (the head kernel, the split-K combine pass, the
two-axis input staging) are now typed dword-aligned, with unchanged machine code.  Largest |got - ref| / bound of the bound-held
cases, the same under every pattern since the bits are: direct 0.18 (linear 7x7x7), Winograd 0.0031 (elu-pass-conv3d-32to32-e8),
bf16 2.5e-5 (d4-bf16-B1-oh0), chains 0.0070 (linear->tclass-h1).  A kernel trace of the transposed Winograd cases showed both sides
of launch_wino_diff's address branch: the two-column kernel 36 times (aligned, out1, out4), the scalar one 60 times.
"""
import pytest
import torch

from tests import _abi_bodies as AB
from tests import _alignment_cases as AC
from tests import _buffer_cases as BC
from tests import _exact_cases as X
from tests import _guard as G
from tests import _lattice as LT
from tests._abi_calls import DEV, pack, rc_ok, sync
from tests.test_exact_gpu import _data, assert_bits

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib(s3r):
    return s3r.load_library()


def across_patterns(body, sixteen=(), bf16_call=False, first=None):
    """body() -> tuple of output tensors, asserting its reference and its guards itself: once aligned (`first`, if given, is the
    aligned run: it may assert refusals too), once per pattern; the bits of every run must equal the aligned run's"""
    base = (first or body)()
    for pid in AC.PATTERNS:
        print(f"\npattern {pid}")
        pat = AC.Pattern(pid, sixteen, bf16_call)
        with G.skews(pat):
            outs = body()
        assert pat.index, "the body built no guarded argument inside the pattern"
        assert len(outs) == len(base)
        for k, (a, b) in enumerate(zip(base, outs)):
            assert a.shape == b.shape and a.dtype == b.dtype
            assert torch.equal(AB.bits(a), AB.bits(b)), f"pattern {pid}: output {k} depends on the address of an argument"


# ---------------------------------------------------------------- s3r_conv_pack_weights + s3r_conv_forward
def _conv(s3r, lib, case, body):
    stem = BC._stem(case.layer)
    sixteen = AC.exception_names("s3r_conv_forward", stem)
    first = (lambda: body(refuse_render_at=(4, 8))) if stem else None     # the exception list's row, asserted on the device
    across_patterns(body, sixteen, case.dtype == "bf16", first)


@pytest.mark.parametrize("case", AC.EXACT_CONV, ids=[c.id for c in AC.EXACT_CONV])
def test_conv_forward_exact(s3r, lib, case):
    """one case per kernel and launch form, on the integer lattice: the expected output is the exact fp64 result"""
    x, p, want = _data(case.data)

    def body(**kw):
        got = AB.conv_forward(s3r, lib, case, x, p, **kw).contiguous()
        assert_bits(got, want, case.data, p, case.id)
        return (got,)

    _conv(s3r, lib, case, body)


@pytest.mark.parametrize("case", AC.BOUND_CONV, ids=[c.id for c in AC.BOUND_CONV])
def test_conv_forward_bound(s3r, lib, case):
    """the transcendental activations (ELU / Tanh pass, sigmoid heads): tests/test_buffers_gpu.py's data and bound"""
    _conv(s3r, lib, case, lambda **kw: (AB.conv_forward_ref64(s3r, lib, case, **kw),))


def test_conv_forward_bf16_row_persistent(s3r, lib):
    """the bf16 row-persistent kernel (tile code 40: e2 from 128 images up) equals the plane-reuse kernel (code 22) bit for bit
    (tests/test_bf16_gpu.py::test_rows_kernel_equals_the_plane_kernel_bitwise), wherever its arguments lie"""
    e2 = s3r.arch_spec.ENCODER[1]
    rows, plane = (BC.ConvCase(f"e2-bf16-B128-tile{t}", e2, 112, 128, "bf16", tile=t) for t in (40, 22))
    x, p = AB.random_conv_data(rows)
    want = AB.conv_forward(s3r, lib, plane, x, p)

    def body():
        got = AB.conv_forward(s3r, lib, rows, x, p)
        assert torch.equal(AB.bits(got), AB.bits(want)), "the row-persistent kernel differs from the plane-reuse kernel"
        return (got,)

    across_patterns(body, bf16_call=True)


def test_a_shifted_input_is_a_mismatch(s3r, lib):
    """the harness's self-check: the input moved by ONE element against its reference - what a load that dropped low address bits
    would fetch - must fail the reference assertion, under a skew pattern as at skew 0; the untouched input passes"""
    case = next(c for c in AC.EXACT_CONV if c.id == "tile1-vec0-conv3d_s1_w8")
    x, p, want = _data(case.data)
    shifted = torch.roll(x.reshape(-1), 1).reshape(x.shape)
    assert not torch.equal(shifted, x)
    for pid in ("aligned", "all1"):
        with G.skews(AC.Pattern(pid)):
            assert_bits(AB.conv_forward(s3r, lib, case, x, p).contiguous(), want, case.data, p, case.id)
            got = AB.conv_forward(s3r, lib, case, shifted, p).contiguous()
        with pytest.raises(AssertionError, match="elements differ"):
            assert_bits(got, want, case.data, p, case.id)


# ---------------------------------------------------------------- chains and the network's stage entries
@pytest.mark.parametrize("pair", AC.CHAIN_PAIRS, ids=[n for n, _, _ in AC.CHAIN_PAIRS])
def test_chain_forward(s3r, lib, pair):
    """one chain per hand-off kind; ws NaN / zero, ws_fresh 1 then 0, as tests/test_buffers_gpu.py; the skewed ws moves every
    intermediate and every internal scratch off its 256-byte grid"""
    across_patterns(lambda: AB.chain_forward(s3r, lib, pair))


@pytest.mark.parametrize("case", X.CHAIN_CASES, ids=[c.id for c in X.CHAIN_CASES])
def test_chain_forward_exact(s3r, lib, case):
    """tests/test_exact_gpu.py::test_chain_handoff on guarded, skewed arguments, bit for bit against fp64: the stem writing e2's
    transformed planes (s3r_chain_forward's render pointer: the exception list's row, refused at 4 and 8 bytes, launched at 16 and
    144) and the bf16 chain d3 + head in one launch (bf16 x at 16 / 144 bytes, the workspace at 4 / 36 floats)"""
    bf = case.dtype == "bf16"
    x, ps = case.make()
    x = x.to(DEV)
    ps = [{k: None if v is None else v.to(DEV).contiguous() for k, v in p.items()} for p in ps]
    want = LT.expected(case.second.layer, case.intermediate(x, ps[0]), ps[1])
    B = case.first.B
    xin = x.to(torch.bfloat16).permute(0, *range(2, x.dim()), 1).contiguous() if bf else x.contiguous()
    stem = BC._stem(case.first.layer)

    def body(refuse=()):
        arr = (s3r._lib.Layer * 2)()
        keep = []
        for i, (d, p) in enumerate(zip((case.first, case.second), ps)):
            desc = s3r._lib.make_desc(d.layer, B, d.n_in, tag=i, dtype=s3r._lib.DTYPE[case.dtype])
            pk, wb = pack(lib, s3r, desc, p["w"], f"packed{i}")
            sc = None if p["scale"] is None else G.Guarded(f"scale{i}", d.layer.cout, torch.float32, DEV, "in", data=p["scale"])
            sh = G.Guarded(f"shift{i}", d.layer.cout, torch.float32, DEV, "in", data=p["shift"])
            arr[i].desc, arr[i].packed_w = desc, pk.t.data_ptr()
            arr[i].scale, arr[i].shift = (sc.ptr if sc else None), sh.ptr
            keep += [pk, wb, sh] + ([sc] if sc else [])
        need = lib.s3r_chain_workspace_elems(arr, 2)
        assert need > 0, lib.s3r_last_error()
        xb = G.Guarded("x", xin.shape, xin.dtype, DEV, "in", data=xin)
        outs = []
        for fill in ("nan", "zero"):
            y = G.Guarded("y", want.shape, torch.float32, DEV, "out")
            ws = G.Guarded("ws", need, torch.float32, DEV, "scratch", fill=fill)
            for off in refuse:
                before = AB.bits(y.t).clone()
                assert lib.s3r_chain_forward(arr, 2, xb.ptr + off, y.ptr, ws.ptr, need, 1, None) == -1
                assert b"16-byte aligned" in lib.s3r_last_error() and torch.equal(AB.bits(y.t), before)
            rc_ok(lib, lib.s3r_chain_forward(arr, 2, xb.ptr, y.ptr, ws.ptr, need, 1, None), case.id)
            sync()
            G.check_all(xb, y, ws, *keep)
            outs.append(y.t.clone())
        assert torch.equal(AB.bits(outs[0]), AB.bits(outs[1])), "the result depends on the workspace contents"
        assert_bits(outs[0], want, case.second, ps[1], case.id)
        return (outs[0],)

    refuse = (4, 8) if stem else ((2, 4, 8) if bf else ())
    across_patterns(body, AC.exception_names("s3r_chain_forward", stem), bf, first=lambda: body(refuse))


@pytest.mark.parametrize("B,precision,u8", [(1, "fp32", False), (3, "fp32", True), (1, "bf16", True), (3, "bf16", False)],
                         ids=["B1-fp32-f32", "B3-fp32-u8", "B1-bf16-u8", "B3-bf16-f32"])
def test_encoder_forward(s3r, lib, B, precision, u8):
    entry = "s3r_encoder_forward_u8" if u8 else "s3r_encoder_forward"
    across_patterns(lambda: (AB.encoder_forward(s3r, lib, B, precision, u8, fresh=(1, 0)),), AC.exception_names(entry),
                    precision == "bf16")


@pytest.mark.parametrize("B,precision,in_halo", [(1, "fp32", 0), (3, "fp32", 1), (1, "bf16", 1), (3, "bf16", 0)],
                         ids=["B1-fp32-h0", "B3-fp32-h1", "B1-bf16-h1", "B3-bf16-h0"])
def test_decoder_forward(s3r, lib, B, precision, in_halo):
    across_patterns(lambda: (AB.decoder_forward(s3r, lib, B, precision, in_halo, fresh=(1, 0)),), bf16_call=precision == "bf16")


# ---------------------------------------------------------------- cost volume, linear
@pytest.mark.parametrize("shape,oh", AC.CV_CASES, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else f"oh{v}")
def test_cost_volume(s3r, lib, oracle, shape, oh):
    across_patterns(lambda: (AB.cost_volume(s3r, lib, oracle, shape, oh),))


@pytest.mark.parametrize("shape,oh", AC.CV_BF16_CASES, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else f"oh{v}")
def test_cost_volume_bf16(s3r, lib, oracle, shape, oh):
    across_patterns(lambda: (AB.cost_volume_bf16(s3r, lib, oracle, shape, oh),), bf16_call=True)


@pytest.mark.parametrize("shape,kind", AC.CV_PLANE_CASES, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else v)
def test_cost_volume_planes(s3r, lib, shape, kind):
    across_patterns(lambda: (AB.cost_volume_planes(s3r, lib, shape, kind),))


@pytest.mark.parametrize("shape,act", AC.LINEAR_CASES, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else v)
def test_linear_forward(s3r, lib, shape, act):
    """(the split-K scratch skewed with the rest)"""
    across_patterns(lambda: (AB.linear_forward(s3r, lib, shape, act),))


# ---------------------------------------------------------------- Chamfer, IoU, disparity, channels-last hand-off
@pytest.mark.parametrize("n,m", AC.CHAMFER_SIZES)
def test_chamfer_forward(s3r, lib, oracle, n, m):
    across_patterns(lambda: AB.chamfer_forward(s3r, lib, oracle, n, m))


@pytest.mark.parametrize("shape", AC.IOU_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_voxel_iou(s3r, lib, oracle, shape):
    across_patterns(lambda: (AB.voxel_iou(s3r, lib, oracle, shape),))


@pytest.mark.parametrize("shape", AC.WTA_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_disparity_wta(s3r, lib, oracle, shape):
    across_patterns(lambda: AB.disparity_wta(s3r, lib, oracle, shape))


@pytest.mark.parametrize("shape", AC.EPE_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_disparity_epe(s3r, lib, oracle, shape):
    across_patterns(lambda: AB.disparity_epe(s3r, lib, oracle, shape))


@pytest.mark.parametrize("shape", AC.METRICS_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_disparity_metrics(s3r, lib, shape):
    pred, gt = AB.metric_case(*shape)
    across_patterns(lambda: AB.disparity_metrics(s3r, lib, pred, gt))


@pytest.mark.parametrize("case", AC.SOFT_CASES, ids=[c[0] for c in AC.SOFT_CASES])
def test_disparity_soft(s3r, lib, case):
    """fp32 features at 4 bytes, bf16 ones at 16 and 144; with and without upsampling; NULL confidence maps mixed in"""
    across_patterns(lambda: AB.disparity_soft(s3r, lib, case), bf16_call=case[1] == AB.BF16)


@pytest.mark.parametrize("shape", AC.CL_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_channels_last_to_f32(s3r, lib, shape):
    across_patterns(lambda: (AB.channels_last_to_f32(s3r, lib, shape),), bf16_call=True)


# ---------------------------------------------------------------- through the modules: torch views at storage offset 1
def off1(t):
    """t's values in a view that starts ONE element into a larger buffer (tests/test_ingest_soak_gpu.py's construction): 4 bytes off
    for fp32, 2 for bf16, 1 for 8-bit"""
    t = t.to(DEV)
    buf = torch.zeros(t.numel() + 1, dtype=t.dtype, device=DEV)
    buf[1:].copy_(t.contiguous().flatten())
    v = buf[1:].view(t.shape)
    assert v.storage_offset() == 1 and v.data_ptr() % 16 == t.element_size()
    return v


def off1_cl(t):
    """the same for a logical (B, C, ...) bf16 tensor in channels-last memory (what the bf16 modules hand each other)"""
    nd = t.dim()
    phys = off1(t.permute(0, *range(2, nd), 1).contiguous())
    return phys.permute(0, nd - 1, *range(1, nd - 1))


def same_bits(f, views):
    """f on the offset views and on their clones (fresh, aligned allocations): the same bits"""
    got, want = f(*views), f(*[v.clone(memory_format=torch.preserve_format) for v in views])
    got, want = (r if isinstance(r, (tuple, list)) else (r,) for r in (got, want))
    assert len(got) == len(want) and len(got) > 0
    for a, b in zip(got, want):
        assert a.shape == b.shape and a.dtype == b.dtype and torch.equal(AB.bits(a), AB.bits(b))


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_modules_take_views_at_storage_offset_1(s3r, precision):
    bf = precision == "bf16"
    g = torch.Generator().manual_seed(3)
    enc, dec, cv = s3r.Encoder(precision=precision), s3r.Decoder(precision=precision), s3r.CostVolume(precision=precision)
    s3r.seed_module(enc, 3)
    s3r.seed_module(dec, 4)
    enc.to(DEV), dec.to(DEV)
    left8, right8 = (torch.randint(0, 256, (2, 3, 224, 224), generator=g, dtype=torch.uint8) for _ in range(2))
    for l, r in ((left8, right8), (left8.float() / 255.0, right8.float() / 255.0)):      # renders: copied once by the module
        same_bits(enc.forward_pair, (off1(l), off1(r)))
    same_bits(enc, (off1(left8.float() / 255.0),))
    feats = enc.forward_pair(left8.to(DEV), right8.to(DEV))
    view = off1_cl if bf else off1
    fl, fr = view(feats[:2]), view(feats[2:])
    same_bits(cv, (fl, fr))
    same_bits(lambda a, b: cv.forward_padded(a, b).clone(), (fl, fr))
    vol = cv(feats[:2], feats[2:])
    same_bits(dec, (view(vol),))
    same_bits(lambda a, b: s3r.disparity_soft(a, b, 28, 0.7, out_size=(224, 224), scale=8.0, confidence=True), (fl, fr))
    same_bits(lambda a, b: s3r.disparity_soft(a, b, 28, 0.7), (fl, fr))
    if bf:
        same_bits(s3r.modules.channels_last_to_f32, (fl,))
        same_bits(s3r.modules.channels_last_to_f32, (view(vol),))
    else:
        same_bits(lambda a, b: s3r.disparity_wta(a, b, 28), (fl, fr))
        same_bits(lambda a, b: cv.forward_wino(a, b).clone(), (fl, fr))
        same_bits(lambda a, b: cv.forward_wino2(a, b).clone(), (fl, fr))


def test_functions_take_views_at_storage_offset_1(s3r):
    g = torch.Generator().manual_seed(9)
    head = s3r.PointHead()
    s3r.seed_module(head, 5)
    head.to(DEV)
    latent = torch.randn(3, s3r.arch_spec.LATENT_C, 4, 4, 4, generator=g)
    same_bits(head, (off1(latent),))
    same_bits(head, (off1(latent)[1:],))                          # a linear layer on latent[1:]
    clouds = torch.rand(3, 1025, 3, generator=g).to(DEV), torch.rand(3, 2048, 3, generator=g).to(DEV)
    same_bits(s3r.chamfer_distance, (clouds[0][1:], clouds[1][1:]))      # sliced at a sample: 3075 floats in
    same_bits(s3r.chamfer_distance, (off1(clouds[0]), off1(clouds[1])))
    a, b = torch.rand(4, 4097, generator=g), torch.rand(4, 4097, generator=g)
    same_bits(s3r.voxel_iou, (off1(a)[1:], off1(b)[1:]))                 # a sliced batch with an odd voxel count
    pred, gt = AB.metric_case(5, 1001)
    same_bits(s3r.disparity_epe, (off1(pred)[1:], off1(gt)[1:]))
    same_bits(s3r.disparity_metrics, (off1(pred)[1:], off1(gt)[1:]))
    fl, fr = torch.randn(2, 5, 7, 13, generator=g), torch.randn(2, 5, 7, 13, generator=g)
    same_bits(lambda x, y: s3r.disparity_wta(x, y, 4), (off1(fl), off1(fr)))
    same_bits(lambda x, y: s3r.disparity_soft(x, y, 4, 0.5, out_size=(37, 100), scale=2.5, confidence=True), (off1(fl), off1(fr)))
