"""The call bodies of tests/test_buffers_gpu.py, shared with tests/test_alignment_gpu.py.

One function per C-ABI entry point: it puts every argument into a guarded allocation (tests/_guard.py), makes the call, checks the
guards of every argument (`G.check_all`), asserts the entry's reference — the per-element fp64 bound of tests/_ref64.py at HALF, or
bit equality with the oracle — and returns the output tensors it compared (clones), so that a caller can compare the bits of two
runs.  The guarded allocations take their skews from an enclosing `with G.skews(...)` (none: every payload 256-byte aligned, which
is how tests/test_buffers_gpu.py runs them); a body never looks at an address itself.
"""
import ctypes as C
import zlib

import numpy as np
import torch

from tests import _buffer_cases as BC
from tests import _guard as G
from tests import _ref64 as R
from tests._abi_calls import DEV, interior as _interior, pack as _pack, pad as _pad, rc_ok as _rc, sync as _sync

HALF = 0.5
F32, BF16 = 0, 1


def check_values(layer, form, got, ref, mag, what):
    bnd = R.bound(layer, ref, mag, form)
    ratio, i = R.worst(got, ref, bnd)
    print(f"\nratio {form} {ratio:.3e} {what}")
    assert ratio <= HALF, (what, form, ratio, i, float(got.reshape(-1)[i]), float(ref.reshape(-1)[i]), float(bnd.reshape(-1)[i]))


def bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


# ---------------------------------------------------------------- s3r_conv_pack_weights + s3r_conv_forward
def random_conv_data(case):
    """the data tests/test_buffers_gpu.py::test_conv_forward gives a case: (x, params), rounded to bf16 where the bf16 path reads bf16"""
    l, nd, bf = case.layer, R.ndim(case.layer), case.dtype == "bf16"
    stem, head = BC._stem(l), BC._head(l, case.n_in)
    p = R.make_params(l, zlib.crc32(case.id.encode()) % 1000, DEV)
    if bf and not stem and not head:                      # the MFMA layers of the bf16 path see bf16 weights
        p["w"] = p["w"].to(torch.bfloat16).float()
    g = torch.Generator().manual_seed(len(case.id))
    x = torch.randn((case.B, l.cin) + (case.n_in,) * nd, generator=g).to(DEV)
    if bf and not stem:
        x = x.to(torch.bfloat16).float()
    return x, p


def conv_forward(s3r, lib, case, x, p, refuse_render_at=()):
    """`case` (a tests/_buffer_cases.py::ConvCase or a tests/_exact_cases.py::XCase) on the logical input x and the parameters p,
    over NaN-filled and over zero-filled scratch: guards, the same bits from both, and the interior of y as a logical (B, cout, ...)
    tensor (bf16 on the channels-last path).  refuse_render_at: byte offsets at which the stem's render pointer must be refused
    (S3R_ERR_INVALID, "16-byte aligned", y untouched) before the call proper is made"""
    l, nd, bf = case.layer, R.ndim(case.layer), case.dtype == "bf16"
    stem = BC._stem(l)
    head = BC._head(l, case.n_in)
    ih = case.in_halo if case.in_halo >= 0 else BC.need_halo(l, case.n_in, case.dtype)
    desc = s3r._lib.make_desc(l, case.B, case.n_in, tile=case.tile, in_halo=ih, out_halo=case.out_halo, ksplit=case.ksplit,
                              dtype=s3r._lib.DTYPE[case.dtype], algo=case.algo)
    pk, wb = _pack(lib, s3r, desc, p["w"])
    cl_in, cl_out = bf and not stem, bf and not head
    xp, _ = _pad(x.to(torch.bfloat16) if cl_in else x, ih, cl_in)
    xb = G.Guarded("x", xp.shape, xp.dtype, DEV, "in", data=xp)
    sc = None if p["scale"] is None else G.Guarded("scale", l.cout, torch.float32, DEV, "in", data=p["scale"])
    sh = G.Guarded("shift", l.cout, torch.float32, DEV, "in", data=p["shift"])
    n_out = s3r._lib.load().s3r_conv_out_size(C.byref(desc))
    oh = case.out_halo
    ysp = (n_out + 2 * oh,) * nd
    yshape = (case.B,) + ysp + (l.cout,) if cl_out else (case.B, l.cout) + ysp
    sp = tuple(range(1, 1 + nd)) if cl_out else tuple(range(2, 2 + nd))
    ydt = torch.bfloat16 if cl_out else torch.float32
    need = lib.s3r_conv_scratch_elems(C.byref(desc))
    assert need >= 0, lib.s3r_last_error()
    outs = []
    for fill in ("nan", "zero"):
        y = G.Guarded("y", yshape, ydt, DEV, "out", halo=oh, spatial=sp, halo_zeros=BC.zero_halo_writer(case))
        scr = G.Guarded("scratch", need, torch.float32, DEV, "scratch", fill=fill)
        for off in refuse_render_at:
            before = bits(y.t).clone()
            rc = lib.s3r_conv_forward(C.byref(desc), xb.ptr + off, pk.t.data_ptr(), sc.ptr if sc else None, sh.ptr, y.ptr, scr.ptr, need, None)
            _sync()
            assert rc == -1 and b"16-byte aligned" in lib.s3r_last_error(), (case.id, off, rc, lib.s3r_last_error())
            assert torch.equal(bits(y.t), before), "a refused call wrote its output"
        _rc(lib, lib.s3r_conv_forward(C.byref(desc), xb.ptr, pk.t.data_ptr(), sc.ptr if sc else None, sh.ptr, y.ptr, scr.ptr, need, None),
            case.id)
        _sync()
        G.check_all(xb, wb, pk, sh, y, scr, *([sc] if sc else []))
        outs.append(y.t.clone())
    assert torch.equal(outs[0].view(torch.int16 if cl_out else torch.int32), outs[1].view(torch.int16 if cl_out else torch.int32)), \
        "the result depends on the scratch contents"
    return _interior(outs[0], oh, sp, cl_out)


def conv_forward_ref64(s3r, lib, case, **kw):
    """tests/test_buffers_gpu.py::test_conv_forward: random data, every element within HALF its fp64 bound"""
    x, p = random_conv_data(case)
    got = conv_forward(s3r, lib, case, x, p, **kw)
    ref, mag = R.ref64(case.layer, x, p)
    check_values(case.layer, case.form, got.float(), ref, mag, case.id)
    return got


# ---------------------------------------------------------------- s3r_chain_forward: the composition matrix
def chain_case(s3r, lib, parts, B, out_halo):
    layers = [q.layer for q in parts]
    params = [R.make_params(q.layer, 31 + i, DEV) for i, q in enumerate(parts)]
    arr = (s3r._lib.Layer * len(parts))()
    keep = []
    for i, q in enumerate(parts):
        d = s3r._lib.make_desc(q.layer, B, q.n_in, tag=i, algo=q.algo, tile=q.tile,
                               out_halo=out_halo if i == len(parts) - 1 else 0)
        pk, wb = _pack(lib, s3r, d, params[i]["w"], f"packed{i}")
        sc = None if params[i]["scale"] is None else G.Guarded(f"scale{i}", q.layer.cout, torch.float32, DEV, "in", data=params[i]["scale"])
        sh = G.Guarded(f"shift{i}", q.layer.cout, torch.float32, DEV, "in", data=params[i]["shift"])
        arr[i].desc, arr[i].packed_w = d, pk.t.data_ptr()
        arr[i].scale, arr[i].shift = (sc.ptr if sc else None), sh.ptr
        keep += [pk, wb, sh] + ([sc] if sc else [])
    return layers, params, arr, keep


def chain_forward(s3r, lib, pair):
    """one (name, producer, consumer) of BC.CHAIN_PAIRS: workspace NaN / zero, ws_fresh 1 then 0; (y of input 0, y of input 1)"""
    name, p, c = pair
    B = 2
    last = c.layer
    oh = 0 if last.op == "linear" or BC._head(last, c.n_in) else 1
    layers, params, arr, keep = chain_case(s3r, lib, [p, c], B, oh)
    need = lib.s3r_chain_workspace_elems(arr, 2)
    assert need > 0, lib.s3r_last_error()
    nd0 = R.ndim(p.layer)
    g = torch.Generator().manual_seed(5)
    xs = [torch.randn((B, p.layer.cin) + (p.n_in,) * nd0, generator=g).to(DEV) for _ in range(2)]
    n_out = s3r._lib.load().s3r_conv_out_size(C.byref(arr[1].desc))
    nd1 = R.ndim(last)
    yshape = (B, last.cout) if last.op == "linear" else (B, last.cout) + (n_out + 2 * oh,) * nd1
    sp = tuple(range(2, 2 + nd1))
    zeros = BC.zero_halo_writer(BC.ConvCase("", last, c.n_in, B, algo=c.algo, tile=c.tile))

    def run(x, ws, fresh):
        xb = G.Guarded("x", x.shape, torch.float32, DEV, "in", data=x)
        y = G.Guarded("y", yshape, torch.float32, DEV, "out", halo=oh, spatial=sp, halo_zeros=zeros)
        _rc(lib, lib.s3r_chain_forward(arr, 2, xb.ptr, y.ptr, ws.ptr, need, fresh, None), name)
        _sync()
        G.check_all(xb, y, ws, *keep)
        return y.t.clone()

    ws = G.Guarded("ws", need, torch.float32, DEV, "scratch", fill="nan")
    y1 = run(xs[0], ws, 1)
    y1z = run(xs[0], G.Guarded("ws", need, torch.float32, DEV, "scratch", fill="zero"), 1)
    assert torch.equal(y1.view(torch.int32), y1z.view(torch.int32)), "the result depends on the workspace contents"
    y2 = run(xs[1], ws, 0)                                   # the same arena, not re-zeroed
    y2f = run(xs[1], G.Guarded("ws", need, torch.float32, DEV, "scratch", fill="nan"), 1)
    assert torch.equal(y2.view(torch.int32), y2f.view(torch.int32)), "stale bytes across calls (ws_fresh = 0)"
    forms = ["wino" if BC.has_wino(BC.ConvCase("", q.layer, q.n_in, B, algo=q.algo, tile=q.tile)) else "direct" for q in (p, c)]
    ref, bnd = R.chain_ref64(layers, forms, xs[0], params)
    got = y1 if last.op == "linear" else _interior(y1, oh, sp, False)
    ratio, i = R.worst(got, ref, bnd)
    print(f"\nratio chain {ratio:.3e} {name}")
    assert ratio <= HALF, (name, forms, ratio, i)
    return got.clone(), (y2 if last.op == "linear" else _interior(y2, oh, sp, False)).clone()


# ---------------------------------------------------------------- the network's stage entries
def encoder_forward(s3r, lib, B, precision, u8, fresh=(1,)):
    """the encoder entry against the module on the same renders; one call per entry of `fresh` (ws_fresh) into the same workspace"""
    enc = s3r.Encoder(precision=precision)
    s3r.seed_module(enc, 3)
    enc.to(DEV)
    g = torch.Generator().manual_seed(B)
    left8, right8 = (torch.randint(0, 256, (B, 3, 224, 224), generator=g, dtype=torch.uint8) for _ in range(2))
    left, right = (t.float() / 255.0 for t in (left8, right8))
    want = enc.forward_pair(left.to(DEV), right.to(DEV))
    arr, n = enc._layer_array(2 * B, torch.device(DEV))
    need = lib.s3r_chain_workspace_elems(arr, n)
    src = (left8, right8) if u8 else (left, right)
    lb = G.Guarded("left", src[0].shape, src[0].dtype, DEV, "in", data=src[0].to(DEV))
    rb = G.Guarded("right", src[1].shape, src[1].dtype, DEV, "in", data=src[1].to(DEV))
    bf = precision == "bf16"
    fshape = (2 * B, 28, 28, 32) if bf else (2 * B, 32, 28, 28)
    ws = G.Guarded("ws", need, torch.float32, DEV, "scratch")
    fn = lib.s3r_encoder_forward_u8 if u8 else lib.s3r_encoder_forward
    out = None
    for f in fresh:
        feat = G.Guarded("features", fshape, torch.bfloat16 if bf else torch.float32, DEV, "out")
        _rc(lib, fn(arr, n, lb.ptr, rb.ptr, feat.ptr, ws.ptr, need, f, None), "encoder")
        _sync()
        G.check_all(lb, rb, feat, ws)
        got = feat.t.permute(0, 3, 1, 2) if bf else feat.t
        assert torch.equal(got.float(), want.float()), "the entry differs from the module on the same renders"
        out = feat.t.clone()
    return out


def decoder_forward(s3r, lib, B, precision, in_halo, fresh=(1,)):
    dec = s3r.Decoder(precision=precision)
    s3r.seed_module(dec, 4)
    dec.to(DEV)
    bf = precision == "bf16"
    vol = torch.randn((B, 64, 28, 28, 28), generator=torch.Generator().manual_seed(B), device="cpu").to(DEV)
    if bf:
        vol = vol.to(torch.bfloat16).float()
    want = dec(vol.permute(0, 2, 3, 4, 1).contiguous().to(torch.bfloat16).permute(0, 4, 1, 2, 3) if bf else vol)
    arr, n = dec._layer_array(B, torch.device(DEV), in_halo=in_halo)
    need = lib.s3r_chain_workspace_elems(arr, n)
    vp, _ = _pad(vol.to(torch.bfloat16) if bf else vol, in_halo, bf)
    vb = G.Guarded("volume", vp.shape, vp.dtype, DEV, "in", data=vp)
    ws = G.Guarded("ws", need, torch.float32, DEV, "scratch")
    out = None
    for f in fresh:
        occ = G.Guarded("occupancy", (B, 1, 32, 32, 32), torch.float32, DEV, "out")
        _rc(lib, lib.s3r_decoder_forward(arr, n, vb.ptr, occ.ptr, ws.ptr, need, f, None), "decoder")
        _sync()
        G.check_all(vb, occ, ws)
        assert torch.equal(occ.t.reshape(want.shape), want), "the entry differs from the module on the same volume"
        out = occ.t.clone()
    return out


# ---------------------------------------------------------------- cost volume
def feats(shape, seed=11):
    B, Cc, D, H, W = shape
    g = torch.Generator().manual_seed(seed)
    return torch.randn(B, Cc, H, W, generator=g), torch.randn(B, Cc, H, W, generator=g)


def cost_volume(s3r, lib, oracle, shape, oh):
    B, Cc, D, H, W = shape
    fl, fr = feats(shape)
    want = oracle.cost_volume(fl, fr, D)
    a = G.Guarded("left", fl.shape, torch.float32, DEV, "in", data=fl.to(DEV))
    b = G.Guarded("right", fr.shape, torch.float32, DEV, "in", data=fr.to(DEV))
    # (the plain volume's kernel stores whole padded planes d = halo .. halo + D - 1, their halo rows as +0.0: include/s3r.h)
    v = G.Guarded("volume", (B, 2 * Cc, D + 2 * oh, H + 2 * oh, W + 2 * oh), torch.float32, DEV, "out", halo=oh, spatial=(2, 3, 4),
                  halo_zeros=True)
    _rc(lib, lib.s3r_cost_volume_forward(a.ptr, b.ptr, v.ptr, B, Cc, D, H, W, oh, None), "cost_volume")
    _sync()
    G.check_all(a, b, v)
    assert torch.equal(_interior(v.t, oh, (2, 3, 4), False).cpu(), want)
    return v.t.clone()


def cost_volume_bf16(s3r, lib, oracle, shape, oh):
    B, Cc, D, H, W = shape
    fl, fr = (t.to(torch.bfloat16).float() for t in feats(shape, 2))
    want = oracle.cost_volume(fl, fr, D).to(torch.bfloat16)
    a = G.Guarded("left", (B, H, W, Cc), torch.bfloat16, DEV, "in", data=fl.permute(0, 2, 3, 1).to(DEV).to(torch.bfloat16))
    b = G.Guarded("right", (B, H, W, Cc), torch.bfloat16, DEV, "in", data=fr.permute(0, 2, 3, 1).to(DEV).to(torch.bfloat16))
    v = G.Guarded("volume", (B, D + 2 * oh, H + 2 * oh, W + 2 * oh, 2 * Cc), torch.bfloat16, DEV, "out", halo=oh, spatial=(1, 2, 3))
    _rc(lib, lib.s3r_cost_volume_forward_bf16(a.ptr, b.ptr, v.ptr, B, Cc, D, H, W, oh, None), "cost_volume_bf16")
    _sync()
    G.check_all(a, b, v)
    assert torch.equal(_interior(v.t, oh, (1, 2, 3), True).cpu(), want)
    return v.t.clone()


def cost_volume_planes(s3r, lib, shape, kind):
    """plane layouts: guards, and the same bits as the call into a plain zero-initialised buffer"""
    B, Cc, D, H, W = shape
    fl, fr = feats(shape, 7)
    if kind == "wino":
        n = 6 * B * 2 * Cc * (D + 2) * (H // 4) * (W + 2)
        fn = lib.s3r_cost_volume_forward_wino
    else:
        n = 36 * B * 2 * Cc * (D // 4) * (H // 4) * (W + 2)
        fn = lib.s3r_cost_volume_forward_wino2
    a = G.Guarded("left", fl.shape, torch.float32, DEV, "in", data=fl.to(DEV))
    b = G.Guarded("right", fr.shape, torch.float32, DEV, "in", data=fr.to(DEV))
    planes = G.Guarded("planes", n, torch.float32, DEV, "scratch", fill="zero")
    plain = torch.zeros(n, device=DEV)
    _rc(lib, fn(a.ptr, b.ptr, planes.ptr, B, Cc, D, H, W, None), kind)
    _rc(lib, fn(a.ptr, b.ptr, plain.data_ptr(), B, Cc, D, H, W, None), kind)
    _sync()
    G.check_all(a, b, planes)
    assert torch.equal(planes.t.view(torch.int32), plain.view(torch.int32))
    return planes.t.clone()


# ---------------------------------------------------------------- linear
def linear_forward(s3r, lib, shape, act, bias=True):
    """bias=False: the call is made with bias = NULL (include/s3r.h: NULL = 0) and held to the reference without a shift"""
    B, cin, cout = shape
    l = s3r.arch_spec.Layer("t", "linear", cin, cout, 1, 1, 0, False, act)
    p = R.make_params(l, cin + cout, DEV)
    if not bias:
        p["shift"] = None
    x = torch.randn(B, cin, generator=torch.Generator().manual_seed(B)).to(DEV)
    xb = G.Guarded("x", x.shape, torch.float32, DEV, "in", data=x)
    wb = G.Guarded("w", p["w"].shape, torch.float32, DEV, "in", data=p["w"])
    bb = G.Guarded("bias", cout, torch.float32, DEV, "in", data=p["shift"]) if bias else None
    need = lib.s3r_linear_scratch_elems(B, cin, cout)
    outs = []
    for fill in ("nan", "zero"):
        y = G.Guarded("y", (B, cout), torch.float32, DEV, "out")
        scr = G.Guarded("scratch", need, torch.float32, DEV, "scratch", fill=fill)
        _rc(lib, lib.s3r_linear_forward(xb.ptr, wb.ptr, bb.ptr if bias else None, y.ptr, B, cin, cout, s3r._lib.ACT[act], scr.ptr, need,
                                        None), "linear")
        _sync()
        G.check_all(xb, wb, y, scr, *([bb] if bias else []))
        outs.append(y.t.clone())
    assert torch.equal(outs[0].view(torch.int32), outs[1].view(torch.int32))
    ref, mag = R.ref64(l, x, p)
    check_values(l, "direct", outs[0], ref, mag, shape)
    return outs[0]


def linear_descriptor(s3r, lib, shape, act):
    """the same layer as an S3R_OP_LINEAR descriptor through s3r_conv_pack_weights + s3r_conv_forward, with a folded BatchNorm: the
    one route on which the linear kernels' scale[o] branch holds a vector"""
    B, cin, cout = shape
    l = s3r.arch_spec.Layer("t", "linear", cin, cout, 1, 1, 0, True, act)
    return conv_forward_ref64(s3r, lib, BC.ConvCase("linear-desc-" + "x".join(map(str, shape)) + "-" + act, l, 1, B))


# ---------------------------------------------------------------- Chamfer, IoU, disparity, channels-last hand-off
def chamfer_forward(s3r, lib, oracle, n, m):
    B = 2
    g = torch.Generator().manual_seed(n * 7 + m)
    p, q = torch.rand(B, n, 3, generator=g), torch.rand(B, m, 3, generator=g)
    want = oracle.chamfer_distance(p, q)
    pb = G.Guarded("p", p.shape, torch.float32, DEV, "in", data=p.to(DEV))
    qb = G.Guarded("q", q.shape, torch.float32, DEV, "in", data=q.to(DEV))
    d1, d2 = G.Guarded("dist1", (B, n), torch.float32, DEV, "out"), G.Guarded("dist2", (B, m), torch.float32, DEV, "out")
    i1, i2 = G.Guarded("idx1", (B, n), torch.int32, DEV, "out"), G.Guarded("idx2", (B, m), torch.int32, DEV, "out")
    _rc(lib, lib.s3r_chamfer_forward(pb.ptr, qb.ptr, d1.ptr, d2.ptr, i1.ptr, i2.ptr, B, n, m, None), "chamfer")
    _sync()
    G.check_all(pb, qb, d1, d2, i1, i2)
    for got, w in zip((d1.t, d2.t, i1.t, i2.t), want):
        assert torch.equal(got.cpu(), w)
    return d1.t.clone(), d2.t.clone(), i1.t.clone(), i2.t.clone()


def voxel_iou(s3r, lib, oracle, shape):
    B, V = shape
    g = torch.Generator().manual_seed(V)
    a, b = torch.rand(B, V, generator=g), torch.rand(B, V, generator=g)
    want = oracle.voxel_iou(a, b, 0.5)
    ab = G.Guarded("pred", a.shape, torch.float32, DEV, "in", data=a.to(DEV))
    bb = G.Guarded("gt", b.shape, torch.float32, DEV, "in", data=b.to(DEV))
    out = G.Guarded("iou", B, torch.float32, DEV, "out")
    _rc(lib, lib.s3r_voxel_iou(ab.ptr, bb.ptr, 0.5, out.ptr, B, V, None), "iou")
    _sync()
    G.check_all(ab, bb, out)
    assert torch.equal(out.t.cpu(), want)
    return out.t.clone()


def disparity_wta(s3r, lib, oracle, shape):
    B, Cc, H, W, D = shape
    g = torch.Generator().manual_seed(W)
    fl, fr = torch.randn(B, Cc, H, W, generator=g), torch.randn(B, Cc, H, W, generator=g)
    want = oracle.disparity_wta(fl, fr, D)
    a = G.Guarded("left", fl.shape, torch.float32, DEV, "in", data=fl.to(DEV))
    b = G.Guarded("right", fr.shape, torch.float32, DEV, "in", data=fr.to(DEV))
    dl, dr = G.Guarded("disp_l", (B, H, W), torch.float32, DEV, "out"), G.Guarded("disp_r", (B, H, W), torch.float32, DEV, "out")
    _rc(lib, lib.s3r_disparity_wta(a.ptr, b.ptr, dl.ptr, dr.ptr, B, Cc, H, W, D, None), "wta")
    _sync()
    G.check_all(a, b, dl, dr)
    assert torch.equal(dl.t.cpu(), want[0]) and torch.equal(dr.t.cpu(), want[1])
    return dl.t.clone(), dr.t.clone()


def disparity_epe(s3r, lib, oracle, shape):
    B, P = shape
    g = torch.Generator().manual_seed(P)
    pred, gt = torch.rand(B, P, generator=g) * 200, torch.rand(B, P, generator=g) * 200
    gt[:, ::3] = float("inf")
    gt[:, 1::5] = -1.0
    want_e, want_n = oracle.disparity_epe(pred, gt)
    pb = G.Guarded("pred", pred.shape, torch.float32, DEV, "in", data=pred.to(DEV))
    gb = G.Guarded("gt", gt.shape, torch.float32, DEV, "in", data=gt.to(DEV))
    e, n = G.Guarded("epe", B, torch.float32, DEV, "out"), G.Guarded("count", B, torch.int32, DEV, "out")
    _rc(lib, lib.s3r_disparity_epe(pb.ptr, gb.ptr, e.ptr, n.ptr, B, P, None), "epe")
    _sync()
    G.check_all(pb, gb, e, n)
    assert torch.equal(n.t.cpu(), want_n)
    assert (e.t.cpu() - want_e).abs().max().item() <= 1e-6 * want_e.abs().max().item()    # fp64 sums, fp32 result
    return e.t.clone(), n.t.clone()


def channels_last_to_f32(s3r, lib, shape):
    B, Cc, P = shape
    x = torch.randn(B, P, Cc, generator=torch.Generator().manual_seed(P)).to(torch.bfloat16)
    xb = G.Guarded("x", x.shape, torch.bfloat16, DEV, "in", data=x.to(DEV))
    y = G.Guarded("y", (B, Cc, P), torch.float32, DEV, "out")
    _rc(lib, lib.s3r_channels_last_to_f32(xb.ptr, y.ptr, B, Cc, P, None), "channels_last_to_f32")
    _sync()
    G.check_all(xb, y)
    assert torch.equal(y.t.cpu(), x.float().permute(0, 2, 1))
    return y.t.clone()


# ---------------------------------------------------------------- sub-pixel read-out and stereo metrics
def soft_feats(shape, seed):
    B, Cc, H, W, _ = shape
    g = torch.Generator().manual_seed(seed)
    return torch.randn(B, Cc, H, W, generator=g), torch.randn(B, Cc, H, W, generator=g)


def cl_bf16(x):
    """fp32 (B,C,H,W) -> logical (B,C,H,W) bf16 in channels-last memory, as the bf16 encoder emits it"""
    return x.to(torch.bfloat16).contiguous(memory_format=torch.channels_last)


def disparity_soft(s3r, lib, case):
    """tests/test_disparity_soft_gpu.py::test_guarded_buffers: the entry on guarded buffers (NULL confidence maps: buffers beside the
    call that nothing may touch) against the module's read-out on the same features, bit for bit"""
    _, dt, shape, (OH, OW), conf = case
    B, Cc, H, W, D = shape
    fl, fr = (t.to(DEV) for t in soft_feats(shape, 23 + sum(shape)))
    if dt == BF16:
        fl, fr = cl_bf16(fl), cl_bf16(fr)
        phys = [x.permute(0, 2, 3, 1) for x in (fl, fr)]
        a = G.Guarded("left", phys[0].shape, torch.bfloat16, DEV, "in", data=phys[0])
        b = G.Guarded("right", phys[1].shape, torch.bfloat16, DEV, "in", data=phys[1])
    else:
        a = G.Guarded("left", fl.shape, torch.float32, DEV, "in", data=fl)
        b = G.Guarded("right", fr.shape, torch.float32, DEV, "in", data=fr)
    outs = [G.Guarded(n, (B, OH, OW), torch.float32, DEV, "out") for n in ("disp_l", "disp_r")]
    if conf:
        outs += [G.Guarded(n, (B, OH, OW), torch.float32, DEV, "out") for n in ("conf_l", "conf_r")]
        cptr = [outs[2].ptr, outs[3].ptr]
    else:                     # NULL confidence: buffers beside the call that nothing may touch
        outs += [G.Guarded(n, (B, OH, OW), torch.float32, DEV, "in", data=torch.full((B, OH, OW), 7.0, device=DEV))
                 for n in ("conf_l", "conf_r")]
        cptr = [None, None]
    rc = lib.s3r_disparity_soft(a.ptr, b.ptr, dt, outs[0].ptr, outs[1].ptr, cptr[0], cptr[1], B, Cc, H, W, D, 0.7, OH, OW,
                                8.0, None)
    assert rc == 0, lib.s3r_last_error().decode()
    torch.cuda.synchronize()
    G.check_all(a, b, *outs)
    want = s3r.disparity_soft(fl, fr, D, 0.7, out_size=(OH, OW), scale=8.0, confidence=True)
    for o, w in zip(outs[:4 if conf else 2], want):
        assert torch.equal(o.t, w)
    return tuple(o.t.clone() for o in outs[:4 if conf else 2])


def metric_case(B=5, P=1000):
    g = torch.Generator().manual_seed(31)
    gt = torch.rand(B, P, generator=g) * 120
    pred = gt + (torch.rand(B, P, generator=g) - 0.5) * 16
    gt[0, ::7] = float("inf")
    gt[1, ::5] = float("nan")
    gt[2, 1::3] = -1.0
    gt[3] = float("inf")                                          # an all-invalid sample
    gt[3, ::2] = -2.0
    gt[4, :3] = torch.tensor([10.0, 10.0, 100.0])                 # errors of exactly 1, 3 and 0.05 gt: not counted
    pred[4, :3] = torch.tensor([11.0, 13.0, 105.0])
    return pred, gt


def disparity_metrics(s3r, lib, pred, gt):
    """tests/test_disparity_soft_gpu.py::test_metrics_match_numpy on (pred, gt): counts equal numpy's, the EPE within 1e-6 of the
    fp64 one and bit-equal to the EPE kernel's"""
    from tests import _disp64 as D64
    pb = G.Guarded("pred", pred.shape, torch.float32, DEV, "in", data=pred.to(DEV))
    gb = G.Guarded("gt", gt.shape, torch.float32, DEV, "in", data=gt.to(DEV))
    e = G.Guarded("epe", pred.shape[0], torch.float32, DEV, "out")
    c = G.Guarded("counts", (pred.shape[0], 4), torch.int32, DEV, "out")
    assert lib.s3r_disparity_metrics(pb.ptr, gb.ptr, e.ptr, c.ptr, pred.shape[0], pred.shape[1], None) == 0
    torch.cuda.synchronize()
    G.check_all(pb, gb, e, c)
    want_e, want_c = D64.metrics(pred.numpy(), gt.numpy())
    assert np.array_equal(c.t.cpu().numpy(), want_c)
    assert (np.abs(e.t.cpu().double().numpy() - want_e) <= 1e-6 * want_e.max()).all()
    epe, cnt = s3r.disparity_epe(pred.to(DEV), gt.to(DEV))
    assert torch.equal(e.t, epe) and torch.equal(c.t[:, 0], cnt)  # the EPE kernel's bits
    return e.t.clone(), c.t.clone()
