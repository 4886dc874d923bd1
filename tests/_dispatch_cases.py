"""The host-side bookkeeping of the forward dispatcher (csrc/s3r_conv_forward.hip, csrc/s3r_plan_*.hip), as tests/golden/dispatch_golden.json
pins it: size answers and scratch refusals (no GPU), and the profiler records of one forward per kernel path (GPU).

Shared by tests/golden/make_dispatch_golden.py (which writes the file) and tests/test_dispatch_golden_{cpu,gpu}.py (which compare
with it).  Data never matters here: every forward runs on zero-filled buffers, packed weights included.
"""
from __future__ import annotations

import ctypes as C
import dataclasses

import s3r
from s3r import arch_spec as spec

from tests import _buffer_cases as BC
from tests import _exact_cases as X
from tests import _linear_cases as LC

L = spec.Layer
P = s3r._lib
REC_INTS = ("family", "tag", "launches", "algo", "launch_form")
REC_DOUBLES = ("flops", "bytes", "exec_flops")
DUMMY = 1 << 20                    # a non-null 16-byte aligned pointer that is never dereferenced: the refusals come before any launch


def desc_of(c, **kw):
    ih = c.in_halo if c.in_halo >= 0 else BC.need_halo(c.layer, c.n_in, c.dtype)
    return P.make_desc(c.layer, c.B, c.n_in, tile=c.tile, in_halo=ih, out_halo=c.out_halo, ksplit=c.ksplit, dtype=P.DTYPE[c.dtype],
                       algo=c.algo, **kw)


def _linear(B, cin, cout, act="none"):
    return BC.ConvCase(f"linear-{B}x{cin}x{cout}-{act}", L("t", "linear", cin, cout, 1, 1, 0, True, act), 1, B)


HOST_CASES = BC.CONV_CASES + [_linear(*shape) for shape in LC.SWEEP]
assert len({c.id for c in HOST_CASES}) == len(HOST_CASES)


# ---------------------------------------------------------------- host only
def sizes(lib, c):
    d = desc_of(c)
    n = C.c_int64(-1)
    rc = lib.s3r_conv_packed_elems(C.byref(d), C.byref(n))
    return dict(out_size=lib.s3r_conv_out_size(C.byref(d)), packed_rc=rc, packed_elems=n.value,
                scratch_elems=lib.s3r_conv_scratch_elems(C.byref(d)), wino_input_elems=lib.s3r_conv_wino_input_elems(C.byref(d)),
                wino_input_layout=lib.s3r_conv_wino_input_layout(C.byref(d)))


def refusals(lib, c):
    """s3r_conv_forward over dummy pointers with scratch = NULL and with one float too few; None: the layer needs no scratch"""
    d = desc_of(c)
    need = lib.s3r_conv_scratch_elems(C.byref(d))
    if need <= 0:
        return None
    out = {}
    for name, scr, n in (("null", None, need), ("short", DUMMY, need - 1)):
        rc = lib.s3r_conv_forward(C.byref(d), DUMMY, DUMMY, DUMMY, DUMMY, DUMMY, scr, n, None)
        out[name] = [rc, lib.s3r_last_error().decode()]
    return out


def host_part(lib):
    return dict(sizes={c.id: sizes(lib, c) for c in HOST_CASES},
                refusals={c.id: r for c in HOST_CASES for r in [refusals(lib, c)] if r is not None})


# ---------------------------------------------------------------- GPU: one forward per branch of the dispatcher
@dataclasses.dataclass(frozen=True)
class Chain:
    id: str
    parts: tuple                   # of (layer, n_in, algo, tile, ksplit)
    B: int
    dtype: str = "fp32"


def _single_cases():
    by_id = {c.id: c for c in BC.CONV_CASES}
    ids = [c.id for c in BC.CONV_CASES if "-B1-oh" in c.id and c.layer.name != "t"]      # every network layer, fp32 and bf16
    ids += ["staged-conv2d-20to33-k5-e9", "dilated-conv2d-32to32-d2-e16",
            "unfolded-conv2d-3to16-k7s2-e33", "unfolded-conv3d-2to24-k4s2-elu-e10", "unfolded-subbatch-conv2d-8to16-k7-e200",
            "d2s-deconv2d-32to24-k3s3-e7", "d2s-deconv2d-16to40-k4s4-sigmoid-e5",
            "tclass-deconv2d-32to33-k4s2-e7", "tclass-noTap-deconv2d-16to16-k2s3-e5", "tclass-staged-deconv3d-8to12-k4s2-e5",
            "tclass-inplace-h1-deconv2d-64to32-k4s2-e16", "tclass-perclass-deconv3d-16to16-k5s4-e3"]
    ids += [f"wino1-{f}-conv2d-32to48-e40" for f in ("serial", "class-parallel", "dual")] + ["wino1-serial-conv3d-64to64-e12"]
    ids += [f"wino2-tile{t}-{tag}" for t in (3, 4, 5) for tag in ("conv2d-64to96-e20", "conv3d-32to64-e12")]
    ids += ["wsd-class-parallel-deconv3d-32to24-e12-B1"] + [f"wino3-tile{t}-deconv3d-64to32-e8" for t in (6, 7, 8)]
    ids += ["tile3-conv3d-64to70-e12", "splitk2-conv3d-64to33-s2-e9", "leaky-splitk2-finish-conv3d-64to32-s2-e9", "tanh-pass-conv2d-32to16-e8"]
    cases = [by_id[i] for i in ids]
    # (the table has the transposed two-axis layer in its class-parallel form only: the same row in the serial one)
    cases.append(dataclasses.replace(by_id["wsd-class-parallel-deconv3d-32to24-e12-B1"], id="wsd-serial-deconv3d-32to24-e12-B1", tile=0))
    # a linear row whose epilogue holds the activation, and one whose activation is a pass behind it
    cases += [_linear(3, 32, 5, "relu"), _linear(9, 33, 100, "tanh")]
    return cases


def _chain_cases():
    out = []
    seen = set()
    for c in X.HEAD_CHAIN_CASES:                  # the fp32 conv + head launch: one row per route
        route = c.id.split("+head-")[0]
        if route in seen:
            continue
        seen.add(route)
        f, h = c.first, c.second
        out.append(Chain(f"fused-{route}", ((f.layer, f.n_in, c.algo, c.tile, 0), (h.layer, h.n_in, 0, -1, 0)), f.B))
    c = next(c for c in X.CHAIN_CASES if c.id == "d3+head-bf16")
    out.append(Chain("fused-d3+head-bf16", ((c.first.layer, c.first.n_in, 0, -1, 0), (c.second.layer, c.second.n_in, 0, -1, 0)), c.first.B, "bf16"))
    # tests/test_handoff3d_gpu.py: (a) a split-K direct layer and (b) a class-parallel two-axis layer writing a two-axis consumer's
    # plane sets, (d) a class-parallel transposed layer writing its consumer's difference tensors
    conv = lambda n, ci, co, **kw: L(n, "conv3d", ci, co, kw.get("k", 3), kw.get("s", 1), kw.get("p", 1))
    dcv = lambda n, ci, co: L(n, "deconv3d", ci, co, 4, 2, 1)
    W = P.ALGO_WINOGRAD
    out += [Chain("handoff-a-64to32-e12-ks4", ((conv("ha", 64, 32, s=2), 12, 0, -1, 4), (conv("hb", 32, 32), 6, 0, -1, 0)), 3),
            Chain("handoff-b-k3-e8", ((conv("ha", 32, 32), 8, W, 4, 0), (conv("hb", 32, 32), 8, 0, -1, 0)), 3),
            Chain("handoff-d-e4", ((dcv("ta", 32, 32), 4, W, 1, 0), (dcv("tb", 32, 40), 8, 0, -1, 0)), 3)]
    return out


SINGLE_CASES = _single_cases()
CHAIN_CASES = _chain_cases()
GPU_IDS = [c.id for c in SINGLE_CASES] + [c.id for c in CHAIN_CASES]
assert len(set(GPU_IDS)) == len(GPU_IDS)


def _read_records(lib, cap=256):
    buf = (P.ProfRecord * cap)()
    n = lib.s3r_profile_read(buf, cap)
    assert 0 <= n < cap, n
    return [dict([(k, int(getattr(r, k))) for k in REC_INTS] + [(k, float(getattr(r, k))) for k in REC_DOUBLES]) for r in buf[:n]]


def _zeros(n, torch):
    return torch.zeros(max(int(n), 4), dtype=torch.float32, device="cuda:0")


def _layer_bufs(lib, d, torch):
    n = C.c_int64(0)
    assert lib.s3r_conv_packed_elems(C.byref(d), C.byref(n)) == 0, lib.s3r_last_error()
    return _zeros(n.value, torch), _zeros(d.cout, torch), _zeros(d.cout, torch)


def _padded_elems(batch, channels, edge, halo, nd):
    return batch * channels * (edge + 2 * halo) ** nd


def _run_single(lib, c, torch):
    d = desc_of(c)
    nd = spec.ndim(c.layer)
    n_out = lib.s3r_conv_out_size(C.byref(d))
    assert n_out > 0, lib.s3r_last_error()
    need = lib.s3r_conv_scratch_elems(C.byref(d))
    assert need >= 0, lib.s3r_last_error()
    pk, sc, sh = _layer_bufs(lib, d, torch)
    x = _zeros(_padded_elems(c.B, c.layer.cin, c.n_in, d.in_halo, nd), torch)          # (fp32 sizes: a bf16 tensor takes half of it)
    y = _zeros(_padded_elems(c.B, c.layer.cout, n_out, c.out_halo, nd), torch)
    scr = _zeros(need, torch)
    rc = lib.s3r_conv_forward(C.byref(d), x.data_ptr(), pk.data_ptr(), sc.data_ptr(), sh.data_ptr(), y.data_ptr(), scr.data_ptr(), need, None)
    assert rc == 0, (c.id, lib.s3r_last_error())
    torch.cuda.synchronize()


def _run_chain(lib, c, torch):
    n = len(c.parts)
    arr = (P.Layer * n)()
    keep = []
    for i, (layer, n_in, algo, tile, ks) in enumerate(c.parts):
        d = P.make_desc(layer, c.B, n_in, tag=i, algo=algo, tile=tile, ksplit=ks, dtype=P.DTYPE[c.dtype])
        pk, sc, sh = _layer_bufs(lib, d, torch)
        arr[i].desc, arr[i].packed_w, arr[i].scale, arr[i].shift = d, pk.data_ptr(), sc.data_ptr(), sh.data_ptr()
        keep += [pk, sc, sh]
    need = lib.s3r_chain_workspace_elems(arr, n)
    assert need >= 0, (c.id, lib.s3r_last_error())
    first, n0 = c.parts[0][0], c.parts[0][1]
    last, n1 = c.parts[-1][0], c.parts[-1][1]
    x = _zeros(_padded_elems(c.B, first.cin, n0, 0, spec.ndim(first)), torch)
    y = _zeros(_padded_elems(c.B, last.cout, spec.out_size(last, n1), 0, spec.ndim(last)), torch)
    ws = _zeros(need, torch)
    rc = lib.s3r_chain_forward(arr, n, x.data_ptr(), y.data_ptr(), ws.data_ptr(), need, 1, None)
    assert rc == 0, (c.id, lib.s3r_last_error())
    torch.cuda.synchronize()


def gpu_part(lib):
    """{case id: the profiler's records of one forward, in the order s3r_profile_read gives them (aux records nested in their layer's)}"""
    import torch
    out = {}
    assert lib.s3r_profile_enable(256) == 0 and lib.s3r_profile_detail(1) == 0
    try:
        for cases, run in ((SINGLE_CASES, _run_single), (CHAIN_CASES, _run_chain)):
            for c in cases:
                assert lib.s3r_profile_reset() == 0
                run(lib, c, torch)
                out[c.id] = _read_records(lib)
    finally:
        lib.s3r_profile_detail(0)
        lib.s3r_profile_enable(0)
    return out


def compute_units():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count
