"""The 3D hand-off passes (csrc/s3r_wino_handoff.hip, wino_handoff_kernel): a producer's finish pass that writes its consumer's operand
— the two-axis plane sets (S3R_LAYOUT_WINO_3D) or [x | Dh | Dd | Ddh] (S3R_LAYOUT_DIFF) — in place of the producer's finish pass
and the consumer's transform / difference pass.  The four kinds of pair s3r_chain_forward plans:

  (a) split-K direct convolution   -> two-axis Conv3d          v4 -> v5
  (b) class-parallel two-axis      -> two-axis Conv3d          v5 -> v6
  (c) class-parallel two-axis      -> transposed Winograd      v6 -> d1
  (d) class-parallel transposed    -> transposed Winograd      d1 -> d2

Everything here is BITWISE: a pair as a two-layer chain (hand-off planned) against the same two layers as one-layer calls (which
never hand off), same forced algorithm / form / split-K on both sides.  No tolerance exists in this file.  The shapes are the
network's own pairs and the smallest that reach every path: a partial last group (edges 5, 6, 7), a whole one (8), a channel block
that does not divide cout (edge 11: blocks of 3 channels over 32), a consumer cout that is no multiple of 16, pairs the planner
must decline (ksplit 1; the semi-fused / serial forms; transposed edges 2 and 3, which have no Winograd form) — those must equal
the two passes too, with today's launch counts.

(a)-like pairs at 32 -> 32 channels can split K by 1 and 2 only (split-K divides cin / 16); ksplit 4 runs at 64 -> 32.
"""
import ctypes as C

import pytest
import torch

from tests import _guard as G

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def lib(s3r):
    return s3r.load_library()


def _layer(s3r, name, op, cin, cout, k=3, s=1, p=1):
    return s3r.arch_spec.Layer(name, op, cin, cout, k, s, p)


def _cases(s3r):
    """id -> (a, b, input edge, overrides {layer name: (algo, tile, ksplit)}, hand-off expected (None: the library's own forms))"""
    L, spec = s3r._lib, s3r.arch_spec
    dec = {l.name: (l, n) for l, n, _ in spec.stage_table("decoder")}
    W = L.ALGO_WINOGRAD
    conv = lambda n, ci, co, **kw: _layer(s3r, n, "conv3d", ci, co, **kw)
    dcv = lambda n, ci, co: _layer(s3r, n, "deconv3d", ci, co, 4, 2, 1)
    out = {}
    for pa, pb in (("v4", "v5"), ("v5", "v6"), ("v6", "d1"), ("d1", "d2")):
        out[f"net-{pa}-{pb}"] = (dec[pa][0], dec[pb][0], dec[pa][1], {}, None)
    # (a)-like: direct stride 2 -> two-axis k3; 12^3 -> 6^3: one full group + a partial one; 10^3 -> 5^3
    for edge in (12, 10):
        for cin, ks in ((32, 1), (32, 2), (64, 2), (64, 4)):
            out[f"a-{cin}to32-e{edge}-ks{ks}"] = (conv("ha", cin, 32, s=2), conv("hb", 32, 32), edge, {"ha": (L.ALGO_AUTO, -1, ks)}, ks > 1)
    # (b)-like: two-axis k3 -> two-axis k3 at edges 5, 7, 8 (11: channel blocks of 3), -> k4 valid at input edges 5 and 7
    for edge in (5, 7, 8, 11):
        out[f"b-k3-e{edge}"] = (conv("ha", 32, 32), conv("hb", 32, 32), edge, {"ha": (W, 4, 0)}, True)
    for edge in (5, 7):
        out[f"b-k4-e{edge}"] = (conv("ha", 32, 32), conv("hb", 32, 32, k=4, p=0), edge, {"ha": (W, 4, 0)}, True)
    out["b-k3-e8-semi"] = (conv("ha", 32, 32), conv("hb", 32, 32), 8, {"ha": (W, 5, 0)}, False)      # semi-fused producer: declined
    out["b-k3-e8-auto"] = (conv("ha", 32, 32), conv("hb", 32, 32), 8, {}, None)
    # (c)-like: two-axis -> transposed; edges 2 and 3 have neither form (declined)
    out["c-k3-e4"] = (conv("ha", 32, 32), dcv("tb", 32, 24), 4, {"ha": (W, 4, 0)}, True)
    out["c-k4-e7"] = (conv("ha", 32, 32, k=4, p=0), dcv("tb", 32, 32), 7, {"ha": (W, 4, 0)}, True)
    for edge in (2, 3):
        out[f"c-k3-e{edge}"] = (conv("ha", 32, 32), dcv("tb", 32, 32), edge, {}, False)
    # (d)-like: transposed -> transposed; 2 -> 4 and 3 -> 6: the producer / the consumer has no Winograd form (declined)
    out["d-e4"] = (dcv("ta", 32, 32), dcv("tb", 32, 40), 4, {"ta": (W, 1, 0)}, True)
    out["d-e4-serial"] = (dcv("ta", 32, 32), dcv("tb", 32, 32), 4, {"ta": (W, 0, 0)}, False)
    out["d-e4-auto"] = (dcv("ta", 32, 32), dcv("tb", 32, 32), 4, {}, None)
    for edge in (2, 3):
        out[f"d-e{edge}"] = (dcv("ta", 32, 32), dcv("tb", 32, 32), edge, {}, False)
    return out


_IDS = (["net-v4-v5", "net-v5-v6", "net-v6-d1", "net-d1-d2"] +
        [f"a-{c}to32-e{e}-ks{k}" for e in (12, 10) for c, k in ((32, 1), (32, 2), (64, 2), (64, 4))] +
        [f"b-k3-e{e}" for e in (5, 7, 8, 11)] + ["b-k4-e5", "b-k4-e7", "b-k3-e8-semi", "b-k3-e8-auto", "c-k3-e4", "c-k4-e7", "c-k3-e2",
                                                 "c-k3-e3", "d-e4", "d-e4-serial", "d-e4-auto", "d-e2", "d-e3"])


class _Pair:
    """the pair as a chain, and the same two layers (same parameters, same overrides) as chains of one"""

    def __init__(self, s3r, case):
        a, b, edge, over, expect = case
        H = s3r.modules._HipChain
        self.a, self.b, self.edge, self.expect = a, b, edge, expect
        self.mid = s3r.arch_spec.out_size(a, edge)
        self.pair, self.first, self.second = H([a, b], edge, precision="fp32"), H([a], edge, precision="fp32"), H([b], self.mid, precision="fp32")
        s3r.seed_module(self.pair, 41)
        sd = self.pair.state_dict()
        self.first.load_state_dict({k: v for k, v in sd.items() if k.startswith(a.name + ".")})
        self.second.load_state_dict({k: v for k, v in sd.items() if k.startswith(b.name + ".")})
        for m in (self.pair, self.first, self.second):
            m.to(DEV)
            for name, (algo, tile, ks) in over.items():
                if name in m.names:
                    if algo:
                        m.algo_override[name] = algo
                    if tile >= 0:
                        m.tile_override[name] = tile
                    if ks:
                        m.ksplit_override[name] = ks

    def x(self, B):
        return torch.randn((B, self.a.cin) + (self.edge,) * 3, generator=torch.Generator().manual_seed(100 * self.edge + B)).to(DEV)

    def stepwise(self, x):
        mid = self.first._run(x)
        return mid, self.second._run(mid)


_MEMO = {}


def _pair(s3r, cid):
    if cid not in _MEMO:
        _MEMO.clear()                                     # (one case's modules at a time)
        _MEMO[cid] = _Pair(s3r, _cases(s3r)[cid])
    return _MEMO[cid]


def _profile(s3r, fn):
    """{tag: [launches of the layer's record, number of aux passes nested in it]} of whatever fn enqueues"""
    L = s3r._lib
    L.profile_enable(256)
    L.profile_detail(1)
    try:
        L.profile_reset()
        fn()
        torch.cuda.synchronize()
        recs = L.profile_read()
    finally:
        L.profile_detail(0)
        L.profile_enable(0)
    out = {}
    for r in recs:
        if r["family"] == "conv_mfma":
            out.setdefault(r["tag"], [0, 0])[0] += r["launches"]
        elif r["family"] == "aux":
            out.setdefault(r["tag"], [0, 0])[1] += 1
    return out


def _counts(s3r, p, B):
    x = p.x(B)
    mid = p.first._run(x)
    chain = _profile(s3r, lambda: p.pair._run(x))
    one_a = _profile(s3r, lambda: p.first._run(x))
    one_b = _profile(s3r, lambda: p.second._run(mid))
    return chain[0], chain[1], one_a[0], one_b[0]


def _taken(counts):
    ca, cb, sa, sb = counts
    if ca == sa and cb == sb:
        return False
    # the producer keeps its passes (the finish pass became the hand-off pass), the consumer loses its operand pass: one launch fewer
    assert ca == sa and cb == [sb[0] - 1, sb[1] - 1], counts
    return True


# ---------------------------------------------------------------- A, D: bit-identity and batch invariance
@pytest.mark.parametrize("cid", _IDS)
def test_pair_equals_the_two_layers_run_singly(s3r, cid):
    """A: the chain's output equals the two one-layer calls bitwise, at B = 1 and B = 3; D: sample 0 of the B = 3 chain equals the B = 1
    chain bitwise; C: the launch and aux-pass counts say the hand-off ran exactly where the forms allow it."""
    p = _pair(s3r, cid)
    got = {}
    for B in (1, 3):
        x = p.x(B)
        _, want = p.stepwise(x)
        got[B] = p.pair._run(x)
        assert torch.equal(got[B], want), (cid, B, float((got[B] - want).abs().max()))
        assert torch.isfinite(got[B]).all()
    x3 = p.x(3)
    assert torch.equal(p.pair._run(x3[:1].contiguous()), got[3][:1]), (cid, "sample 0 depends on the batch")
    taken = _taken(_counts(s3r, p, 3))
    if p.expect is not None:
        assert taken == p.expect, (cid, "planned" if taken else "declined")


# ---------------------------------------------------------------- B: guards, halos, poison
def _align(n):
    return -(-n // 256) * 256


@pytest.mark.parametrize("cid", ["net-v5-v6", "net-d1-d2", "a-64to32-e12-ks4", "b-k3-e7", "b-k3-e11", "b-k4-e5", "c-k3-e4", "c-k4-e7", "d-e4"])
def test_handoff_region_guards_and_zeros(s3r, lib, cid):
    """B: s3r_chain_forward on guarded buffers, the workspace NaN-filled and then initialised by ws_fresh = 1: the guards are intact, the
    output equals the one-layer calls, the region holds the consumer's operand and nothing else — the halo of the plain tensor and
    the last row / depth of the difference tensors are +0.0 by bit pattern, the difference tensors are the differences of the plain
    tensor bitwise, the rest of the region and the gap behind it stay zero.  Then the operand is overwritten with NaN and the chain
    runs again WITHOUT re-initialising: every element of the operand is written again, the halo with +0.0."""
    p = _pair(s3r, cid)
    B = 2
    a, b = p.a, p.b
    x = p.x(B)
    mid, want = p.stepwise(x)
    assert _taken(_counts(s3r, p, B)), cid
    arr, n = p.pair._layer_array(B, torch.device(DEV))
    need = lib.s3r_chain_workspace_elems(arr, n)
    assert need > 0, lib.s3r_last_error()
    xb = G.Guarded("x", x.shape, torch.float32, DEV, "in", data=x)
    ws = G.Guarded("ws", need, torch.float32, DEV, "scratch", fill="nan")
    h_in = 1 if a.op == "deconv3d" else a.p
    off = _align(B * a.cin * (p.edge + 2 * h_in) ** 3) if h_in else 0
    h = 1 if b.op == "deconv3d" else b.p
    op, Cc = p.mid + 2 * h, a.cout
    plain = B * Cc * op ** 3
    if b.op == "deconv3d":
        operand = 4 * plain
    else:
        sg = -(-p.mid // 4) if b.k == 3 else (p.mid - 2) // 2
        operand = (36 if b.k == 3 else 25) * B * Cc * sg * sg * op
    region = _align(off + max(plain, operand))
    bits = ws.t.view(torch.int32)
    for fresh in (1, 0):
        y = G.Guarded("y", want.shape, torch.float32, DEV, "out")
        rc = lib.s3r_chain_forward(arr, n, xb.ptr, y.ptr, ws.ptr, need, fresh, None)
        assert rc == 0, lib.s3r_last_error()
        torch.cuda.synchronize()
        G.check_all(xb, y, ws)
        assert torch.equal(y.t, want), (cid, fresh)
        assert not torch.isnan(ws.t[off:off + operand]).any(), (cid, fresh, "operand not fully written")
        assert not bits[off + operand:region].any(), (cid, fresh, "write behind the operand")
        if b.op == "deconv3d":
            t = ws.t[off:off + operand].view(4, B, Cc, op, op, op)
            xp = torch.zeros_like(t[0])
            xp[:, :, 1:-1, 1:-1, 1:-1] = mid
            assert torch.equal(t[0].view(torch.int32), xp.view(torch.int32)), (cid, fresh, "plain tensor / its +0.0 halo")
            dh, dd, ddh = torch.zeros_like(xp), torch.zeros_like(xp), torch.zeros_like(xp)
            dh[:, :, :, :-1] = xp[:, :, :, :-1] - xp[:, :, :, 1:]
            dd[:, :, :-1] = xp[:, :, :-1] - xp[:, :, 1:]
            ddh[:, :, :-1] = dh[:, :, :-1] - dh[:, :, 1:]
            for k, (name, ref) in enumerate((("Dh", dh), ("Dd", dd), ("Ddh", ddh)), 1):
                assert torch.equal(t[k].view(torch.int32), ref.view(torch.int32)), (cid, fresh, name)
        ws.t[off:off + operand] = float("nan")           # (next round: no re-initialisation, so every element must be written again)


# ---------------------------------------------------------------- C: the plan does what it says, on the network's own chain
@pytest.mark.parametrize("B", [3, 32])
def test_network_chain_passes_and_launches(s3r, B):
    """C: v4 .. d2 as one chain at a small and at the benchmark's batch (the library's own forms): each of v4, v5, v6, d1 carries exactly one
    aux pass — its hand-off pass —, d2 no operand pass, and the chain makes four launches fewer than the five layers run singly; the
    outputs agree bitwise."""
    spec = s3r.arch_spec
    rows = [(l, n) for l, n, _ in spec.stage_table("decoder") if l.name in ("v4", "v5", "v6", "d1", "d2")]
    H = s3r.modules._HipChain
    chain = H([l for l, _ in rows], rows[0][1], precision="fp32")
    s3r.seed_module(chain, 7)
    chain.to(DEV)
    singles = []
    for l, n in rows:
        m = H([l], n, precision="fp32")
        m.load_state_dict({k: v for k, v in chain.state_dict().items() if k.startswith(l.name + ".")})
        singles.append(m.to(DEV))
    x = torch.randn((B, rows[0][0].cin) + (rows[0][1],) * 3, generator=torch.Generator().manual_seed(B)).to(DEV)
    acts = [x]
    for m in singles:
        acts.append(m._run(acts[-1]))
    got = chain._run(x)
    assert torch.equal(got, acts[-1]), float((got - acts[-1]).abs().max())
    rec = _profile(s3r, lambda: chain._run(x))
    one = [_profile(s3r, lambda m=m, t=t: m._run(t))[0] for m, t in zip(singles, acts)]
    for i in range(4):
        assert rec[i][1] == 1, (rows[i][0].name, rec)
    assert rec[4][1] == one[4][1] - 1, ("d2", rec, one)
    assert sum(r[0] for r in rec.values()) == sum(o[0] for o in one) - 4, (rec, one)
