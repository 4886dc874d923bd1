#!/usr/bin/env python3
"""sha256 of every answer the host-side planner gives over a fixed walk of descriptors and chains: run under two builds
(S3R_LIB=...) to show that a planner change kept every size, layout, refusal and message.  Needs no GPU.
    python tools/plan_digest.py [--dump FILE]

The walk: every case of tests/_dispatch_cases.HOST_CASES; every arch_spec stage table as a chain (and layer by layer) at the batches
where a plan changes; a seeded sample of single descriptors and of 2-3-layer chains, half drawn freely and half made by changing one
or two fields of a valid case.  Per descriptor: the six size queries, s3r_last_error after every negative answer, and — only where the
layer needs scratch — the refusals of s3r_conv_forward over dummy pointers (scratch NULL, and one float short): nothing is enqueued."""
import ctypes as C
import hashlib
import json
import os
import random
import re
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import s3r
from s3r import arch_spec as spec
from tests import _buffer_cases as BC
from tests import _dispatch_cases as DC

P = s3r._lib
FIELDS = [n for n, _ in P.ConvDesc._fields_]
BATCHES = (1, 2, 32, 113, 114, 158, 159, 256, 300)
N_SINGLES, N_CHAINS = 4000, 600

# value sets: first the common values (drawn with weight), then the edges the planner branches on and a few it must refuse
VALUES = dict(
    op=[0, 0, 0, 1, 1, 2, 3],
    ndim=[2, 2, 3, 3, 3, 1, 4],
    cin=[1, 3, 8, 9, 12, 16, 24, 32, 32, 33, 64, 64, 0],
    cout=[1, 2, 7, 16, 24, 32, 32, 33, 48, 64, 64, 70, 96, 128, 130, 0],
    k=[1, 2, 3, 3, 3, 4, 4, 5, 7, 0],
    stride=[1, 1, 1, 2, 2, 3, 4, -1],      # (not 0: s3r_conv_wino_input_elems divides by it before anything validates the descriptor)
    pad=[0, 1, 1, 1, 2, 3, -1],
    dilation=[0, 1, 1, 1, 1, 2, 3, -1],
    out_pad=[0, 0, 0, 0, 1, 2, -1],
    in_size=[3, 4, 5, 7, 8, 12, 14, 16, 28, 32, 60, 61, 124, 125, 128, 0],
    batch=[1, 2, 3, 32, 113, 114, 158, 159, 256, 300, 0],
    dtype=[0, 0, 0, 0, 1, 1, 2],
    act=[0, 1, 1, 2, 3, 4, 5, 6, -1],
    act_param=[0.0, 0.01, 0.3, 1.0, 1.5, -0.1],
    in_halo=[0, 1, 1, 1, 2, 3, 8, 9, -1],
    out_halo=[0, 0, 1, 1, 2, 3, 8, 9, -1],
    in_layout=[0, 0, 0, 0, 0, 0, 2, 3, 4, 5, 6, 1],
    out_layout=[0, 0, 0, 0, 0, 0, 0, 0, 4, 5, 6, 2, 1],
    algo=[0, 0, 0, 1, 2, 2, 3],
    tile=[-1] * 12 + list(range(0, 11)) + list(range(17, 24)) + [40],
    ksplit=[0, 0, 0, 0, 1, 2, 4, 3, -1],
)
SAMPLED = ("op", "ndim", "cin", "cout", "k", "stride", "pad", "dilation", "out_pad", "in_size", "batch", "dtype", "act", "act_param",
           "in_halo", "out_halo", "in_layout", "out_layout", "algo", "tile", "ksplit")
assert set(SAMPLED) == set(VALUES)


def fields_of(d):
    return {n: getattr(d, n) for n in FIELDS}


def desc_from(f):
    d = P.ConvDesc()
    for n in FIELDS:
        setattr(d, n, f.get(n, 0))
    return d


def free_fields(rng):
    f = {n: rng.choice(VALUES[n]) for n in SAMPLED}
    f["tag"] = 0
    if rng.random() < 0.6:                   # most layers are described the way a caller would: plain, the halo the kernel reads, no overrides
        f.update(in_layout=0, out_layout=0, tile=-1, ksplit=0, in_halo=1 if f["op"] == 1 else max(f["pad"], 0))
    return f


def mutated(rng, base):
    f = dict(base)
    for n in rng.sample(SAMPLED, rng.choice((1, 2))):
        f[n] = rng.choice(VALUES[n])
    return f


# ---------------------------------------------------------------- the queries
def err(lib):
    return lib.s3r_last_error().decode("utf-8", "replace")


def single(lib, f):
    """every single-descriptor answer; [answer, message] where the answer is negative"""
    d = desc_from(f)
    rec = {}

    def put(name, v):
        rec[name] = [v, err(lib)] if v < 0 else v

    put("out_size", lib.s3r_conv_out_size(C.byref(d)))
    n = C.c_int64(-1)
    rc = lib.s3r_conv_packed_elems(C.byref(d), C.byref(n))
    put("packed_rc", rc)
    rec["packed_elems"] = n.value
    need = lib.s3r_conv_scratch_elems(C.byref(d))
    put("scratch_elems", need)
    put("wino_input_elems", lib.s3r_conv_wino_input_elems(C.byref(d)))
    put("wino_input_layout", lib.s3r_conv_wino_input_layout(C.byref(d)))
    if need > 0:                             # (as tests/_dispatch_cases.refusals: never where no scratch is needed — that call would launch)
        for name, scr, n_scr in (("null", None, need), ("short", DC.DUMMY, need - 1)):
            rc = lib.s3r_conv_forward(C.byref(d), DC.DUMMY, DC.DUMMY, DC.DUMMY, DC.DUMMY, DC.DUMMY, scr, n_scr, None)
            rec["forward_" + name] = [rc, err(lib)]
    return rec


def chain(lib, layers):
    arr = (P.Layer * len(layers))()
    for i, f in enumerate(layers):
        arr[i].desc = desc_from(f)
    need = lib.s3r_chain_workspace_elems(arr, len(layers))
    return [need, err(lib)] if need < 0 else need


# ---------------------------------------------------------------- the walk
def host_case_items():
    return [("single", c.id, fields_of(DC.desc_of(c))) for c in DC.HOST_CASES]


def stage_items():
    items = []
    for stage in ("encoder", "decoder", "decoder_down", "point_head"):
        rows = spec.stage_table(stage)
        for dt in ("fp32", "bf16"):
            if dt == "bf16" and stage == "point_head":
                continue
            for B in BATCHES:
                for h0 in (0, 1):
                    layers = [fields_of(P.make_desc(l, B, n, tag=i, in_halo=h0 if i == 0 else 0, dtype=P.DTYPE[dt])) for i, (l, n, _) in enumerate(rows)]
                    items.append(("chain", f"{stage}-{dt}-B{B}-h{h0}", layers))
                for l, n, _ in rows:
                    f = fields_of(P.make_desc(l, B, n, in_halo=BC.need_halo(l, n, dt), dtype=P.DTYPE[dt]))
                    items.append(("single", f"{stage}-{l.name}-{dt}-B{B}", f))
    return items


def sampled_single_items(rng):
    bases = [f for _, _, f in host_case_items()]
    items = []
    for i in range(N_SINGLES):
        f = free_fields(rng) if i % 2 == 0 else mutated(rng, rng.choice(bases))
        items.append(("single", f"s{i}", f))
    return items


def _chain_bases():
    out = []
    for _, p, c, _ in BC.CHAIN_PAIRS:
        for B in (1, 3, 32):
            out.append([fields_of(P.make_desc(q.layer, B, q.n_in, tag=i, algo=q.algo, tile=q.tile)) for i, q in enumerate((p, c))])
    for stage in ("encoder", "decoder"):
        rows = spec.stage_table(stage)
        for n in (2, 3):
            for i0 in range(len(rows) - n + 1):
                for B in (2, 32, 159):
                    out.append([fields_of(P.make_desc(l, B, e, tag=i)) for i, (l, e, _) in enumerate(rows[i0:i0 + n])])
    return out


def sampled_chain_items(lib, rng):
    bases = _chain_bases()
    items = []
    for i in range(N_CHAINS):
        n = rng.choice((2, 3))
        if i % 2 == 0:                       # free: each layer drawn, then aimed at its producer's output (most of the time)
            layers = []
            for j in range(n):
                f = free_fields(rng)
                if j > 0 and rng.random() < 0.85:
                    prev = layers[-1]
                    edge = lib.s3r_conv_out_size(C.byref(desc_from(prev)))
                    f.update(cin=prev["cout"], in_size=max(edge, 1), batch=prev["batch"], dtype=prev["dtype"])
                    if prev["op"] != 2 and f["op"] != 2:
                        f["ndim"] = prev["ndim"]
                layers.append(f)
        else:
            layers = [dict(f) for f in rng.choice(bases)]
            j = rng.randrange(len(layers))
            layers[j] = mutated(rng, layers[j])
        items.append(("chain", f"c{i}", layers))
    return items


def template(msg):
    return re.sub(r"-?\d+", "#", msg)


def main():
    t0 = time.time()
    lib = s3r.load_library()
    rng = random.Random(0)
    groups = [("host_cases", host_case_items()), ("stage_tables", stage_items()), ("sampled_singles", sampled_single_items(rng)),
              ("sampled_chains", sampled_chain_items(lib, rng))]
    dump = {}
    messages = set()
    print(f"library: {P.LIB_PATH}")
    for name, items in groups:
        answers = {}
        ok = refused = 0
        for kind, key, what in items:
            a = single(lib, what) if kind == "single" else chain(lib, what)
            answers[key] = a
            verdict = a["scratch_elems"] if kind == "single" else a
            if isinstance(verdict, list):
                refused += 1
            else:
                ok += 1
            for v in (a.values() if isinstance(a, dict) else [a]):
                if isinstance(v, list):
                    messages.add(template(v[1]))
        blob = json.dumps(answers, sort_keys=True).encode()
        dump[name] = answers
        print(f"{name:16s} items {len(items):5d}  accepted {ok:5d}  refused {refused:5d}  sha256 {hashlib.sha256(blob).hexdigest()}")
    print(f"distinct refusal messages (numbers masked): {len(messages)}")
    print(f"walk: {time.time() - t0:.1f} s", file=sys.stderr)
    if "--dump" in sys.argv:
        with open(sys.argv[sys.argv.index("--dump") + 1], "w") as fh:
            json.dump(dict(answers=dump, messages=sorted(messages)), fh, indent=1, sort_keys=True)


if __name__ == "__main__":
    main()
