"""s3r_optim_step without a device: the header's wording and signatures, every refusal (all host-side: nothing is enqueued, so they run
without a GPU), the scratch query against its formula, tests/_optim64.py's restatement over ten steps against torch.optim.SGD / Adam /
AdamW in float64 within the derived bound compounded over the steps, the mutants of the restatement that the bit-for-bit comparison of
tests/test_optimizer_gpu.py must catch (on the check function and the inputs that file uses), and what the shared data must cover."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from tests import _optim64 as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32


@pytest.fixture(scope="module")
def lib(s3r):
    return s3r.load_library()


@pytest.fixture(scope="module")
def header():
    with open(os.path.join(ROOT, "include", "s3r.h")) as f:
        return f.read()


# ---------------------------------------------------------------- header, bindings, exports
def _proto(header, ret, name):
    plain = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    m = re.search(r"\b%s\s+%s\s*\(([^)]*)\)\s*;" % (ret, name), plain)
    assert m, f"{name} is not declared in include/s3r.h"
    return [" ".join(a.split()) for a in m.group(1).split(",")]


def test_header_prototypes_match_the_bindings(s3r, lib, header):
    L = s3r._lib
    assert _proto(header, "int64_t", "s3r_optim_scratch_elems") == ["const s3r_optim_tensor* t", "int n_tensors"]
    assert _proto(header, "int", "s3r_optim_state_init") == ["float* state", "float lr", "void* hip_stream"]
    assert _proto(header, "int", "s3r_optim_set_lr") == ["float* state", "float lr", "void* hip_stream"]
    assert _proto(header, "int", "s3r_optim_step") == ["const s3r_optim_desc* d", "const s3r_optim_tensor* t", "int n_tensors", "float* state",
                                                       "float* scratch", "int64_t scratch_elems", "void* hip_stream"]
    assert L.SIGNATURES["s3r_optim_scratch_elems"] == (C.c_int64, [C.POINTER(L.OptimTensor), C.c_int])
    assert L.SIGNATURES["s3r_optim_state_init"] == (C.c_int, [C.c_void_p, C.c_float, C.c_void_p])
    assert L.SIGNATURES["s3r_optim_step"] == (C.c_int, [C.POINTER(L.OptimDesc), C.POINTER(L.OptimTensor), C.c_int, C.c_void_p, C.c_void_p,
                                                        C.c_int64, C.c_void_p])
    assert lib.s3r_optim_step.argtypes == L.SIGNATURES["s3r_optim_step"][1]
    assert C.sizeof(L.OptimTensor) == 40 and C.sizeof(L.OptimDesc) == 28
    assert [n for n, _ in L.OptimTensor._fields_] == ["param", "grad", "m", "v", "elems"]
    assert [n for n, _ in L.OptimDesc._fields_] == ["kind", "flags", "beta1", "beta2", "eps", "weight_decay", "max_norm"]
    assert lib.s3r_abi_version() == 8 and "#define S3R_ABI_VERSION 8" in header
    for name, value in (("S3R_OPTIM_TENSORS_PER_LAUNCH", L.OPTIM_TENSORS_PER_LAUNCH), ("S3R_OPTIM_MAX_TENSORS", L.OPTIM_MAX_TENSORS),
                        ("S3R_OPTIM_STATE_DWORDS", 8), ("S3R_OPT_SGD", L.OPT_SGD), ("S3R_OPT_ADAM", L.OPT_ADAM),
                        ("S3R_OPT_DECOUPLED_DECAY", L.OPT_DECOUPLED_DECAY), ("S3R_OPT_NESTEROV", L.OPT_NESTEROV), ("S3R_OPT_CLIP", L.OPT_CLIP),
                        ("S3R_OPT_SKIP_NONFINITE", L.OPT_SKIP_NONFINITE)):
        assert re.search(r"#define %s %d\b" % (name, value), header), name
    assert {"SGD", "Adam", "AdamW"} <= set(s3r.__all__)
    assert all(issubclass(getattr(s3r, n), torch.optim.Optimizer) for n in ("SGD", "Adam", "AdamW"))


def test_the_header_states_the_contract(header):
    at = header.index("#define S3R_OPTIM_TENSORS_PER_LAUNCH")
    comment = " ".join(re.sub(r"\n \*", " ", header[header[:at].rfind("/* The optimizer step"):at]).split())
    for wording in ("BY VALUE in kernel arguments", "no pointer table in device memory", "ON THE DEVICE", "no powf", "BAKED at enqueue time",
                    "m = g", "a = mu * m; m = a + g", "t = mu * m; g = g + t", "w = lr * weight_decay; s = w * p; p = p - s",
                    "a = beta1 * m; b = (1.f - beta1) * g; m = a + b", "r = sqrtf(vh); d = r + eps; u = mh / d",
                    "chunks of 512 consecutive elements", "ascending tensor order", "d = grad_norm + 1e-6f; c = max_norm / d",
                    "a NaN stays a NaN", "poisons only its own element", "`skipped` grows by one", "before anything is enqueued",
                    "4-byte alignment only", "hipStream_t", "no memset"):
        assert wording in comment, wording


# ---------------------------------------------------------------- refusals (host-only)
A = 0x10000      # non-NULL addresses: every case is refused before anything could dereference them


def _tensors(L, rows):
    return (L.OptimTensor * len(rows))(*[L.OptimTensor(*r) for r in rows])


def _ok_list(L, n=2, elems=600):
    return _tensors(L, [(A * (8 * i + 1), A * (8 * i + 2), A * (8 * i + 3), A * (8 * i + 4), elems) for i in range(n)])


def _step(lib, L, d, t, n, state=A * 999, scratch=A * 998, scratch_elems=1 << 20):
    return lib.s3r_optim_step(C.byref(d) if d is not None else None, t, n, state, scratch, scratch_elems, None)


def _adam(L, **kw):
    f = dict(kind=L.OPT_ADAM, flags=0, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.0, max_norm=0.0)
    f.update(kw)
    return L.OptimDesc(*[f[n] for n, _ in L.OptimDesc._fields_])


def _sgd(L, **kw):
    return _adam(L, **dict(dict(kind=L.OPT_SGD, beta1=0.0, beta2=0.0, eps=0.0), **kw))


def _refused(lib, rc, *words):
    assert rc == -1, rc
    msg = lib.s3r_last_error().decode()
    for w in words:
        assert w in msg, (w, msg)


def test_null_pointers_are_refused(s3r, lib):
    L = s3r._lib
    _refused(lib, _step(lib, L, None, _ok_list(L), 2), "null descriptor")
    _refused(lib, _step(lib, L, _adam(L), None, 2), "null tensor list")
    _refused(lib, _step(lib, L, _adam(L), _ok_list(L), 2, state=None), "null state")
    for col, word in ((0, "null param or grad"), (1, "null param or grad"), (2, "null m"), (3, "null v")):
        row = [A, 2 * A, 3 * A, 4 * A, 600]
        row[col] = None
        _refused(lib, _step(lib, L, _adam(L), _tensors(L, [tuple(row)]), 1), "tensor 0", word)
    # SGD with momentum needs m; without it m may be NULL and v always may: the refusal below is then the scratch's, past the list's checks
    _refused(lib, _step(lib, L, _sgd(L, beta1=0.9), _tensors(L, [(A, 2 * A, None, None, 600)]), 1), "null m")
    _refused(lib, _step(lib, L, _sgd(L, flags=L.OPT_CLIP), _tensors(L, [(A, 2 * A, None, None, 600)]), 1, scratch=None), "scratch")


def test_sizes_and_counts_are_refused(s3r, lib):
    L = s3r._lib
    for elems in (0, -1, 1 << 31):
        _refused(lib, _step(lib, L, _adam(L), _tensors(L, [(A, 2 * A, 3 * A, 4 * A, elems)]), 1), "elems")
        assert lib.s3r_optim_scratch_elems(_tensors(L, [(A, 2 * A, 3 * A, 4 * A, elems)]), 1) == -1
    for n in (0, -3, L.OPTIM_MAX_TENSORS + 1):
        _refused(lib, _step(lib, L, _adam(L), _ok_list(L), n), "n_tensors")
        assert lib.s3r_optim_scratch_elems(_ok_list(L), n) == -1
    assert lib.s3r_optim_scratch_elems(None, 1) == -1


def test_a_short_scratch_is_refused_only_where_the_norm_needs_it(s3r, lib):
    L = s3r._lib
    t = _ok_list(L, 3, 1025)
    need = lib.s3r_optim_scratch_elems(t, 3)
    assert need == 3 * 3 + 3
    for flags in (L.OPT_CLIP, L.OPT_SKIP_NONFINITE, L.OPT_CLIP | L.OPT_SKIP_NONFINITE):
        _refused(lib, _step(lib, L, _adam(L, flags=flags, max_norm=1.0), t, 3, scratch_elems=need - 1), "scratch", str(need))
        _refused(lib, _step(lib, L, _adam(L, flags=flags, max_norm=1.0), t, 3, scratch=None, scratch_elems=need), "scratch")


@pytest.mark.parametrize("field,value", [("beta1", 1.0), ("beta1", -0.1), ("beta1", float("nan")), ("beta2", 1.0), ("beta2", float("inf")),
                                         ("beta2", -1e-3), ("eps", -1e-8), ("eps", float("nan")), ("weight_decay", -0.1),
                                         ("weight_decay", float("inf")), ("max_norm", -1.0), ("max_norm", float("nan")),
                                         ("max_norm", float("inf"))])
def test_hyper_parameters_out_of_range_are_refused(s3r, lib, field, value):
    L = s3r._lib
    _refused(lib, _step(lib, L, _adam(L, **{field: value}), _ok_list(L), 2), field)
    if field in ("beta1", "weight_decay", "max_norm"):
        _refused(lib, _step(lib, L, _sgd(L, **{field: value}), _ok_list(L), 2), field)


def test_unknown_kinds_and_flags_are_refused(s3r, lib):
    L = s3r._lib
    _refused(lib, _step(lib, L, _adam(L, kind=2), _ok_list(L), 2), "unknown kind")
    _refused(lib, _step(lib, L, _adam(L, kind=-1), _ok_list(L), 2), "unknown kind")
    _refused(lib, _step(lib, L, _adam(L, flags=16), _ok_list(L), 2), "unknown flag")
    _refused(lib, _step(lib, L, _adam(L, flags=L.OPT_NESTEROV), _ok_list(L), 2), "nesterov")
    _refused(lib, _step(lib, L, _sgd(L, flags=L.OPT_NESTEROV), _ok_list(L), 2), "nesterov")          # (no momentum)
    _refused(lib, _step(lib, L, _sgd(L, flags=L.OPT_DECOUPLED_DECAY), _ok_list(L), 2), "decoupled")


def test_overlaps_and_duplicates_are_refused(s3r, lib):
    L = s3r._lib
    n = 600
    for row in ((A, 9 * A, A + 4 * (n - 1), 4 * A, n), (A, 9 * A, 3 * A, A - 4 * (n - 1), n), (A, 9 * A, 3 * A, 3 * A + 4, n)):
        _refused(lib, _step(lib, L, _adam(L), _tensors(L, [row]), 1), "overlap")
    _refused(lib, _step(lib, L, _adam(L), _tensors(L, [(A, 2 * A, 3 * A, 4 * A, n), (5 * A, 6 * A, 7 * A, 8 * A, n), (A, 9 * A, 10 * A, 11 * A, n)]), 3),
             "same param", "0", "2")


def test_state_init_and_set_lr_refusals(s3r, lib):
    for fn in (lib.s3r_optim_state_init, lib.s3r_optim_set_lr):
        _refused(lib, fn(None, 1e-3, None), "null state")
        for lr in (-1e-3, float("nan"), float("inf")):
            _refused(lib, fn(A, lr, None), "lr")


def test_scratch_query_is_its_formula(s3r, lib):
    L = s3r._lib
    for sizes in (R.SIZES, (1,), (512,), (513,), R.boundary_sizes(2 * L.OPTIM_TENSORS_PER_LAUNCH + 1)):
        t = _tensors(L, [(A, A, A, A, n) for n in sizes])
        assert lib.s3r_optim_scratch_elems(t, len(sizes)) == R.scratch_elems(sizes) == sum(-(-n // 512) for n in sizes) + len(sizes)


def test_python_classes_refuse_what_the_kernels_do_not_serve(s3r):
    p = torch.nn.Parameter(torch.zeros(4))
    for cls in (s3r.SGD, s3r.Adam, s3r.AdamW):
        with pytest.raises(ValueError, match="GPU only"):
            cls([p], lr=0.1)
        with pytest.raises(ValueError, match="fp32"):
            cls([torch.nn.Parameter(torch.zeros(4, dtype=torch.bfloat16))], lr=0.1)


# ---------------------------------------------------------------- the restatement against torch in float64
def _torch_run(d, ts0, all_gs, lr):
    ps = [torch.nn.Parameter(torch.from_numpy(np.asarray(t["p"], np.float64).copy())) for t in ts0]
    wd = float(F(d.wd))
    if d.kind == "sgd":
        opt = torch.optim.SGD(ps, lr=float(F(lr)), momentum=float(F(d.beta1)), weight_decay=wd, nesterov=d.nesterov)
    else:
        cls = torch.optim.AdamW if d.decoupled else torch.optim.Adam
        opt = cls(ps, lr=float(F(lr)), betas=(float(F(d.beta1)), float(F(d.beta2))), eps=float(F(d.eps)), weight_decay=wd)
    for gs in all_gs:
        for p, g in zip(ps, gs):
            p.grad = torch.from_numpy(np.asarray(g, np.float64).copy())
        if d.clip is not None:
            torch.nn.utils.clip_grad_norm_(ps, float(F(d.clip)))
        opt.step()
    return [p.detach().numpy() for p in ps]


TORCH_RULES = [f"{r}-{n}" for r in R.RULES for n in ("plain", "clip", "clip_loose")]


@pytest.mark.parametrize("data", ["shared", "unit"])
@pytest.mark.parametrize("case", TORCH_RULES)
def test_ten_steps_against_torch_in_float64(case, data):
    """torch forms its update in another order (step_size = lr / bc1, sqrt(v) / sqrt(bc2) + eps, addcdiv), so the comparison is by the
    derived bound: E32 is tests/_optim64.py's one-step bound compounded over the ten steps along the float64 restatement (each step's
    bound takes the bounds of the step before as its inputs' errors); torch's float64 result is an evaluation of the same real function
    with unit round-off 2^-53 and no more than a small multiple of our operations on any path, so it is within 8 E64 (the same
    propagation with u = 2^-53) of the float64 restatement.  Allowed: |restatement32 - torch64| <= E32 + 8 E64."""
    d = R.CASES[case]
    sizes, steps, lr = (1, 3, 513, 2049), 10, 1e-2
    rng = np.random.default_rng(len(case))
    if data == "shared":
        ts = R.tensor_list(sizes, seed=3)
        all_gs = [R.grads(sizes, 3, k) for k in range(steps)]
    else:
        ts = [dict(p=rng.standard_normal(n).astype(F), m=np.zeros(n, F), v=np.zeros(n, F)) for n in sizes]
        all_gs = [[rng.standard_normal(n).astype(F) for n in sizes] for _ in range(steps)]
    t32, s32 = ts, R.fresh_state(lr)
    t64, s64, E32, E64 = ts, R.fresh_state(lr), None, None
    for gs in all_gs:
        t32, s32 = R.step32(d, t32, gs, s32)
        E32 = R.bound_step(d, t64, gs, s64, E32, R.U)
        E64 = R.bound_step(d, t64, gs, s64, E64, R.U64)
        t64, s64, _ = R.step64(d, t64, gs, s64)
    assert s32["step"] == steps
    want = _torch_run(d, ts, all_gs, lr)
    worst32 = worst64 = 0.0
    for a, b, w, e32, e64 in zip(t32, t64, want, E32, E64):
        allowed = e32["p"] + 8 * e64["p"]
        assert np.isfinite(a["p"]).all() and not np.isnan(allowed).any()
        dist = np.abs(a["p"].astype(np.float64) - w)
        assert (dist <= allowed).all(), (case, float((dist / allowed).max()))
        d64 = np.abs(b["p"] - w)
        assert (d64 <= 8 * e64["p"]).all(), (case, float((d64 / (8 * e64["p"])).max()))
        worst32 = max(worst32, float((dist / allowed).max()))
        worst64 = max(worst64, float((d64 / (8 * e64["p"])).max()))
    print(f"\n{case} {data}: largest |restatement32 - torch64| / allowed = {worst32:.3g}; |restatement64 - torch64| / (8 E64) = {worst64:.3g}")


def test_one_step_bound_holds_between_the_two_forms():
    """|step32 - step64| from the SAME state within bound_step, on the shared data, at every step of every rule"""
    worst = 0.0
    for name in ("sgd_nesterov_wd-clip", "adam_l2-plain", "adamw-clip"):
        d = R.CASES[name]
        ts, st = R.tensor_list(nan_m=False), R.fresh_state(R.LR)
        for k in range(R.STEPS):
            gs = R.grads(step=k)
            bnd = R.bound_step(d, ts, gs, st)
            t64, _, _ = R.step64(d, ts, gs, st)
            ts, st = R.step32(d, ts, gs, st)
            for a, b, e in zip(ts, t64, bnd):
                for key in ("p", "m", "v"):
                    dist = np.abs(a[key].astype(np.float64) - b[key])
                    assert (dist <= e[key]).all(), (name, k, key)
                    with np.errstate(all="ignore"):
                        r = np.where(e[key] > 0, dist / e[key], 0.0)
                    worst = max(worst, float(r[np.isfinite(r)].max(initial=0.0)))
    print(f"\nlargest one-step |fp32 - float64| / bound = {worst:.3g}")
    assert worst > 0


# ---------------------------------------------------------------- mutants, on the GPU tests' check function and inputs
NAN_AT = (2, 6, 100)          # tests/test_optimizer_gpu.py plants its NaN here: step 2, tensor 6 (2047 elements), element 100
KILLS = {"no_bias_correction": ["adam-plain", "adamw-clip"], "decay_swapped": ["adam_l2-plain", "adamw-plain"],
         "eps_in_sqrt": ["adam-plain"], "no_nesterov": ["sgd_nesterov_wd-plain"], "first_step_mu_times_nan": ["sgd_momentum-plain"],
         "descending_chunks": ["sgd-clip", "adam-skip"], "unclamped": ["sgd-clip_loose", "adamw-clip_loose"],
         "count_on_skip": ["sgd_momentum-skip", "adam-clip_skip"]}


def test_every_mutant_has_its_kills():
    assert set(KILLS) == set(R.MUTANTS) and all(c in R.CASES for cs in KILLS.values() for c in cs)


@pytest.mark.parametrize("mutant", R.MUTANTS)
def test_mutant_is_caught_by_the_gpu_tests_check(mutant):
    for case in KILLS[mutant]:
        d = R.CASES[case]
        nan_at = NAN_AT if d.skip else None
        good = R.run32(d, nan_at=nan_at)
        bad = R.run32(d, mutant=mutant, nan_at=nan_at)
        R.assert_same([t for t, _ in good][-1], R.state_words(good[-1][1]), *good[-1], d)            # the check passes on the rule itself
        with pytest.raises(AssertionError):
            for (gt, gst), (bt, bst) in zip(good, bad):
                R.assert_same(bt, R.state_words(bst), gt, gst, d, case)


def test_stock_rule_equals_itself_on_every_case():
    for name, d in R.CASES.items():
        a, b = R.run32(d, steps=2), R.run32(d, steps=2)
        R.assert_same(a[-1][0], R.state_words(a[-1][1]), *b[-1], d, name)


# ---------------------------------------------------------------- what the shared data must cover
def test_the_shared_data_covers_the_paths():
    assert any(n >= 512 for n in R.SIZES) and any(n % 512 for n in R.SIZES) and any(n % 2048 == 0 for n in R.SIZES)
    assert any(n < 4 for n in R.SIZES) and any(n > 2048 and n % 2048 for n in R.SIZES)
    tpl = 64
    assert [len(R.boundary_sizes(n)) for n in (tpl - 1, tpl, tpl + 1, 2 * tpl + 1)] == [63, 64, 65, 129]
    assert all(1 <= n <= 40 for n in R.boundary_sizes(129))
    for k in range(R.STEPS):
        gs = R.grads(step=k)
        with np.errstate(all="ignore"):
            sq = np.concatenate([(g * g).astype(F) for g in gs])
        assert ((sq > 0) & (sq < 2.0 ** -126)).any(), "no denormal g * g"
        assert (sq > 2.0 ** 30).any() and (sq >= 2.0 ** -126).any()
        norm = R.norm32(gs)
        assert np.isfinite(norm) and 1.0 < norm < 2.0 ** 100        # clip (max_norm 1): norm > max_norm; clip_loose (2^100): norm < max_norm
        assert R.coef32(norm, 1.0) < 1 and R.coef32(norm, 2.0 ** 100) == 1 and R.coef32(norm, 2.0 ** 100, clamp=False) > 1
    # the skip cases: the planted NaN makes exactly one step's norm non-finite, and the run continues as if it never happened
    d = R.CASES["adam-skip"]
    with_nan, clean = R.run32(d, nan_at=NAN_AT), R.run32(d)
    assert [st["skipped"] for _, st in with_nan] == [0, 0, 1, 1, 1] and [st["step"] for _, st in with_nan] == [1, 2, 2, 3, 4]
    assert np.isnan(with_nan[2][1]["norm"]) and all(st["skipped"] == 0 for _, st in clean)
    R.assert_same(with_nan[2][0], R.state_words(dict(with_nan[1][1], skipped=1, norm=F(np.nan))), with_nan[1][0],
                  dict(with_nan[1][1], skipped=1, norm=F(np.nan)), d)
