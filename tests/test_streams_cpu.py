"""The case table of tests/test_streams_gpu.py against include/s3r.h: no entry point that takes a stream can skip the two
instruments, every training entry has its refused call, every case stays under the size cap, every pre-state is one the header
allows the library to read.  Host-only: size queries plan without a device."""
import os

import pytest
import torch

from tests import _stream_cases as SC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib(s3r):
    return s3r.load_library()


@pytest.fixture(scope="module")
def protos():
    with open(os.path.join(ROOT, "include", "s3r.h")) as f:
        return SC.stream_prototypes(f.read())


@pytest.fixture(scope="module")
def plans(lib):
    return {c.id: c.plan(lib, None) for c in SC.CASES}


def test_parser_finds_the_stream_taking_prototypes(protos, s3r):
    """the parse agrees with the ctypes table: the prototypes whose LAST argument is a pointer named stream"""
    assert len(protos) == 23, sorted(protos)
    assert {"s3r_conv_pack_weights", "s3r_chain_forward", "s3r_head_backward", "s3r_disparity_metrics"} <= set(protos)
    assert not {"s3r_conv_scratch_elems", "s3r_profile_read", "s3r_last_error"} & set(protos)
    for name in protos:
        assert name in s3r._lib.SIGNATURES


@pytest.mark.parametrize("instrument", list(SC.INSTRUMENTS))
def test_every_stream_taking_entry_is_under_both_instruments(protos, instrument):
    covered = {e for c in SC.INSTRUMENTS[instrument] for e in c.entries}
    print(f"\n{instrument}: {len(SC.INSTRUMENTS[instrument])} cases cover {sorted(covered)}")
    assert covered == set(protos), (sorted(set(protos) - covered), sorted(covered - set(protos)))


def test_every_training_entry_has_a_refused_call(plans):
    assert {c.entries[0] for c in SC.REFUSALS if c.id != SC.CONV_AT_THE_LDS_LIMIT} == set(SC.TRAINING)
    assert SC.BY_ID[SC.CONV_AT_THE_LDS_LIMIT] in SC.REFUSALS          # ... and the forward's refusal past the two-axis form's LDS limit
    for c in SC.REFUSALS:
        assert plans[c.id].refuse is not None, c.id
    # a refused call that leaves its outputs untouched needs outputs to look at
    assert all(any(a.role == "out" for a in plans[c.id].args) for c in SC.REFUSALS)


def test_every_family_has_its_misplaced_stream_case():
    assert sorted(c.family for c in SC.MUTANTS) == sorted(SC.FAMILIES)


def test_case_ids_are_unique():
    assert len(SC.BY_ID) == len(SC.CASES)


@pytest.mark.parametrize("case", SC.CASES, ids=[c.id for c in SC.CASES])
def test_case_stays_under_the_cap_and_its_prestates_are_safe(plans, protos, case):
    plan = plans[case.id]
    assert 0 < plan.nbytes <= SC.CAP_BYTES, (case.id, plan.nbytes)
    assert len({a.name for a in plan.args}) == len(plan.args)
    comment = " ".join(protos[e] for e in case.entries)
    for a in plan.args:
        assert a.role in ("in", "out", "zero", "scr"), a
        assert SC.safe_prestate(a, comment) is not None, (case.id, a.name, "this pre-state is not documented as safe to read")
    assert any(a.role in ("out", "zero") for a in plan.args)


def test_prestate_patterns_differ_from_every_fill():
    """an input's pre-state is the poison, which no data set holds; an output's pre-state differs from the poison the stream fills it
    with, so a fill that ran shows — the scratch NaN for floats, the halo sentinel for int32, whose poison is its guard pattern"""
    from tests import _guard as G
    for dt in (torch.float32, torch.bfloat16):
        b = G._BITS[dt]
        assert SC.prestate(SC.Arg("x", (1,), dt, "in")) == b[2] and SC.prestate(SC.Arg("y", (1,), dt, "out")) == b[4] != b[2]
    b = G._BITS[torch.int32]
    assert SC.prestate(SC.Arg("i", (1,), torch.int32, "in")) == b[1]
    assert SC.prestate(SC.Arg("n", (1,), torch.int32, "out")) == b[3] != b[2] and b[3] < 0
    assert SC.safe_prestate(SC.Arg("i", (1,), torch.int32, "in"), "no promise here") is None


def test_every_output_of_the_table_has_a_prestate_that_its_fill_changes(plans):
    from tests import _guard as G
    for cid, plan in plans.items():
        for a in plan.args:
            if a.role == "out":
                assert SC.prestate(a) != G._BITS[a.dtype][2], (cid, a.name)


# the prototypes whose own comment says what a NaN does; the others' float pre-states rest on "a float is never an address"
NAN_DOCUMENTED = {"s3r_linear_backward", "s3r_chamfer_forward", "s3r_chamfer_backward", "s3r_voxel_iou", "s3r_voxel_bce_forward",
                  "s3r_voxel_bce_backward", "s3r_head_backward"}


def test_float_prestates_follow_the_headers_nan_wording(protos):
    x = SC.Arg("x", (1,), torch.float32, "in")
    got = {name for name, comment in protos.items() if SC.safe_prestate(x, comment) == "NaN (header)"}
    assert got == NAN_DOCUMENTED, (sorted(got - NAN_DOCUMENTED), sorted(NAN_DOCUMENTED - got))
    for name in set(protos) - got:
        assert SC.safe_prestate(x, protos[name]) == "NaN (data only)", name
    for dt in (torch.float32, torch.bfloat16):                     # the answer follows the comment, not the type alone
        a = SC.Arg("x", (1,), dt, "in")
        assert SC.safe_prestate(a, "a NaN in x propagates") == "NaN (header)"
        assert SC.safe_prestate(a, "says nothing of it") == "NaN (data only)"


def test_two_slice_shape_is_the_smallest(lib):
    """s3r_linear_backward's grad_x slabs appear with the second 128-o chunk: the scratch query shows them"""
    assert lib.s3r_linear_backward_scratch_elems(2, 33, 128) == 2 * 128
    assert lib.s3r_linear_backward_scratch_elems(2, 33, 129) == 2 * 129 + 2 * 2 * 33


@pytest.mark.parametrize("case", SC.CASES, ids=[c.id for c in SC.CASES])
def test_both_data_sets_fit_the_arguments_and_differ(plans, case):
    plan = plans[case.id]
    d0, d1 = plan.data(0), plan.data(1)
    ins = [a for a in plan.args if a.role == "in"]
    assert ins
    for a in ins:
        for d in (d0, d1):
            assert tuple(d[a.name].shape) == tuple(a.shape) and d[a.name].dtype == a.dtype, (case.id, a.name, d[a.name].shape, a.shape)
    assert any(not torch.equal(d0[a.name], d1[a.name]) for a in ins), "the second set must differ from the one present at capture"
