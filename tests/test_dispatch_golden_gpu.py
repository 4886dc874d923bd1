"""The GPU half of tests/golden/dispatch_golden.json: the profiler records (s3r_profile_detail(1): aux records nested in their
layer's, in order) of one forward per kernel path of the dispatcher — tests/_dispatch_cases.py holds the table — on zero-filled
buffers.  Every field but `ms` is compared: integers exactly, doubles to a relative 1e-12 (a handful of host double operations on
exact integers: this allows re-association and nothing else).

launch_conv_mfma plans a direct layer's launches against the device's compute-unit count: on a device with another count than
the file's, `launches` and `launch_form` of the direct conv_mfma records are left out, and the test says so."""
import json
import os

import pytest
import torch

from tests import _dispatch_cases as DC

pytestmark = pytest.mark.gpu
F_MFMA = 0


@pytest.fixture(scope="module")
def golden(golden_dir):
    return json.load(open(os.path.join(golden_dir, "dispatch_golden.json")))


@pytest.fixture(scope="module")
def records(s3r):
    return DC.gpu_part(s3r.load_library())


def test_the_golden_covers_every_case(golden):
    assert sorted(golden["gpu"]) == sorted(DC.GPU_IDS)
    assert all(golden["gpu"][i] for i in DC.GPU_IDS)


@pytest.mark.parametrize("cid", DC.GPU_IDS)
def test_profiler_records(golden, records, cid):
    same_device = golden["compute_units"] == torch.cuda.get_device_properties(0).multi_processor_count
    got, want = records[cid], golden["gpu"][cid]
    assert len(got) == len(want), (cid, got, want)
    for i, (g, w) in enumerate(zip(got, want)):
        skip = ()
        if not same_device and w["family"] == F_MFMA and w["algo"] == 0:
            skip = ("launches", "launch_form")
            print(f"\n{cid} record {i}: another compute-unit count than the golden's {golden['compute_units']}: launches and launch_form not compared")
        for k in DC.REC_INTS:
            assert k in skip or g[k] == w[k], (cid, i, k, g, w)
        for k in DC.REC_DOUBLES:
            assert abs(g[k] - w[k]) <= 1e-12 * abs(w[k]), (cid, i, k, g, w)
