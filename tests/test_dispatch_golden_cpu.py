"""The host-only half of tests/golden/dispatch_golden.json: for every descriptor of tests/_buffer_cases.py::CONV_CASES and the
linear rows of tests/_linear_cases.py, the answers of the five size queries, and — where the layer needs scratch — the return code and
the s3r_last_error() text of s3r_conv_forward called without it and with one float too few.  Compared EXACTLY: the file was written
(tests/golden/make_dispatch_golden.py) by the build before the dispatcher was taken apart, and holds results only."""
import json
import os

import pytest

from tests import _dispatch_cases as DC


@pytest.fixture(scope="module")
def lib(s3r):
    return s3r.load_library()


@pytest.fixture(scope="module")
def golden(golden_dir):
    doc = json.load(open(os.path.join(golden_dir, "dispatch_golden.json")))
    assert doc["generated_at_commit"] not in ("", "unknown")
    return doc["host"]


def test_the_golden_covers_every_case(golden):
    assert sorted(golden["sizes"]) == sorted(c.id for c in DC.HOST_CASES)
    assert len(golden["refusals"]) >= 100 and set(golden["refusals"]) <= set(golden["sizes"])
    for cid, r in golden["refusals"].items():      # every one IS a workspace refusal that states the need
        assert golden["sizes"][cid]["scratch_elems"] > 0
        for rc, text in r.values():
            assert rc == -3 and str(golden["sizes"][cid]["scratch_elems"]) in text and "got" in text, (cid, rc, text)


@pytest.mark.parametrize("case", DC.HOST_CASES, ids=[c.id for c in DC.HOST_CASES])
def test_size_answers_and_scratch_refusals(lib, golden, case):
    assert DC.sizes(lib, case) == golden["sizes"][case.id]
    assert DC.refusals(lib, case) == golden["refusals"].get(case.id)
