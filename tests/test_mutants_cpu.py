"""The kernel-mutant table (tests/mutants/table.py) against today's sources, without a GPU: a kernel change that moves an anchor,
or a test rename that empties a `kills` entry, fails HERE and names the stale mutant."""
import os
import re
import runpy
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "stereo-3d-reconstruction_amd", "csrc")
MUTANTS = runpy.run_path(os.path.join(ROOT, "tests", "mutants", "table.py"))["MUTANTS"]
IDS = [m["id"] for m in MUTANTS]
# what a mutant may not contain: it changes values, never synchronisation, LDS-DMA, launches or assembly
FORBIDDEN = ["__syncthreads", "waitcnt", "barrier", "buffer_load_lds", "hipLaunchKernelGGL", "asm", "<<<"]
# (s3r_wino_gemm.hip has no entry of its own: s3r_wino.h's mutants rebuild it, and its serial form is in their kills;
#  nor has s3r_bf16_plane.hip: s3r_bf16.h's mutant rebuilds it, and its tiles 22 and 6 are in that mutant's kills)
FILES_NAMED = ["s3r_conv_glds.hip", "s3r_wino.h", "s3r_wino_axis1.hip", "s3r_wino_axis2.hip", "s3r_wino_handoff.hip",
               "s3r_deconv_wino3.hip", "s3r_bf16.h", "s3r_bf16_tap.hip", "s3r_conv_bf16.hip", "s3r_pointwise.hip", "s3r_general.hip", "s3r_ordered.h", "s3r_chamfer.hip",
               "s3r_disparity.hip", "s3r_batchnorm.hip", "s3r_voxel_loss.hip", "s3r_conv_bwd.hip", "s3r_cost_volume_bwd.hip"]


def _srcs():
    with open(os.path.join(CSRC, "Makefile")) as f:
        return re.search(r"^SRCS\s*:=\s*(.*)$", f.read(), re.M).group(1).split()


def split_kills(kills):
    """kills -> (node ids, the -k expression or None)"""
    if "-k" in kills:
        i = kills.index("-k")
        assert kills.count("-k") == 1 and i == len(kills) - 2, "one -k expression, at the end"
        return kills[:i], kills[i + 1]
    return list(kills), None


def test_table_shape():
    assert len(MUTANTS) >= 25
    assert len(set(IDS)) == len(IDS), "mutant ids are not unique"
    for m in MUTANTS:
        assert set(m) <= {"id", "file", "anchor", "replacement", "kills", "models", "equivalent"}, m["id"]
        assert re.fullmatch(r"[a-z0-9_]+", m["id"]), m["id"]
        assert m["kills"] and m["models"].strip(), m["id"]
        nodes, _ = split_kills(m["kills"])
        assert nodes and all(n.startswith("tests/test_") for n in nodes), m["id"]
    equivalent = [m["id"] for m in MUTANTS if m.get("equivalent")]
    assert len(equivalent) <= 2, equivalent
    assert {m["file"] for m in MUTANTS} >= set(FILES_NAMED), "a file the table must cover has no mutant"


def test_every_file_is_built_by_the_makefile():
    srcs = _srcs()

    def users(header):
        """the units of SRCS that include a header of csrc/"""
        if not header.endswith(".h") or not os.path.isfile(os.path.join(CSRC, header)):
            return []
        return [u for u in srcs if re.search(r'^#include "%s"' % re.escape(header), open(os.path.join(CSRC, u)).read(), re.M)]

    for m in MUTANTS:
        assert m["file"] in srcs or users(m["file"]), (m["id"], m["file"])
    assert set(users("s3r_wino.h")) == {"s3r_wino_axis1.hip", "s3r_wino_gemm.hip", "s3r_wino_axis2.hip", "s3r_wino_handoff.hip"}
    assert set(users("s3r_bf16.h")) == {"s3r_bf16_tap.hip", "s3r_bf16_plane.hip", "s3r_conv_bf16.hip", "s3r_plan_params.hip"}


@pytest.mark.parametrize("m", MUTANTS, ids=IDS)
def test_anchor_occurs_once_and_the_replacement_differs(m):
    with open(os.path.join(CSRC, m["file"])) as f:
        text = f.read()
    assert text.count(m["anchor"]) == 1, f"mutant {m['id']} is stale: its anchor occurs {text.count(m['anchor'])} times in {m['file']}"
    assert m["replacement"] != m["anchor"]
    assert text.replace(m["anchor"], m["replacement"]) != text


@pytest.mark.parametrize("m", MUTANTS, ids=IDS)
def test_no_mutant_touches_synchronisation_dma_launches_or_assembly(m):
    for word in FORBIDDEN:
        assert word not in m["anchor"] and word not in m["replacement"], (m["id"], word)


def test_the_build_tool_refuses_a_stale_anchor(tmp_path):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import build_mutants
    finally:
        sys.path.pop(0)
    with open(os.path.join(CSRC, "s3r_ordered.h")) as f:
        text = f.read()
    with pytest.raises(SystemExit, match="occurs 0 times"):
        build_mutants.mutate(text, dict(id="stale", file="s3r_ordered.h", anchor="no such text", replacement="x"))
    with pytest.raises(SystemExit, match="not once"):
        build_mutants.mutate(text, dict(id="twice", file="s3r_ordered.h", anchor="float", replacement="double"))
    for header in ("s3r_ordered.h", "s3r_wino.h"):
        assert build_mutants.header_users(header) and all(u in _srcs() for u in build_mutants.header_users(header)), header
    assert build_mutants.header_users("no_such.h") == []


def test_every_kills_entry_collects():
    """one child per distinct kills list (pytest --collect-only): every node id exists and every -k expression selects something"""
    seen = {}
    for m in MUTANTS:
        seen.setdefault(tuple(m["kills"]), m["id"])
    env = dict(os.environ, PYTHONDONTWRITEBYTECODE="1")
    todo = list(seen.items())
    for i in range(0, len(todo), 4):                # four children at a time
        procs = [(mid, kills, subprocess.Popen([sys.executable, "-m", "pytest", "--collect-only", "-q", "-p", "no:cacheprovider", *kills],
                                               cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True))
                 for kills, mid in todo[i:i + 4]]
        for mid, kills, p in procs:
            out, _ = p.communicate()
            assert p.returncode == 0, f"mutant {mid}: {kills} does not collect:\n{out[-2000:]}"
            n = re.search(r"(\d+)(?:/\d+)? tests? collected", out)
            assert n and int(n.group(1)) >= 1, f"mutant {mid}: {kills} selects no test:\n{out[-2000:]}"
            for node in split_kills(list(kills))[0]:        # every node id by itself, not only their union
                assert node.split("::")[0] + "::" in out, f"mutant {mid}: {node} collected nothing"
