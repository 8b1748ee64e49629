"""The many-loop pose graphs (tests/pose_graph_many_loops_cases.py) on the referee alone: the generator builds the separator counts it was designed for, the model
solves every case with every stop decision clear of its threshold, and the header, lili_om_amd.api and the option's range agree."""
import os
import re
import subprocess

import pytest

from lili_om_amd import api
from tests import pose_graph_cases as Cs
from tests import pose_graph_many_loops_cases as Ms
from tests import pose_graph_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = Ms.designed_cases()
IDS = [c["name"] for c in CASES]


def test_separator_counts_are_as_designed():
    got = {c["name"]: len(Ms.separators(c)) for c in CASES}
    assert got == {c["name"]: c["n_sep"] for c in CASES}
    by = {c["name"]: c for c in CASES}
    assert len(by["loops_33"]["loops"]) == api.PG_MAX_LOOPS + 1 and 6 * got["loops_33"] == 402
    assert 6 * got["loops_64_sep128"] == api.PG_MAX_REDUCED and 6 * got["loops_64_sep129"] == api.PG_MAX_REDUCED + 6
    assert len(by["loops_64_sep128"]["loops"]) == 64 and len(by["loops_64_sep129"]["loops"]) == 64
    assert len(by["loops_200"]["loops"]) == 200 and got["loops_200"] == 403
    # the tile edges: k T - 6, k T, k T + 6 for the first k past the single-workgroup solve, and for k + 1
    T = api.PG_REDUCED_TILE
    k = api.PG_MAX_REDUCED // T + 1
    assert (k - 1) * T <= api.PG_MAX_REDUCED < k * T
    edges = [6 * got[n] for n in IDS if n.startswith("tile_edge_")]
    assert edges == [k * T - 6, k * T, k * T + 6, (k + 1) * T - 6, (k + 1) * T, (k + 1) * T + 6]
    # a separator pair with several loops, both orientations among them; loops between adjacent nodes
    pairs = [(a, b) for a, b, _, _ in by["many_shared_endpoint"]["loops"]]
    assert pairs.count((330, 20)) == 2 and (21, 331) in pairs and (331, 21) in pairs and sum(1 for _, b in pairs if b == 20) >= 4
    assert any(abs(a - b) == 1 for a, b, _, _ in by["many_adjacent_endpoints"]["loops"])
    # every case but the first needs the raised cap; all fit it
    assert all(api.PG_MAX_LOOPS < len(c["loops"]) <= api.PG_MAX_LOOPS_EXT for c in CASES)
    full = Ms.loops_1024()
    assert len(full["loops"]) == api.PG_MAX_LOOPS_EXT and len(Ms.separators(full)) == full["n_sep"] == 2060
    assert 6 * 2060 <= 6 * (2 * api.PG_MAX_LOOPS_EXT + api.PG_MAX_NODES // api.PG_SEGMENT) == 12672


@pytest.mark.parametrize("c", CASES, ids=IDS)
def test_model_solves_with_clear_decisions(c):
    g, X, s, d0 = Cs.reference(c)
    print(f"model [{c['name']}] N {g.n} loops {len(g.loops)} separators {c['n_sep']}: iterations {s['iterations']} termination {s['termination']} cost {s['initial_cost']:.9e} -> "
          f"{s['final_cost']:.9e}; D0 position {d0[0]:.2e} m angle {d0[1]:.2e} rad")
    assert s["termination"] in M.CONVERGED and s["final_cost"] < s["initial_cost"]
    assert Cs.decisions_clear(s), s["margins"]


def test_model_solves_the_full_size_case_with_clear_decisions():
    c = Ms.loops_1024()
    X, s = M.gauss_newton(Cs.build_model(c), solver="sparse", **c["options"])
    assert s["termination"] in M.CONVERGED and s["iterations"] == 4 and Cs.decisions_clear(s), s["margins"]


def test_constants_agree(tmp_path):
    """LILI_PG_MAX_LOOPS_EXT in the header = api.PG_MAX_LOOPS_EXT = the option's upper end; the tile and the single-workgroup bound of lili_kernels.h = api's"""
    src = tmp_path / "c.c"
    src.write_text('#include <stdio.h>\n#include "lili_hip.h"\nint main(void){printf("%d %d\\n", LILI_PG_MAX_LOOPS, LILI_PG_MAX_LOOPS_EXT);return 0;}')
    exe = tmp_path / "c"
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    assert [int(v) for v in subprocess.check_output([str(exe)]).split()] == [api.PG_MAX_LOOPS, api.PG_MAX_LOOPS_EXT] == [32, 1024]
    kern = open(os.path.join(ROOT, "lili_om_amd", "csrc", "lili_kernels.h")).read()
    assert int(re.search(r"kPgMaxReduced = (\d+);", kern).group(1)) == api.PG_MAX_REDUCED == Ms.MAX_REDUCED
    T = int(re.search(r"kPgTile = (\d+),", kern).group(1))
    assert T == api.PG_REDUCED_TILE == Ms.TILE and T % 6 == 0 and T % 16 == 0
    assert Ms.MAX_LOOPS_EXT == api.PG_MAX_LOOPS_EXT
    # the option's range, as lili_set_option checks it
    body = open(os.path.join(ROOT, "lili_om_amd", "csrc", "lili_api.hip")).read()
    body = body[body.index('"pose_graph_max_loops") == 0'):]
    assert "value < LILI_PG_MAX_LOOPS || value > LILI_PG_MAX_LOOPS_EXT" in body[:400]
    # the option is set by the GPU tests of this feature
    assert 'set_option("pose_graph_max_loops"' in open(os.path.join(ROOT, "tests", "test_pose_graph_many_loops_gpu.py")).read()
