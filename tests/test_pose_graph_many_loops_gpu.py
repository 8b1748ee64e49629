"""The global pose graph beyond LILI_PG_MAX_LOOPS loops (option "pose_graph_max_loops") against the referee on the graphs of
tests/pose_graph_many_loops_cases.py, by the rules of tests/test_pose_graph_gpu.py:
  cap           the 33rd loop is refused at the default and accepted with the option raised, up to the option's value; the option is not lowered below the loop count;
  evaluate      every block to 1e-12 of its largest entry, as test_evaluate_matches_model;
  solve         iterations, termination, cost sequence; poses within max(10 D0, 64 ulp of the largest coordinate), D0 = the spread of the model's own two solvers;
  full size     1024 loops, 12 360 reduced unknowns: judged by the model's evaluate at the returned poses and by the model's sparse solve;
  bytes         graphs the single-workgroup solve takes return the same bytes with the option raised; two solves of the blocked path return the same bytes;
  failure       a non-positive pivot in the blocked solve ends with NUMERICAL_FAILURE and the poses untouched.
The measured device - model differences are in the docstring of test_solve_matches_model and in DESIGN.md §7k."""
import ctypes as C

import numpy as np
import pytest

import lili_om_amd as L
from lili_om_amd import api
from tests import pose_graph_cases as Cs
from tests import pose_graph_many_loops_cases as Ms
from tests import pose_graph_model as M
from tests.test_pose_graph_gpu import _block_error, _cost_floor, _pose_tolerance

pytestmark = pytest.mark.gpu

CASES = Ms.designed_cases()
IDS = [c["name"] for c in CASES]
BY = {c["name"]: c for c in CASES}


@pytest.fixture()
def pg(gpu_ctx):
    """a graph that takes LILI_PG_MAX_LOOPS_EXT loops; the context goes back to the default afterwards"""
    g = L.PoseGraph(gpu_ctx, max_loops=api.PG_MAX_LOOPS_EXT)
    g.reset()
    yield g
    g.reset()
    gpu_ctx.set_option("pose_graph_max_loops", api.PG_MAX_LOOPS)


def _load(pg, c):
    pg.reset()
    assert pg.append(c["poses"]) == 0
    for a, b, m, v in c["loops"]:
        pg.add_loop(a, b, m, v)
    if c["estimates"] is not None:
        pg.set_poses(c["estimates"])
    assert pg.info() == (c["poses"].shape[0], len(c["loops"]))


def _solve(pg, c):
    _load(pg, c)
    s = pg.solve(pg.options(**c["options"]))
    return pg.poses(), s, bytes(pg.last_summary)


# ---------------------------------------------------------------- the cap
def test_cap_follows_the_option(pg, gpu_ctx):
    lib, h, ptr = gpu_ctx.lib, gpu_ctx.h, api._ptr
    c = BY["loops_33"]
    meas, var = np.ascontiguousarray(c["loops"][0][2]), np.full(6, 0.1)
    # out of range: refused, the value stays
    for v in (api.PG_MAX_LOOPS - 1, api.PG_MAX_LOOPS_EXT + 1, 0, -1):
        assert lib.lili_set_option(h, b"pose_graph_max_loops", v) == -1
    # at the default the 33rd loop is refused and the graph is untouched
    gpu_ctx.set_option("pose_graph_max_loops", api.PG_MAX_LOOPS)
    pg.reset()
    pg.append(c["poses"])
    for a, b, m, v in c["loops"][:api.PG_MAX_LOOPS]:
        pg.add_loop(a, b, m, v)
    X0, cost0 = pg.poses(), pg.evaluate()[0]
    a, b = c["loops"][api.PG_MAX_LOOPS][0:2]
    assert lib.lili_pose_graph_add_loop(h, a, b, ptr(meas), ptr(var)) == -1
    assert b"more than LILI_PG_MAX_LOOPS loops" in lib.lili_last_error(h)
    assert pg.info() == (200, api.PG_MAX_LOOPS) and pg.poses().tobytes() == X0.tobytes() and pg.evaluate()[0] == cost0
    # raised with the graph loaded: the same loop is accepted, up to the new value and not beyond
    gpu_ctx.set_option("pose_graph_max_loops", api.PG_MAX_LOOPS + 8)
    for k in range(8):
        assert lib.lili_pose_graph_add_loop(h, a + k, b + k, ptr(meas), ptr(var)) == 0
    assert lib.lili_pose_graph_add_loop(h, a, b, ptr(meas), ptr(var)) == -1 and pg.info() == (200, api.PG_MAX_LOOPS + 8)
    # not lowered below the loop count (LILI_E_STATE), and the value stays: lowering to the count itself is fine and refuses the next loop
    assert lib.lili_set_option(h, b"pose_graph_max_loops", api.PG_MAX_LOOPS + 7) == -3
    assert lib.lili_set_option(h, b"pose_graph_max_loops", api.PG_MAX_LOOPS) == -3
    gpu_ctx.set_option("pose_graph_max_loops", api.PG_MAX_LOOPS_EXT)
    assert lib.lili_pose_graph_add_loop(h, a, b, ptr(meas), ptr(var)) == 0 and pg.info() == (200, api.PG_MAX_LOOPS + 9)
    gpu_ctx.set_option("pose_graph_max_loops", api.PG_MAX_LOOPS + 9)
    assert lib.lili_pose_graph_add_loop(h, a, b, ptr(meas), ptr(var)) == -1
    # an emptied graph lets the option down again
    pg.reset()
    gpu_ctx.set_option("pose_graph_max_loops", api.PG_MAX_LOOPS)
    # the Python constructor sets it
    g2 = L.PoseGraph(gpu_ctx, max_loops=40)
    g2.append(c["poses"])
    for a, b, m, v in c["loops"]:
        g2.add_loop(a, b, m, v)
    assert g2.info() == (200, 33)
    with pytest.raises(L.LiliError):
        L.PoseGraph(gpu_ctx, max_loops=api.PG_MAX_LOOPS_EXT + 1)


def test_cap_at_the_largest_value(pg, gpu_ctx):
    c = BY["loops_33"]
    pg.append(c["poses"])
    a, b, m, v = c["loops"][0]
    for k in range(api.PG_MAX_LOOPS_EXT):
        pg.add_loop(10 + k % 150, 199 - k % 7, m, v)
    assert gpu_ctx.lib.lili_pose_graph_add_loop(gpu_ctx.h, a, b, api._ptr(np.ascontiguousarray(m)), api._ptr(np.full(6, 0.1))) == -1
    assert pg.info() == (200, api.PG_MAX_LOOPS_EXT)


# ---------------------------------------------------------------- evaluate
@pytest.mark.parametrize("c", CASES, ids=IDS)
def test_evaluate_matches_model(pg, c):
    _load(pg, c)
    g = Cs.build_model(c)
    cost_m, g_m, D_m, S_m, LB_m = g.evaluate()
    cost, grad, D, S, LB = pg.evaluate(pg.options())
    dc = abs(cost - cost_m) / cost_m
    dg = np.abs(grad - g_m).max() / np.abs(g_m).max()
    dD, dS, dL = _block_error(D, D_m), _block_error(S, S_m), _block_error(LB, LB_m)
    print(f"evaluate [{c['name']}]: cost {dc:.2e} gradient {dg:.2e} diagonal {dD:.2e} sub {dS:.2e} loop {dL:.2e} (of the largest entry per block)")
    assert dc <= 1e-12 and dg <= 1e-12 and dD <= 1e-12 and dS <= 1e-12 and dL <= 1e-12
    assert (D == np.swapaxes(D, 1, 2)).all()


# ---------------------------------------------------------------- solve
@pytest.mark.parametrize("c", CASES, ids=IDS)
def test_solve_matches_model(pg, c):
    """Measured on MI355X, device - model (position m / angle rad), D0 in brackets:
    loops_33 6.3e-15 (6.8e-15) / 1.1e-15 (6.7e-16); loops_64_sep128 3.3e-15 (1.4e-14) / 1.0e-15 (3.0e-15); loops_64_sep129 4.4e-15 (9.8e-15) / 1.4e-15 (1.3e-15);
    tile_edge_858 5.4e-15 (2.7e-15) / 1.8e-15 (1.0e-15); tile_edge_864 6.2e-15 (4.0e-15) / 1.1e-15 (1.1e-15); tile_edge_870 4.4e-15 (5.6e-15) / 8.9e-16 (2.0e-15);
    tile_edge_954 3.6e-15 (2.7e-15) / 1.9e-15 (1.1e-15); tile_edge_960 5.9e-15 (6.1e-15) / 1.6e-15 (1.0e-15); tile_edge_966 3.8e-15 (8.9e-15) / 1.1e-15 (1.6e-15);
    loops_200 8.9e-15 (5.8e-15) / 1.7e-15 (9.0e-16); many_shared_endpoint 5.2e-15 (3.4e-15) / 2.2e-15 (1.0e-15); many_adjacent_endpoints 3.8e-15 (3.1e-15) / 1.1e-15 (1.0e-15).
    The bound is max(10 D0, 64 ulp of the largest coordinate = 5.7e-14): no case needs more than a sixth of it."""
    g, X_m, s_m, d0 = Cs.reference(c)
    assert Cs.decisions_clear(s_m)
    X, s, _ = _solve(pg, c)
    dp, da = M.pose_difference(X, X_m)
    tp, ta = _pose_tolerance(d0, X_m)
    print(f"solve [{c['name']}] N {g.n} loops {len(g.loops)} reduced {6 * c['n_sep']}: iterations {s['iterations']} (model {s_m['iterations']}) termination {s['termination']} "
          f"(model {s_m['termination']}) cost {s['initial_cost']:.9e} -> {s['final_cost']:.9e} (model {s_m['initial_cost']:.9e} -> {s_m['final_cost']:.9e}); device - model: position "
          f"{dp:.2e} m (D0 {d0[0]:.2e}, bound {tp:.2e}), angle {da:.2e} rad (D0 {d0[1]:.2e}, bound {ta:.2e}); kernels {pg.kernel_ms():.3f} ms")
    print("   costs device", [f"{v:.9e}" for v in s["cost"]], "model", [f"{v:.9e}" for v in s_m["cost"]])
    assert (s["n_nodes"], s["n_loops"]) == (g.n, len(g.loops))
    assert s["iterations"] == s_m["iterations"] and s["termination"] == s_m["termination"]
    floor = _cost_floor(g)
    for a, b in zip([s["initial_cost"], s["final_cost"]] + s["cost"], [s_m["initial_cost"], s_m["final_cost"]] + s_m["cost"]):
        assert abs(a - b) <= 1e-6 * b or max(a, b) <= floor, (a, b, floor)
    assert len(s["grad_inf"]) == len(s_m["grad_inf"])
    assert dp <= tp and da <= ta


def test_full_size_1024_loops(pg):
    c = Ms.loops_1024()
    g = Cs.build_model(c)
    X_m, s_m = M.gauss_newton(g, solver="sparse", **c["options"])
    assert Cs.decisions_clear(s_m)
    X, s, _ = _solve(pg, c)
    c0, g0 = g.evaluate()[0:2]
    c1, g1 = g.evaluate(X)[0:2]
    r = np.abs(g1).max() / np.abs(g0).max()
    dp, da = M.pose_difference(X, X_m)
    print(f"full size N {g.n} loops {len(g.loops)} reduced {6 * c['n_sep']}: iterations {s['iterations']} (model {s_m['iterations']}) termination {s['termination']} cost "
          f"{s['initial_cost']:.9e} -> {s['final_cost']:.9e} (model's evaluate: {c0:.9e} -> {c1:.9e}), model's |g|inf {np.abs(g0).max():.2e} -> {np.abs(g1).max():.2e} ({r:.1e}); "
          f"device - model's sparse solve: position {dp:.2e} m angle {da:.2e} rad; kernels {pg.kernel_ms():.2f} ms")
    print("   costs", [f"{v:.9e}" for v in s["cost"]], "model", [f"{v:.9e}" for v in s_m["cost"]], "steps", [f"{v:.1e}" for v in s["step_inf"]])
    costs = [s["initial_cost"]] + s["cost"]
    assert all(b <= a for a, b in zip(costs, costs[1:])) and c1 <= c0
    assert s["termination"] in M.CONVERGED
    assert r <= 1e-6
    assert s["iterations"] == s_m["iterations"] and s["termination"] == s_m["termination"]
    floor = _cost_floor(g)
    for a, b in zip(costs + [s["final_cost"]], [s_m["initial_cost"]] + s_m["cost"] + [s_m["final_cost"]]):
        assert abs(a - b) <= 1e-6 * b or max(a, b) <= floor, (a, b, floor)


# ---------------------------------------------------------------- bytes
def test_raised_option_returns_the_same_bytes(gpu_ctx):
    """what the single-workgroup solve takes is solved by it whatever the option says: every case of the 32-loop suite, and 768 unknowns from 64 loops (which the
    default cannot hold: there the comparison is between the option at 64 and at its largest value)"""
    g = L.PoseGraph(gpu_ctx)
    try:
        for c in Cs.solve_cases():
            runs = []
            for cap in (api.PG_MAX_LOOPS, api.PG_MAX_LOOPS_EXT):
                g.reset()
                gpu_ctx.set_option("pose_graph_max_loops", cap)
                runs.append(_solve(g, c))
            assert runs[0][0].tobytes() == runs[1][0].tobytes() and runs[0][2] == runs[1][2], c["name"]
        c = BY["loops_64_sep128"]
        runs = []
        for cap in (64, api.PG_MAX_LOOPS_EXT):
            g.reset()
            gpu_ctx.set_option("pose_graph_max_loops", cap)
            runs.append(_solve(g, c))
        assert runs[0][0].tobytes() == runs[1][0].tobytes() and runs[0][2] == runs[1][2]
        assert runs[0][1]["termination"] in M.CONVERGED
    finally:
        g.reset()
        gpu_ctx.set_option("pose_graph_max_loops", api.PG_MAX_LOOPS)


def test_two_blocked_solves_from_reset_return_the_same_bytes(pg):
    out = []
    for name in ("loops_64_sep129", "tile_edge_870"):
        runs = [_solve(pg, BY[name]) for _ in range(2)]
        assert runs[0][0].tobytes() == runs[1][0].tobytes() and runs[0][2] == runs[1][2], name
        out.append(runs[0][0].tobytes())
    assert out[0] != out[1]


# ---------------------------------------------------------------- numerical failure
def test_non_positive_pivot_in_the_blocked_solve(pg):
    """One loop whose variance is so small that its squared weight overflows: the segments' pivots are finite and positive (a loop touches separators only), the
    separator's diagonal block of the reduced system is infinite, and the pivot behind it is inf - inf: not positive.  129 separators: the blocked solve."""
    c = BY["loops_64_sep129"]
    _load(pg, c)
    a, b, m, _ = c["loops"][5]
    pg.add_loop(a + 100, b + 100, m, 1e-310)      # two more separators, in the middle of the matrix
    before = pg.poses()
    s = pg.solve(pg.options(**c["options"]))
    assert s["termination"] == M.NUMERICAL_FAILURE and s["iterations"] == 0
    assert pg.poses().tobytes() == before.tobytes()
    # and the context goes on: the same graph without that loop solves
    X, s, _ = _solve(pg, c)
    assert s["termination"] in M.CONVERGED
