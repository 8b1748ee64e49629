"""Marginal covariances of the global pose graph on the device (lili_pose_graph_marginals, PoseGraph.marginals / relative_covariance; DESIGN.md §7k "Marginal
covariances") against the referee (tests/pose_graph_marginals_model.py) on the graphs of tests/pose_graph_cases.py and tests/pose_graph_many_loops_cases.py:
  model        every case is solved on the device first with its own options (the linearisation point is a converged one: the solve's gate would end there), then every
               requested block within max(10 D0(case), 64 eps) of the model block's largest entry, D0 = the spread of the model's own routes at the same estimates;
               every node where the dense routes fit, the designed subset beyond (pose_graph_marginals_model.case_nodes); the pairs of case_pairs;
  properties   with no model in the loop: symmetric, positive definite blocks; the two orders of a pair are transposes bit for bit; information never hurts; the
               relative covariance of neighbours on a zero-residual chain is the odometry's;
  behaviour    the same bytes on every run and whatever "pose_graph_max_loops" says, nothing disturbed (estimates, a following solve), sub-ranges are slices, the
               non-positive pivot, refusals;
  full size    N = LILI_PG_MAX_NODES with 4 loops.
The loop cap (12 360 reduced unknowns) is run by tools/pose_graph_marginals_time.py only: its CPU referee is too slow for a test.  The referees are computed once per
session.  The measured device / bound ratios are in DESIGN.md §7k."""
import ctypes as C

import numpy as np
import pytest

import lili_om_amd as L
from lili_om_amd import api
from tests import pose_graph_cases as Cs
from tests import pose_graph_many_loops_cases as Ms
from tests import pose_graph_marginals_model as MM
from tests import pose_graph_model as M

pytestmark = pytest.mark.gpu

EPS = MM.EPS
_SMALL = ["n1_prior_only", "n2", "n3_loop_2_0", "chain_511", "chain_512", "chain_513", "chain_1025", "endpoint_node0", "endpoint_last_from_lt_to",
          "endpoint_on_multiple_of_S", "endpoints_either_side_of_S", "adjacent_endpoints", "shared_endpoint", "same_pair_twice", "both_directions",
          "crossing_and_nested", "max_loops", "strong_loop"]
_MANY = ["loops_64_sep128", "loops_64_sep129", "tile_edge_858", "tile_edge_864", "tile_edge_870", "loops_200"]
BY = {c["name"]: c for c in Cs.solve_cases() + Ms.designed_cases()}
CASES = [BY[n] for n in _SMALL + _MANY]
IDS = [c["name"] for c in CASES]


@pytest.fixture()
def pg(gpu_ctx):
    """a graph that takes LILI_PG_MAX_LOOPS_EXT loops; the context goes back to the default afterwards"""
    g = L.PoseGraph(gpu_ctx, max_loops=api.PG_MAX_LOOPS_EXT)
    g.reset()
    yield g
    g.reset()
    gpu_ctx.set_option("pose_graph_max_loops", api.PG_MAX_LOOPS)


def _load(pg, c, loops=True):
    pg.reset()
    assert pg.append(c["poses"]) == 0
    for a, b, m, v in (c["loops"] if loops else []):
        pg.add_loop(a, b, m, v)
    if c["estimates"] is not None:
        pg.set_poses(c["estimates"])


def _solved(pg, c):
    _load(pg, c)
    s = pg.solve(pg.options(**c["options"]))
    assert s["termination"] in M.CONVERGED
    return pg.poses()


def _check_blocks(cov):
    """symmetric to 4 eps of the largest entry, positive definite"""
    cov = cov.reshape(-1, 6, 6)
    assert np.isfinite(cov).all()
    scale = np.abs(cov).reshape(-1, 36).max(axis=1)
    asym = np.abs(cov - np.swapaxes(cov, 1, 2)).reshape(-1, 36).max(axis=1)
    assert (asym <= 4 * EPS * scale).all(), float((asym / scale).max())
    assert (np.linalg.eigvalsh(cov)[:, 0] > 0).all()


# ---------------------------------------------------------------- device against model
@pytest.mark.parametrize("c", CASES, ids=IDS)
def test_marginals_match_model(pg, c):
    X = _solved(pg, c)
    g = Cs.build_model(c)
    nodes, pairs = MM.case_nodes(c), MM.case_pairs(c)
    cov, cross = pg.marginals(pairs=pairs)
    info = pg.last_marginals
    assert pg.poses().tobytes() == X.tobytes()
    assert (info["status"], info["n_nodes"], info["n_loops"]) == (0, g.n, len(g.loops)) and info["reduced_unknowns"] == 6 * len(MM.separators(c))
    cov_m, cross_m, d0, routes = MM.referee(c["name"], g, X, nodes, pairs)
    tol = MM.tolerance(d0)
    e_d, e_x = MM.block_error(cov[nodes], cov_m), MM.block_error(cross, cross_m)
    print(f"marginals [{c['name']}] N {g.n} loops {len(g.loops)} reduced {info['reduced_unknowns']}: {len(nodes)} nodes, {len(pairs)} pairs, routes {routes}; device - model: "
          f"diagonal {e_d:.2e} cross {e_x:.2e} of the block's largest entry (D0 {d0:.2e}, bound {tol:.2e}, ratio {max(e_d, e_x) / tol:.2f}); kernels {info['kernel_ms']:.3f} ms")
    _check_blocks(cov)
    # (i, i) is the diagonal block; the two orders of a pair are transposes of each other bit for bit
    where = {p: k for k, p in enumerate(pairs)}
    both = 0
    for (i, j), k in where.items():
        if i == j:
            assert cross[k].tobytes() == cov[i].tobytes()
        elif (j, i) in where:
            assert cross[k].tobytes() == np.ascontiguousarray(cross[where[(j, i)]].T).tobytes()
            both += 1
    assert both >= 2 or g.n < 2
    assert e_d <= tol and e_x <= tol


# ---------------------------------------------------------------- properties with no model in the loop
@pytest.mark.parametrize("name", ["endpoint_node0", "crossing_and_nested"])
def test_information_never_hurts(pg, name):
    c = BY[name]
    X = _solved(pg, c)
    with_loops, _ = pg.marginals()
    _load(pg, c, loops=False)
    pg.set_poses(X)
    without, _ = pg.marginals()
    assert pg.last_marginals["n_loops"] == 0
    lam = np.linalg.eigvalsh(with_loops - without)[:, -1]
    scale = np.abs(without).reshape(-1, 36).max(axis=1)
    print(f"information never hurts [{name}]: largest eigenvalue of Sigma(with loops) - Sigma(without), of the block's largest entry: {float((lam / scale).max()):.2e}")
    assert (lam <= 1e-9 * scale).all()
    assert (np.trace(with_loops, axis1=1, axis2=2) < np.trace(without, axis1=1, axis2=2)).any()      # and the loops do help somewhere


def test_relative_covariance_of_neighbours_on_a_zero_residual_chain(pg):
    _, given = Cs.circuit(600, 77)
    pg.reset()
    pg.append(given)
    for i in (0, 255, 511, 512):      # separator + interior, two interior nodes, interior + the separator on its right, separator 512 + interior
        rel = pg.relative_covariance(i, i + 1)
        err = np.abs(rel - np.diag(M.ODOM_VAR)).max() / M.ODOM_VAR.max()
        print(f"relative covariance ({i}, {i + 1}) - diag(odom_var): {err:.2e}")
        assert err <= 1e-9


# ---------------------------------------------------------------- behaviour
def _raw(pg, first, n, pairs, fill=None):
    """the C call on sentinel-filled buffers -> rc, cov, cross, info"""
    pr = np.ascontiguousarray(pairs, np.int32).reshape(-1, 2)
    cov, cross, info = np.full((max(n, 1), 36), -7.5), np.full((max(len(pr), 1), 36), -7.5), api.PgMarginalsInfo()
    rc = pg.lib.lili_pose_graph_marginals(pg.ctx.h, None, first, n, api._ptr(cov), api._ptr(pr) if len(pr) else None, len(pr), api._ptr(cross) if len(pr) else None, C.byref(info))
    return rc, cov, cross, info


@pytest.mark.parametrize("name", ["max_loops", "tile_edge_864"], ids=["single_workgroup", "blocked"])
def test_same_bytes_on_every_run(pg, name):
    c = BY[name]
    out = []
    for _ in range(2):
        _solved(pg, c)
        cov, cross = pg.marginals(pairs=MM.case_pairs(c))
        out.append(cov.tobytes() + cross.tobytes())
    assert out[0] == out[1]


def test_a_call_disturbs_nothing(pg):
    c = BY["crossing_and_nested"]
    _load(pg, c)
    X0 = pg.poses()
    pg.solve(pg.options(**c["options"]))
    want = pg.poses().tobytes() + bytes(pg.last_summary)
    _load(pg, c)
    pg.marginals(pairs=MM.case_pairs(c))
    assert pg.poses().tobytes() == X0.tobytes()
    pg.solve(pg.options(**c["options"]))
    assert pg.poses().tobytes() + bytes(pg.last_summary) == want


def test_sub_ranges_are_slices(pg):
    c = BY["endpoint_on_multiple_of_S"]
    X = _solved(pg, c)
    n = X.shape[0]
    pairs = MM.case_pairs(c)
    full, cross = pg.marginals(pairs=pairs)
    for first, k in ((0, 1), (100, 50), (511, 3), (n - 1, 1), (0, n)):
        part, _ = pg.marginals(first, k)
        assert part.tobytes() == full[first:first + k].tobytes()
    part, cross2 = pg.marginals(0, 0, pairs=pairs)      # pairs alone
    assert part.shape == (0, 6, 6) and cross2.tobytes() == cross.tobytes()


def test_same_bytes_whatever_the_loop_option_says(pg, gpu_ctx):
    c = BY["max_loops"]      # 32 loops: fits the default
    out = []
    for v in (api.PG_MAX_LOOPS, api.PG_MAX_LOOPS_EXT):
        gpu_ctx.set_option("pose_graph_max_loops", v)
        _solved(pg, c)
        cov, cross = pg.marginals(pairs=MM.case_pairs(c))
        out.append(cov.tobytes() + cross.tobytes())
        pg.reset()
    assert out[0] == out[1]


def test_non_positive_pivot(pg):
    """the overflowing-weight graph of test_pose_graph_many_loops_gpu.test_non_positive_pivot_in_the_blocked_solve: a loop whose squared weight overflows makes a
    separator's block of the reduced system infinite and the pivot behind it inf - inf"""
    c = BY["loops_64_sep129"]
    _load(pg, c)
    a, b, m, _ = c["loops"][5]
    pg.add_loop(a + 100, b + 100, m, 1e-310)
    before = pg.poses()
    rc, cov, cross, info = _raw(pg, 0, before.shape[0], [(0, 5), (7, 7)])
    assert rc == -6 and info.status == M.NUMERICAL_FAILURE      # LILI_E_NUMERIC
    assert (info.n_nodes, info.n_loops, info.reduced_unknowns) == (600, 65, 6 * 131)
    assert (cov == -7.5).all() and (cross == -7.5).all()
    assert pg.poses().tobytes() == before.tobytes()
    with pytest.raises(L.LiliError):
        pg.marginals()
    assert pg.last_marginals["status"] == M.NUMERICAL_FAILURE
    # and the context goes on: the same graph without that loop
    _solved(pg, c)
    cov, _ = pg.marginals()
    _check_blocks(cov)


def test_refusals(pg, gpu_ctx):
    lib, h, ptr = gpu_ctx.lib, gpu_ctx.h, api._ptr
    # an empty graph
    rc, cov, cross, _ = _raw(pg, 0, 1, [])
    assert rc == -3 and (cov == -7.5).all()
    # ... which is judged behind the options and in front of the range and the pairs
    buf, pr, o = np.full((3, 36), -7.5), np.array([[0, 5]], np.int32), pg.options()
    o.odom_var[2] = 0.0
    assert lib.lili_pose_graph_marginals(h, C.byref(o), 0, 1, ptr(buf), None, 0, None, None) == -1 and b"a variance is not positive" in lib.lili_last_error(h)
    assert lib.lili_pose_graph_marginals(h, None, 4, 1, ptr(buf), ptr(pr), 1, ptr(buf), None) == -3 and b"pose_graph_marginals: the graph is empty" in lib.lili_last_error(h)
    assert (buf == -7.5).all() and pg.info() == (0, 0)
    c = BY["n3_loop_2_0"]
    _load(pg, c)
    X0, cost0 = pg.poses(), pg.evaluate()[0]
    # the options in front of the range, the range in front of the pairs
    assert lib.lili_pose_graph_marginals(h, C.byref(o), 4, 1, ptr(buf), ptr(pr), 1, ptr(buf), None) == -1 and b"a variance is not positive" in lib.lili_last_error(h)
    assert lib.lili_pose_graph_marginals(h, None, 4, 1, ptr(buf), ptr(pr), 1, ptr(buf), None) == -1 and b"range outside the graph" in lib.lili_last_error(h)
    assert lib.lili_pose_graph_marginals(h, None, 0, 1, ptr(buf), ptr(pr), 1, ptr(buf), None) == -1 and b"a pair names a node outside the graph" in lib.lili_last_error(h)
    assert (buf == -7.5).all() and pg.info() == (3, 1) and pg.poses().tobytes() == X0.tobytes() and pg.evaluate()[0] == cost0
    for first, n, pairs in ((0, 4, []), (3, 1, []), (-1, 1, []), (2, 2, []), (0, -1, [(0, 1)]), (0, 0, []), (0, 1, [(0, 3)]), (0, 1, [(-1, 0)]), (0, 3, [(1, 2), (3, 3)])):
        rc, cov, cross, _ = _raw(pg, first, n, pairs)
        assert rc == -1 and (cov == -7.5).all() and (cross == -7.5).all(), (first, n, pairs)
    buf, pr = np.full((3, 36), -7.5), np.array([[0, 1]], np.int32)
    assert lib.lili_pose_graph_marginals(None, None, 0, 3, ptr(buf), None, 0, None, None) == -1
    assert lib.lili_pose_graph_marginals(h, None, 0, 3, None, None, 0, None, None) == -1                   # entries expected, no buffer
    assert lib.lili_pose_graph_marginals(h, None, 0, 3, ptr(buf), None, 1, ptr(buf), None) == -1          # pairs expected
    assert lib.lili_pose_graph_marginals(h, None, 0, 3, ptr(buf), ptr(pr), 1, None, None) == -1           # cross expected
    assert lib.lili_pose_graph_marginals(h, None, 0, 3, ptr(buf), ptr(pr), -1, ptr(buf), None) == -1
    too_many = np.zeros((api.PG_MAX_PAIRS + 1, 2), np.int32)
    big = np.full((api.PG_MAX_PAIRS + 1, 36), -7.5)
    assert lib.lili_pose_graph_marginals(h, None, 0, 0, None, ptr(too_many), api.PG_MAX_PAIRS + 1, ptr(big), None) == -1 and (big == -7.5).all()
    o = pg.options()
    o.odom_var[2] = 0.0
    assert lib.lili_pose_graph_marginals(h, C.byref(o), 0, 3, ptr(buf), None, 0, None, None) == -1
    assert (buf == -7.5).all()
    # what is allowed: no info, n = 0 with pairs, LILI_PG_MAX_PAIRS pairs
    assert lib.lili_pose_graph_marginals(h, None, 0, 3, ptr(buf), None, 0, None, None) == 0 and np.isfinite(buf).all()
    many = np.zeros((api.PG_MAX_PAIRS, 2), np.int32)
    many[:, 0], many[:, 1] = np.arange(api.PG_MAX_PAIRS) % 3, (np.arange(api.PG_MAX_PAIRS) // 3) % 3
    cov, cross = pg.marginals(0, 0, pairs=many)
    assert cov.shape == (0, 6, 6) and cross.shape == (api.PG_MAX_PAIRS, 6, 6) and cross[9:18].tobytes() == cross[0:9].tobytes()


# ---------------------------------------------------------------- one larger run
def test_full_size(pg):
    c = Cs.full_size()
    X = _solved(pg, c)
    g = Cs.build_model(c)
    n = g.n
    cov, _ = pg.marginals()
    info = pg.last_marginals
    print(f"marginals [full size] N {n} loops {len(g.loops)} reduced {info['reduced_unknowns']}: kernels {info['kernel_ms']:.3f} ms")
    _check_blocks(cov)
    sep = MM.separators(c)
    assert len(sep) == 64 + 7 and info["reduced_unknowns"] == 6 * len(sep)      # 64 fixed separators and the loops' eight endpoints, one of which is node 0
    nodes = set(sep) | {(s + (sep[k + 1] if k + 1 < len(sep) else n)) // 2 for k, s in enumerate(sep)}
    nodes |= {int(v) for v in np.random.default_rng(3).integers(0, n, 32)}
    nodes = sorted(nodes)
    cov_m, _, d0, routes = MM.referee(c["name"], g, X, nodes, [])
    tol = MM.tolerance(d0)
    e_d = MM.block_error(cov[nodes], cov_m)
    print(f"   {len(nodes)} nodes, routes {routes}: device - model {e_d:.2e} of the block's largest entry (D0 {d0:.2e}, bound {tol:.2e}, ratio {e_d / tol:.2f})")
    assert e_d <= tol
