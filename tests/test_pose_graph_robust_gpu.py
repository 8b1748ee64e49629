"""Robust loop factors and the damped solve on the device (lili_pose_graph_add_loop_robust, lili_pose_graph_loop_status, lili_pose_graph_solve_lm)
against the referee (tests/pose_graph_robust_model.py) on the graphs of tests/pose_graph_robust_cases.py, judged as tests/test_pose_graph_gpu.py judges:
  evaluate      cost and gradient to 1e-12 of the largest entry, every block to 1e-12 of that block's largest entry, the diagonal blocks symmetric;
  loop_status   chi2 to 1e-12 relative, weight to 1e-12 absolute, a sub-range the slice of the full result byte for byte;
  solve, solve_lm   attempts, termination, the accepted pattern and the lambda sequence (exactly) equal the model's; costs to 1e-6 relative above the cost floor;
                final poses within max(10 D0, 64 ulp), D0 the spread of the model's two linear solvers;
  the effect    a loss leaves the device's solution at most a fifth as far from the device's own clean solve as its plain solve; every false loop ends <= 0.05;
  marginals     n40 with Cauchy loops against the dense inverse of the model's weighted H;
  nothing that exists moves, two runs return the same bytes, and every refusal leaves the graph, the estimates and the output buffers untouched.
The model's solves are computed once per case (pose_graph_robust_cases.reference) and shared."""
import ctypes as C

import numpy as np
import pytest

import lili_om_amd as L
from lili_om_amd import api
from tests import pose_graph_cases as Cs
from tests import pose_graph_marginals_model as MM
from tests import pose_graph_model as M
from tests import pose_graph_robust_cases as RC
from tests import pose_graph_robust_model as R

pytestmark = pytest.mark.gpu

ROBUST = RC.robust_cases()
BRANCH = RC.huber_branch_cases()
LM = RC.lm_cases()
EPS = np.finfo(np.float64).eps


def _ids(cs):
    return [c["name"] for c in cs]


@pytest.fixture()
def pg(gpu_ctx):
    g = L.PoseGraph(gpu_ctx)
    g.reset()
    yield g
    g.reset()
    gpu_ctx.set_option("pose_graph_max_loops", api.PG_MAX_LOOPS)


def _load(pg, c, robust_call=True):
    """robust_call False: through lili_pose_graph_add_loop (only for a case without a loss)"""
    pg.reset()
    pg.set_max_loops(max(c["max_loops"] or 0, api.PG_MAX_LOOPS))
    assert pg.append(c["poses"]) == 0
    for a, b, m, v in c["loops"]:
        if robust_call:
            pg.add_loop(a, b, m, v, loss=c["loss"], scale=c["scale"])
        else:
            assert c["loss"] == R.NONE
            pg.add_loop(a, b, m, v)
    if c["estimates"] is not None:
        pg.set_poses(c["estimates"])
    assert pg.info() == (c["poses"].shape[0], len(c["loops"]))


def _pose_tolerance(d0, X):
    floor = 64.0 * np.spacing(np.abs(X[:, 0:3]).max())
    return max(10.0 * d0[0], floor), max(10.0 * d0[1], floor)


def _cost_floor(g):
    w = max(1.0 / np.sqrt(g.prior_var.min()), 1.0 / np.sqrt(g.odom_var.min()), max([1.0 / np.sqrt(l[3].min()) for l in g.loops], default=0.0))
    return 0.5 * (g.n + len(g.loops)) * (64.0 * EPS * max(1.0, np.abs(g.X[:, 0:3]).max()) * w) ** 2


def _block_error(A, B):
    A, B = A.reshape(A.shape[0], -1), B.reshape(B.shape[0], -1)
    scale = np.abs(B).max(axis=1)
    err = np.abs(A - B).max(axis=1)
    return float(np.max(np.where(scale > 0, err / np.where(scale > 0, scale, 1.0), np.where(err > 0, np.inf, 0.0)), initial=0.0))


# ---------------------------------------------------------------- evaluate, loop_status
@pytest.mark.parametrize("c", ROBUST + BRANCH, ids=_ids(ROBUST + BRANCH))
def test_evaluate_matches_model(pg, c):
    _load(pg, c)
    g = RC.build_model(c)
    cost_m, g_m, D_m, S_m, LB_m = g.evaluate()
    cost, grad, D, S, LB = pg.evaluate()
    dc = abs(cost - cost_m) / cost_m
    dg = np.abs(grad - g_m).max() / np.abs(g_m).max()
    dD, dS, dL = _block_error(D, D_m), _block_error(S, S_m), _block_error(LB, LB_m)
    print(f"evaluate [{c['name']}]: cost {dc:.2e} gradient {dg:.2e} diagonal {dD:.2e} sub {dS:.2e} loop {dL:.2e} (of the largest entry per block)")
    assert dc <= 1e-12 and dg <= 1e-12 and dD <= 1e-12 and dS <= 1e-12 and dL <= 1e-12
    assert (D == np.swapaxes(D, 1, 2)).all()
    # the robust cost is not half the squared weighted residual: the pitfall the gate has to avoid
    plain = 0.5 * float(np.sum(g.linearize(g.X)[0] ** 2))
    assert abs(plain - cost_m) > 1e-6 * cost_m or c["name"] == "chain3_huber_below"


@pytest.mark.parametrize("c", ROBUST + BRANCH + LM[:1], ids=_ids(ROBUST + BRANCH + LM[:1]))
def test_loop_status_matches_model(pg, c):
    _load(pg, c)
    g = RC.build_model(c)
    d2_m, w_m = g.loop_status()
    X0 = pg.poses()
    d2, w = pg.loop_status()
    e2, ew = float(np.abs(d2 - d2_m).max() / d2_m.max()), float(np.abs(w - w_m).max())
    print(f"loop_status [{c['name']}]: chi2 {np.abs(d2 / d2_m - 1.0).max():.2e} relative, weight {ew:.2e} absolute; weights {np.round(w[:8], 4)}")
    assert (np.abs(d2 - d2_m) <= 1e-12 * d2_m).all() and ew <= 1e-12 and e2 <= 1e-12
    if c["loss"] == R.NONE:
        assert (w == 1.0).all()
    if c["name"] == "chain3_huber_below":
        assert w[0] == 1.0
    if c["name"] == "chain3_huber_above":
        assert 0.998 < w[0] < 1.0
    n = len(c["loops"])
    first, cnt = (n // 3, max(n // 2, 1)) if n > 1 else (0, 1)
    sd2, sw = pg.loop_status(first, cnt)
    assert sd2.tobytes() == d2[first:first + cnt].tobytes() and sw.tobytes() == w[first:first + cnt].tobytes()
    assert pg.poses().tobytes() == X0.tobytes()


# ---------------------------------------------------------------- solves
def _check_solve(c, g, X_m, s_m, d0, s, X, kind, ms):
    dp, da = M.pose_difference(X, X_m)
    tp, ta = _pose_tolerance(d0, X_m)
    print(f"{kind} [{c['name']}] N {g.n} loops {len(g.loops)}: attempts {s['iterations']} (model {s_m['iterations']}) termination {s['termination']} (model {s_m['termination']}) "
          f"cost {s['initial_cost']:.9e} -> {s['final_cost']:.9e} (model {s_m['initial_cost']:.9e} -> {s_m['final_cost']:.9e}); device - model: position {dp:.2e} m "
          f"(D0 {d0[0]:.2e}, bound {tp:.2e}), angle {da:.2e} rad (D0 {d0[1]:.2e}, bound {ta:.2e}); kernels {ms:.3f} ms")
    print("   costs device", [f"{v:.9e}" for v in s["cost"]], "model", [f"{v:.9e}" for v in s_m["cost"]])
    assert (s["n_nodes"], s["n_loops"]) == (g.n, len(g.loops))
    assert s["iterations"] == s_m["iterations"] and s["termination"] == s_m["termination"]
    floor = _cost_floor(g)
    assert len(s["cost"]) == len(s_m["cost"])
    for a, b in zip([s["initial_cost"], s["final_cost"]] + s["cost"], [s_m["initial_cost"], s_m["final_cost"]] + s_m["cost"]):
        assert abs(a - b) <= 1e-6 * b or max(a, b) <= floor, (a, b, floor)
    assert len(s["grad_inf"]) == len(s_m["grad_inf"])
    assert dp <= tp and da <= ta


@pytest.mark.parametrize("c", ROBUST + BRANCH, ids=_ids(ROBUST + BRANCH))
def test_gauss_newton_on_robust_loops_matches_model(pg, c):
    g, X_m, s_m, d0 = RC.reference(c, "gn")
    assert Cs.decisions_clear(s_m)
    _load(pg, c)
    s = pg.solve(pg.options(**c["options"]))
    _check_solve(c, g, X_m, s_m, d0, s, pg.poses(), "solve", pg.kernel_ms())


@pytest.mark.parametrize("c", ROBUST + BRANCH + LM, ids=_ids(ROBUST + BRANCH + LM))
def test_solve_lm_matches_model(pg, c):
    g, X_m, s_m, d0 = RC.reference(c, "lm")
    assert Cs.decisions_clear(s_m)
    _load(pg, c)
    before = pg.poses()
    s = pg.solve_lm(pg.options(**c["lm_options"]), pg.lm_options(**c["lm"]))
    X = pg.poses()
    print(f"   pattern {''.join('A' if a else 'r' for a in s['accepted'])} lambda {s['lambda']} -> {s['final_lambda']}")
    assert s["accepted"] == s_m["accepted"] and s["lambda"] == s_m["lambda"] and s["final_lambda"] == s_m["final_lambda"]
    assert (s["steps_accepted"], s["steps_rejected"]) == (s_m["steps_accepted"], s_m["steps_rejected"])
    _check_solve(c, g, X_m, s_m, d0, s, X, "solve_lm", pg.kernel_ms())
    if c["expect"] == R.LAMBDA_LIMIT:
        assert s["termination"] == api.PG_LAMBDA_LIMIT and X.tobytes() == before.tobytes() and s["final_cost"] == s["initial_cost"]
    if c["graph"] == "cost_increases":      # the graph plain Gauss-Newton gives up on
        _load(pg, c)
        assert pg.solve()["termination"] == api.PG_COST_INCREASED and pg.poses().tobytes() == before.tobytes()


# ---------------------------------------------------------------- the effect
@pytest.mark.parametrize("name", ["n40", "seg_edges"])
def test_a_loss_keeps_a_false_loop_from_bending_the_map(pg, name):
    plain_c, clean_c = RC.plain_case(name), RC.plain_case(name, with_false=False)
    _load(pg, clean_c)
    assert pg.solve(pg.options(**clean_c["options"]))["termination"] in M.CONVERGED
    clean = pg.poses()
    _load(pg, plain_c)
    assert pg.solve(pg.options(**plain_c["options"]))["termination"] in M.CONVERGED + (M.MAX_ITERATIONS,)
    d_plain = RC.distance(pg.poses(), clean)
    for loss in RC.LOSS_NAMES:
        c = RC.robust_case(name, loss)
        _load(pg, c)
        pg.solve(pg.options(**c["options"]))
        d = RC.distance(pg.poses(), clean)
        _, w = pg.loop_status()
        print(f"{name} {loss}: {d:.4f} m from the device's clean solve (plain {d_plain:.4f} m), false loops' weights {np.round(w[c['n_true']:], 4)}, true loops' {np.round(w[:c['n_true']], 4)}")
        assert d <= 0.2 * d_plain
        assert (w[c["n_true"]:] <= 0.05).all()
        if name == "n40" and loss == "huber":
            assert (w[:c["n_true"]] == 1.0).all()


# ---------------------------------------------------------------- marginals
def test_marginals_of_the_weighted_information(pg):
    c = RC.robust_case("n40", "cauchy")
    _load(pg, c)
    pg.solve(pg.options(**c["options"]))
    X = pg.poses()
    g = RC.build_model(c)
    nodes, pairs = MM.case_nodes(c), MM.case_pairs(c)
    cov, cross = pg.marginals(pairs=pairs)
    assert pg.poses().tobytes() == X.tobytes()
    cov_m, cross_m, d0, routes = MM.referee("robust_" + c["name"], g, X, nodes, pairs)
    dense = np.linalg.inv(g.hessian(X))
    assert MM.block_error(cov_m, np.array([dense[6 * i:6 * i + 6, 6 * i:6 * i + 6] for i in nodes])) <= MM.tolerance(d0)
    tol = MM.tolerance(d0)
    e_d, e_x = MM.block_error(cov[nodes], cov_m), MM.block_error(cross, cross_m)
    # and it is not the unweighted matrix's inverse
    plain = RC.build_model(dict(c, loss=R.NONE))
    e_plain = MM.block_error(cov[nodes], np.array([np.linalg.inv(plain.hessian(X))[6 * i:6 * i + 6, 6 * i:6 * i + 6] for i in nodes]))
    print(f"marginals [{c['name']}]: device - model diagonal {e_d:.2e} cross {e_x:.2e} of the block's largest entry (D0 {d0:.2e}, bound {tol:.2e}); against the unweighted H {e_plain:.2e}")
    assert e_d <= tol and e_x <= tol and e_plain > 1e3 * tol


# ---------------------------------------------------------------- nothing that exists moves; determinism
def test_loss_none_is_add_loop_byte_for_byte(pg):
    c = RC.plain_case("seg_edges")
    out = []
    for robust_call in (False, True):
        _load(pg, c, robust_call)
        ev = pg.evaluate()
        pg.solve(pg.options(**c["options"]))
        out.append((pg.poses().tobytes(), bytes(pg.last_summary), ev[0], b"".join(np.ascontiguousarray(a).tobytes() for a in ev[1:])))
    assert out[0] == out[1]


def test_solve_after_solve_lm_is_a_fresh_solve(gpu_ctx, pg):
    c = RC.robust_case("n40", "huber")
    lm = LM[0]
    fresh = L.Context(0)
    try:
        g2 = L.PoseGraph(fresh)
        _load(g2, c)
        g2.solve(g2.options(**c["options"]))
        want = (g2.poses().tobytes(), bytes(g2.last_summary))
        g2.reset()
    finally:
        fresh.close()
    _load(pg, lm)
    pg.solve_lm(pg.options(**lm["lm_options"]), pg.lm_options(diagonal_damping=1))
    _load(pg, c)
    ev0 = pg.evaluate()
    cov0 = pg.marginals()[0]
    pg.solve(pg.options(**c["options"]))
    assert (pg.poses().tobytes(), bytes(pg.last_summary)) == want
    # evaluate and marginals after a damped solve carry no damping either
    _load(pg, c)
    pg.solve_lm(pg.options(**c["lm_options"]))
    _load(pg, c)
    ev1 = pg.evaluate()
    assert ev0[0] == ev1[0] and all(a.tobytes() == b.tobytes() for a, b in zip(ev0[1:], ev1[1:]))
    assert pg.marginals()[0].tobytes() == cov0.tobytes()


@pytest.mark.parametrize("c", [ROBUST[7], LM[0], LM[1]], ids=_ids([ROBUST[7], LM[0], LM[1]]))
def test_two_runs_of_solve_lm_return_the_same_bytes(pg, c):
    runs = []
    for _ in range(2):
        _load(pg, c)
        pg.solve_lm(pg.options(**c["lm_options"]), pg.lm_options(**c["lm"]))
        runs.append((pg.poses().tobytes(), bytes(pg.last_summary)))
    assert runs[0] == runs[1]


# ---------------------------------------------------------------- refusals
def test_refusals_leave_everything_untouched(pg, gpu_ctx):
    lib, h, ptr = gpu_ctx.lib, gpu_ctx.h, api._ptr
    c = RC.robust_case("n40", "cauchy")
    nan, inf = float("nan"), float("inf")
    # an empty graph
    pg.reset()
    s = api.PgLmSummary()
    C.memset(C.byref(s), 0x5A, C.sizeof(s))
    assert lib.lili_pose_graph_solve_lm(h, None, None, C.byref(s)) == -3 and bytes(s) == b"\x5a" * C.sizeof(s)
    out = np.full((2, 4), 7.5)
    assert lib.lili_pose_graph_loop_status(h, None, 0, 1, ptr(out[0]), ptr(out[1])) == -1 and (out == 7.5).all()
    # ... comes behind solve_lm's own options, and those behind the options of lili_pose_graph_solve; a null summary in front of all
    bad, bad_lm = pg.options(max_iterations=0), pg.lm_options(lambda_factor=1.0)
    assert lib.lili_pose_graph_solve_lm(h, None, C.byref(bad_lm), C.byref(s)) == -1 and b"lambda_factor above 1" in lib.lili_last_error(h)
    assert lib.lili_pose_graph_solve_lm(h, C.byref(bad), C.byref(bad_lm), C.byref(s)) == -1 and b"max_iterations" in lib.lili_last_error(h)
    assert lib.lili_pose_graph_solve_lm(h, C.byref(bad), C.byref(bad_lm), None) == -1 and b"null summary" in lib.lili_last_error(h)
    assert bytes(s) == b"\x5a" * C.sizeof(s) and pg.info() == (0, 0) and pg.poses().shape == (0, 7)
    _load(pg, c)
    n, nl = pg.info()
    X0, cost0, st0 = pg.poses(), pg.evaluate()[0], pg.loop_status()

    def unchanged():
        st = pg.loop_status()
        return pg.info() == (n, nl) and pg.poses().tobytes() == X0.tobytes() and pg.evaluate()[0] == cost0 and st[0].tobytes() == st0[0].tobytes() and st[1].tobytes() == st0[1].tobytes()

    # add_loop_robust: what add_loop refuses ...
    meas, var = c["loops"][0][2].copy(), np.full(6, 0.1)
    bad_var, bad_meas, off_meas = var.copy(), meas.copy(), meas.copy()
    bad_var[2] = 0.0
    bad_meas[0] = inf
    off_meas[3:7] *= 1.0 - 1e-5
    for args in ((5, 5, ptr(meas), ptr(var)), (-1, 5, ptr(meas), ptr(var)), (5, n, ptr(meas), ptr(var)), (5, 9, None, ptr(var)), (5, 9, ptr(meas), None),
                 (5, 9, ptr(meas), ptr(bad_var)), (5, 9, ptr(bad_meas), ptr(var)), (5, 9, ptr(off_meas), ptr(var)), (5, 9, ptr(meas), ptr(np.full(6, nan)))):
        assert lib.lili_pose_graph_add_loop_robust(h, *args, api.PG_LOSS_HUBER, 1.0) == -1
        assert lib.lili_pose_graph_add_loop_robust(h, *args, api.PG_LOSS_NONE, 0.0) == -1
    # ... an unknown loss, and a scale that is not positive and finite where there is a loss
    for loss in (-1, 4, 99):
        assert lib.lili_pose_graph_add_loop_robust(h, 5, 9, ptr(meas), ptr(var), loss, 1.0) == -1
    for loss in (api.PG_LOSS_HUBER, api.PG_LOSS_CAUCHY, api.PG_LOSS_GEMAN_MCCLURE):
        for scale in (0.0, -1.0, nan, inf):
            assert lib.lili_pose_graph_add_loop_robust(h, 5, 9, ptr(meas), ptr(var), loss, scale) == -1
    assert unchanged()
    with pytest.raises(L.LiliError):
        pg.add_loop(5, 9, meas, 0.1, loss="tukey")
    # the loop cap holds for the robust call too
    for k in range(api.PG_MAX_LOOPS - nl):
        pg.add_loop(10 + (k % 8), 25 + (k % 8), meas, 0.1, loss="huber")
    assert lib.lili_pose_graph_add_loop_robust(h, 5, 9, ptr(meas), ptr(var), api.PG_LOSS_HUBER, 1.0) == -1 and pg.info() == (n, api.PG_MAX_LOOPS)
    _load(pg, c)
    assert unchanged()
    # loop_status
    out = np.full((2, 8), 7.5)
    for first, cnt in ((-1, 1), (0, 0), (0, nl + 1), (nl, 1), (nl - 1, 2), (1, -1)):
        assert lib.lili_pose_graph_loop_status(h, None, first, cnt, ptr(out[0]), ptr(out[1])) == -1
    assert lib.lili_pose_graph_loop_status(h, None, 0, 1, None, ptr(out[1])) == -1 and lib.lili_pose_graph_loop_status(h, None, 0, 1, ptr(out[0]), None) == -1
    o = pg.options(odom_var=[1, 1, 0, 1, 1, 1])
    assert lib.lili_pose_graph_loop_status(h, C.byref(o), 0, 1, ptr(out[0]), ptr(out[1])) == -1 and b"a variance is not positive" in lib.lili_last_error(h)
    assert lib.lili_pose_graph_loop_status(h, C.byref(o), nl, 1, ptr(out[0]), ptr(out[1])) == -1 and b"range outside the graph's loops" in lib.lili_last_error(h)      # the range first
    assert lib.lili_pose_graph_loop_status(h, C.byref(o), nl, 1, None, ptr(out[1])) == -1 and b"null argument" in lib.lili_last_error(h)
    assert (out == 7.5).all() and unchanged()
    # solve_lm: the options of lili_pose_graph_solve, then its own
    C.memset(C.byref(s), 0x5A, C.sizeof(s))
    for kw in (dict(max_iterations=0), dict(max_iterations=1001), dict(function_tolerance=-1.0), dict(gradient_tolerance=nan), dict(parameter_tolerance=inf),
               dict(prior_var=[1, 1, 1, 0, 1, 1]), dict(odom_var=[1, 1, nan, 1, 1, 1])):
        o = pg.options(**kw)
        assert lib.lili_pose_graph_solve_lm(h, C.byref(o), None, C.byref(s)) == -1
    for kw in (dict(initial_lambda=0.0), dict(initial_lambda=-1.0), dict(initial_lambda=nan), dict(initial_lambda=inf), dict(lambda_factor=1.0), dict(lambda_factor=0.5),
               dict(lambda_factor=nan), dict(lambda_factor=inf), dict(lambda_lower=0.0), dict(lambda_lower=nan), dict(lambda_upper=1e-11), dict(lambda_upper=inf),
               dict(lambda_upper=nan), dict(lambda_lower=2.0, lambda_upper=1.0), dict(diagonal_damping=2), dict(diagonal_damping=-1)):
        o = pg.lm_options(**kw)
        assert lib.lili_pose_graph_solve_lm(h, None, C.byref(o), C.byref(s)) == -1, kw
    assert lib.lili_pose_graph_solve_lm(h, None, None, None) == -1
    assert bytes(s) == b"\x5a" * C.sizeof(s) and unchanged()
    # and the context still works: lambda_upper == lambda_lower is allowed
    d = api.PgLmOptions()
    lib.lili_pg_lm_default_options(C.byref(d))
    assert (d.initial_lambda, d.lambda_factor, d.lambda_lower, d.lambda_upper, d.diagonal_damping) == (1e-5, 10.0, 1e-10, 1e8, 0)
    assert pg.solve_lm(pg.options(**c["lm_options"]))["termination"] in M.CONVERGED
    assert pg.kernel_ms() > 0.0
