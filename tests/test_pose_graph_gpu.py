"""Global pose graph on the device (lili_pose_graph*, lili_om_amd.PoseGraph) against the referee (tests/pose_graph_model.py) on the graphs of
tests/pose_graph_cases.py:
  evaluate     cost and gradient to 1e-12 of the largest entry, every diagonal, sub-diagonal and loop block to 1e-12 of the largest entry OF THAT BLOCK (the weights span
               eight decades), the diagonal blocks symmetric; with the reference's variances and with unit variances;
  solve        the number of iterations, the termination code and the sequence of costs; final poses within max(10 D0(case), 64 ulp of the largest coordinate), D0 = the
               spread between the model's own two linear solvers (position by difference, rotation by angle) — the measured differences are printed;
  full size    N = LILI_PG_MAX_NODES with 4 loops, judged by the model's vectorised evaluate;
  determinism, incremental use, set / get, refusals, and one loop closure end to end through LoopClosure, the graph, correct_poses and the archive.
The model's solves are computed once per case (pose_graph_cases.reference) and shared.

The costs are compared to 1e-6 relative — the size of the function tolerance that decides on them — above a floor below which a cost is rounding: a residual carries
about 64 ulp of the largest coordinate times its weight, so F factors leave 0.5 F (64 eps |p| w)^2."""
import ctypes as C

import numpy as np
import pytest

import lili_om_amd as L
from lili_om_amd import api
from tests import pose_graph_cases as Cs
from tests import pose_graph_model as M

pytestmark = pytest.mark.gpu

SOLVES = Cs.solve_cases()
IDS = [c["name"] for c in SOLVES]
EPS = np.finfo(np.float64).eps


@pytest.fixture()
def pg(gpu_ctx):
    g = L.PoseGraph(gpu_ctx)
    g.reset()
    yield g
    g.reset()


def _load(pg, c):
    pg.reset()
    assert pg.append(c["poses"]) == 0
    for a, b, m, v in c["loops"]:
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


# ---------------------------------------------------------------- evaluate
def _block_error(A, B):
    """largest |A - B| per block relative to that block's largest entry; blocks that are exactly zero on both sides count as equal"""
    A, B = A.reshape(A.shape[0], -1), B.reshape(B.shape[0], -1)
    scale = np.abs(B).max(axis=1)
    err = np.abs(A - B).max(axis=1)
    return float(np.max(np.where(scale > 0, err / np.where(scale > 0, scale, 1.0), np.where(err > 0, np.inf, 0.0)), initial=0.0))


@pytest.mark.parametrize("unit", [False, True], ids=["reference_variances", "unit_variances"])
@pytest.mark.parametrize("c", SOLVES, ids=IDS)
def test_evaluate_matches_model(pg, c, unit):
    _load(pg, c)
    pv, ov = (np.ones(6), np.ones(6)) if unit else (M.PRIOR_VAR, M.ODOM_VAR)
    g = Cs.build_model(c, pv, ov)
    cost_m, g_m, D_m, S_m, LB_m = g.evaluate()
    cost, grad, D, S, LB = pg.evaluate(pg.options(prior_var=pv, odom_var=ov))
    dc = abs(cost - cost_m) / cost_m if cost_m > 0 else abs(cost)
    dg = np.abs(grad - g_m).max() / np.abs(g_m).max() if np.abs(g_m).max() > 0 else np.abs(grad).max()
    dD, dS, dL = _block_error(D, D_m), _block_error(S, S_m) if g.n > 1 else 0.0, _block_error(LB, LB_m) if len(g.loops) else 0.0
    print(f"evaluate [{c['name']} {'unit' if unit else 'reference'} variances]: cost {dc:.2e} gradient {dg:.2e} diagonal {dD:.2e} sub {dS:.2e} loop {dL:.2e} (of the largest entry per block)")
    assert dc <= 1e-12 and dg <= 1e-12 and dD <= 1e-12 and dS <= 1e-12 and dL <= 1e-12
    assert (D == np.swapaxes(D, 1, 2)).all()


# ---------------------------------------------------------------- solve
@pytest.mark.parametrize("c", SOLVES, ids=IDS)
def test_solve_matches_model(pg, c):
    g, X_m, s_m, d0 = Cs.reference(c)
    assert Cs.decisions_clear(s_m)
    _load(pg, c)
    before = pg.poses()
    s = pg.solve(pg.options(**c["options"]))
    X = pg.poses()
    dp, da = M.pose_difference(X, X_m)
    tp, ta = _pose_tolerance(d0, X_m)
    print(f"solve [{c['name']}] N {g.n} loops {len(g.loops)}: iterations {s['iterations']} (model {s_m['iterations']}) termination {s['termination']} (model {s_m['termination']}) "
          f"cost {s['initial_cost']:.9e} -> {s['final_cost']:.9e} (model {s_m['initial_cost']:.9e} -> {s_m['final_cost']:.9e}); device - model: position {dp:.2e} m "
          f"(D0 {d0[0]:.2e}, bound {tp:.2e}), angle {da:.2e} rad (D0 {d0[1]:.2e}, bound {ta:.2e}); kernels {pg.kernel_ms():.3f} ms")
    print("   costs device", [f"{v:.9e}" for v in s["cost"]], "model", [f"{v:.9e}" for v in s_m["cost"]])
    assert (s["n_nodes"], s["n_loops"]) == (g.n, len(g.loops))
    assert s["iterations"] == s_m["iterations"] and s["termination"] == s_m["termination"]
    floor = _cost_floor(g)
    for a, b in zip([s["initial_cost"], s["final_cost"]] + s["cost"], [s_m["initial_cost"], s_m["final_cost"]] + s_m["cost"]):
        assert abs(a - b) <= 1e-6 * b or max(a, b) <= floor, (a, b, floor)
    assert len(s["grad_inf"]) == len(s_m["grad_inf"])      # one per linearisation
    if c["expect"] == M.COST_INCREASED:
        assert X.tobytes() == before.tobytes()
    assert dp <= tp and da <= ta


def test_full_size(pg):
    c = Cs.full_size()
    g = Cs.build_model(c)
    _load(pg, c)
    s = pg.solve(pg.options(**c["options"]))
    X = pg.poses()
    c0, g0 = g.evaluate()[0:2]
    c1, g1 = g.evaluate(X)[0:2]
    r = np.abs(g1).max() / np.abs(g0).max()
    print(f"full size N {g.n} loops {len(g.loops)}: iterations {s['iterations']} termination {s['termination']} cost {s['initial_cost']:.9e} -> {s['final_cost']:.9e} "
          f"(model's evaluate: {c0:.9e} -> {c1:.9e}), model's |g|inf {np.abs(g0).max():.2e} -> {np.abs(g1).max():.2e} ({r:.1e}); kernels {pg.kernel_ms():.2f} ms")
    print("   costs", [f"{v:.9e}" for v in s["cost"]], "steps", [f"{v:.1e}" for v in s["step_inf"]])
    costs = [s["initial_cost"]] + s["cost"]
    assert all(b <= a for a, b in zip(costs, costs[1:])) and c1 <= c0
    assert s["termination"] in M.CONVERGED
    assert r <= 1e-6


def test_two_solves_from_reset_return_the_same_bytes(pg):
    out = []
    for c in (next(c for c in SOLVES if c["name"] == "crossing_and_nested"), next(c for c in SOLVES if c["name"] == "chain_1025")):
        runs = []
        for _ in range(2):
            _load(pg, c)
            pg.solve(pg.options(**c["options"]))
            runs.append((pg.poses().tobytes(), bytes(pg.last_summary)))
        assert runs[0] == runs[1], c["name"]
        out.append(runs[0])
    assert out[0] != out[1]


def test_incremental_use_matches_model(pg):
    """append in pieces -> solve -> append more -> add a loop -> solve: the chain measurements stay frozen while the estimates move"""
    script = Cs.incremental_script()
    g, ref = Cs.run_script_on_model(script)
    _, ref2 = Cs.run_script_on_model(script, solver="dense")
    pg.reset()
    k, firsts = 0, []
    for step in script:
        if step[0] == "append":
            firsts.append(pg.append(step[2], prev=step[1]))
        elif step[0] == "loop":
            pg.add_loop(step[1], step[2], step[3], step[4])
        else:
            X_m, s_m = ref[k]
            assert Cs.decisions_clear(s_m)
            d0 = M.pose_difference(X_m, ref2[k][0])
            s = pg.solve(pg.options(**step[1]))
            X = pg.poses()
            dp, da = M.pose_difference(X, X_m)
            tp, ta = _pose_tolerance(d0, X_m)
            print(f"incremental solve {k}: N {X.shape[0]} iterations {s['iterations']} (model {s_m['iterations']}) termination {s['termination']} (model {s_m['termination']}) "
                  f"cost {s['final_cost']:.9e} (model {s_m['final_cost']:.9e}); device - model: position {dp:.2e} (D0 {d0[0]:.2e}, bound {tp:.2e}) angle {da:.2e} (D0 {d0[1]:.2e}, bound {ta:.2e})")
            assert s["iterations"] == s_m["iterations"] and s["termination"] == s_m["termination"]
            assert abs(s["final_cost"] - s_m["final_cost"]) <= 1e-6 * s_m["final_cost"] and abs(s["initial_cost"] - s_m["initial_cost"]) <= 1e-6 * s_m["initial_cost"]
            assert dp <= tp and da <= ta
            k += 1
    assert firsts == [0, 100, 180] and k == 2 and pg.info() == (300, 2)


def test_set_get_round_trip(pg):
    c = next(c for c in SOLVES if c["name"] == "adjacent_endpoints")
    _load(pg, c)
    X0 = pg.poses()
    assert np.abs(X0 - c["poses"]).max() <= 4 * EPS * np.abs(c["poses"]).max()
    new = Cs.perturbed(c["poses"][50:60], 9)
    pg.set_poses(new, first=50)
    X1 = pg.poses()
    assert X1[:50].tobytes() == X0[:50].tobytes() and X1[60:].tobytes() == X0[60:].tobytes()
    assert X1[50:60, 0:3].tobytes() == new[:, 0:3].tobytes() and np.abs(X1[50:60, 3:7] - new[:, 3:7]).max() <= 4 * EPS
    assert pg.poses(55, 3).tobytes() == X1[55:58].tobytes()
    # quaternions are normalised on entry
    scaled = new.copy()
    scaled[:, 3:7] *= 1.0 + 5e-7
    pg.set_poses(scaled, first=50)
    assert np.abs(np.linalg.norm(pg.poses(50, 10)[:, 3:7], axis=1) - 1.0).max() <= 4 * EPS
    # the measurements stayed: the cost is the model's for the moved estimates
    g = Cs.build_model(c)
    g.X = pg.poses()
    assert abs(pg.evaluate()[0] - g.cost(g.X)) <= 1e-12 * g.cost(g.X)


def test_refusals_leave_everything_untouched(pg, gpu_ctx):
    lib, h, ptr = gpu_ctx.lib, gpu_ctx.h, api._ptr
    c = next(c for c in SOLVES if c["name"] == "adjacent_endpoints")
    one = np.ascontiguousarray(c["poses"][0:1])
    nan, off = one.copy(), one.copy()
    nan[0, 1] = np.nan
    off[0, 3:7] *= 1.0 + 1e-5
    # an empty graph
    pg.reset()
    first = C.c_int(-7)
    assert lib.lili_pose_graph_append(h, ptr(one), ptr(one), 1, C.byref(first)) == -1          # prev on an empty graph
    assert lib.lili_pose_graph_append(h, None, None, 1, C.byref(first)) == -1
    assert lib.lili_pose_graph_append(h, None, ptr(one), 0, C.byref(first)) == -1
    assert lib.lili_pose_graph_append(h, None, ptr(nan), 1, C.byref(first)) == -1
    assert lib.lili_pose_graph_append(h, None, ptr(off), 1, C.byref(first)) == -1
    assert first.value == -7 and pg.info() == (0, 0)
    s = api.PgSummary()
    C.memset(C.byref(s), 0x5A, C.sizeof(s))
    assert lib.lili_pose_graph_solve(h, None, C.byref(s)) == -3 and bytes(s) == b"\x5a" * C.sizeof(s)
    # ... refuses evaluate too; a null argument and the options are judged in front of it
    cost, g1, bad = C.c_double(7.5), np.full((1, 36), 7.5), pg.options(max_iterations=0)
    assert lib.lili_pose_graph_evaluate(h, None, C.byref(cost), ptr(g1), ptr(g1), None, None) == -3 and b"pose_graph_evaluate: the graph is empty" in lib.lili_last_error(h)
    assert lib.lili_pose_graph_evaluate(h, C.byref(bad), C.byref(cost), ptr(g1), ptr(g1), None, None) == -1 and b"max_iterations" in lib.lili_last_error(h)
    assert lib.lili_pose_graph_evaluate(h, C.byref(bad), None, ptr(g1), ptr(g1), None, None) == -1 and b"null argument" in lib.lili_last_error(h)
    assert lib.lili_pose_graph_solve(h, C.byref(bad), C.byref(s)) == -1 and b"max_iterations" in lib.lili_last_error(h)
    assert lib.lili_pose_graph_solve(h, C.byref(bad), None) == -1 and b"null summary" in lib.lili_last_error(h)
    assert cost.value == 7.5 and (g1 == 7.5).all() and bytes(s) == b"\x5a" * C.sizeof(s) and pg.info() == (0, 0) and pg.poses().shape == (0, 7)
    _load(pg, c)
    n, nl = pg.info()
    X0, cost0 = pg.poses(), pg.evaluate()[0]
    meas, var = c["loops"][0][2].copy(), np.full(6, 0.1)

    def unchanged():
        return pg.info() == (n, nl) and pg.poses().tobytes() == X0.tobytes() and pg.evaluate()[0] == cost0

    # append
    assert lib.lili_pose_graph_append(h, None, ptr(one), 1, C.byref(first)) == -1               # no prev on a non-empty graph
    assert lib.lili_pose_graph_append(h, ptr(nan), ptr(one), 1, C.byref(first)) == -1
    assert lib.lili_pose_graph_append(h, ptr(off), ptr(one), 1, C.byref(first)) == -1
    big = np.repeat(one, api.PG_MAX_NODES - n + 1, 0)
    assert lib.lili_pose_graph_append(h, ptr(one), ptr(big), big.shape[0], C.byref(first)) == -1      # a full graph
    assert first.value == -7 and unchanged()
    # add_loop
    bad_var, bad_meas, off_meas = var.copy(), meas.copy(), meas.copy()
    bad_var[2] = 0.0
    bad_meas[0] = np.inf
    off_meas[3:7] *= 1.0 - 1e-5
    for args in ((5, 5, ptr(meas), ptr(var)), (-1, 5, ptr(meas), ptr(var)), (5, n, ptr(meas), ptr(var)), (5, 9, None, ptr(var)), (5, 9, ptr(meas), None),
                 (5, 9, ptr(meas), ptr(bad_var)), (5, 9, ptr(bad_meas), ptr(var)), (5, 9, ptr(off_meas), ptr(var)), (5, 9, ptr(meas), ptr(np.full(6, np.nan)))):
        assert lib.lili_pose_graph_add_loop(h, *args) == -1
    assert unchanged()
    # get / set / info
    out = np.full((4, 7), 7.5)
    for first_id, cnt in ((-1, 2), (n - 1, 2), (0, 0), (n, 1)):
        assert lib.lili_pose_graph_get(h, first_id, cnt, ptr(out)) == -1
        assert lib.lili_pose_graph_set(h, first_id, cnt, ptr(one)) == -1
    assert lib.lili_pose_graph_get(h, 0, 1, None) == -1 and lib.lili_pose_graph_set(h, 0, 1, None) == -1
    assert lib.lili_pose_graph_set(h, 3, 1, ptr(nan)) == -1 and lib.lili_pose_graph_set(h, 3, 1, ptr(off)) == -1
    a, b = C.c_int(-7), C.c_int(-7)
    assert lib.lili_pose_graph_info(h, None, C.byref(b)) == -1 and lib.lili_pose_graph_info(h, C.byref(a), None) == -1 and (a.value, b.value) == (-7, -7)
    assert (out == 7.5).all() and unchanged()
    # options, as lili_s2m_solve_lm refuses them, and the variances
    C.memset(C.byref(s), 0x5A, C.sizeof(s))
    for kw in (dict(max_iterations=0), dict(max_iterations=1001), dict(function_tolerance=-1.0), dict(gradient_tolerance=float("nan")), dict(parameter_tolerance=float("inf")),
               dict(prior_var=[1, 1, 1, 0, 1, 1]), dict(odom_var=[1, 1, -1, 1, 1, 1]), dict(odom_var=[1, 1, float("nan"), 1, 1, 1])):
        o = pg.options(**kw)
        assert lib.lili_pose_graph_solve(h, C.byref(o), C.byref(s)) == -1
        cost, g, D, S, LB = C.c_double(7.5), np.full((n, 6), 7.5), np.full((n, 36), 7.5), np.full((n - 1, 36), 7.5), np.full((nl, 36), 7.5)
        assert lib.lili_pose_graph_evaluate(h, C.byref(o), C.byref(cost), ptr(g), ptr(D), ptr(S), ptr(LB)) == -1
        assert cost.value == 7.5 and (g == 7.5).all() and (D == 7.5).all() and (S == 7.5).all() and (LB == 7.5).all()
    assert lib.lili_pose_graph_solve(h, None, None) == -1
    cost, g, D, S, LB = C.c_double(7.5), np.full((n, 6), 7.5), np.full((n, 36), 7.5), np.full((n - 1, 36), 7.5), np.full((nl, 36), 7.5)
    for null in range(5):
        args = [C.byref(cost), ptr(g), ptr(D), ptr(S), ptr(LB)]
        args[null] = None
        assert lib.lili_pose_graph_evaluate(h, None, *args) == -1
    assert cost.value == 7.5 and (g == 7.5).all() and (D == 7.5).all() and (S == 7.5).all() and (LB == 7.5).all()
    assert bytes(s) == b"\x5a" * C.sizeof(s) and unchanged()
    ms = C.c_float(7.5)
    assert lib.lili_pose_graph_kernel_ms(h, None) == -1
    # the loop cap
    for k in range(api.PG_MAX_LOOPS - nl):
        pg.add_loop(10 + k, 100 + k, meas, 0.1)
    assert lib.lili_pose_graph_add_loop(h, 5, 9, ptr(meas), ptr(var)) == -1 and pg.info() == (n, api.PG_MAX_LOOPS)
    # and the context still works
    _load(pg, c)
    assert pg.solve(pg.options(**c["options"]))["termination"] in M.CONVERGED


# ---------------------------------------------------------------- end to end
def test_loop_closure_end_to_end():
    """a revisit with drift: LoopClosure.perform on a tiny archive -> add_loop_from_icp -> solve -> correct_poses -> KeyframeArchive.set_poses.  One node per keyframe."""
    from lili_om_amd import synth
    from tests.test_loop_icp_gpu import _keyframe, _path, _quat
    q_bl = np.array([0.999, 0.01, -0.02, 0.03]) / np.linalg.norm([0.999, 0.01, -0.02, 0.03])
    t_bl = np.array([0.1, -0.05, 0.2])
    world = synth.OutdoorScene().sample_surfaces(45.0, 45.0, 0.5, np.random.default_rng(11)).astype(np.float32)
    ts, Rs = _path(12)
    kfs = [_keyframe(world, ts[k], Rs[k], radius=12.0, seed=k) for k in range(12)]
    qs, edge, surf = [_quat(R) for R in Rs], [k[0] for k in kfs], [k[1] for k in kfs]
    # three more keyframes at the places of keyframes 0 .. 2, their odometry poses drifted by 0.25 m and 0.02 rad
    drift_q = np.array([np.cos(0.01), 0.0, 0.0, np.sin(0.01)])
    ts2 = [M.qrot(drift_q, np.asarray(t)) + np.array([0.2, -0.15, 0.0]) for t in ts[:3]]
    qs2 = [M.qnormalize(M.qmul(drift_q, np.asarray(q))) for q in qs[:3]]
    ts, qs, edge, surf = list(ts) + ts2, list(qs) + qs2, edge + edge[:3], surf + surf[:3]
    times = np.array([2.0 * k for k in range(12)] + [200.0, 202.0, 204.0])
    width = 3
    ctx = L.Context(0)
    try:
        arch = L.KeyframeArchive(ctx, q_bl=q_bl, t_bl=t_bl)
        for k in range(15):
            arch.push(edge[k], surf[k], None, times[k], ts[k], qs[k])
        loop = L.LoopClosure(ctx, archive=arch, variant="livox", lc_map_width=3, q_bl=q_bl, t_bl=t_bl, lc_icp_thres=5.0, slide_window_width=width)
        found = loop.perform(None, None, np.asarray(ts[12], np.float32), 206.0)
        assert found is not None and found[:2] == (12, 0)
        latest, his = found[:2]
        a_ts, a_qs, _ = arch.poses()
        kf_poses = np.hstack([a_ts, a_qs])
        graph = L.PoseGraph(ctx)
        graph.reset()
        graph.append(kf_poses)
        ids = np.arange(15, dtype=np.int32)
        m = graph.add_loop_from_icp(ids[latest], ids[his], loop.last["transform"], kf_poses[latest], kf_poses[his], loop.last["fitness"])
        s = graph.solve(max_iterations=2)
        sol = graph.poses()

        def residual(P):
            return float(np.linalg.norm(M.factor_error(P[latest], P[his], m)[0]))

        r0, r1 = residual(kf_poses), residual(sol)
        print(f"end to end: fitness {loop.last['fitness']:.4f} iterations {s['iterations']} termination {s['termination']} cost {s['initial_cost']:.6e} -> {s['final_cost']:.6e} "
              f"loop residual {r0:.4f} -> {r1:.4f}")
        assert s["iterations"] >= 1 and s["final_cost"] < s["initial_cost"] and r1 < r0
        abs_poses = np.vstack([kf_poses[0:1], kf_poses])[:, [3, 4, 5, 6, 0, 1, 2]]
        out = L.correct_poses(sol, ids, width, abs_poses, kf_poses)
        arch.set_poses(0, out["keyframe_poses"][:, 0:3], out["keyframe_poses"][:, 3:7])
        n_ts, n_qs, _ = arch.poses()
        fixed = 15 - width + 1      # keyframes 0 .. 12 sit on their solved nodes, the window's tail is re-chained behind them
        assert np.hstack([n_ts, n_qs])[:fixed].tobytes() == sol[:fixed].tobytes()
        tail_old = M.between(kf_poses[13], kf_poses[14])
        tail_new = M.between(np.hstack([n_ts, n_qs])[13], np.hstack([n_ts, n_qs])[14])
        assert np.abs(tail_old - tail_new).max() <= 1e-9
    finally:
        ctx.close()
