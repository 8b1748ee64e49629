"""Per-frame trajectory on the device (lili_local_graph*, lili_om_amd.LocalGraph) against the referee (tests/local_graph_model.py) on the
cases of tests/local_graph_cases.py:
  walk      propagated poses, end state and measurements bit for bit;
  evaluate  cost, gradient and J^T J to 1e-12 of the largest entry, J^T J symmetric and exactly zero outside the block tridiagonal;
  solve     the whole decision sequence (iterations, accept / reject, dogleg case, reuse flag, termination), the radius per candidate, final cost and poses;
  one call  lili_local_graph byte-identical to propagate followed by solve;
  refusals  every LILI_E_ARG condition leaves sentinel-filled outputs untouched and the context usable;
  n = 0 and n = LILI_LOCAL_MAX_FRAMES.
The model's results are computed once per case and shared."""
import ctypes as C

import numpy as np
import pytest

import lili_om_amd as L
from lili_om_amd import api
from tests import local_graph_cases as Cs
from tests import local_graph_model as M

pytestmark = pytest.mark.gpu

SOLVES = Cs.solve_cases()
WALKS = Cs.walk_cases()
_ref = {}


def _model_solve(c):
    if ("solve", c["name"]) not in _ref:
        ch = M.Chain(c["left"], c["right"], c["meas"])
        _ref[("solve", c["name"])] = (ch,) + M.dogleg(ch, c["x0"], **c["options"])
    return _ref[("solve", c["name"])]


def _model_walk(c):
    if ("walk", c["name"]) not in _ref:
        _ref[("walk", c["name"])] = M.walk(**Cs.walk_kwargs(c))
    return _ref[("walk", c["name"])]


def _angle(qa, qb):
    qa, qb = qa / np.linalg.norm(qa), qb / np.linalg.norm(qb)
    return 2.0 * np.arccos(min(1.0, abs(float(qa @ qb))))


@pytest.fixture(scope="module")
def lg(gpu_ctx):
    return L.LocalGraph(gpu_ctx)


# ---------------------------------------------------------------- walk
@pytest.mark.parametrize("c", WALKS, ids=[c["name"] for c in WALKS])
def test_walk_bit_for_bit(lg, c):
    poses_m, (P, R, V), meas_m = _model_walk(c)
    poses, (Pd, Rd, Vd), meas = lg.propagate(**Cs.walk_kwargs(c))
    for name, a, b in (("poses", poses, poses_m), ("P", Pd, P), ("R", Rd, R), ("V", Vd, V), ("measurements", meas, meas_m)):
        d = np.abs(a - b).max() if a.size else 0.0
        print(f"walk [{c['name']}] {name}: max |device - model| = {d:.3e}")
    assert poses.tobytes() == poses_m.tobytes()
    assert Pd.tobytes() == P.tobytes() and Rd.tobytes() == R.tobytes() and Vd.tobytes() == V.tobytes()
    assert meas.tobytes() == meas_m.tobytes()


# ---------------------------------------------------------------- evaluate
def _check_evaluate(lg, c, x, what):
    ch = M.Chain(c["left"], c["right"], c["meas"])
    cost_m, r, J = ch.evaluate(x)
    g_m, H_m = J.T @ r, J.T @ J
    cost, g, H = lg.evaluate(c["left"], c["right"], c["meas"], x)
    dc, dg, dh = abs(cost - cost_m) / cost_m, np.abs(g - g_m).max() / np.abs(g_m).max(), np.abs(H - H_m).max() / np.abs(H_m).max()
    print(f"evaluate [{c['name']} {what}]: cost {dc:.2e} gradient {dg:.2e} JtJ {dh:.2e} (relative to the largest entry)")
    assert dc <= 1e-12 and dg <= 1e-12 and dh <= 1e-12
    assert np.abs(H - H.T).max() <= 1e-13 * np.abs(H).max()
    bi = np.arange(6 * c["n"]) // 6
    assert (H[np.abs(bi[:, None] - bi[None, :]) > 1] == 0.0).all()


@pytest.mark.parametrize("c", [c for c in SOLVES if c["n"] and c["name"] != "e"], ids=[c["name"] for c in SOLVES if c["n"] and c["name"] != "e"])
def test_evaluate_matches_model(lg, c):
    _check_evaluate(lg, c, c["x0"], "initial state")
    for k, x in enumerate(Cs.hard_states(c)):
        _check_evaluate(lg, c, x, f"hard state {k}")


def test_evaluate_at_the_truth_of_exact_measurements(lg):
    """family e: cost and gradient are rounding noise there, so only J^T J is compared relatively; the gradient is below the gradient tolerance on both sides"""
    c = next(s for s in SOLVES if s["name"] == "e")
    ch = M.Chain(c["left"], c["right"], c["meas"])
    _, r, J = ch.evaluate(c["x0"])
    cost, g, H = lg.evaluate(c["left"], c["right"], c["meas"], c["x0"])
    assert np.abs(H - J.T @ J).max() <= 1e-12 * np.abs(J.T @ J).max()
    assert cost <= 1e-25 and np.abs(g).max() <= 1e-10 and np.abs(J.T @ r).max() <= 1e-10


# ---------------------------------------------------------------- solve
def _compare_solve(c, x, info, what):
    ch, x_m, info_m, log_m = _model_solve(c)
    log = info["log"]
    print(f"solve [{c['name']} {what}]: model {info_m}  device iterations {info['iterations']} successful {info['successful_steps']} {info['termination']} cost {info['final_cost']:.12g} mu {info['final_mu']:g}")
    assert info["termination"] == info_m["termination"]
    assert info["iterations"] == info_m["iterations"] and info["successful_steps"] == info_m["successful_steps"]
    assert len(log) == len(log_m)
    assert [e["accepted"] for e in log] == [e["accepted"] for e in log_m]
    assert [e["case"] for e in log] == [e["case"] for e in log_m]
    assert [e["reused"] for e in log] == [e["reused"] for e in log_m]
    assert [e["it"] for e in log] == [e["it"] for e in log_m]
    # the radius: the same double while only the initial value and halvings have entered it, 1e-12 relative once 3 |step| has (an accepted step with rho > 0.75)
    exact = True
    for a, b in zip(log, log_m):
        if exact:
            assert a["radius"] == b["radius"], (a, b)
        else:
            assert abs(a["radius"] - b["radius"]) <= 1e-12 * b["radius"], (a, b)
        if b["accepted"] and b["rho"] > 0.75 and 3.0 * b["dogleg_norm"] > b["radius"]:
            exact = False
    assert abs(info["final_radius"] - info_m["radius"]) <= 1e-12 * info_m["radius"]
    assert info["final_mu"] == info_m["mu"]
    if info_m["cost"] > 1e-25:
        d_cost = abs(info["final_cost"] - info_m["cost"]) / info_m["cost"]
        d0 = abs(info["initial_cost"] - info_m["initial_cost"]) / info_m["initial_cost"]
    else:
        d_cost, d0 = abs(info["final_cost"] - info_m["cost"]), abs(info["initial_cost"] - info_m["initial_cost"])
    dt = max([np.linalg.norm(x[k, 0:3] - x_m[k, 0:3]) for k in range(c["n"])] + [0.0])
    da = max([_angle(x[k, 3:7], x_m[k, 3:7]) for k in range(c["n"])] + [0.0])
    print(f"solve [{c['name']} {what}]: d_cost {d_cost:.3e} d_initial_cost {d0:.3e} d_t {dt:.3e} m d_angle {da:.3e} rad")
    assert d_cost <= 1e-6 and d0 <= 1e-12
    assert dt < 1e-4 and da < 1e-4


@pytest.mark.parametrize("c", SOLVES, ids=[c["name"] for c in SOLVES])
def test_solve_matches_model(lg, c):
    opt = lg.options(**c["options"]) if c["options"] else None
    x, info = lg.solve(c["left"], c["right"], c["meas"], c["x0"], opt)
    _compare_solve(c, x, info, "solve")
    s = lg.last_summary
    assert list(s.dogleg_case[s.lm.n_logged:]) == [0] * (api.LM_MAX_LOG - s.lm.n_logged) and s.lm.n_surf == 0 and s.lm.n_edge == 0


def test_n0_and_cap(lg):
    c0 = next(s for s in SOLVES if s["name"] == "f")
    x, info = lg.solve(c0["left"], c0["right"], c0["meas"], np.zeros((0, 7)))
    cost_m = M.Chain(c0["left"], c0["right"], c0["meas"]).evaluate(np.zeros((0, 7)), want_jac=False)[0]
    assert x.shape == (0, 7) and info["iterations"] == 0 and info["successful_steps"] == 0 and not info["log"] and info["termination"] == "gradient_tolerance"
    assert abs(info["initial_cost"] - cost_m) <= 1e-12 * cost_m and info["final_cost"] == info["initial_cost"]
    cost, g, H = lg.evaluate(c0["left"], c0["right"], c0["meas"], np.zeros((0, 7)))
    assert abs(cost - cost_m) <= 1e-12 * cost_m and g.size == 0 and H.size == 0
    w0 = next(w for w in WALKS if w["n"] == 0)
    poses, meas, info = lg.run(c0["right"], **Cs.walk_kwargs(w0))
    assert poses.shape == (0, 7) and meas.shape == (1, 7) and meas.tobytes() == _model_walk(w0)[2].tobytes() and info["iterations"] == 0
    cg = next(s for s in SOLVES if s["name"] == "g")
    assert cg["n"] == api.LOCAL_MAX_FRAMES
    one_more = np.zeros((api.LOCAL_MAX_FRAMES + 1, 7)); one_more[:, 3] = 1.0
    with pytest.raises(L.LiliError):
        lg.solve(cg["left"], cg["right"], np.vstack([cg["meas"], cg["meas"][:1]]), one_more)


# ---------------------------------------------------------------- one call
@pytest.mark.parametrize("name", ["200hz_n2", "200hz_n16", "f32_positions", "rates_3rad_s", "2khz_n3", "200hz_n0"])
def test_one_call_equals_propagate_then_solve(lg, name):
    c = next(w for w in WALKS if w["name"] == name)
    kw = Cs.walk_kwargs(c)
    poses0, (P, R, V), meas0 = lg.propagate(**kw)
    # the right keyframe's solved pose: the propagated end state, moved a little — what a window solve does to it
    right = np.concatenate([P + np.array([0.03, -0.02, 0.01]), M.mat_to_quat(R.tolist())])
    right[3:7] /= np.linalg.norm(right[3:7])
    x2, info2 = lg.solve(c["left"], right, meas0, poses0)
    s2 = bytes(lg.last_summary)
    x1, meas1, info1 = lg.run(right, **kw)
    s1 = bytes(lg.last_summary)
    print(f"one call [{name}]: {info1['iterations']} iterations, {info1['termination']}, cost {info1['initial_cost']:.6g} -> {info1['final_cost']:.6g}")
    assert x1.tobytes() == x2.tobytes() and meas1.tobytes() == meas0.tobytes() and s1 == s2
    if c["n"]:
        # and the result is the model's on the same problem (decisions are not asserted: these problems were not chosen for stable ones)
        ch = M.Chain(c["left"], right, meas0)
        x_m, info_m, _ = M.dogleg(ch, poses0)
        assert info1["final_cost"] <= info1["initial_cost"]
        if info_m["termination"] == info1["termination"] and info_m["iterations"] == info1["iterations"]:
            assert abs(info1["final_cost"] - info_m["cost"]) <= 1e-6 * info_m["cost"]


def test_kernel_time_option(lg, gpu_ctx):
    """option "local_graph_time": two events around the launch, read by lili_local_graph_kernel_ms (tools/local_graph_time.py); the results do not depend on it"""
    c = SOLVES[0]
    x0, _ = lg.solve(c["left"], c["right"], c["meas"], c["x0"])
    gpu_ctx.set_option("local_graph_time", 1)
    try:
        x1, _ = lg.solve(c["left"], c["right"], c["meas"], c["x0"])
        ms = lg.kernel_ms()
    finally:
        gpu_ctx.set_option("local_graph_time", 0)
    assert x1.tobytes() == x0.tobytes() and 0.0 < ms < 100.0


# ---------------------------------------------------------------- refusals
SENTINEL = -7.25


def _walk_struct(lg, c, **change):
    kw = Cs.walk_kwargs(c)
    kw.update(change)
    return lg._walk(**kw)


def test_refusals_leave_outputs_untouched(lg, gpu_ctx):
    lib, h = lg.lib, gpu_ctx.h
    c = WALKS[0]
    n = c["n"]
    a = SOLVES[0]
    right = a["right"]
    anchors = np.concatenate([a["left"], a["right"]])
    nan7 = np.full(7, np.nan)

    def outputs():
        return dict(poses=np.full((api.LOCAL_MAX_FRAMES, 7), SENTINEL), end=np.full(15, SENTINEL), meas=np.full((api.LOCAL_MAX_FRAMES + 1, 7), SENTINEL),
                    cost=C.c_double(SENTINEL), grad=np.full(96, SENTINEL), jtj=np.full(96 * 96, SENTINEL), summary=(C.c_ubyte * C.sizeof(api.LocalGraphSummary))(*([0xA5] * C.sizeof(api.LocalGraphSummary))))

    def untouched(o):
        return all((o[k] == SENTINEL).all() for k in ("poses", "end", "meas", "grad", "jtj")) and o["cost"].value == SENTINEL and all(b == 0xA5 for b in o["summary"])

    p = api._ptr
    st = c["stamps"]
    last = int(np.searchsorted(st, c["T"][-1]))
    dup = st.copy(); dup[c["ii0"] + 1] = dup[c["ii0"]] = c["T"][0]
    bad_T = c["T"].copy(); bad_T[2] = bad_T[1]
    nan_acc = c["acc"].copy(); nan_acc[c["ii0"] + 3, 1] = np.nan
    long_st = 100.0 + np.arange(6000) * 1e-4
    bad_walks = {
        "buffer ends at the closing step": dict(stamps=st[:last], acc=c["acc"][:last], gyr=c["gyr"][:last]),
        "buffer ends inside the walk": dict(stamps=st[:c["ii0"] + 4], acc=c["acc"][:c["ii0"] + 4], gyr=c["gyr"][:c["ii0"] + 4]),
        "ii0 negative": dict(ii0=-1),
        "ii0 beyond the buffer": dict(ii0=len(st)),
        "dt1 + dt2 == 0": dict(stamps=dup),
        "stamps not increasing": dict(T=bad_T),
        "sample not finite": dict(acc=nan_acc),
        "scan stamp not finite": dict(T=np.array([c["T"][0], np.nan, c["T"][2], c["T"][3]])),
        "start state not finite": dict(R0=np.full((3, 3), np.inf)),
        "left anchor not finite": dict(left=nan7),
        "more samples than LILI_IMU_MAX_SAMPLES": dict(stamps=long_st, acc=np.zeros((6000, 3)), gyr=np.zeros((6000, 3)), ii0=0, T=np.array([100.00005, 100.2, 100.4, 100.55])),
    }
    s = api.LocalGraphSummary
    for what, change in bad_walks.items():
        wk, nn = _walk_struct(lg, c, **change)
        o = outputs()
        rc1 = lib.lili_local_graph_propagate(h, C.byref(wk), nn, p(o["poses"]), p(o["end"]), p(o["meas"]))
        rc2 = lib.lili_local_graph(h, C.byref(wk), nn, p(right), None, p(o["poses"]), p(o["meas"]), C.cast(o["summary"], C.POINTER(s)))
        assert rc1 == -1 and rc2 == -1, (what, rc1, rc2)
        assert untouched(o), what
    wk, nn = _walk_struct(lg, c)
    o = outputs()
    for what, rc in {
        "propagate: n too large": lib.lili_local_graph_propagate(h, C.byref(wk), api.LOCAL_MAX_FRAMES + 1, p(o["poses"]), p(o["end"]), p(o["meas"])),
        "propagate: n negative": lib.lili_local_graph_propagate(h, C.byref(wk), -1, p(o["poses"]), p(o["end"]), p(o["meas"])),
        "propagate: null walk": lib.lili_local_graph_propagate(h, None, n, p(o["poses"]), p(o["end"]), p(o["meas"])),
        "propagate: null poses": lib.lili_local_graph_propagate(h, C.byref(wk), n, None, p(o["end"]), p(o["meas"])),
        "propagate: null end": lib.lili_local_graph_propagate(h, C.byref(wk), n, p(o["poses"]), None, p(o["meas"])),
        "propagate: null meas": lib.lili_local_graph_propagate(h, C.byref(wk), n, p(o["poses"]), p(o["end"]), None),
        "run: null right": lib.lili_local_graph(h, C.byref(wk), n, None, None, p(o["poses"]), p(o["meas"]), C.cast(o["summary"], C.POINTER(s))),
        "run: right not finite": lib.lili_local_graph(h, C.byref(wk), n, p(nan7), None, p(o["poses"]), p(o["meas"]), C.cast(o["summary"], C.POINTER(s))),
        "run: null summary": lib.lili_local_graph(h, C.byref(wk), n, p(right), None, p(o["poses"]), p(o["meas"]), None),
    }.items():
        assert rc == -1, what
    assert untouched(o)
    # the chain calls
    x0 = a["x0"].copy()
    bad_meas = a["meas"].copy(); bad_meas[0, 4] = np.inf
    bad_opt = lg.options(max_iterations=0)
    bad_opt2 = lg.options(initial_radius=-1.0)
    x_in = np.vstack([x0, np.full((api.LOCAL_MAX_FRAMES - a["n"], 7), SENTINEL)])
    o = outputs()
    sp = C.cast(o["summary"], C.POINTER(s))
    for what, rc in {
        "solve: n too large": lib.lili_local_graph_solve(h, api.LOCAL_MAX_FRAMES + 1, p(anchors), p(a["meas"]), p(x_in), None, sp),
        "solve: n negative": lib.lili_local_graph_solve(h, -1, p(anchors), p(a["meas"]), p(x_in), None, sp),
        "solve: null anchors": lib.lili_local_graph_solve(h, a["n"], None, p(a["meas"]), p(x_in), None, sp),
        "solve: null meas": lib.lili_local_graph_solve(h, a["n"], p(anchors), None, p(x_in), None, sp),
        "solve: null poses": lib.lili_local_graph_solve(h, a["n"], p(anchors), p(a["meas"]), None, None, sp),
        "solve: null summary": lib.lili_local_graph_solve(h, a["n"], p(anchors), p(a["meas"]), p(x_in), None, None),
        "solve: measurement not finite": lib.lili_local_graph_solve(h, a["n"], p(anchors), p(bad_meas), p(x_in), None, sp),
        "solve: anchor not finite": lib.lili_local_graph_solve(h, a["n"], p(np.concatenate([nan7, a["right"]])), p(a["meas"]), p(x_in), None, sp),
        "solve: max_iterations 0": lib.lili_local_graph_solve(h, a["n"], p(anchors), p(a["meas"]), p(x_in), C.byref(bad_opt), sp),
        "solve: negative radius": lib.lili_local_graph_solve(h, a["n"], p(anchors), p(a["meas"]), p(x_in), C.byref(bad_opt2), sp),
        "evaluate: null cost": lib.lili_local_graph_evaluate(h, a["n"], p(anchors), p(a["meas"]), p(x_in), None, p(o["grad"]), p(o["jtj"])),
        "evaluate: null gradient": lib.lili_local_graph_evaluate(h, a["n"], p(anchors), p(a["meas"]), p(x_in), C.byref(o["cost"]), None, p(o["jtj"])),
        "evaluate: measurement not finite": lib.lili_local_graph_evaluate(h, a["n"], p(anchors), p(bad_meas), p(x_in), C.byref(o["cost"]), p(o["grad"]), p(o["jtj"])),
        "evaluate: n too large": lib.lili_local_graph_evaluate(h, 17, p(anchors), p(a["meas"]), p(x_in), C.byref(o["cost"]), p(o["grad"]), p(o["jtj"])),
    }.items():
        assert rc == -1, what
    nan_x = x_in.copy(); nan_x[0, 5] = np.nan
    assert lib.lili_local_graph_solve(h, a["n"], p(anchors), p(a["meas"]), p(nan_x), None, sp) == -1
    assert untouched(o) and x_in[:a["n"]].tobytes() == x0.tobytes() and (x_in[a["n"]:] == SENTINEL).all()
    # the context still solves case a
    x, info = lg.solve(a["left"], a["right"], a["meas"], a["x0"])
    _compare_solve(a, x, info, "after the refusals")
