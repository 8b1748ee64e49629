"""The arithmetic inside one pose-graph factor on the device (lili_pose_graph.hip: pg_log, pg_jr_inv, pg_error, the Jacobian blocks of k_pg_linearize, the frozen
measurement of k_pg_append, the retraction of pg_candidate) on the hard states of tests/pose_graph_factor_cases.py, against the multi-precision
referee tests/pose_graph_factor_referee.py.

evaluate, loop_status: per state reset, append, add_loop / add_loop_robust, set_poses, evaluate, loop_status; EVERY entry of every output obeys
    |device - referee| <= max(10 D, 64 eps) A(entry)
with A the entry's magnitude sum (the referee's) and D the f64 model's own largest |model - referee| / A of that state and array
(tests/test_pose_graph_factor_cases_cpu.py caps it: 64 eps up to 3.0 rad, eps / delta at pi -/+ delta).  10 over D: D is one sample of a rounding error whose size
the formula's conditioning fixes, and the device's sin, cos and atan2 may differ from libm's by an ulp or two; 64 eps: a 6-row Gram of products of roughly
30-flop entries.  An entry whose A is 0 must be exactly 0.  The diagonal blocks are bit-symmetric.  A state whose quaternions go in negated, or 9e-7 long or short of
unit norm (all of them, only set_poses', only prev's; prev is not the pose the graph holds), also agrees with its plain twin's device result under the same bound (not bit for bit: the host's normalisation rounds).

One Gauss-Newton step at large retractions (solve with max_iterations = 1 and every tolerance 0): chains whose last node is off by up to 3.0 rad and 10 m land on
the given poses within max(10 D1, 64 eps max |p|), the cost under the rounding floor; where the step is not exact (two moved nodes, a loop) the poses are the
referee's mp iteration's and the candidate's cost agrees to 1e-9 (a chain's, which sits next to zero, to 1e-9 plus its rounding floor's cross term); step_inf to 64 eps relative; a step that raises the cost leaves the poses byte for byte.

The mp work is done once per session (pose_graph_factor_cases.reference / step_reference)."""
import numpy as np
import pytest

import lili_om_amd as L
from tests import pose_graph_factor_cases as FC
from tests import pose_graph_model as M
from tests import pose_graph_robust_model as RM

pytestmark = pytest.mark.gpu

EPS = FC.EPS
STATES = FC.states()
BY_NAME = {s["name"]: s for s in STATES}
GROUPS = {}
for _s in STATES:
    GROUPS.setdefault(_s["name"].split("/")[0], []).append(_s)
STEPS = FC.chain_step_cases() + FC.loop_step_cases()
_worst = {}      # (frame family, theta label) -> array -> [device ratio, D]


@pytest.fixture()
def pg(gpu_ctx):
    g = L.PoseGraph(gpu_ctx)
    g.reset()
    yield g
    g.reset()


def _evaluate(pg, st):
    pg.reset()
    if st["prev"] is None:
        assert pg.append(st["given"]) == 0
    else:
        assert pg.append(st["given"][0:1]) == 0 and pg.append(st["given"][1:], prev=st["prev"]) == 1
    for a, b, m, v, kind, k in st["loops"]:
        if kind == RM.NONE:
            pg.add_loop(a, b, m, v)
        else:
            pg.add_loop(a, b, m, v, loss=kind, scale=k)
    pg.set_poses(st["estimates"])
    assert pg.info() == (FC.N, len(st["loops"]))
    opt = pg.options(prior_var=st["prior_var"], odom_var=st["odom_var"])
    cost, grad, D, S, LB = pg.evaluate(opt)
    d2, w = pg.loop_status(options=opt)
    return dict(cost=cost, gradient=grad, diag=D, sub=S, loop=LB, d2=d2, w=w)


@pytest.mark.parametrize("group", list(GROUPS), ids=list(GROUPS))
def test_every_entry_against_the_referee(pg, group):
    bad = []
    for st in GROUPS[group]:
        ref, D = FC.reference(st)
        dev = _evaluate(pg, st)
        twin = _evaluate(pg, BY_NAME[st["twin"]]) if st["twin"] is not None else None
        line = []
        for k in FC.ARRAYS:
            bound = max(10.0 * D[k], 64.0 * EPS)
            ratio = FC.ratio(dev[k], ref[k], ref["A_" + k])
            line.append(f"{k} {ratio / EPS:.3g} ({D[k] / EPS:.3g})")
            row = _worst.setdefault((st["family"], st["theta"][0]), {}).setdefault(k, [0.0, 0.0])
            row[0], row[1] = max(row[0], ratio), max(row[1], D[k])
            if not ratio <= bound:
                bad.append((st["name"], k, f"{ratio / EPS:.4g} eps", f"bound {bound / EPS:.4g} eps"))
            if twin is not None:
                rt = FC.ratio(dev[k], twin[k], ref["A_" + k])
                if not rt <= bound:
                    bad.append((st["name"], k, "against its twin", f"{rt / EPS:.4g} eps", f"bound {bound / EPS:.4g} eps"))
        print(f"[{st['name']}] |device - referee| / A in eps (D): " + "  ".join(line))
        if not (dev["diag"] == np.swapaxes(dev["diag"], 1, 2)).all():
            bad.append((st["name"], "diag", "not bit-symmetric"))
    assert not bad, bad


def test_report_per_theta():
    """the table of DESIGN.md §7k: per theta the largest |device - referee| / A beside D (in eps), over the exact-frame (X) and the generic-frame (S) states the
    tests above ran"""
    print()
    for family in ("X", "S"):
        for label, _, _ in FC.THETAS:
            if (family, label) in _worst:
                print(f"theta {label:>9} [{family}]: " + "  ".join(f"{k} {v[0] / EPS:.3g} ({v[1] / EPS:.3g})" for k, v in _worst[(family, label)].items()))


def _cost_floor(g):
    w = max(1.0 / np.sqrt(g.prior_var.min()), 1.0 / np.sqrt(g.odom_var.min()), max([1.0 / np.sqrt(l[3].min()) for l in g.loops], default=0.0))
    return 0.5 * (g.n + len(g.loops)) * (64.0 * EPS * max(1.0, np.abs(g.X[:, 0:3]).max()) * w) ** 2


@pytest.mark.parametrize("c", STEPS, ids=[c["name"] for c in STEPS])
def test_one_gauss_newton_step(pg, c):
    ref, g, X_m, s_m, d1 = FC.step_reference(c)
    pg.reset()
    assert pg.append(c["given"]) == 0
    for a, b, m, v in c["loops"]:
        pg.add_loop(a, b, m, v)
    pg.set_poses(c["estimates"])
    X0 = pg.poses()
    s = pg.solve(max_iterations=1, function_tolerance=0.0, gradient_tolerance=0.0, parameter_tolerance=0.0)
    X = pg.poses()
    truth = M.normalize_poses(c["given"]) if c["exact"] else ref["poses"]
    dp, da = M.pose_difference(X, truth)
    floor = 64.0 * EPS * np.abs(truth[:, 0:3]).max()
    tp, ta = max(10.0 * d1[0], floor), max(10.0 * d1[1], floor)
    ds = abs(s["step_inf"][0] - ref["step_inf"]) / ref["step_inf"]
    print(f"[{c['name']}] termination {s['termination']} cost {s['initial_cost']:.6e} -> {s['cost'][0]:.6e} (referee {ref['cost']:.6e} -> {ref['new_cost']:.6e}); "
          f"position {dp:.2e} m (D1 {d1[0]:.2e}, bound {tp:.2e}) angle {da:.2e} rad (D1 {d1[1]:.2e}, bound {ta:.2e}); step_inf {ds / EPS:.3g} eps relative")
    assert s["iterations"] == 1 and len(s["cost"]) == 1
    assert ds <= 64.0 * EPS
    if c["expect"] == "rejected":
        assert s["termination"] == M.COST_INCREASED and X.tobytes() == X0.tobytes()
        assert abs(s["cost"][0] - ref["new_cost"]) <= 1e-9 * ref["new_cost"] and s["final_cost"] == s["initial_cost"]
        return
    assert s["termination"] == M.MAX_ITERATIONS and s["final_cost"] == s["cost"][0] and X.tobytes() != X0.tobytes()
    assert dp <= tp and da <= ta
    if c["exact"]:
        assert s["final_cost"] <= _cost_floor(g), (s["final_cost"], _cost_floor(g))
    elif c["loops"]:
        assert abs(s["cost"][0] - ref["new_cost"]) <= 1e-9 * ref["new_cost"]
    else:
        # a chain's candidate sits next to a zero of the cost: its residuals r carry the absolute rounding d the floor is made of (64 eps |p| / s per factor), and
        # (r + d)^2 / 2 - r^2 / 2 = r d + d^2 / 2 is at most 2 sqrt(cost floor) + floor summed over the factors (Cauchy-Schwarz)
        floor_c = _cost_floor(g)
        assert abs(s["cost"][0] - ref["new_cost"]) <= 1e-9 * ref["new_cost"] + 2.0 * np.sqrt(ref["new_cost"] * floor_c) + floor_c
