"""Designed graphs for the robust loop factors and the damped solve (tests/test_pose_graph_robust_model_cpu.py, tests/test_pose_graph_robust_gpu.py): the smallest
graphs at which each part can go wrong.

Poses come from pose_graph_cases.circuit.  A true loop (a, b) measures between(true[a], true[b]); a FALSE loop (a, b) carries between(true[a], true[c]) with
c != b — what an ICP reports that registered a repeated place.  Variance 0.1 and scale 1 unless said otherwise.

A case is a dict: name, poses, estimates (None), loops [(from, to, meas, var)] — the true loops first, then the false ones —, n_true, loss (the kind every loop
carries), scale, options (the Gauss-Newton solve's and the damped solve's tolerances), lm (the damped solve's own options), expect, and max_loops (the context's
"pose_graph_max_loops" the case needs, or None).  Tolerances per case are chosen on the MODEL's sequences so that pose_graph_cases.decisions_clear holds for the
Gauss-Newton solve and for the damped one (the CPU test asserts it)."""
import numpy as np

from tests import pose_graph_cases as Cs
from tests import pose_graph_model as M
from tests import pose_graph_robust_model as R

S = Cs.S
LOSS_NAMES = ("huber", "cauchy", "geman_mcclure")


def _graph(name, n, seed, laps, true_pairs, false_triples, var=0.1):
    true, given = Cs.circuit(n, seed, laps=laps)
    loops = [(int(a), int(b), M.between(true[a], true[b]), var) for a, b in true_pairs]
    loops += [(int(a), int(b), M.between(true[a], true[c]), var) for a, b, c in false_triples]
    return dict(name=name, poses=given, estimates=None, loops=loops, n_true=len(true_pairs))


_GRAPHS = {}


def graph(name):
    """the loss-free description of a designed graph, built once"""
    if name not in _GRAPHS:
        if name == "n40":                # inside one segment
            g = _graph(name, 40, 71, 2.0, [(38, 2), (30, 12)], [(35, 8, 20)])
        elif name == "seg_edges":        # robust loops on fixed separators, on adjacent nodes, on both sides of a segment edge
            g = _graph(name, 2 * S + 80, 72, 3.0, [(S + 1, S - 1), (2 * S + 66, 40), (2 * S, S)], [(1000, 100, 600), (700, S, 300)])
        elif name == "blocked_72":       # 146 separators = 876 reduced unknowns: the blocked Cholesky
            g = _graph(name, 600, 73, 2.0, [(330 + j, 20 + j) for j in range(66)], [(500 + 7 * j, 250 + 5 * j, 100 + 5 * j) for j in range(6)])
            g["max_loops"] = 72
        else:
            raise KeyError(name)
        g.setdefault("max_loops", None)
        _GRAPHS[name] = g
    return _GRAPHS[name]


# The stop of every (graph, loss), for the Gauss-Newton solve and the damped one alike (the damping stays small on these graphs and the two walk the same costs),
# chosen on the model's sequence of relative cost drops.  Where consecutive drops lie a factor 100 apart, a function tolerance between them; where the solve
# converges linearly (drops a factor 5 to 90 apart: no threshold is a factor 10 clear of both neighbours), a fixed number of iterations instead.
_STOP = {
    ("n40", "huber"): dict(function_tolerance=1e-8),                 # 1.0e-3, 6.4e-10
    ("n40", "cauchy"): dict(function_tolerance=1e-9),                # 2.5e-7, 4.0e-11
    ("n40", "geman_mcclure"): dict(function_tolerance=1e-8),         # 1.4e-6, 5.5e-10
    ("seg_edges", "huber"): dict(function_tolerance=1e-6),           # 1.2e-4, 2.1e-8
    ("seg_edges", "cauchy"): dict(function_tolerance=1e-30, max_iterations=12),
    ("seg_edges", "geman_mcclure"): dict(function_tolerance=1e-30, max_iterations=8),
    ("blocked_72", "huber"): dict(function_tolerance=1e-5),          # 4.0e-3, 1.7e-7
    ("blocked_72", "cauchy"): dict(function_tolerance=2e-7),         # 4.1e-6, 9.5e-9
    ("blocked_72", "geman_mcclure"): dict(function_tolerance=1e-30, max_iterations=10),
}
_MAX_ITERATIONS = 16


def robust_case(name, loss, scale=1.0):
    g = dict(graph(name))
    stop = dict(max_iterations=_MAX_ITERATIONS)
    stop.update(_STOP[(name, loss)])
    g.update(name=f"{name}_{loss}", graph=name, loss=R.LOSSES[loss], loss_name=loss, scale=scale, options=stop, lm_options=dict(stop), lm={},
             expect=M.MAX_ITERATIONS if "max_iterations" in _STOP[(name, loss)] else None)
    return g


# the stops of the loss-free solves the effect is measured against, chosen the same way (the model's drops: n40 plain 1.3e-6, 3.4e-10; n40 clean 2.9e-2, 1.8e-9;
# seg_edges clean 2.6e-4, 3.7e-8; seg_edges plain a factor 40 apart: six iterations, the last step 1.5e-4 m against 3.5 m of damage)
_PLAIN_STOP = {("n40", True): dict(function_tolerance=1e-8), ("n40", False): dict(function_tolerance=1e-7),
               ("seg_edges", True): dict(function_tolerance=1e-30, max_iterations=6), ("seg_edges", False): dict(function_tolerance=1e-6)}


def plain_case(name, with_false=True):
    """the same graph without a loss: with the false loops (what plain least squares makes of them) or without (the clean solve)"""
    g = dict(graph(name))
    if not with_false:
        g["loops"] = g["loops"][:g["n_true"]]
    stop = dict(max_iterations=_MAX_ITERATIONS)
    stop.update(_PLAIN_STOP[(name, bool(with_false))])
    g.update(name=f"{name}_{'plain' if with_false else 'clean'}", graph=name, loss=R.NONE, loss_name="none", scale=1.0, options=stop, lm_options=dict(stop), lm={},
             expect=M.MAX_ITERATIONS if "max_iterations" in _PLAIN_STOP[(name, bool(with_false))] else None)
    return g


def robust_cases():
    return [robust_case(n, l) for n in ("n40", "seg_edges", "blocked_72") for l in LOSS_NAMES]


def _cost_increases():
    return next(c for c in Cs.solve_cases() if c["name"] == "cost_increases")


def lm_cases():
    """the damped solve on the graph plain Gauss-Newton gives up on (pose_graph_cases' cost_increases), loss NONE, max_iterations 40.  The model's sequences:
    damping 0 — nine rejected attempts, then relative cost drops 0.21, 0.28, 0.76, 0.77, 0.24, 1.5e-3, 8.6e-5, ... (a factor 10 apart from there on): the function
    tolerance sits between 0.21 and 1.5e-3 and ends the solve at attempt 15;  damping 1 — r r r A r A r A r A A A A A, the drops never a factor 100 apart, but
    |g|inf falls from 7.4e4 to 1.7e2 between attempts 14 and 15: the gradient tolerance sits between them."""
    base = _cost_increases()
    stops = {0: dict(function_tolerance=1.8e-2), 1: dict(function_tolerance=1e-30, gradient_tolerance=3.5e3)}
    out = []
    for diag in (0, 1):
        c = dict(base)
        c.update(name=f"lm_rejects_damping_{diag}", graph="cost_increases", n_true=1, loss=R.NONE, loss_name="none", scale=1.0, max_loops=None,
                 lm_options=dict(max_iterations=40, **stops[diag]), lm=dict(diagonal_damping=diag), expect=None)
        out.append(c)
    c = dict(base)
    c.update(name="lm_lambda_limit", graph="cost_increases", n_true=1, loss=R.NONE, loss_name="none", scale=1.0, max_loops=None,
             lm_options=dict(max_iterations=40, **stops[0]), lm=dict(lambda_upper=1e2), expect=R.LAMBDA_LIMIT)
    out.append(c)
    return out


def huber_branch_cases():
    """a chain of 3 nodes and one Huber loop whose d at the initial estimate sits 0.1 % below, then 0.1 % above, its scale: the two branches of the weight"""
    true, given = Cs.circuit(3, 74, rot_total=0.2, trans_total=1.0)
    meas = M.between(true[2], true[0])
    g = R.RobustGraph()
    g.append(None, given)
    g.add_loop(2, 0, meas, np.full(6, 0.1))
    d = float(np.sqrt(g.loop_status()[0][0]))
    out = []
    for tag, k in (("below", d * 1.001), ("above", d / 1.001)):
        out.append(dict(name=f"chain3_huber_{tag}", graph="chain3", poses=given, estimates=None, loops=[(2, 0, meas, 0.1)], n_true=1, loss=R.HUBER, loss_name="huber",
                        scale=k, max_loops=None, options=dict(function_tolerance=_CHAIN3_FTOL, max_iterations=_MAX_ITERATIONS),
                        lm_options=dict(function_tolerance=_CHAIN3_FTOL, max_iterations=_MAX_ITERATIONS), lm={}, expect=None, d=d))
    return out


_CHAIN3_FTOL = 1e-7


def build_model(case, prior_var=M.PRIOR_VAR, odom_var=M.ODOM_VAR):
    g = R.RobustGraph(prior_var, odom_var)
    g.append(None, case["poses"])
    for a, b, m, v in case["loops"]:
        g.add_loop(a, b, m, np.full(6, v), case["loss"], case["scale"])
    if case["estimates"] is not None:
        g.X = M.normalize_poses(case["estimates"])
    return g


_reference = {}


def reference(case, kind):
    """the model's solve of a case, computed once: kind "gn" (M.gauss_newton on the robust graph, the case's options) or "lm" (levenberg_marquardt, lm_options and
    lm) -> (graph, X, summary, D0), D0 the pose spread of the model's two linear solvers; the two must agree on attempts, pattern and termination"""
    key = (case["name"], kind)
    if key not in _reference:
        g = build_model(case)
        second = Cs.second_solver(case)
        if kind == "gn":
            X, s = M.gauss_newton(g, solver="sparse", **case["options"])
            X2, s2 = M.gauss_newton(g, solver=second, **case["options"])
        else:
            X, s = R.levenberg_marquardt(g, solver="sparse", **case["lm_options"], **case["lm"])
            X2, s2 = R.levenberg_marquardt(g, solver=second, **case["lm_options"], **case["lm"])
            assert s["accepted"] == s2["accepted"] and s["lambda"] == s2["lambda"], key
        assert (s["iterations"], s["termination"]) == (s2["iterations"], s2["termination"]), key
        _reference[key] = (g, X, s, M.pose_difference(X, X2))
    return _reference[key]


def distance(Xa, Xb):
    """largest position difference between two solutions (m)"""
    return float(np.linalg.norm(np.asarray(Xa)[:, 0:3] - np.asarray(Xb)[:, 0:3], axis=1).max())
