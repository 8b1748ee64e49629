"""Designed graphs for the global pose graph (tests/test_pose_graph_model_cpu.py, tests/test_pose_graph_gpu.py): the smallest shapes at which the nested-dissection
elimination can go wrong, S = LILI_PG_SEGMENT.

A case is a dict: name, poses (N, 7: the poses as given at append time — the chain measurements come from them), estimates (N, 7 or None: what set_poses writes
before the solve; None = the given poses), loops [(from, to, meas (7), var)], options (the solve's), expect (None = a convergence code, else the termination).

Every graph is a drifting circuit: the true trajectory is a closed circle, the given poses are its dead-reckoned copy with random-walk drift, a loop measurement is
between(true[from], true[to]) — what a perfect ICP would report.  Graphs without a loop start from estimates perturbed in the tangent space instead (a chain alone is
at its optimum where it was appended); their tolerances are set so that the quadratically shrinking steps cross them with room to spare."""
import numpy as np

from tests import pose_graph_model as M

S = 512
MAX_NODES, MAX_LOOPS = 32768, 32


def circuit(n, seed, length=30.0, rot_total=0.03, trans_total=0.3, laps=1.0):
    """-> true (n, 7), given (n, 7): a circle of circumference `length` driven `laps` times; the drift is a random walk whose standard deviation after n steps is
    rot_total (rad) / trans_total (m)"""
    rng = np.random.default_rng(seed)
    radius = length / (2.0 * np.pi)
    ang = 2.0 * np.pi * laps * np.arange(n) / max(n - 1, 1)
    true = np.zeros((n, 7))
    true[:, 0], true[:, 1], true[:, 2] = radius * np.cos(ang), radius * np.sin(ang), 0.2 * np.sin(3.0 * ang)
    yaw = ang + 0.5 * np.pi
    roll = 0.05 * np.sin(2.0 * ang)
    qy = np.stack([np.cos(0.5 * yaw), 0 * yaw, 0 * yaw, np.sin(0.5 * yaw)], -1)
    qr = np.stack([np.cos(0.5 * roll), np.sin(0.5 * roll), 0 * roll, 0 * roll], -1)
    true[:, 3:7] = M.qnormalize(M.qmul(qy, qr))
    rel = M.between(true[:-1], true[1:]) if n > 1 else np.zeros((0, 7))
    given = np.zeros((n, 7))
    given[0] = true[0]
    k = max(n - 1, 1)
    noise = np.concatenate([rng.normal(0, rot_total / np.sqrt(k), (n, 3)), rng.normal(0, trans_total / np.sqrt(k), (n, 3))], 1)
    for i in range(1, n):
        step = M.retract(rel[i - 1], noise[i])
        given[i, 0:3] = given[i - 1, 0:3] + M.qrot(given[i - 1, 3:7], step[0:3])
        given[i, 3:7] = M.qnormalize(M.qmul(given[i - 1, 3:7], step[3:7]))
    return true, given


def perturbed(poses, seed, rot=3e-3, trans=3e-2):
    rng = np.random.default_rng(seed)
    n = poses.shape[0]
    return M.retract(poses, np.concatenate([rng.normal(0, rot, (n, 3)), rng.normal(0, trans, (n, 3))], 1))


def _loop(true, a, b, var):
    return (int(a), int(b), M.between(true[a], true[b]), float(var))


# Tolerances per case: chosen on the MODEL's sequences so that every stop decision is at least a factor 10 clear of its threshold (the CPU test asserts it) and the
# solve ends at an iteration whose cost still drops by more than rounding.  A chain's cost goes to zero, so its step size decides; a looped graph ends by the
# function tolerance.
def _chain(name, n, seed, ptol=1e-4):
    _, given = circuit(n, seed)
    return dict(name=name, poses=given, estimates=perturbed(given, seed + 100), loops=[],
                options=dict(parameter_tolerance=ptol, function_tolerance=1e-30, gradient_tolerance=1e-30), expect=None)


def _looped(name, n, seed, pairs, var=0.1, ftol=None, options=None, expect=None, **kw):
    true, given = circuit(n, seed, **kw)
    opt = dict(options or {})
    if ftol is not None:
        opt["function_tolerance"] = ftol
    return dict(name=name, poses=given, estimates=None, loops=[_loop(true, a, b, v if v is not None else var) for a, b, v in [(p + (None,))[:3] for p in pairs]],
                options=opt, expect=expect)


def solve_cases():
    cs = []
    _, g1 = circuit(1, 1)
    cs.append(dict(name="n1_prior_only", poses=g1, estimates=None, loops=[], options={}, expect=None))                                  # 1
    cs.append(_chain("n2", 2, 2, ptol=5e-3))                                                                                              # 2
    cs.append(_looped("n3_loop_2_0", 3, 3, [(2, 0)], rot_total=0.2, trans_total=1.0))                                                     # 3 (the default tolerances)
    for n in (S - 1, S, S + 1, 2 * S + 1):                                                                                                # 4
        cs.append(_chain(f"chain_{n}", n, 10 + n))
    cs.append(_looped("endpoint_node0", 200, 20, [(199, 0)], ftol=1e-7))                                                                  # 5, 6
    cs.append(_looped("endpoint_last_from_lt_to", 200, 21, [(3, 199)], ftol=1e-8))                                                        # 6, 12 (from < to)
    cs.append(_looped("endpoint_on_multiple_of_S", S + 80, 22, [(S + 70, S), (S + 79, 7)]))                                               # 7 (the default tolerances)
    cs.append(_looped("endpoints_either_side_of_S", S + 80, 23, [(S + 1, S - 1), (S + 75, 3)], ftol=1e-7))                                # 8
    cs.append(_looped("adjacent_endpoints", 200, 24, [(150, 151), (195, 5)], ftol=1e-8))                                                  # 9
    cs.append(_looped("shared_endpoint", 200, 25, [(190, 10), (150, 10)], ftol=1e-7, laps=2.0))                                           # 10
    cs.append(_looped("same_pair_twice", 200, 26, [(190, 10), (190, 10, 0.2)], ftol=1e-8))                                                # 11
    cs.append(_looped("both_directions", 200, 27, [(190, 10), (20, 180)], ftol=1e-9))                                                     # 12
    cs.append(_looped("crossing_and_nested", 260, 28, [(200, 20), (250, 100), (180, 60), (240, 5)], ftol=1e-7, laps=2.0))                 # 13
    rng = np.random.default_rng(29)
    pairs = []
    while len(pairs) < MAX_LOOPS:                                                                                                         # 14
        a, b = (int(v) for v in rng.integers(0, 200, 2))
        if abs(a - b) > 3:
            pairs.append((a, b))
    cs.append(_looped("max_loops", 200, 29, pairs, ftol=1e-8, laps=3.0))
    cs.append(_looped("circuit_2048", 2048, 30, [(2040, 8), (1500, 476), (1100, 76)], var=0.3, ftol=1e-7, laps=2.0))                      # 15
    cs.append(_looped("strong_loop", 200, 31, [(195, 4)], var=1e-6, ftol=1e-9))                                                           # 16
    # 17: a strong loop measurement rotated by about pi — the first Gauss-Newton step lands ten times further away than it started
    true, given = circuit(60, 32)
    m = M.between(true[55], true[3])
    m[3:7] = M.qnormalize(M.qmul(m[3:7], np.array([np.cos(0.5 * 3.1), 0.0, 0.0, np.sin(0.5 * 3.1)])))
    cs.append(dict(name="cost_increases", poses=given, estimates=None, loops=[(55, 3, m, 1e-6)], options={}, expect=M.COST_INCREASED))
    cs.append(_looped("two_iterations", 200, 33, [(196, 2)], ftol=1e-8, options=dict(max_iterations=2), expect=M.MAX_ITERATIONS))         # 18
    return cs


def full_size(n=MAX_NODES, seed=40):
    """N = LILI_PG_MAX_NODES (or smaller for the CPU check of the same generator), 4 loops, eight laps.  The function tolerance sits where the model's cost still
    drops by 70 times the rounding of its own sum (relative 3e-14), so the solve ends by convergence and not on a cost that rounding raised."""
    true, given = circuit(n, seed, laps=8.0, rot_total=0.02, trans_total=0.2)
    per = (n - 1) / 8.0
    pairs = [(int(7.5 * per), int(0.5 * per)), (int(6.25 * per), int(2.25 * per)), (n - 1, int(3.0 * per)), (int(5.1 * per), 0)]
    return dict(name=f"full_{n}", poses=given, estimates=None, loops=[_loop(true, a, b, 0.3) for a, b in pairs], options=dict(function_tolerance=1e-11), expect=None)


def build_model(case, prior_var=M.PRIOR_VAR, odom_var=M.ODOM_VAR):
    g = M.Graph(prior_var, odom_var)
    g.append(None, case["poses"])
    for a, b, m, v in case["loops"]:
        g.add_loop(a, b, m, np.full(6, v))
    if case["estimates"] is not None:
        g.X = M.normalize_poses(case["estimates"])
    return g


def second_solver(case):
    """the dense solve where the matrix fits comfortably, SuperLU in the natural order (a second elimination order) beyond that"""
    return "dense" if case["poses"].shape[0] <= 300 else "natural"


_reference = {}


def reference(case):
    """the model's solve of a case, computed once: (graph, X, summary, D0) — D0 = (position, angle): the largest pose difference between the model's two linear
    solvers, the yardstick of the device's tolerance"""
    if case["name"] not in _reference:
        g = build_model(case)
        X, s = M.gauss_newton(g, solver="sparse", **case["options"])
        X2, s2 = M.gauss_newton(g, solver=second_solver(case), **case["options"])
        assert (s["iterations"], s["termination"]) == (s2["iterations"], s2["termination"]), case["name"]
        _reference[case["name"]] = (g, X, s, M.pose_difference(X, X2))
    return _reference[case["name"]]


def incremental_script(ftol1=1e-8, ftol2=1e-7):
    """append in pieces -> loop -> solve -> append more (in the odometry's own frame, which the first solve has left) -> loop -> solve"""
    true, given = circuit(300, 50, laps=2.0)
    return [("append", None, given[0:100]), ("append", given[99], given[100:180]), ("loop", 170, 10, M.between(true[170], true[10]), 0.1),
            ("solve", dict(function_tolerance=ftol1)), ("append", given[179], given[180:300]), ("loop", 290, 120, M.between(true[290], true[120]), 0.1),
            ("solve", dict(function_tolerance=ftol2))]


def decisions_clear(summary):
    """every stop decision of a model solve a factor 10 clear of its threshold, every accept decision 1e-12 of the cost clear of rounding"""
    for name, v, thr in summary["margins"]:
        if name == "increase":
            if not (abs(v - thr) >= 1e-12 * thr or thr == 0.0):
                return False
        elif not (v >= 10.0 * thr or v <= 0.1 * thr):
            return False
    return True


def run_script_on_model(script, solver="sparse"):
    """-> the graph, [(X, summary) per solve]"""
    g, out = M.Graph(), []
    for step in script:
        if step[0] == "append":
            g.append(step[1], step[2])
        elif step[0] == "loop":
            g.add_loop(step[1], step[2], step[3], np.full(6, step[4]))
        else:
            X, s = M.gauss_newton(g, solver=solver, **step[1])
            g.X = X
            out.append((X, s))
    return g, out
