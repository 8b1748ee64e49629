"""States for the pose graph's factor arithmetic (tests/test_pose_graph_factor_cases_cpu.py, tests/test_pose_graph_factors_gpu.py): three-node graphs on which ONE
factor has a prescribed residual rotation theta about a prescribed axis, composed in mp (tests/pose_graph_factor_referee.py) and rounded once.

How a state is made.  The given poses G_0 .. G_2 are appended (that freezes Z = between(G_i-1, G_i) on the device); then
  prior, chain (1, 2)   set_poses moves the factor's second node B to (p_B + R_B u, q_B Exp(rot axis)): R_Z^T R_A^T R_B = Exp(rot axis), translation residual u;
  a loop (from, to)     the estimates stay at the given poses and the loop's measurement is between(G_from, G_to) o (-R u, Exp(-rot axis)): the same residual.
rot = theta, or pi - delta, or pi + delta (the far side: q_e.w < 0, Log must return pi - delta about the opposite axis).

What keeps a state honest.  The referee takes the f64 numbers the library is given as exact, so the residual it computes is the one the device is asked for only
as far as rounding the composed quaternion once leaves it alone: half an ulp of a component of size 1 is 1e-16 rad, 1e-4 of a 1e-12 rad residual.  Two frame families:
  X ("exact")    every given rotation is one of the unit quaternions 1, i, j, k and every position a small dyadic number: products with them are exact in f64 and in
                 mp alike, so q_e IS the composed Exp(rot axis), bit for bit, and a zero residual is exactly zero everywhere.  Used for every theta <= 1e-3, for the
                 coordinate axis (whose exact zeros a generic frame would fill with 1e-17 noise), for the 1e-9 m translation residual (the factor's two nodes sit at
                 the origin, so 1e-9 keeps its 16 digits) and for the negated / rescaled inputs (all of them at once, set_poses' alone, prev's alone).
  S ("generic")  random rotations and positions, except that the rotation that multiplies Exp(rot axis) is a unit: the moved node's own given rotation (prior,
                 chain), or q_to = q_from j for a loop.  Every product on the device rounds as it does in the field (absolute errors of an ulp in q_e), while the
                 prescribed angle survives in the referee to 1e-15.  A loop's translation residual is zero only with p_to = p_from (d = 0 exactly): a generic d
                 rounds differently in R_A^T (p_B - p_A) than in the measurement.  Used for theta >= 0.09.
Variances: six distinct values per factor, (0.25, 1, 4, 0.5, 2, 8) times the reference's prior / odometry variances (loops: times 0.1), or times 1 ("unit")."""
import zlib

import mpmath as mp
import numpy as np

from tests import pose_graph_factor_referee as R
from tests import pose_graph_model as M
from tests import pose_graph_robust_model as RM

EPS = float(np.finfo(np.float64).eps)
PATTERN = np.array([0.25, 1.0, 4.0, 0.5, 2.0, 8.0])
N = 3

# label, side, value: plain = the angle itself; near / far = pi -/+ delta
THETAS = [("0", "plain", "0"), ("1e-12", "plain", "1e-12"), ("1e-8", "plain", "1e-8"), ("1e-3", "plain", "1e-3"), ("0.09", "plain", "0.09"),
          ("0.0999999", "plain", "0.0999999"), ("0.1000001", "plain", "0.1000001"), ("0.11", "plain", "0.11"), ("0.5", "plain", "0.5"), ("pi/2", "plain", "pi/2"),
          ("2.0", "plain", "2.0"), ("3.0", "plain", "3.0"), ("pi-1e-3", "near", "1e-3"), ("pi-1e-6", "near", "1e-6"), ("pi-1e-8", "near", "1e-8"),
          ("pi+1e-3", "far", "1e-3"), ("pi+1e-6", "far", "1e-6"), ("pi+1e-8", "far", "1e-8")]
THETA = {t[0]: t for t in THETAS}
SUBSET = ["0", "1e-8", "0.1000001", "2.0", "pi-1e-6"]
AXES = {"generic": ("0.36", "-0.48", "0.8"), "coordinate": ("0", "1", "0"), "tiny": ("0.6", "0.8", "1e-9")}
KINDS = {"prior": (-1, 0), "chain": (1, 2), "loop_gt": (2, 0), "loop_lt": (0, 2), "loop_adj": (1, 2)}
UNITS = [(1.0, 0.0, 0.0, 0.0), (0.0, 0.0, 1.0, 0.0), (0.0, 1.0, 0.0, 0.0)]
X_SMALL = [(0.5, -1.0, 0.25), (2.0, -1.5, 0.5), (3.25, 1.0, -0.75)]
X_LARGE = [(1000.0, 990.0, 1010.0), (1024.0, 1000.0, 1002.0), (1040.0, 985.0, 1015.0)]


def _small_angle(label):
    return label in ("0", "1e-12", "1e-8", "1e-3")


def _rot(th):
    _, side, v = th
    if side == "plain":
        return mp.pi / 2 if v == "pi/2" else mp.mpf(v)
    return mp.pi - mp.mpf(v) if side == "near" else mp.pi + mp.mpf(v)


def expected_angle(th):
    """what Log must return (mp; call inside mp.workdps)"""
    _, side, v = th
    return _rot(th) if side == "plain" else mp.pi - mp.mpf(v)


def _round(v):
    return [float(x) for x in v]


J_UNIT = np.array([0.0, 0.0, 1.0, 0.0])
# a variant hands some of the quaternions in scaled by c: the factor, and the inputs it applies to
VARIANTS = {"negated": (-1.0, ("given", "prev", "meas", "estimates")), "up": (1.0 + 9e-7, ("given", "prev", "meas", "estimates")),
            "down": (1.0 - 9e-7, ("given", "prev", "meas", "estimates")), "set_negated": (-1.0, ("estimates",)), "prev_negated": (-1.0, ("prev",))}


def _rotations(kind, family, rng):
    """the given rotations.  X: the units.  S: random, except the one that multiplies Exp(rot axis): the moved node's own (prior: k, chain: i), q_to = q_from j
    for a loop (a signed permutation of q_from's numbers, so q_from^-1 q_to = j exactly)"""
    if family == "X":
        return np.array(UNITS)
    a, b = KINDS[kind]
    q = M.qnormalize(rng.normal(0, 1, (N, 4)))
    q[b] = {"prior": (0.0, 0.0, 0.0, 1.0), "chain": UNITS[2]}.get(kind, M.qmul(q[a], J_UNIT) + 0.0)
    return q


def _positions(kind, family, lever, rng):
    """the given positions.  lever: "small" (a few metres), "large" (|d| about 30 m at coordinates near 1e3 m), "zero" (the factor's two nodes on one point: d = 0
    exactly), "origin" (that point is the origin, so a 1e-9 m residual keeps its digits).  For the prior the lever that matters is the one of chain factor (0, 1),
    whose first node is the one the state moves."""
    if family == "X":
        P = np.array(X_LARGE if lever == "large" else X_SMALL)
    else:
        P = 1000.0 + rng.uniform(-20.0, 20.0, (N, 3)) if lever == "large" else rng.uniform(-3.0, 3.0, (N, 3))
    a, b = KINDS[kind]
    a = 1 if kind == "prior" else a
    if lever in ("zero", "origin"):
        P[b] = P[a] = 0.0 if lever == "origin" else P[a]
    return P


def _prev_of(G0):
    """the pose handed to the second append for node 0: NOT the pose the graph holds, so the measurement of node 1 has to come from it"""
    xi = np.concatenate([0.25 * np.array([0.6, 0.0, 0.8]), [0.25, -0.5, 0.125]])
    return M.retract(G0[None], xi[None])[0]


def state(name, kind, theta, axis="generic", family=None, u=(0.0, 0.0, 0.0), lever="small", variances="ref", loss="none", variant=None, use_prev=False):
    """-> dict: name, kind, theta (the THETAS entry), axis, factor (the index of the factor under test), given, prev, estimates, loops [(from, to, meas, var,
    loss, scale)], prior_var, odom_var, twin (the plain state's name for a variant).  loss: "none", "huber_below", "huber_above", "huber_far", "cauchy", "gm".
    The random frame of a state is seeded by its name (a variant's: by its twin's)."""
    th = THETA[theta]
    twin = name[:name.rindex("/")] if variant is not None else None
    if family is None:
        family = "X" if _small_angle(theta) or axis == "coordinate" or variant is not None else "S"
    a, b = KINDS[kind]
    u = np.asarray(u, np.float64)
    u_tiny = bool(0 < np.abs(u).max() < 1e-6)
    is_loop = kind.startswith("loop")
    if family == "X" and (kind == "prior" or (u_tiny and kind == "chain")):
        lever = "origin"
    elif u_tiny:
        lever = "zero"
    if family == "S":
        assert not _small_angle(theta) and axis != "coordinate" and not u_tiny
        assert not is_loop or lever == "zero" or np.abs(u).max() >= 1.0
    rng = np.random.default_rng(zlib.crc32((twin or name).encode()))
    G = np.hstack([_positions(kind, family, lever, rng), _rotations(kind, family, rng)])
    scale = dict(ref=(M.PRIOR_VAR, M.ODOM_VAR, np.full(6, 0.1)), unit=(np.ones(6), np.ones(6), np.ones(6)))[variances]
    prior_var, odom_var, loop_var = (PATTERN * s for s in scale)
    E = G.copy()
    loops = []
    with mp.workdps(R.DPS):
        rot = _rot(th)
        um = R.vec(u)
        if not is_loop:
            pB, qB = R.pose(G[b])
            E[b, 3:7] = _round(R.compose_rotation(qB, rot, AXES[axis]))
            mv = R.mv(R.qmat(qB), um)
            E[b, 0:3] = _round([pB[i] + mv[i] for i in range(3)])
        else:
            t, q = R.between(R.pose(G[a]), R.pose(G[b]))
            qz = R.compose_rotation(R.vals(q), -rot, AXES[axis])
            mv = R.mv(R.qmat(R.vec(qz)), um)
            loops.append([a, b, np.array(_round([t[i] - mv[i] for i in range(3)]) + _round(qz)), loop_var, RM.NONE, 1.0])
    st = dict(name=name, kind=kind, theta=th, axis=axis, family=family, lever=lever, factor=(0 if kind == "prior" else 2 if kind == "chain" else N), given=G,
              prev=_prev_of(G[0]) if use_prev else None, estimates=E, loops=loops, prior_var=prior_var, odom_var=odom_var, twin=twin, loss=loss, variant=variant)
    if loss != "none":
        assert is_loop
        with mp.workdps(R.DPS):
            g = referee_graph(st)
            d = mp.sqrt(g.factor(g.X, N)["d2"])
            kind_k = dict(huber_below=(RM.HUBER, d * (1 + mp.mpf("1e-4"))), huber_above=(RM.HUBER, d * (1 - mp.mpf("1e-4"))), huber_far=(RM.HUBER, d / 50),
                          cauchy=(RM.CAUCHY, d / 2), gm=(RM.GEMAN_MCCLURE, d))[loss]
        loops[0][4], loops[0][5] = kind_k[0], float(kind_k[1])
    if variant is not None:
        c, which = VARIANTS[variant]
        if "given" in which:
            st["given"] = G.copy()
            st["given"][:, 3:7] *= c
        if "estimates" in which:
            st["estimates"] = E.copy()
            st["estimates"][:, 3:7] *= c
        if "prev" in which and st["prev"] is not None:
            st["prev"][3:7] *= c
        if "meas" in which:
            for l in loops:
                l[2] = l[2].copy()
                l[2][3:7] *= c
    return st


def referee_graph(st):
    return R.Graph(st["given"], st["estimates"], st["loops"], st["prior_var"], st["odom_var"], prev=st["prev"], split=1)


def model_graph(st):
    g = RM.RobustGraph(st["prior_var"], st["odom_var"])
    if st["prev"] is None:
        g.append(None, st["given"])
    else:
        g.append(None, st["given"][0:1])
        g.append(st["prev"], st["given"][1:])
    for a, b, m, v, kind, k in st["loops"]:
        g.add_loop(a, b, m, v, kind, k)
    g.X = M.normalize_poses(st["estimates"])
    return g


def _build():
    S = []
    axes = list(AXES)
    # every theta: the chain factor about each axis, one loop kind (from > to) with the axes taken in turn
    for label, _, _ in THETAS:
        for ax in axes:
            S.append(state(f"chain/{label}/{ax}", "chain", label, ax))
    for i, (label, _, _) in enumerate(THETAS):
        ax = axes[i % 3]
        S.append(state(f"loop_gt/{label}/{ax}", "loop_gt", label, ax, lever="zero"))
    # the other factor kinds at the five angles
    for kind in ("prior", "loop_lt", "loop_adj"):
        for i, label in enumerate(SUBSET):
            S.append(state(f"{kind}/{label}", kind, label, axes[(i + 1) % 3] if kind != "prior" else "generic", lever="zero" if kind != "prior" else "small"))
    # the losses on the loop (2, 0); at theta = 0 the residual is the 10 m translation
    for loss in ("huber_below", "huber_above", "huber_far", "cauchy", "gm"):
        for label in SUBSET:
            S.append(state(f"{loss}/{label}", "loop_gt", label, "tiny" if label == "2.0" else "generic", u=(6.0, -8.0, 0.0) if label == "0" else (0.0, 0.0, 0.0),
                           lever="zero", loss=loss))
    # the inputs: every quaternion handed in negated, or 9e-7 long or short of unit norm; only set_poses' negated; only prev's negated; each next to its plain
    # twin.  The second append goes through a `prev` that is not the pose the graph holds for node 0.
    for label in SUBSET:
        S.append(state(f"inputs/{label}", "loop_gt", label, "generic", family="X", u=(0.25, 0.5, -1.0), use_prev=True))
        for variant in VARIANTS:
            S.append(state(f"inputs/{label}/{variant}", "loop_gt", label, "generic", family="X", u=(0.25, 0.5, -1.0), use_prev=True, variant=variant))
    # translations: d = 0 exactly, |d| about 30 m at coordinates near 1e3 m, residuals of 1e-9 m and 10 m (0 m is everywhere above)
    for label in SUBSET:
        S.append(state(f"lever_zero/{label}", "chain", label, "generic", lever="zero"))
        S.append(state(f"lever_large/{label}", "chain", label, "tiny", lever="large"))
        S.append(state(f"lever_large_10m/{label}", "loop_lt", label, "generic", lever="large", u=(-6.0, 0.0, 8.0)))
        S.append(state(f"residual_1e-9/{label}", "chain", label, "generic", family="X", u=(6e-10, 0.0, -8e-10)))
        S.append(state(f"residual_10m/{label}", "chain", label, "generic", u=(0.0, 8.0, 6.0)))
    # unit variances
    for label in SUBSET:
        S.append(state(f"unit_var/chain/{label}", "chain", label, "generic", variances="unit"))
        S.append(state(f"unit_var/loop/{label}", "loop_gt", label, "generic", variances="unit", lever="zero"))
    return S


_states = []


def states():
    if not _states:
        _states.extend(_build())
    return _states


ARRAYS = ("cost", "gradient", "diag", "sub", "loop", "d2", "w")
_reference = {}


def model_outputs(st):
    g = model_graph(st)
    cost, grad, D, S, LB = g.evaluate()
    d2, w = g.loop_status()
    return dict(cost=cost, gradient=grad, diag=D, sub=S, loop=LB, d2=d2, w=w)


def ratio(value, ref, A):
    """max over entries of |value - ref| / A; an entry whose A is 0 must equal the referee's exactly (inf otherwise)"""
    value, ref, A = np.atleast_1d(np.asarray(value, np.float64)), np.atleast_1d(np.asarray(ref, np.float64)), np.atleast_1d(np.asarray(A, np.float64))
    if value.size == 0:
        return 0.0
    err = np.abs(value - ref)
    return float(np.max(np.where(A > 0, err / np.where(A > 0, A, 1.0), np.where(err > 0, np.inf, 0.0))))


def reference(st):
    """the referee's outputs of a state and D, computed once: (ref dict, D dict per array): D = the f64 model's largest |model - referee| / A"""
    if st["name"] not in _reference:
        ref = R.evaluate(referee_graph(st))
        mod = model_outputs(st)
        _reference[st["name"]] = (ref, {k: ratio(mod[k], ref[k], ref["A_" + k]) for k in ARRAYS})
    return _reference[st["name"]]


def cap(st):
    """the cap on D: 64 eps up to 3.0 rad, eps / delta at pi -/+ delta"""
    _, side, v = st["theta"]
    return 64.0 * EPS if side == "plain" else EPS / float(v)


# ---- one Gauss-Newton step at large retractions ------------------------------------------------------------------------
STEP_ROTATIONS = ("1e-9", "1e-3", "0.5", "2.0", "3.0")


def _generic_chain(n, seed):
    rng = np.random.default_rng(seed)
    G = np.zeros((n, 7))
    G[:, 0:3] = rng.uniform(-3.0, 3.0, (n, 3))
    G[:, 3:7] = M.qnormalize(rng.normal(0, 1, (n, 4)))
    return G


def _exact_chain(n):
    G = np.zeros((n, 7))
    G[:, 0:3], G[:, 3:7] = X_SMALL[:n], UNITS[:n]
    return G


def chain_step_cases():
    """Chains whose estimates are the given poses retracted by a rotation and a translation.  moved 1: the last node; the linear system's solution is then the
    node's own -e, and q Exp(-e), p - R R_e^T e_v IS the given pose: one Gauss-Newton step is exact ("exact": judged against the given poses).  moved 2: the last
    two nodes; the factor between them has its FIRST node turned, and R_Z^T [d]x omega is only the first order of (Exp(omega) - I) d, so the step is not
    exact: judged against the referee's own mp iteration, and at 3.0 rad with 10 m on three nodes that step more than doubles the
    cost ("rejected").  Rotations up to 1e-3 rad sit in the exact frames of the states above, where a 1e-9 rad residual keeps its digits."""
    cs = []
    for n in (2, 3):
        for ri, rot in enumerate(STEP_ROTATIONS):
            for trans in (0.0, 10.0):
                for moved in (1, 2):
                    G = _exact_chain(n) if float(rot) <= 1e-3 else _generic_chain(n, 500 + 10 * n + ri)
                    xi = np.zeros((n, 6))
                    for k, node in enumerate(range(n - moved, n)):
                        ax = np.array([[0.36, -0.48, 0.8], [0.6, 0.0, -0.8]][k])
                        xi[node, 0:3] = float(rot) * ax
                        xi[node, 3:6] = trans * np.array([[0.0, 0.6, 0.8], [-0.8, 0.6, 0.0]][k])
                    name = f"chain{n}/rot{rot}/trans{trans:g}/moved{moved}"
                    cs.append(dict(name=name, given=G, estimates=M.retract(G, xi), loops=[], exact=moved == 1,
                                   expect="rejected" if name == "chain3/rot3.0/trans10/moved2" else "accepted"))
    return cs


def loop_step_cases():
    """N = 3 with a loop (2, 0) consistent with the given poses; nodes 1 and 2 are off by up to 0.5 / 2.0 rad: the step is not exact, the cost still falls; and one
    strong loop whose measurement is rotated by 3.1 rad about z as tests/pose_graph_cases.py "cost_increases" has it: the step is rejected"""
    cs = []
    G = _generic_chain(3, 777)
    for rot in (0.5, 2.0):
        xi = np.zeros((3, 6))
        xi[2, 0:3] = rot * np.array([0.36, -0.48, 0.8])
        xi[1, 0:3] = 0.3 * rot * np.array([0.0, 0.6, 0.8])
        xi[2, 3:6] = (0.5, -0.25, 1.0)
        cs.append(dict(name=f"loop3/rot{rot:g}", given=G, estimates=M.retract(G, xi), loops=[(2, 0, M.between(G[2], G[0]), np.full(6, 0.1))], exact=False,
                       expect="accepted"))
    G = _generic_chain(3, 2)
    m = M.between(G[2], G[0])
    m[3:7] = M.qnormalize(M.qmul(m[3:7], np.array([np.cos(0.5 * 3.1), 0.0, 0.0, np.sin(0.5 * 3.1)])))
    cs.append(dict(name="loop3/rejected", given=G, estimates=G.copy(), loops=[(2, 0, m, np.full(6, 1e-6))], exact=False, expect="rejected"))
    return cs


def step_referee_graph(c):
    return R.Graph(c["given"], c["estimates"], [(a, b, m, v, RM.NONE, 1.0) for a, b, m, v in c["loops"]], M.PRIOR_VAR, M.ODOM_VAR)


def step_model_graph(c):
    g = M.Graph()
    g.append(None, c["given"])
    for a, b, m, v in c["loops"]:
        g.add_loop(a, b, m, v)
    g.X = M.normalize_poses(c["estimates"])
    return g


_step_reference = {}


def step_reference(c):
    """(the referee's mp iteration, the model's one iteration (X, summary), D1 = (position, angle): the model's miss of the truth — the given poses where the step is exact, else the referee's candidate), computed once"""
    if c["name"] not in _step_reference:
        ref = R.gauss_newton_step(step_referee_graph(c))
        g = step_model_graph(c)
        X, s = M.gauss_newton(g, solver="dense", max_iterations=1, function_tolerance=0.0, gradient_tolerance=0.0, parameter_tolerance=0.0)
        truth = M.normalize_poses(c["given"]) if c["exact"] else ref["poses"]
        _step_reference[c["name"]] = (ref, g, X, s, M.pose_difference(X, truth))
    return _step_reference[c["name"]]
