"""The referee of the local pose graph (tests/local_graph_model.py) and the cases it is run on (tests/local_graph_cases.py), without a GPU:
  * the model's analytic Jacobians against central differences of its own residuals, on every solve case and on hard states;
  * its final cost against scipy.optimize.least_squares run to convergence on the same residuals;
  * the stability of the decision sequence of EVERY committed case (no decision within rounding of a threshold), from the model alone;
  * each family's log shows the branches it is there for;
  * the model's walk on its designed inputs (index bookkeeping, the refusals' conditions);
  * FrameTrajectory against a hand-written sequence.
"""
import numpy as np
import pytest

from tests import local_graph_cases as Cs
from tests import local_graph_model as M

CASES = Cs.solve_cases()
IDS = [c["name"] for c in CASES]


def _solve(c):
    if "result" not in c:
        ch = M.Chain(c["left"], c["right"], c["meas"])
        c["result"] = (ch,) + M.dogleg(ch, c["x0"], **c["options"])
    return c["result"]


def _numeric_jacobian(ch, x, h=1e-6):
    N = 6 * ch.n
    J = np.zeros((6 * (ch.n + 1), N))
    for i in range(N):
        d = np.zeros(N)
        d[i] = h
        J[:, i] = (ch.residuals(ch.plus(x, d)) - ch.residuals(ch.plus(x, -d))) / (2.0 * h)
    return J


@pytest.mark.parametrize("c", [c for c in CASES if c["n"]], ids=[c["name"] for c in CASES if c["n"]])
def test_analytic_jacobians_match_central_differences(c):
    """central differences with h = 1e-6 on residuals of size O(1) carry a truncation error ~h^2 and a rounding error ~eps / h: 1e-8 relative is an order above both"""
    ch = M.Chain(c["left"], c["right"], c["meas"])
    for x in [c["x0"]] + Cs.hard_states(c):
        J = ch.evaluate(x)[2]
        Jn = _numeric_jacobian(ch, x)
        err = np.abs(J - Jn).max() / np.abs(Jn).max()
        print(f"{c['name']}: |J - J_numeric| / |J| = {err:.2e}")
        assert err <= 1e-8
        off = np.abs(J.T @ J)
        for i in range(6 * ch.n):
            for j in range(6 * ch.n):
                if abs(i // 6 - j // 6) > 1:
                    assert off[i, j] == 0.0


@pytest.mark.parametrize("c", CASES, ids=IDS)
def test_final_cost_against_converged_least_squares(c):
    """scipy's trust-region solver from the model's final point, in the local coordinates around it, to machine tolerances: the converged cost of the basin the
    model ended in.  The model never ends below it (1e-12 relative for the rounding of the two cost sums) and ends below where it started; the excess is what the
    1e-6 function tolerance (or the iteration limit) leaves — printed, recorded in DESIGN.md §7j, not bounded."""
    from scipy.optimize import least_squares
    ch, x, info, log = _solve(c)
    if c["n"] == 0:
        assert info["cost"] == info["initial_cost"] and info["iterations"] == 0
        return
    res = least_squares(lambda d: ch.residuals(ch.plus(x, d)), np.zeros(6 * ch.n), method="trf", xtol=1e-15, ftol=1e-15, gtol=1e-15, max_nfev=2000)
    converged = float(res.cost)
    excess = (info["cost"] - converged) / max(converged, 1e-300)
    print(f"{c['name']}: initial {info['initial_cost']:.9g} final {info['cost']:.12g} converged {converged:.12g} excess {excess:.3e} ({info['termination']}, {info['iterations']} iterations)")
    assert info["cost"] >= converged * (1.0 - 1e-12) - 1e-300
    if c["name"] != "e":
        assert info["cost"] < info["initial_cost"]


@pytest.mark.parametrize("c", CASES, ids=IDS)
def test_decision_sequence_is_stable(c):
    """no candidate of any committed case decides within rounding of a threshold: rho against min_relative_decrease (factor two) and the radius thresholds 0.25 /
    0.75 (1 %), the two norms that choose the dogleg case against the radius (1e-6 relative), the cost change against the function tolerance and the step
    against the parameter tolerance (10 %)"""
    ch, x, info, log = _solve(c)
    for e in log:
        assert not (0.5e-3 <= e["rho"] <= 2e-3), e
        assert abs(e["rho"] - 0.25) > 0.0025 and abs(e["rho"] - 0.75) > 0.0075, e
        assert abs(e["gn_norm"] - e["radius"]) > 1e-6 * e["radius"] and abs(e["cauchy_norm"] - e["radius"]) > 1e-6 * e["radius"], e
        assert not (0.9e-6 <= abs(e["cost"] - e["new_cost"]) / e["cost"] <= 1.1e-6), e
        assert not (0.9 <= e["step"] / (1e-8 * (e["xnorm"] + 1e-8)) <= 1.1), e
    assert info["termination"] in ("function_tolerance", "max_iterations", "gradient_tolerance"), info


def test_families_reach_their_branches():
    by = {c["name"]: _solve(c) for c in CASES}
    for name in ("a1", "a2", "g"):      # three iterations, all Gauss-Newton steps, the last candidate triggers the function tolerance and is not taken
        _, _, info, log = by[name]
        assert info["termination"] == "function_tolerance" and info["iterations"] == 3 and info["successful_steps"] == 2
        assert [e["case"] for e in log] == [1, 1, 1] and [e["accepted"] for e in log] == [True, True, False] and not any(e["reused"] for e in log)
    _, _, info, log = by["b"]           # scaled gradient three times with the radius tripling, then Gauss-Newton steps
    assert [e["case"] for e in log[:4]] == [2, 2, 2, 1] and all(e["case"] == 1 for e in log[3:])
    assert np.allclose([e["radius"] for e in log[:4]], [0.1, 0.3, 0.9, 2.7], rtol=1e-12, atol=0.0)      # 3 |step|, |step| = the radius to rounding
    assert info["termination"] == "function_tolerance" and not log[-1]["accepted"] and all(e["accepted"] for e in log[:-1])
    _, _, info, log = by["c"]           # scaled gradient, then interpolated; one rejected step whose successor reuses the subproblem; a rho < 0.25 halving; the iteration limit
    cases = [e["case"] for e in log]
    assert cases[0] == 2 and 3 in cases and cases.index(3) > 0
    rejected = [i for i, e in enumerate(log) if not e["accepted"]]
    assert len(rejected) == 1 and log[rejected[0] + 1]["reused"] and log[rejected[0] + 1]["radius"] == 0.5 * log[rejected[0]]["radius"]
    halved = [i for i, e in enumerate(log[:-1]) if e["accepted"] and e["rho"] < 0.25]
    assert halved and all(log[i + 1]["radius"] == 0.5 * log[i]["radius"] for i in halved)
    assert info["termination"] == "max_iterations" and info["iterations"] == 15
    _, _, info, log = by["d"]           # at least six rejected Gauss-Newton steps in a row from ONE linearisation, then the interpolated step, more rejections, the iteration limit
    k = 0
    while log[k]["case"] == 1 and not log[k]["accepted"]:
        k += 1
    assert k >= 6 and all(e["reused"] for e in log[1:k + 1]) and not log[0]["reused"] and log[k]["case"] == 3
    assert len({(e["gn_norm"], e["cauchy_norm"], e["cost"]) for e in log[:k + 1]}) == 1
    assert sum(1 for e in log[k:] if not e["accepted"]) >= 1
    assert info["termination"] == "max_iterations" and info["iterations"] == 15
    _, _, info, log = by["e"]           # the state at the truth of exact measurements: the gradient tolerance ends the first iteration
    assert info["termination"] == "gradient_tolerance" and info["iterations"] == 1 and not log
    _, _, info, log = by["f"]
    assert info["iterations"] == 0 and not log
    assert by["g"][0].n == M.MAX_FRAMES == Cs.MAX_FRAMES


WALKS = Cs.walk_cases()


@pytest.mark.parametrize("c", WALKS, ids=[c["name"] for c in WALKS])
def test_walk_model_on_its_cases(c):
    rng = M.walk_indices(c["stamps"], c["ii0"], c["T"])
    assert rng is not None and rng[0] == c["ii0"]
    poses, (P, R, V), meas = M.walk(**Cs.walk_kwargs(c))
    n = c["n"]
    assert poses.shape == (n, 7) and meas.shape == (n + 1, 7) and np.isfinite(poses).all() and np.isfinite(meas).all() and np.isfinite(R).all()
    if c["name"] == "empty_interval":
        st, T = c["stamps"], c["T"]
        assert any(not ((st >= T[f - 1]) & (st < T[f])).any() for f in range(1, n + 2))
    if c["name"] == "sample_at_scan_stamp":
        assert sum(1 for t in c["T"] if (c["stamps"] == t).any()) >= 3
    if c["name"] == "clamps":
        assert (np.abs(c["acc"]) > 18.0).sum() >= 18
    if c["name"] == "2khz_n3":
        assert rng[1] - rng[0] + 1 > 256
    if c["name"] == "f32_positions":
        assert (poses[:, 0:3] == poses[:, 0:3].astype(np.float32).astype(np.float64)).all()


def test_walk_clamp_quirk_shows():
    """the opening interpolation of a frame's interval is NOT clamped, that of the closing interval is: with the clamp applied everywhere the walk's result changes"""
    c = next(w for w in WALKS if w["name"] == "clamps")
    ref = M.walk(**Cs.walk_kwargs(c))
    kw = Cs.walk_kwargs(c)
    kw["acc"] = np.clip(c["acc"], [-15.0, -15.0, -18.0], [15.0, 15.0, 18.0])      # clamping every sample first = clamping the opening interpolation too
    other = M.walk(**kw)
    assert np.abs(ref[0] - other[0]).max() > 1e-9


def test_walk_refusal_conditions():
    c = WALKS[0]
    st = c["stamps"]
    assert M.walk_indices(st[:10], c["ii0"], c["T"]) is None                                     # the buffer ends inside the walk
    last = int(np.searchsorted(st, c["T"][-1]))
    assert M.walk_indices(st[:last], c["ii0"], c["T"]) is None and M.walk_indices(st[:last + 1], c["ii0"], c["T"]) is not None      # imu_buf[ii] at the closing step
    assert M.walk_indices(st, -1, c["T"]) is None
    dup = st.copy()
    dup[c["ii0"] + 1] = dup[c["ii0"]] = c["T"][0]                                                # dt1 + dt2 == 0 at the opening interpolation
    assert M.walk_indices(dup, c["ii0"], c["T"]) is None


def test_frame_trajectory_bookkeeping():
    from lili_om_amd import FrameTrajectory
    pose = lambda i: np.array([float(i), 0.0, 0.0, 1.0, 0.0, 0.0, 0.0])      # noqa: E731
    tr = FrameTrajectory()
    with pytest.raises(ValueError):
        tr.append(np.zeros((0, 7)), pose(1))
    tr.start(pose(0))
    assert len(tr) == 1 and tr.keyframe_id_in_frame == [0]
    assert tr.append([pose(1), pose(2)], pose(3)) == 3           # two scans, then the keyframe
    assert tr.append(np.zeros((0, 7)), pose(4)) == 4             # two keyframes in a row
    assert tr.append([pose(5)], pose(6)) == 6
    assert tr.keyframe_id_in_frame == [0, 3, 4, 6] and len(tr) == 7
    assert (tr.poses[:, 0] == np.arange(7.0)).all()
    assert (tr.keyframes()[:, 0] == [0.0, 3.0, 4.0, 6.0]).all() and tr.last_keyframe()[0] == 6.0
    tr.rewrite(tr.poses + 1.0)
    assert (tr.poses[:, 0] == np.arange(7.0) + 1.0).all() and tr.keyframe_id_in_frame == [0, 3, 4, 6]
    with pytest.raises(Exception):
        tr.rewrite(np.zeros((3, 7)))
    with pytest.raises(ValueError):
        tr.start(pose(0))
    with pytest.raises(ValueError):
        tr.append(np.zeros((17, 7)), pose(9))
