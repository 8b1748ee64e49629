"""The joint keyframe window on the device (lili_window_evaluate / lili_window_solve, lili_om_amd.WindowSolver) against the repository's referee:
oracle/lo_window.py (Problem, imu_factor, speed_bias_prior, Marginalization, ceres_lm) on the synthetic window of tests/window_harness.py, the lidar
rows of the oracle exactly as tests/test_window_gpu.py builds them (same association, CauchyLoss(1) + corrector per residual).

Bounds.  Lidar-only evaluation: 1e-12 relative to the largest entry, the bound the project holds its Grams to; gradient and J^T J are
the two parts of one Gram, so both are measured against the largest entry of the two.  With IMU factors and priors the rows are whitened by sqrt_info
(entries 1e2 .. 1e5): the difference to the oracle was measured on the GPU (figures in DESIGN.md §7h and at EVAL_BOUND below) and is asserted at 100 x
the measured value, never above the 1e-8 ceiling.  Solves: Ceres' decisions (iterations, successful steps, accept / reject sequence, termination) equal
the oracle's, final cost within 1e-6 relative, every keyframe within 1e-4 m / 1e-4 rad / 1e-4 in speed-bias (the bounds of tests/test_window_gpu.py).
Every solve first checks ON THE ORACLE ALONE that the decision sequence is not a coin toss under rounding (_stable)."""
import numpy as np
import pytest

import lili_om_amd as L
from lili_om_amd import synth
from oracle import lo_window as W
from tests import window_harness as H

pytestmark = pytest.mark.gpu

MASK = L.MASK_SURF | L.MASK_EDGE
# Evaluation with IMU factors / priors, relative to the largest entry — measured on an MI355X: 1.07e-15 at worst (IMU + speed-bias priors alone, perturbed
# state 1, J^T J; with the marginalisation prior 4.7e-16, n_kf = 2 / 4: 3.3e-16 / 4.5e-16; cost and gradient below that everywhere).  Asserted at 100 x the
# measured value; the ceiling the issue sets is 1e-8.
EVAL_BOUND = min(100 * 1.07e-15, 1e-8)
# Solves, measured against the oracle's end state: speed-bias branch d_cost 2.4e-16, 1.2e-16 m, 1.3e-18 rad, speed-bias 2.6e-16; marginalisation branch 1.2e-16,
# 2.2e-16 m, 1.3e-18 rad, 2.2e-16; n_kf = 2: 0, 5.6e-17 m, 4.9e-19 rad, 5.4e-16; n_kf = 4: 1.8e-16, 1.6e-16 m, 5.6e-17 rad, 2.2e-16 (bounds: 1e-6, 1e-4, 1e-4, 1e-4).
# Joint against lidar-only: the solutions lie 9.1e-3 m apart, IMU residual norm 1.16 against 19.4.


def _angle(qa, qb):
    d = W.qmul(W.qinv(qa), qb)
    return 2.0 * np.arctan2(np.linalg.norm(d[1:]), abs(d[0]))


def make_window_n(n_kf, seed=41, n_surf=2500, n_edge=200):
    """H.make_window's loop for n_kf keyframes (H.N_KF is a module constant): same room, same generator, same draws in the same order per keyframe —
    for n_kf = 3 it is H.make_window."""
    room = synth.make_room(seed=seed, n_query=10, n_edge_query=10)
    rng = np.random.default_rng(seed + 1)
    P = L.make_params("livox")
    ba, bg = np.array([0.02, -0.01, 0.015]), np.array([0.002, -0.001, 0.0015])
    kfs = []
    for k in range(n_kf):
        p, q, v, _, _ = H.trajectory(k * H.DT_KF)
        Q2, T2 = L.api.assoc_transform(p, q, P)
        pick = rng.choice(room["map_xyz"].shape[0], n_surf, replace=True)
        qw = room["map_xyz"][pick].astype(np.float64) + rng.normal(0, 0.01, (n_surf, 3)) + rng.uniform(-0.15, 0.15, (n_surf, 3))
        epick = rng.choice(room["edge_map_xyz"].shape[0], n_edge, replace=True)
        ew = room["edge_map_xyz"][epick].astype(np.float64) + rng.normal(0, 0.02, (n_edge, 3))
        Qi = W.qinv(Q2)
        q_local = np.array([W.qrot(Qi, x - T2) for x in qw], np.float32)
        e_local = np.array([W.qrot(Qi, x - T2) for x in ew], np.float32)
        q_refl = (np.float32(10.0) + rng.integers(0, 30, n_surf).astype(np.float32) * np.float32(0.1) + np.float32(0.05))
        kfs.append(dict(t_true=p, q_true=q, sb_true=np.concatenate([v, ba, bg]), q_xyz=q_local, q_refl=q_refl, eq_xyz=e_local))
    pres = []
    for k in range(n_kf - 1):
        s = H.imu_between(k * H.DT_KF, (k + 1) * H.DT_KF, ba, bg)
        pre = W.Preintegration(s[0][1], s[0][2], ba + 0.003, bg - 0.0004)
        for dt, acc, gyr in s[1:]:
            pre.push_back(dt, acc, gyr)
        pres.append(dict(pre=pre, samples=s, ba=ba + 0.003, bg=bg - 0.0004))
    init = []
    for k, kf in enumerate(kfs):
        t0, q0 = synth.perturbed_pose(kf["t_true"], kf["q_true"], np.random.default_rng(seed + 10 + k), 0.04, 0.4)
        init.append(dict(t=np.asarray(t0, np.float64), q=np.asarray(q0, np.float64), sb=kf["sb_true"] + np.concatenate([rng.normal(0, 0.05, 3), rng.normal(0, 0.004, 3), rng.normal(0, 0.0005, 3)])))
    return dict(room=room, P=P, kfs=kfs, pres=pres, init=init)


def cut(win, k0, k1):
    """keyframes k0 .. k1 - 1 of a window as a window of their own"""
    return dict(room=win["room"], P=win["P"], kfs=win["kfs"][k0:k1], pres=win["pres"][k0:k1 - 1], init=[dict(s) for s in win["init"][k0:k1]])


def build_problem(win, lidar_block, sb_priors=True, marg=None, imu=True):
    """H.build_problem for any number of keyframes; marg = (Marginalization, names of its kept blocks) instead of the speed-bias priors."""
    n = len(win["kfs"])
    pb = W.Problem()
    for k, s in enumerate(win["init"]):
        pb.add_parameter(f"t{k}", s["t"])
        pb.add_parameter(f"q{k}", s["q"], quat=True)
        pb.add_parameter(f"sb{k}", s["sb"])
    if marg is not None:
        pb.add_residual(marg[0].factor(), marg[1])
    elif sb_priors:
        for k in range(n - 1):
            prior = win["init"][k]["sb"].copy()
            pb.add_residual(lambda sb, prior=prior: W.speed_bias_prior(prior, sb), [f"sb{k}"])
    if imu:
        for k in range(n - 1):
            pre = win["pres"][k]["pre"]
            pb.add_residual(lambda ti, qi, sbi, tj, qj, sbj, pre=pre: W.imu_factor(pre, ti, qi, sbi, tj, qj, sbj),
                            [f"t{k}", f"q{k}", f"sb{k}", f"t{k + 1}", f"q{k + 1}", f"sb{k + 1}"])
    if lidar_block is not None:
        for k in range(n):
            pb.add_residual(lidar_block(k), [f"t{k}", f"q{k}"])
    return pb


def oracle_side(oracle, win):
    """the association of every keyframe at its initial pose on the CPU and the lidar block of tests/test_window_gpu.py::oracle_block"""
    room, P = win["room"], win["P"]
    PO = oracle.params("livox", loss=0)
    tree_s, tree_e = oracle.KdTree(room["map_xyz"]), oracle.KdTree(room["edge_map_xyz"])
    recs = []
    for k, kf in enumerate(win["kfs"]):
        Q2, T2 = L.api.assoc_transform(win["init"][k]["t"], win["init"][k]["q"], P)
        recs.append((oracle.associate_surf(tree_s, room["map_refl"], kf["q_xyz"], kf["q_refl"], Q2, T2, PO), oracle.associate_edge(tree_e, kf["eq_xyz"], Q2, T2, PO)))

    def oracle_block(k):
        def fn(t, q):
            rows = np.concatenate([oracle.linearize_rows(recs[k][0], t, q, PO, kind="surf"), oracle.linearize_rows(recs[k][1], t, q, PO, kind="edge")])
            J, r, cost = H.robust_rows(rows)
            return r, [J[:, :3], J[:, 3:7]], cost
        return fn
    return recs, oracle_block


def gpu_side(gpu_ctx, win, recs=None):
    """one matcher slot per keyframe, correspondences found ONCE at the initial window"""
    room, P = win["room"], win["P"]
    n = len(win["kfs"])
    m = L.ScanToMapMatcher(gpu_ctx, P)
    m.set_input_cloud(L.KIND_SURF, np.c_[room["map_xyz"], room["map_refl"]])
    m.set_input_cloud(L.KIND_EDGE, room["edge_map_xyz"])
    assoc = []
    for k, kf in enumerate(win["kfs"]):
        m.set_queries(k, L.KIND_SURF, np.c_[kf["q_xyz"], kf["q_refl"]])
        m.set_queries(k, L.KIND_EDGE, kf["eq_xyz"])
        m.pose_set(k, win["init"][k]["t"], win["init"][k]["q"])
        assoc.append(L.api.assoc_transform(win["init"][k]["t"], win["init"][k]["q"], P))
    n_gpu = m.associate_window(list(range(n)), [a[1] for a in assoc], [a[0] for a in assoc], MASK)
    if recs is not None:
        for k in range(n):
            assert (recs[k][0]["count"], recs[k][1]["count"]) == n_gpu[k] and n_gpu[k][0] > 1500 and n_gpu[k][1] > 50
    return m


def state_of(win_or_sol, n):
    if "init" in win_or_sol:
        return np.array([np.concatenate([s["t"], s["q"], s["sb"]]) for s in win_or_sol["init"]])
    return np.array([np.concatenate([win_or_sol[f"t{k}"], win_or_sol[f"q{k}"], win_or_sol[f"sb{k}"]]) for k in range(n)])


def values_of(state):
    v = {}
    for k, s in enumerate(np.asarray(state)):
        v[f"t{k}"], v[f"q{k}"], v[f"sb{k}"] = s[0:3].copy(), s[3:7].copy(), s[7:16].copy()
    return v


def perturbed(state, seed, negate_q=None, scale=1):
    """every sigma times `scale`; the draws and their order do not depend on it"""
    rng = np.random.default_rng(seed)
    s = np.array(state, np.float64)
    for k in range(s.shape[0]):
        s[k, 0:3] += rng.normal(0, 0.02 * scale, 3)
        s[k, 3:7] = W.quat_plus(s[k, 3:7], rng.normal(0, 0.004 * scale, 3))
        s[k, 7:16] += np.concatenate([rng.normal(0, 0.03 * scale, 3), rng.normal(0, 0.002 * scale, 3), rng.normal(0, 0.0003 * scale, 3)])
    if negate_q is not None:
        s[negate_q, 3:7] = -s[negate_q, 3:7]
    return s


def compare_evaluation(ws, pb, state, bound, what):
    cost, r, J = pb.evaluate(values_of(state))
    g_o, H_o = J.T @ r, J.T @ J
    c, g, Hm = ws.evaluate(state)
    scale = max(np.abs(H_o).max(), np.abs(g_o).max())
    dc, dg, dh = abs(c - cost) / abs(cost), np.abs(g - g_o).max() / scale, np.abs(Hm - H_o).max() / scale
    print(f"evaluate [{what}]: cost {cost:.9g}  d_cost {dc:.3e}  d_gradient {dg:.3e}  d_JtJ {dh:.3e}  (relative to the largest entry {scale:.3e})")
    assert np.abs(Hm - Hm.T).max() <= 1e-13 * scale
    assert dc <= bound and dg <= bound and dh <= bound, (what, dc, dg, dh)
    return max(dc, dg, dh)


def _stable(log, info):
    """Condition on the input, from the oracle alone: no candidate's rho within a factor of two of min_relative_decrease (1e-3), no candidate within 10 % of
    the function or the parameter tolerance — otherwise the decision sequence would depend on rounding."""
    for e in log:
        assert not (0.5e-3 <= e["rho"] <= 2e-3), e
        assert not (0.9e-6 <= abs(e["cost"] - e["new_cost"]) / e["cost"] <= 1.1e-6), e
        assert e["step"] > 1e-6, e          # parameter tolerance 1e-8 (|x| + 1e-8): nowhere near
    assert info["termination"] in ("function_tolerance", "max_iterations"), info


def compare_solve(ws, pb, state0, n, what):
    log_o = []
    sol_o, info_o = W.ceres_lm(pb, max_num_iterations=15, log=log_o)
    _stable(log_o, info_o)
    final, info = ws.solve(state0)
    log = info["log"]
    print(f"solve [{what}]: oracle {info_o}  device iterations {info['iterations']} successful {info['successful_steps']} {info['termination']} cost {info['final_cost']:.12g}")
    assert info["termination"] == info_o["termination"]
    assert info["iterations"] == info_o["iterations"] and info["successful_steps"] == info_o["successful_steps"]
    assert len(log) == len(log_o)
    accepts_o = [e["rho"] > 1e-3 for e in log_o]
    if info_o["termination"] == "function_tolerance":
        accepts_o[-1] = False             # the candidate that triggers the tolerance is not taken
    assert [e["accepted"] for e in log] == accepts_o
    for a, b in zip(log, log_o):
        assert (a["rho"] > 1e-3) == (b["rho"] > 1e-3) and a["radius"] == b["radius"]
    d_cost = abs(info["final_cost"] - info_o["cost"]) / info_o["cost"]
    dts, das, dsb = [], [], []
    for k in range(n):
        dts.append(np.linalg.norm(final[k, 0:3] - sol_o[f"t{k}"]))
        das.append(_angle(final[k, 3:7], sol_o[f"q{k}"]))
        dsb.append(np.abs(final[k, 7:16] - sol_o[f"sb{k}"]).max())
    print(f"solve [{what}]: d_cost {d_cost:.3e}  d_t {max(dts):.3e} m  d_angle {max(das):.3e} rad  d_speed_bias {max(dsb):.3e}")
    assert d_cost <= 1e-6
    assert max(dts) < 1e-4 and max(das) < 1e-4 and max(dsb) < 1e-4
    return final, info, sol_o, max(dts)


def window_problem(ws, win, n, sb_priors=True, imu=True, mask=MASK, prior=None):
    sb = None
    if sb_priors:
        sb = np.full((n, 9), np.nan)
        for k in range(n - 1):
            sb[k] = win["init"][k]["sb"]
    ws.set_problem(list(range(n)), mask, imu=[p["pre"] for p in win["pres"]] if imu else None, sb_prior=sb, prior=prior, n_kf=n)
    return ws


@pytest.fixture(scope="module")
def win3():
    return H.make_window(n_surf=2500, n_edge=200)


@pytest.fixture(scope="module")
def win4():
    return make_window_n(4)


def test_local_generator_is_the_harness(win3, win4):
    for a, b in zip(win3["kfs"], win4["kfs"][:3]):
        assert np.array_equal(a["q_xyz"], b["q_xyz"]) and np.array_equal(a["eq_xyz"], b["eq_xyz"])


def test_evaluate_against_the_oracle(gpu_ctx, oracle, win3):
    recs, oracle_block = oracle_side(oracle, win3)
    m = gpu_side(gpu_ctx, win3, recs)
    ws = L.WindowSolver(gpu_ctx, m)
    s0 = state_of(win3, 3)
    states = [("initial", s0), ("perturbed 1", perturbed(s0, 5)), ("perturbed 2", perturbed(s0, 6))]
    before = [m.pose_get(k) for k in range(3)]
    # the lidar part alone: the Gram bound
    window_problem(ws, win3, 3, sb_priors=False, imu=False)
    pb = build_problem(win3, oracle_block, sb_priors=False, imu=False)
    for name, s in states:
        compare_evaluation(ws, pb, s, 1e-12, "lidar only, " + name)
    # IMU factors and speed-bias priors alone (mask 0): a lidar-sized cost cannot hide them
    window_problem(ws, win3, 3, mask=0)
    pb = build_problem(win3, None)
    worst = 0.0
    for name, s in states:
        worst = max(worst, compare_evaluation(ws, pb, s, EVAL_BOUND, "IMU + speed-bias priors alone, " + name))
    # the whole problem
    window_problem(ws, win3, 3)
    pb = build_problem(win3, oracle_block)
    for name, s in states:
        worst = max(worst, compare_evaluation(ws, pb, s, EVAL_BOUND, "joint, " + name))
    print(f"evaluate: worst difference with IMU / priors {worst:.3e}")
    after = [m.pose_get(k) for k in range(3)]
    for a, b in zip(before, after):
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def test_solve_speed_bias_prior_branch(gpu_ctx, oracle, win3):
    recs, oracle_block = oracle_side(oracle, win3)
    m = gpu_side(gpu_ctx, win3, recs)
    ws = window_problem(L.WindowSolver(gpu_ctx, m), win3, 3)
    s0 = state_of(win3, 3)
    final, info, sol_o, d_t = compare_solve(ws, H.build_problem(win3, oracle_block), s0, 3, "speed-bias priors, n_kf = 3")
    # ---- state hand-over: the slots hold the final (t, q) bit for bit, and a linearisation there is evaluate's lidar part
    for k in range(3):
        t, q, st = m.pose_get(k)
        assert st == 0 and t.tobytes() == final[k, 0:3].tobytes() and q.tobytes() == final[k, 3:7].tobytes()
    assert ws.last_state().tobytes() == final.tobytes()
    recs_g = m.linearize_window([0, 1, 2], [m.pose_get(k)[0] for k in range(3)], [m.pose_get(k)[1] for k in range(3)], MASK)
    Hl, gl, cl = np.zeros((45, 45)), np.zeros(45), 0.0
    for k, (G, cost, counts) in enumerate(recs_g):
        Pk = np.zeros((7, 6)); Pk[:3, :3] = np.eye(3); Pk[3:, 3:] = W.plus_jacobian(final[k, 3:7])
        Hl[15 * k:15 * k + 6, 15 * k:15 * k + 6] = Pk.T @ G[:7, :7] @ Pk
        gl[15 * k:15 * k + 6] = Pk.T @ G[:7, 7]
        cl += cost
    window_problem(ws, win3, 3, sb_priors=False, imu=False)
    c, g, Hm = ws.evaluate(final)
    scale = max(np.abs(Hl).max(), np.abs(gl).max())
    print(f"hand-over: d_cost {abs(c - cl) / cl:.3e} d_gradient {np.abs(g - gl).max() / scale:.3e} d_JtJ {np.abs(Hm - Hl).max() / scale:.3e}")
    assert abs(c - cl) <= 1e-12 * cl and np.abs(g - gl).max() <= 1e-12 * scale and np.abs(Hm - Hl).max() <= 1e-12 * scale
    # ---- it is the joint problem: the lidar-only solves of the same window end elsewhere, and with larger IMU residuals
    for k in range(3):
        m.pose_set(k, win3["init"][k]["t"], win3["init"][k]["q"])
    m.solve_lm_window([0, 1, 2], MASK)
    lidar_only = s0.copy()
    for k in range(3):
        t, q, _ = m.pose_get(k)
        lidar_only[k, 0:3], lidar_only[k, 3:7] = t, q
    gap = max(np.linalg.norm(lidar_only[k, 0:3] - final[k, 0:3]) for k in range(3))

    def imu_norm(s):
        return np.sqrt(sum(float(r @ r) for r in (W.imu_factor(win3["pres"][k]["pre"], s[k, 0:3], s[k, 3:7], s[k, 7:16], s[k + 1, 0:3], s[k + 1, 3:7], s[k + 1, 7:16])[0] for k in range(2))))
    n_joint, n_lidar = imu_norm(final), imu_norm(lidar_only)
    print(f"joint vs lidar-only: translation gap {gap:.3e} m (difference to the oracle {d_t:.3e} m), IMU residual norm {n_joint:.4g} against {n_lidar:.4g}")
    assert gap > 10 * d_t and gap > 1e-3          # ten times the difference to the oracle measured above, and far above the 1e-4 m bound
    assert n_joint < n_lidar


def last3_system(pb, values):
    """J^T J and J^T r of a problem with every quaternion block entering by the LAST THREE of its four global columns (MarginalizationFactor.cpp:9-11)"""
    sizes = pb.local_sizes()
    offs = dict(zip(pb.order, np.concatenate([[0], np.cumsum(sizes)[:-1]]).astype(int)))
    rows, jrows = [], []
    for fn, names, loss in pb.blocks:
        assert loss is None
        out = fn(*[values[n] for n in names])
        r = np.atleast_1d(np.asarray(out[0], np.float64))
        Jd = np.zeros((len(r), int(sum(sizes))))
        for n, J in zip(names, out[1]):
            J = np.asarray(J, np.float64).reshape(len(r), -1)
            if pb.kind[n]:
                J = J[:, 1:4]
            Jd[:, offs[n]:offs[n] + J.shape[1]] += J
        rows.append(r); jrows.append(Jd)
    r, J = np.concatenate(rows), np.vstack(jrows)
    return J.T @ J, J.T @ r


def test_solve_marginalisation_prior_branch(gpu_ctx, oracle, win4):
    # ---- the first window (keyframes 0, 1, 2) at the oracle's solution: its information, keyframe 0 marginalised
    first = cut(win4, 0, 3)
    _, block1 = oracle_side(oracle, first)
    pb1 = build_problem(first, block1)
    sol1, _ = W.ceres_lm(pb1, max_num_iterations=15)
    A, b = last3_system(pb1, sol1)
    kept = [(f"{p}{k}", sol1[f"{p}{k}"], p == "q") for k in (1, 2) for p in ("t", "q", "sb")]
    M = W.Marginalization(A, b, 15, kept)
    # ---- the next window: keyframes 1, 2 (started a few cm off the linearisation point) and a new one
    nxt = cut(win4, 1, 4)
    rng = np.random.default_rng(77)
    for k in (0, 1):
        nxt["init"][k] = dict(t=sol1[f"t{k + 1}"] + rng.normal(0, 0.02, 3), q=W.quat_plus(sol1[f"q{k + 1}"], rng.normal(0, 0.003, 3)),
                              sb=sol1[f"sb{k + 1}"] + np.concatenate([rng.normal(0, 0.02, 3), rng.normal(0, 0.001, 3), rng.normal(0, 0.0002, 3)]))
    recs, block2 = oracle_side(oracle, nxt)
    names = [f"{p}{k}" for k in (0, 1) for p in ("t", "q", "sb")]
    pb2 = build_problem(nxt, block2, marg=(M, names))
    m = gpu_side(gpu_ctx, nxt, recs)
    prior = dict(block_kind=[0, 1, 2, 0, 1, 2], block_keyframe=[0, 0, 0, 1, 1, 1], x0=[v for _, v, _ in M.kept], J0=M.linearized_jacobians, r0=M.linearized_residuals)
    ws = window_problem(L.WindowSolver(gpu_ctx, m), nxt, 3, sb_priors=False, prior=prior)
    s0 = state_of(nxt, 3)
    # evaluation, also where a kept quaternion has w(q0^-1 q) < 0: the sign branch of MarginalizationFactor::Evaluate
    sneg = perturbed(s0, 9, negate_q=1)
    assert W.qmul(W.qinv(M.kept[4][1]), sneg[1, 3:7])[0] < 0
    for name, s in (("initial", s0), ("perturbed, q1 negated", sneg)):
        compare_evaluation(ws, pb2, s, EVAL_BOUND, "marginalisation prior, " + name)
    window_problem(ws, nxt, 3, sb_priors=False, prior=prior, mask=0)
    pb_alone = build_problem(nxt, None, marg=(M, names))
    for name, s in (("initial", s0), ("perturbed, q1 negated", sneg)):
        compare_evaluation(ws, pb_alone, s, EVAL_BOUND, "marginalisation prior + IMU alone, " + name)
    window_problem(ws, nxt, 3, sb_priors=False, prior=prior)
    compare_solve(ws, pb2, s0, 3, "marginalisation prior, n_kf = 3")


@pytest.mark.parametrize("n_kf", [2, 4])
def test_solve_other_window_sizes(gpu_ctx, oracle, win4, n_kf):
    win = cut(win4, 0, n_kf)
    recs, oracle_block = oracle_side(oracle, win)
    m = gpu_side(gpu_ctx, win, recs)
    ws = window_problem(L.WindowSolver(gpu_ctx, m), win, n_kf)
    pb = build_problem(win, oracle_block)
    compare_evaluation(ws, pb, state_of(win, n_kf), EVAL_BOUND, f"joint, n_kf = {n_kf}")
    final, info, _, _ = compare_solve(ws, pb, state_of(win, n_kf), n_kf, f"speed-bias priors, n_kf = {n_kf}")
    for k in range(n_kf):
        t, q, _ = m.pose_get(k)
        assert t.tobytes() == final[k, 0:3].tobytes() and q.tobytes() == final[k, 3:7].tobytes()


def test_refusals_leave_the_poses_alone(gpu_ctx, win3):
    small = dict(win3)
    m = gpu_side(gpu_ctx, small)
    ws = L.WindowSolver(gpu_ctx, m)
    s0 = state_of(win3, 3)
    before = [m.pose_get(k) for k in range(3)]
    pres = [p["pre"] for p in win3["pres"]]

    def refused(what):
        for call in (lambda: ws.solve(np.zeros((ws.problem.n_kf, 16)) + 1.0 if ws.problem.n_kf != 3 else s0), lambda: ws.evaluate(np.zeros((ws.problem.n_kf, 16)) + 1.0 if ws.problem.n_kf != 3 else s0)):
            with pytest.raises(L.LiliError):
                call()
        for k in range(3):
            t, q, _ = m.pose_get(k)
            assert np.array_equal(t, before[k][0]) and np.array_equal(q, before[k][1]), what

    ws.set_problem([0], MASK, n_kf=1)
    refused("n_kf = 1")
    ws.set_problem([0, 1, 2, 3, 4], MASK, n_kf=5)
    refused("n_kf = 5")
    ws.set_problem([0, 1, 7], MASK, imu=pres)          # slot 7 was never associated
    refused("a slot without records")
    bad = L.api.pack_preintegration(pres[1])
    cov = np.array(bad.covariance).reshape(15, 15)
    cov[4, 4] = -cov[4, 4]
    bad.covariance[:] = cov.reshape(-1).tolist()
    ws.set_problem([0, 1, 2], MASK, imu=[L.api.pack_preintegration(pres[0]), bad])
    refused("a covariance that is not positive definite")
    J0 = np.eye(30)
    prior = dict(block_kind=[0, 1, 2, 0, 1, 2], block_keyframe=[0, 0, 0, 1, 1, 1], x0=np.concatenate([s0[0], s0[1]]), J0=J0[:, :29].copy(), r0=np.zeros(30))
    ws.set_problem([0, 1, 2], MASK, imu=pres, prior=prior)
    refused("n_cols of the prior does not match its blocks")
    # and the same objects, put right, are accepted
    prior["J0"] = J0
    ws.set_problem([0, 1, 2], MASK, imu=pres, prior=prior)
    c, g, _ = ws.evaluate(s0)
    assert np.isfinite(c) and np.isfinite(g).all()
