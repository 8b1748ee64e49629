"""lili_window_cycle (WindowSolver.cycle) against the chain of calls it replaces — lili_window_solve, the host's sign unification, lili_window_marginalize — and its
write-back against tests/cycle_model.py.

The cycle runs the chain's kernels on the chain's doubles (same solve launch, the lidar records at the slots' device poses instead of host copies of the same
doubles, win_build<true> and marg_schur on the same system), so everything the chain also produces is compared BYTE for byte: the summary field by field, the solved
state, J0, r0, x0, the block lists, rank and sweep counts of the prior, the slots' poses.  The chain itself has its referees elsewhere (tests/test_window_solve_gpu.py,
tests/test_marg_gpu.py: the oracle); here the oracle is asked only where the issue of the resident hand-over could hide behind the chain — the second cycle's end state
(compare_solve's bounds: 1e-6 relative cost, 1e-4 m, 1e-4 rad, 1e-4 in speed-bias against the oracle's own second solution).
The gates, the unification and next_state are checked against the plain-float model applied to (state_in, the CHAIN's unified state), bytes again.

Measured on an MI355X: every byte comparison below holds; second cycle on the resident prior, distance to the chain's device result 0 in every field
(decisions 14 / 13 / function_tolerance as the chain), distance to the oracle's second solution d_cost 1.2e-16, 2.2e-15 m, 1.2e-17 rad, speed-bias 2.8e-14."""
import ctypes as C
import re

import numpy as np
import pytest

import lili_om_amd as L
from oracle import lo_window as W
from tests import cycle_model as CM
from tests import lm_branch_cases as B
from tests import marg_harness as MH
from tests import test_window_solve_gpu as S

pytestmark = pytest.mark.gpu

MASK = S.MASK
E_ARG, E_STATE = -1, -3


def unify_host(state):
    s = np.array(state, np.float64)
    for k in range(s.shape[0]):
        if s[k, 3] < 0:
            s[k, 3:7] = -s[k, 3:7]
    return s


def marginalize_chain(ws, state):
    """ws.marginalize as the reference's chain calls it: the speed-bias priors the problem carries enter with the post-solve speed-bias as their mean
    (L/src/BackendFusion.cpp:1045-1057; tests/test_marg_gpu.py::marginalize_at), the problem otherwise as it is"""
    pr = ws.problem
    if not pr.sb_prior:
        return ws.marginalize(state)
    sb = np.ctypeslib.as_array(pr.sb_prior, shape=(pr.n_kf, 9))
    saved = sb.copy()
    for k in range(pr.n_kf):
        if not np.isnan(sb[k, 0]):
            sb[k] = state[k, 7:16]
    try:
        return ws.marginalize(state)
    finally:
        sb[:] = saved


def chain(ws, state0, options=None):
    """the calls the cycle replaces: (raw final state, summary, unified state, next prior)"""
    final, summ = ws.solve(state0, options=options)
    uni = unify_host(final)
    return final, summ, uni, marginalize_chain(ws, uni)


def prior_bytes(p):
    return (tuple(p["block_kind"]), tuple(p["block_keyframe"]), np.concatenate(p["x0"]).tobytes(), p["J0"].tobytes(), p["r0"].tobytes(), p["rank"])


def same_prior(got, want, what):
    assert got["block_kind"] == want["block_kind"] and got["block_keyframe"] == want["block_keyframe"], what
    assert got["J0"].shape == want["J0"].shape and got["rank"] == want["rank"] and tuple(got["sweeps"]) == tuple(want["sweeps"]), (what, got["rank"], want["rank"], got["sweeps"], want["sweeps"])
    d = max(np.abs(got["J0"] - want["J0"]).max(), np.abs(got["r0"] - want["r0"]).max())
    print(f"prior [{what}]: n {got['J0'].shape[0]} rank {got['rank']} sweeps {got['sweeps']}  largest difference to the chain's J0 / r0 {d:.3e}")
    assert np.concatenate(got["x0"]).tobytes() == np.concatenate(want["x0"]).tobytes(), what
    assert got["J0"].tobytes() == want["J0"].tobytes() and got["r0"].tobytes() == want["r0"].tobytes(), (what, d)


def poses_are(mt, state, what):
    for k in range(state.shape[0]):
        t, q, _ = mt.pose_get(k)
        assert t.tobytes() == state[k, 0:3].tobytes() and q.tobytes() == state[k, 3:7].tobytes(), (what, k)


def error_code(call):
    with pytest.raises(L.LiliError) as e:
        call()
    return int(re.match(r"lili error (-?\d+)", str(e.value)).group(1))


def first_window(gpu_ctx, n_kf):
    win, recs = S.cut(MH.win4(), 0, n_kf), None          # (the oracle's records would only re-check the association counts: tests/test_window_solve_gpu.py does)
    mt = S.gpu_side(gpu_ctx, win, recs)
    return win, recs, mt, S.window_problem(L.WindowSolver(gpu_ctx, mt), win, n_kf), S.state_of(win, n_kf)


def second_window(gpu_ctx):
    nxt, recs, _, _, _, _, _ = MH.second_window()
    mt = S.gpu_side(gpu_ctx, nxt, recs)
    return nxt, mt, L.WindowSolver(gpu_ctx, mt), [p["pre"] for p in nxt["pres"]], S.state_of(nxt, 3)


# ---------------------------------------------------------------- 1. cycle == chain, speed-bias branch
@pytest.mark.parametrize("n_kf", [3, 2, 4])
def test_cycle_is_the_chain(gpu_ctx, n_kf):
    win, recs, mt, ws, s0 = first_window(gpu_ctx, n_kf)
    final, summ, uni, prior_c = chain(ws, s0)
    ws.reset_cycle()
    raw = L.WindowCycleResult()
    res = ws.cycle(s0, result=raw)
    assert res["summary"] == summ, (res["summary"], summ)                      # iterations, successful steps, termination, costs, every logged radius / cost / rho
    assert res["solved"].tobytes() == uni.tobytes()
    assert res["prior_updated"] and res["prior_n"] == prior_c["J0"].shape[0] == {2: 15, 3: 21, 4: 36}[n_kf] and res["prior_blocks"] == len(prior_c["block_kind"])
    assert res["rank"] == prior_c["rank"] and res["sweeps"] == tuple(prior_c["sweeps"])
    same_prior(ws.resident_prior(), prior_c, f"cycle against chain, n_kf = {n_kf}")
    poses_are(mt, uni, "slot poses after the cycle")
    assert res["refused"] == [0] * n_kf and res["abs_state"].tobytes() == uni.tobytes()
    # the same cycle on a fresh context: identical bytes, the whole result structure and the prior
    ctx2 = L.Context(0)
    try:
        mt2 = S.gpu_side(ctx2, win, recs)
        ws2 = S.window_problem(L.WindowSolver(ctx2, mt2), win, n_kf)
        raw2 = L.WindowCycleResult()
        ws2.cycle(s0, result=raw2)
        assert bytes(raw2) == bytes(raw)
        assert prior_bytes(ws2.resident_prior()) == prior_bytes(ws.resident_prior())
    finally:
        ctx2.close()


# ---------------------------------------------------------------- 2. the second cycle takes the prior from the device
def test_second_cycle_on_the_resident_prior(gpu_ctx):
    win, recs, mt1, ws1, s0 = first_window(gpu_ctx, 3)
    _, _, uni1, prior1_c = chain(ws1, s0)
    ws1.reset_cycle()
    ws1.cycle(s0)
    nxt, mt2, ws2, pres2, s2 = second_window(gpu_ctx)                           # a new matcher, new maps and associations on the same context
    same_prior(ws2.resident_prior(), prior1_c, "the first cycle's prior after the next window's association")
    # referee: the chain's second solve with the prior uploaded from the host
    ws2.set_problem([0, 1, 2], MASK, imu=pres2, prior=prior1_c)
    final_c, summ_c, uni_c, prior2_c = chain(ws2, s2)
    ws2.set_problem([0, 1, 2], MASK, imu=pres2)
    res = ws2.cycle(s2, use_resident_prior=True)
    summ = res["summary"]
    assert (summ["iterations"], summ["successful_steps"], summ["termination"]) == (summ_c["iterations"], summ_c["successful_steps"], summ_c["termination"])
    assert [e["accepted"] for e in summ["log"]] == [e["accepted"] for e in summ_c["log"]] and [e["radius"] for e in summ["log"]] == [e["radius"] for e in summ_c["log"]]
    d = np.abs(res["solved"] - uni_c)
    print(f"second cycle: distance to the chain's device result  t {d[:, 0:3].max():.3e}  q {d[:, 3:7].max():.3e}  speed-bias {d[:, 7:16].max():.3e}  "
          f"final cost {abs(summ['final_cost'] - summ_c['final_cost']):.3e}  (decisions {summ['iterations']} / {summ['successful_steps']} / {summ['termination']})")
    # the oracle's own second solution, compare_solve's bounds
    sol_o, info_o, log_o = MH.second_solved()
    S._stable(log_o, info_o)
    assert summ["termination"] == info_o["termination"] and summ["iterations"] == info_o["iterations"] and summ["successful_steps"] == info_o["successful_steps"]
    d_cost = abs(summ["final_cost"] - info_o["cost"]) / info_o["cost"]
    dts = [np.linalg.norm(res["solved"][k, 0:3] - sol_o[f"t{k}"]) for k in range(3)]
    das = [S._angle(res["solved"][k, 3:7], sol_o[f"q{k}"]) for k in range(3)]
    dsb = [np.abs(res["solved"][k, 7:16] - sol_o[f"sb{k}"]).max() for k in range(3)]
    print(f"second cycle against the oracle: d_cost {d_cost:.3e}  d_t {max(dts):.3e} m  d_angle {max(das):.3e} rad  d_speed_bias {max(dsb):.3e}")
    assert d_cost <= 1e-6 and max(dts) < 1e-4 and max(das) < 1e-4 and max(dsb) < 1e-4
    # and its new prior is the chain's second marginalisation
    same_prior(ws2.resident_prior(), prior2_c, "second cycle against the chain's second marginalisation")
    assert res["solved"].tobytes() == uni_c.tobytes() and summ == summ_c
    poses_are(mt2, uni_c, "slot poses after the second cycle")


# ---------------------------------------------------------------- 3. the unification comes before the marginalisation
def test_unification_before_marginalisation(gpu_ctx):
    win, recs, mt, ws, s0 = first_window(gpu_ctx, 3)
    start = S.perturbed(s0, 5, negate_q=1)
    final, summ, uni, prior_c = chain(ws, start)
    assert final[1, 3] < 0 and final[0, 3] > 0 and final[2, 3] > 0            # the input condition: the chain's raw solution has w < 0 on keyframe 1 only
    raw_prior = marginalize_chain(ws, final)
    assert raw_prior["J0"].tobytes() != prior_c["J0"].tobytes()               # ... and the prior depends on the sign
    ws.reset_cycle()
    res = ws.cycle(start)
    assert (res["solved"][:, 3] >= 0).all() and res["solved"].tobytes() == uni.tobytes() and res["summary"] == summ
    same_prior(ws.resident_prior(), prior_c, "unified before marginalised")
    poses_are(mt, uni, "slot poses carry the unified q")
    # the next cycle, started with keyframe 0 (the old keyframe 1) negated: MarginalizationFactor's sign branch, prior from the device against prior from the host
    nxt, mt2, ws2, pres2, s2 = second_window(gpu_ctx)
    start2 = np.array(s2)
    start2[0, 3:7] = -start2[0, 3:7]
    q0 = prior_c["x0"][[i for i, (kind, kf) in enumerate(zip(prior_c["block_kind"], prior_c["block_keyframe"])) if (kind, kf) == (1, 0)][0]]
    assert W.qmul(W.qinv(q0), start2[0, 3:7])[0] < 0
    ws2.set_problem([0, 1, 2], MASK, imu=pres2, prior=prior_c)
    _, summ2_c, uni2_c, prior2_c = chain(ws2, start2)
    ws2.set_problem([0, 1, 2], MASK, imu=pres2)
    res2 = ws2.cycle(start2, use_resident_prior=True)
    assert res2["summary"] == summ2_c and res2["solved"].tobytes() == uni2_c.tobytes()
    same_prior(ws2.resident_prior(), prior2_c, "the cycle behind a negated start")


# ---------------------------------------------------------------- 4. the gates
def _between(values):
    """a threshold between two of `values` (the geometric mean of the pair with the largest ratio), and the input condition: no value within 10 % of it"""
    v = sorted(float(x) for x in values)
    assert v[0] > 0
    i = max(range(len(v) - 1), key=lambda k: v[k + 1] / v[k])
    thr = float(np.sqrt(v[i] * v[i + 1]))
    assert all(not (0.9 * thr <= x <= 1.1 * thr) for x in v), (thr, v)
    return thr


def test_gates_against_the_model(gpu_ctx):
    win, recs, mt, ws, s0 = first_window(gpu_ctx, 3)
    final, summ, uni, prior_c = chain(ws, s0)
    mv = CM.moves(s0.tolist(), uni.tolist())                                    # thresholds from the chain's result, not from the call under test
    gates = dict(gate_p=_between([m["p"] for m in mv]), gate_v=_between([m["v"] for m in mv]),
                 gate_ba=_between([x for m in mv for x in m["ba"]]), gate_bg=_between([x for m in mv for x in m["bg"]]))
    print("gates:", gates, "moves:", mv)
    ws.reset_cycle()
    plain = ws.cycle(s0)
    prior_plain = ws.resident_prior()
    # default gates: nothing is refused, and the three states are the model's
    m_solved, m_abs, m_next, m_refused = CM.apply(s0.tolist(), final.tolist())
    assert plain["refused"] == m_refused == [0, 0, 0]
    assert plain["solved"].tobytes() == np.array(m_solved).tobytes() and plain["abs_state"].tobytes() == np.array(m_abs).tobytes()
    assert plain["next_state"].tobytes() == np.array(m_next).tobytes()
    # the chosen gates: one refused and one accepted of each kind
    res = ws.cycle(s0, gates=gates)
    m_solved, m_abs, m_next, m_refused = CM.apply(s0.tolist(), final.tolist(), gates)
    for bit in (CM.BIT_P, CM.BIT_V):
        assert 0 < sum(1 for r in m_refused if r & bit) < 3
    for lo in (3, 6):
        got = [bool(r >> (lo + i) & 1) for r in m_refused for i in range(3)]
        assert any(got) and not all(got)
    assert res["refused"] == m_refused, (res["refused"], m_refused)
    assert res["abs_state"].tobytes() == np.array(m_abs).tobytes() and res["next_state"].tobytes() == np.array(m_next).tobytes()
    # a q gate below every move: every q keeps state_in's bytes, in both states
    tight = ws.cycle(s0, gates=dict(gate_q=min(m["q"] for m in mv) / 2))
    m_q = CM.apply(s0.tolist(), final.tolist(), dict(gate_q=min(m["q"] for m in mv) / 2))
    assert tight["refused"] == m_q[3] == [CM.BIT_Q] * 3 and tight["abs_state"][:, 3:7].tobytes() == s0[:, 3:7].tobytes() == tight["next_state"][:, 3:7].tobytes()
    assert tight["abs_state"].tobytes() == np.array(m_q[1]).tobytes() and tight["next_state"].tobytes() == np.array(m_q[2]).tobytes()
    # the gates change neither the solve nor the prior
    for r in (res, tight):
        assert r["solved"].tobytes() == plain["solved"].tobytes() == uni.tobytes() and r["summary"] == plain["summary"] == summ
    same_prior(ws.resident_prior(), prior_plain, "the prior under other gates")
    same_prior(prior_plain, prior_c, "the prior under the default gates")


# ---------------------------------------------------------------- 5. numerical_failure: on at the unchanged state
def test_numerical_failure_goes_on_at_the_unchanged_state(gpu_ctx):
    v = B.NO_CORRESPONDENCE["invalid_steps"]
    win = B.far_window()
    mt = S.gpu_side(gpu_ctx, win)
    ws = S.window_problem(L.WindowSolver(gpu_ctx, mt), win, 3, sb_priors=False, imu=False)
    s0 = S.state_of(win, 3)
    opts = mt.lm_options(**v["opts"])
    final, summ = ws.solve(s0, options=opts)
    assert summ["termination"] == "numerical_failure" and final.tobytes() == s0.tobytes()
    uni = unify_host(final)
    ws.reset_cycle()
    try:
        prior_c, code_c = marginalize_chain(ws, uni), 0
    except L.LiliError as e:
        prior_c, code_c = None, int(re.match(r"lili error (-?\d+)", str(e)).group(1))
    print(f"numerical_failure: the chain's marginalisation returns {code_c}" + ("" if prior_c is None else f", rank {prior_c['rank']} of {prior_c['J0'].shape[0]}"))
    if prior_c is None:
        assert error_code(lambda: ws.cycle(s0, options=opts)) == code_c
        assert error_code(ws.resident_prior) == E_STATE
    else:
        res = ws.cycle(s0, options=opts)
        assert res["summary"] == summ and res["solved"].tobytes() == uni.tobytes()
        assert res["abs_state"].tobytes() == uni.tobytes() and np.array_equal(res["abs_state"], s0) and res["refused"] == [0, 0, 0]
        same_prior(ws.resident_prior(), prior_c, "numerical_failure")
    ws.reset_cycle()


def test_next_state_on_every_branch_of_matrix_to_quaternion(gpu_ctx):
    """The harness quaternions lie near the identity: the trace branch only.  A window without correspondences, IMU factors and priors ends in numerical_failure at the
    unchanged state, so state_in chooses the q the write-back converts: keyframe k turned almost 180 degrees about axis k reaches branch k of Eigen's matrix -> quaternion,
    a second cycle with w < 0 in front of the same rotations reaches them behind the unification."""
    win = B.far_window()
    mt = S.gpu_side(gpu_ctx, win)
    ws = S.window_problem(L.WindowSolver(gpu_ctx, mt), win, 3, sb_priors=False, imu=False)
    opts = mt.lm_options(**B.NO_CORRESPONDENCE["invalid_steps"]["opts"])
    s0 = S.state_of(win, 3)
    for sign in (1.0, -1.0):
        state = s0.copy()
        for k, q in enumerate(((0.02, 0.99, 0.05, -0.03), (0.03, 0.05, 0.99, -0.02), (0.01, -0.04, 0.06, 0.99))):
            state[k, 3:7] = sign * np.array(CM.normalized([float(v) for v in q]))
        uni = unify_host(state)
        # the input condition, on the model alone: branch k for keyframe k, none the trace branch
        assert [CM.branch_of(CM.matrix_from_quat(CM.normalized(uni[k, 3:7].tolist()))) for k in range(3)] == [0, 1, 2]
        ws.reset_cycle()
        res = ws.cycle(state, options=opts)
        assert res["summary"]["termination"] == "numerical_failure" and res["solved"].tobytes() == uni.tobytes()
        m_solved, m_abs, m_next, m_refused = CM.apply(state.tolist(), state.tolist())
        assert res["refused"] == m_refused == [0, 0, 0]
        assert res["abs_state"].tobytes() == np.array(m_abs).tobytes() and res["next_state"].tobytes() == np.array(m_next).tobytes()
        poses_are(mt, uni, "slot poses carry the unified q")
    ws.reset_cycle()


# ---------------------------------------------------------------- 6. refusals leave everything alone
def test_refusals_leave_everything_alone(gpu_ctx):
    win, recs, mt, ws, s0 = first_window(gpu_ctx, 3)
    pres = [p["pre"] for p in win["pres"]]
    ws.reset_cycle()
    ws.cycle(s0)                                                                 # a resident prior to be left alone
    kept = prior_bytes(ws.resident_prior())
    before = [mt.pose_get(k) for k in range(3)]
    raw = L.WindowCycleResult()
    C.memset(C.byref(raw), 0x5A, C.sizeof(raw))
    pattern = bytes(raw)

    def refused(what, state, code, resident_left=True, **kw):
        got = error_code(lambda: ws.cycle(state, result=raw, **kw))
        assert got == code, (what, got, code)
        assert bytes(raw) == pattern, what
        for k in range(3):
            t, q, _ = mt.pose_get(k)
            assert t.tobytes() == before[k][0].tobytes() and q.tobytes() == before[k][1].tobytes(), what
        if resident_left:
            assert prior_bytes(ws.resident_prior()) == kept, what

    ws.set_problem([0], MASK, n_kf=1)
    refused("n_kf = 1", np.ones((1, 16)), E_ARG)
    ws.set_problem([0, 1, 2, 3, 4], MASK, n_kf=5)
    refused("n_kf = 5", np.ones((5, 16)), E_ARG)
    ws.set_problem([0, 1, 7], MASK, imu=pres)                                    # slot 7 was never associated
    refused("a slot without records", s0, E_STATE)
    ws.set_problem([0, 1, 2], MASK, imu=pres)
    for bad_value, where in ((np.nan, (2, 9)), (np.inf, (0, 4))):
        bad = s0.copy()
        bad[where] = bad_value
        refused("a state that is not finite", bad, E_ARG)
    ws.set_problem([0, 1, 2], MASK, imu=pres, prior=ws.resident_prior())
    refused("a resident and a host prior together", s0, E_ARG, use_resident_prior=True)
    # and after reset_cycle() there is none to use, and none to fetch
    ws.set_problem([0, 1, 2], MASK, imu=pres)
    ws.reset_cycle()
    assert error_code(ws.resident_prior) == E_STATE
    refused("resident requested after reset_cycle()", s0, E_STATE, resident_left=False, use_resident_prior=True)
    assert error_code(ws.resident_prior) == E_STATE


def test_resident_requested_with_none_on_a_fresh_context():
    ctx = L.Context(0)
    try:
        win = S.cut(MH.win4(), 0, 3)
        mt = S.gpu_side(ctx, win)
        ws = L.WindowSolver(ctx, mt)
        ws.set_problem([0, 1, 2], MASK, imu=[p["pre"] for p in win["pres"]])
        before = [mt.pose_get(k) for k in range(3)]
        assert error_code(lambda: ws.cycle(S.state_of(win, 3), use_resident_prior=True)) == E_STATE
        assert error_code(ws.resident_prior) == E_STATE
        for k in range(3):
            t, q, _ = mt.pose_get(k)
            assert t.tobytes() == before[k][0].tobytes() and q.tobytes() == before[k][1].tobytes()
    finally:
        ctx.close()


# ---------------------------------------------------------------- 7. the resident prior survives its neighbours; seeding it
def test_resident_prior_survives_its_neighbours(gpu_ctx):
    win, recs, mt, ws, s0 = first_window(gpu_ctx, 3)
    ws.reset_cycle()
    res = ws.cycle(s0)
    kept = prior_bytes(ws.resident_prior())
    p = ws.resident_prior()
    # the calls that share win_prob / win_marg / win_out with the cycle, then a fresh association
    ws.evaluate(s0)
    final, _ = ws.solve(s0)
    ws.marginalize(unify_host(final))
    A, b = MH.schur_case(15, 21, None)
    L.api.marg_schur(gpu_ctx, A, b, 15)
    nxt, mt2, ws2, pres2, s2 = second_window(gpu_ctx)
    ws2.set_problem([0, 1, 2], MASK, imu=pres2, prior=p)
    ws2.evaluate(s2)
    assert prior_bytes(ws2.resident_prior()) == kept
    # set_resident_prior(p) -> resident_prior() returns p's bytes (here: a prior with fewer rows than columns, as a saved one may be)
    q = dict(p, J0=p["J0"][3:].copy(), r0=p["r0"][3:].copy())
    ws2.set_resident_prior(q)
    back = ws2.resident_prior()
    assert prior_bytes(back)[:5] == prior_bytes(q)[:5] and back["J0"].shape == (18, 21) and back["rank"] == 18
    ws2.set_resident_prior(p)
    assert prior_bytes(ws2.resident_prior()) == kept
    # a cycle seeded that way is the chain with prior = p
    _, summ_c, uni_c, prior2_c = chain(ws2, s2)                                 # (the problem still carries prior = p)
    ws2.set_problem([0, 1, 2], MASK, imu=pres2)
    res2 = ws2.cycle(s2, use_resident_prior=True)
    assert res2["summary"] == summ_c and res2["solved"].tobytes() == uni_c.tobytes()
    same_prior(ws2.resident_prior(), prior2_c, "a cycle on a seeded prior")
    # a bad seed is refused and leaves the resident prior alone
    kept2 = prior_bytes(ws2.resident_prior())
    assert error_code(lambda: ws2.set_resident_prior(dict(p, J0=p["J0"][:, :20].copy()))) == E_ARG
    assert prior_bytes(ws2.resident_prior()) == kept2
