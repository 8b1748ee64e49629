"""The window's next prior on the device (lili_marg_schur, lili_window_marginalize, WindowSolver.marginalize) against the referee of tests/marg_harness.py:
oracle/lo_window.py::Marginalization (LAPACK through numpy) on the last-three-columns system of the reference's factor set.

Compared: J0^T J0, J0^T r0, r0^T r0 (relative to the largest entry of the referee's quantity), the rank, "rows beyond the rank are exactly zero", and the
off-diagonals of J0 J0^T relative to its largest diagonal entry — nothing that depends on the eigenvector basis, the order of the rows or their signs.

Bounds.  The ceiling is 1e-8 (the project's ceiling in tests/test_window_solve_gpu.py); the asserted bound is min(1e-8, 100 x the worst value measured on
an MI355X against the oracle), as EVAL_BOUND is — per group of cases AND per quantity, so that the well-conditioned quantities are not held to the bound of
r0^T r0.  For orientation, two CPU routes to the same Schur complement (eigen pseudo-inverse and
numpy.linalg.solve) differ by 1.5e-15 .. 2.1e-15 relative on these windows.  Measured on an MI355X (d_JtJ, d_Jtr, d_rtr, row orthogonality):
  lili_marg_schur, synthetic systems: (1, 1) 0, 0, 0, 0;  (3, 3) 2.8e-16, 3.2e-16, 1.0e-15, 8.5e-17;  (15, 21) singular Amm 3.6e-15, 4.2e-15, 4.0e-15, 4.6e-16;
    (15, 30) rank-deficient S 3.9e-15, 3.9e-15, 3.5e-15, 2.3e-15;  (15, 45) repeated eigenvalue 1.3e-15, 5.1e-15, 2.44e-14, 7.4e-18   -> SCHUR_WORST
  lili_window_marginalize: speed-bias branch n_kf = 3  2.0e-15, 2.6e-15, 4.75e-12, 1.8e-16;  n_kf = 2  1.1e-15, 3.6e-14, 1.8e-12, 1.3e-16;
    n_kf = 4  1.8e-15, 4.4e-15, 3.7e-13, 2.1e-16;  old prior 3.1e-15, 3.9e-15, 2.7e-12, 4.3e-17;  old prior, q1 negated 1.3e-15, 6.6e-15, 1.8e-13, 4.3e-17;
    the chain's device prior at the device's own solution 2.0e-15, 1.3e-14, 4.74e-12, 1.7e-16   -> MARG_WORST
    (r0^T r0 = bs^T S^+ bs carries the condition number of S, 1e5 on these windows, times the rounding of either eigen-solver; the other three do not)
  lili_window_evaluate of the chain's second window with the device prior against the oracle's prior (cost, gradient, J^T J): 1.6e-15, 2.1e-17, 1.91e-15
    -> CHAIN_EVAL_WORST
  the chain's solves: keyframes 0-2 15 iterations / 15 successful / max_iterations, keyframes 1-3 with the device prior 14 / 13 / function_tolerance, both as the
    oracle; end states d_cost 0 / 1.2e-16, 5.6e-17 / 2.2e-15 m, 2.2e-18 / 1.2e-17 rad, speed-bias 2.6e-16 / 2.8e-14 (bounds 1e-6, 1e-4 m, 1e-4 rad, 1e-4)
  Jacobi sweeps read back (Amm, S): 6, 5 (n_kf = 3); 6, 4 (n_kf = 2); 6, 5 (n_kf = 4); 5, 5 (old prior); 5, 6 (old prior, q1 negated)
No test here reaches the sweep cap (LILI_E_NUMERIC): no finite symmetric input is known that keeps this solver busy for 30 sweeps, so that path — a uniform
return before any write, the host copying nothing — is checked by reading the code only.
The conditions on the inputs (no eigenvalue near eps = 1e-8; solves decided clear of their thresholds) are asserted on the oracle alone in
tests/test_marg_cpu.py and, for the chain's solves, again here by compare_solve (_stable)."""
import ctypes as C

import numpy as np
import pytest

import lili_om_amd as L
from oracle import lo_window as W
from tests import marg_harness as MH
from tests import test_window_solve_gpu as S

pytestmark = pytest.mark.gpu

MASK = S.MASK
# the worst values measured on an MI355X per quantity (J0^T J0, J0^T r0, r0^T r0, row orthogonality; table above); asserted at 100 x, never above the 1e-8 ceiling
SCHUR_WORST = (3.92e-15, 5.07e-15, 2.44e-14, 2.28e-15)
MARG_WORST = (3.08e-15, 3.63e-14, 4.75e-12, 2.11e-16)
CHAIN_EVAL_WORST = 1.91e-15
SCHUR_BOUND = tuple(min(100 * w, 1e-8) for w in SCHUR_WORST)
MARG_BOUND = tuple(min(100 * w, 1e-8) for w in MARG_WORST)
CHAIN_EVAL_BOUND = min(100 * CHAIN_EVAL_WORST, 1e-8)


# ---------------------------------------------------------------- 1. lili_marg_schur on synthetic systems
@pytest.mark.parametrize("m,n,special", MH.SCHUR_CASES)
def test_schur_against_the_oracle(gpu_ctx, m, n, special):
    A, b = MH.schur_case(m, n, special)
    M = W.Marginalization(A, b, m, [])
    J0, r0, rank = L.api.marg_schur(gpu_ctx, A, b, m)
    worst = MH.compare_prior(J0, r0, rank, M, SCHUR_BOUND, f"synthetic ({m}, {n}) {special or ''}")
    _, w_s = MH.spectra(A, m)
    assert rank == int((w_s > MH.EPS).sum())
    # two calls give identical bytes
    J0b, r0b, rankb = L.api.marg_schur(gpu_ctx, A, b, m)
    assert J0.tobytes() == J0b.tobytes() and r0.tobytes() == r0b.tobytes() and rank == rankb
    print(f"schur ({m}, {n}): worst {max(worst):.3e}")


def test_schur_refuses_bad_sizes_and_writes_nothing(gpu_ctx):
    lib = gpu_ctx.lib
    A, b = MH.schur_case(3, 3, None)
    big = np.eye(61)
    for A_, b_, pos, m in ((A, b, 6, 0), (A, b, 6, 6), (big, np.zeros(61), 61, 15), (A, b, 6, -1), (A, b, 1, 1)):
        J0, r0, rank = np.full((61, 61), 7.0), np.full(61, 7.0), C.c_int(-7)
        rc = lib.lili_marg_schur(gpu_ctx.h, A_.ctypes.data, A_.shape[1], b_.ctypes.data, pos, m, J0.ctypes.data, r0.ctypes.data, C.byref(rank))
        assert rc == -1, (pos, m, rc)
        assert (J0 == 7.0).all() and (r0 == 7.0).all() and rank.value == -7
    bad = A.copy()
    bad[1, 2] = np.nan
    with pytest.raises(L.LiliError):
        L.api.marg_schur(gpu_ctx, bad, b, 3)
    with pytest.raises(L.LiliError):
        L.api.marg_schur(gpu_ctx, A, b, 6)
    # and a leading dimension larger than pos is honoured
    wide = np.zeros((6, 9)); wide[:, :6] = A; wide[:, 6:] = np.nan
    J0, r0, rank = np.zeros((3, 3)), np.zeros(3), C.c_int(0)
    assert lib.lili_marg_schur(gpu_ctx.h, wide.ctypes.data, 9, b.ctypes.data, 6, 3, J0.ctypes.data, r0.ctypes.data, C.byref(rank)) == 0
    J1, r1, rank1 = L.api.marg_schur(gpu_ctx, A, b, 3)
    assert J0.tobytes() == J1.tobytes() and r0.tobytes() == r1.tobytes() and rank.value == rank1 == 3


# ---------------------------------------------------------------- 2. WindowSolver.marginalize against the oracle at the oracle's solved state
def marginalize_at(ws, win, n, state, sb_kfs=(), prior=None, imu=None):
    sb = None
    if len(sb_kfs):
        sb = np.full((n, 9), np.nan)
        for k in sb_kfs:
            sb[k] = state[k, 7:16]                      # the reference passes the post-solve speed-bias itself (L:1045-1057)
    ws.set_problem(list(range(n)), MASK, imu=imu if imu is not None else [p["pre"] for p in win["pres"]], sb_prior=sb, prior=prior, n_kf=n)
    return ws.marginalize(state)


@pytest.mark.parametrize("n_kf", [3, 2, 4])
def test_marginalize_speed_bias_branch(gpu_ctx, n_kf):
    win, recs, block, sol, pb, M, kept, A, b, m = MH.first_marginalisation(n_kf)
    mt = S.gpu_side(gpu_ctx, win, recs)
    ws = L.WindowSolver(gpu_ctx, mt)
    state = S.state_of(sol, n_kf)
    before = [mt.pose_get(k) for k in range(n_kf)]
    prior = marginalize_at(ws, win, n_kf, state, sb_kfs=range(n_kf - 1))
    worst = MH.compare_prior(prior["J0"], prior["r0"], prior["rank"], M, MARG_BOUND, f"speed-bias branch, n_kf = {n_kf}")
    MH.check_blocks(prior, kept, state)
    assert prior["J0"].shape[0] == {2: 15, 3: 21, 4: 36}[n_kf] and prior["rank"] == prior["J0"].shape[0]
    for a, c in zip(before, [mt.pose_get(k) for k in range(n_kf)]):
        assert np.array_equal(a[0], c[0]) and np.array_equal(a[1], c[1])
    again = marginalize_at(ws, win, n_kf, state, sb_kfs=range(n_kf - 1))
    assert again["J0"].tobytes() == prior["J0"].tobytes() and again["r0"].tobytes() == prior["r0"].tobytes()
    if n_kf == 3:
        # only the IMU factor between keyframes 0 and 1 enters: another second factor changes nothing
        pres = [p["pre"] for p in win["pres"]]
        other = marginalize_at(ws, win, n_kf, state, sb_kfs=range(n_kf - 1), imu=[pres[0], pres[0]])
        assert other["J0"].tobytes() == prior["J0"].tobytes() and other["r0"].tobytes() == prior["r0"].tobytes()
        # and the prior goes into the next problem as it is
        ws.set_problem([0, 1, 2], MASK, imu=pres, prior=prior)
        c, g, _ = ws.evaluate(state)
        assert np.isfinite(c) and np.isfinite(g).all()
    print(f"marginalize, speed-bias branch n_kf = {n_kf}: worst {max(worst):.3e}, Jacobi sweeps (Amm, S) {prior['sweeps']}")


def test_marginalize_with_an_old_prior(gpu_ctx):
    """the second marginalisation of a chain: the old prior (the referee's first), the IMU factor, the lidar blocks; no speed-bias priors"""
    nxt, recs, block, sol2, pb, M, kept, A, b, m = MH.second_marginalisation()
    _, _, _, _, names, M1, kept1 = MH.second_window()
    mt = S.gpu_side(gpu_ctx, nxt, recs)
    ws = L.WindowSolver(gpu_ctx, mt)
    state = S.state_of(sol2, 3)
    prior = marginalize_at(ws, nxt, 3, state, prior=MH.prior_dict(M1, kept1))
    worst = MH.compare_prior(prior["J0"], prior["r0"], prior["rank"], M, MARG_BOUND, "old prior, n_kf = 3")
    MH.check_blocks(prior, kept, state)
    assert prior["J0"].shape[0] == 21
    # where a kept quaternion has w(q0^-1 q) < 0: the sign branch of MarginalizationFactor::Evaluate
    sneg = state.copy()
    sneg[1, 3:7] = -sneg[1, 3:7]
    vals = S.values_of(sneg)
    Mn, keptn, An, _, mn = MH.referee(MH.marg_problem(nxt, block, vals, old=(M1, names)), vals)
    w_mm, w_s = MH.spectra(An, mn)
    assert w_mm.min() >= 200 and w_s.min() >= 200          # the input condition of tests/test_marg_cpu.py, for this state too
    pn = marginalize_at(ws, nxt, 3, sneg, prior=MH.prior_dict(M1, kept1))
    worst = max(max(worst), max(MH.compare_prior(pn["J0"], pn["r0"], pn["rank"], Mn, MARG_BOUND, "old prior, q1 negated")))
    print(f"marginalize, old prior: worst {worst:.3e}, Jacobi sweeps (Amm, S) {prior['sweeps']} / {pn['sweeps']}")


# ---------------------------------------------------------------- 3. the chain: solve, marginalise, solve — device only against oracle only
def test_chain_device_against_oracle(gpu_ctx):
    win, recs, block, sol1, info1, log1 = MH.solved(3)
    mt = S.gpu_side(gpu_ctx, win, recs)
    ws = S.window_problem(L.WindowSolver(gpu_ctx, mt), win, 3)
    final1, _, _, _ = S.compare_solve(ws, S.build_problem(win, block), S.state_of(win, 3), 3, "chain, keyframes 0-2")
    prior_d = marginalize_at(ws, win, 3, final1, sb_kfs=(0, 1))
    # the oracle doing the same with its own prior
    nxt, recs2, block2, pb2, names, M1, kept1 = MH.second_window()
    MH.compare_prior(prior_d["J0"], prior_d["r0"], prior_d["rank"], M1, MARG_BOUND, "chain, device prior at the device's solution")
    MH.check_blocks(prior_d, kept1, final1)
    mt2 = S.gpu_side(gpu_ctx, nxt, recs2)
    ws2 = L.WindowSolver(gpu_ctx, mt2)
    pres2 = [p["pre"] for p in nxt["pres"]]
    s0 = S.state_of(nxt, 3)
    # lili_window_evaluate of the second window with the device prior and with the oracle's
    prior_o = MH.prior_dict(M1, kept1)
    worst = 0.0
    for name, s in (("initial", s0), ("perturbed", S.perturbed(s0, 9)), ("perturbed, q1 negated", S.perturbed(s0, 9, negate_q=1))):
        ws2.set_problem([0, 1, 2], MASK, imu=pres2, prior=prior_o)
        c_o, g_o, H_o = ws2.evaluate(s)
        ws2.set_problem([0, 1, 2], MASK, imu=pres2, prior=prior_d)
        c_d, g_d, H_d = ws2.evaluate(s)
        scale = max(np.abs(H_o).max(), np.abs(g_o).max())
        dc, dg, dh = abs(c_d - c_o) / abs(c_o), np.abs(g_d - g_o).max() / scale, np.abs(H_d - H_o).max() / scale
        print(f"chain evaluate [{name}]: d_cost {dc:.3e}  d_gradient {dg:.3e}  d_JtJ {dh:.3e}")
        worst = max(worst, dc, dg, dh)
        assert max(dc, dg, dh) <= CHAIN_EVAL_BOUND
    print(f"chain evaluate: worst {worst:.3e}")
    # solve keyframes 1-3 with the device-built prior against the oracle with its own: decisions, termination, final state (compare_solve's bounds)
    ws2.set_problem([0, 1, 2], MASK, imu=pres2, prior=prior_d)
    S.compare_solve(ws2, pb2, s0, 3, "chain, keyframes 1-3 with the device prior")


# ---------------------------------------------------------------- 4. refusals
def test_marginalize_refusals_leave_everything_alone(gpu_ctx):
    win, recs, block, sol, _, _ = MH.solved(3)
    mt = S.gpu_side(gpu_ctx, win)
    ws = L.WindowSolver(gpu_ctx, mt)
    pres = [p["pre"] for p in win["pres"]]
    state = S.state_of(sol, 3)
    before = [mt.pose_get(k) for k in range(3)]
    st = L.api.WindowPriorStorage()
    C.memset(C.byref(st), 0x5A, C.sizeof(st))
    pattern = bytes(st)

    def refused(what, s):
        with pytest.raises(L.LiliError):
            ws.marginalize(s, storage=st)
        assert bytes(st) == pattern, what
        for k in range(3):
            t, q, _ = mt.pose_get(k)
            assert np.array_equal(t, before[k][0]) and np.array_equal(q, before[k][1]), what

    ws.set_problem([0], MASK, n_kf=1)
    refused("n_kf = 1", np.ones((1, 16)))
    ws.set_problem([0, 1, 2, 3, 4], MASK, n_kf=5)
    refused("n_kf = 5", np.ones((5, 16)))
    ws.set_problem([0, 1, 7], MASK, imu=pres)          # slot 7 was never associated
    refused("a slot without records", state)
    ws.set_problem([0, 1, 2], MASK, imu=pres)
    bad = state.copy()
    bad[2, 9] = np.nan
    refused("a NaN in the state", bad)
    bad = state.copy()
    bad[0, 4] = np.inf
    refused("an infinity in the state", bad)
    # and the same objects, put right (with the first cycle's speed-bias priors: without them three directions of this window carry no information), are
    # accepted and fill the storage
    sb = np.full((3, 9), np.nan)
    sb[0], sb[1] = state[0, 7:16], state[1, 7:16]
    ws.set_problem([0, 1, 2], MASK, imu=pres, sb_prior=sb)
    prior = ws.marginalize(state, storage=st)
    assert bytes(st) != pattern and st.prior.n_cols == 21 and prior["rank"] == 21
    assert C.addressof(st.prior.J0.contents) == C.addressof(st.J0) and C.addressof(st.prior.x0.contents) == C.addressof(st.x0)
