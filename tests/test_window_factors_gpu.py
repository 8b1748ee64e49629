"""The window's closed-form factors on the device (win_imu_raw, win_prior_block, win_build of lili_window.hip) against the exact model of
tests/window_factor_cases.py, entry by entry: lili_window_evaluate with kind_mask 0 (no lidar; a matcher without clouds supplies the params) on every
designed case, and lili_window_marginalize with kind_mask 0 on the IMU families for the last-three-columns variant (win_build<true>).

Evaluation.  For every case and every entry of cost, g and H:  |device - model| <= 8 K 2^-53 magnitude, K the family's (window_factor_cases.K, measured by
tests/test_window_factor_cases_cpu.py on oracle/lo_window.py), magnitude the entry's own; H symmetric to the same allowance; entries of magnitude 0 exactly 0;
two calls give identical bytes.  Measured on an MI355X, worst |device - model| / (2^-53 magnitude) per family (allowance 8 K):
  attitude 4.14 (20.7), residual angle 3.52 (17.2), bias step 1.73 (14.5), magnitudes 4.27 (21.3), gravity 1.26 (9.04), covariance 1.98 (22.2), covariance scale 2.20 (21.0),
  covariance preintegrated 1.70 (293), covariance conditioned 1.34e3 (6.95e7: the host's long-double sqrt_info is four orders closer to the exact one than numpy's), covariance
  given 3.06 (18.6), position 2.98 (22.2), prior tables 5.85 (49.9), prior rows 3.21 (28.3), prior quaternion 3.48 (35.9), prior x0 norm 2.19 (17.5), combined 3.76 (45.9).
  H came out exactly symmetric in the IMU families and to 0.42 units with a prior.
Last three columns.  J0^T J0 and J0^T r0 of the device's prior against the model's Schur complement (mpmath), relative to the largest entry of the model's quantity;
allowance 100 x numpy's own difference to the model on the same systems (window_factor_cases.MARG_NUMPY_WORST, tests/test_marg_gpu.py's rule).  The input
condition (every eigenvalue of Amm and S >= 1e-3) is asserted on the model alone; 0 of 75 systems miss it.  Measured on an MI355X (J0^T J0, J0^T r0; allowance):
  attitude 5.5e-15, 5.2e-15 (4e-13, 5e-13);  residual angle 5.2e-15, 4.6e-15 (3e-13, 7e-13);  bias step 5.5e-15, 6.6e-15 (5e-13, 3e-13);
  magnitudes 6.0e-15, 1.5e-13 (1e-12, 4e-11);  gravity 3.5e-15, 2.9e-15 (2e-13, 9e-13);  covariance 5.9e-15, 5.7e-15 (3e-13, 2e-13);
  covariance scale 1.5e-6, 2.5e-6 (2e-3, 7e-4: the Schur complement cancels from 1e13 to 4e3 — numpy loses 1.2e-5 there);  covariance preintegrated 1.5e-13, 7.1e-14
  (2e-11, 2e-11);  covariance conditioned 3.6e-13, 6.1e-13 (7e-11, 9e-11);  position 4.8e-15, 4.1e-15 (2e-13, 2e-13).

Solve.  One lili_window_solve, n_kf = 3 with speed-bias priors, on tests/window_harness.py's window with the tumbling trajectory of window_factor_cases (every
quaternion component large, gravity off the rotation axis): the decisions equal W.ceres_lm's, _stable first (tests/test_window_solve_gpu.py::compare_solve) — the
persistent kernel's win_build sees the same factors.  The window keeps its lidar blocks: lili_window_solve refuses a problem without them (kind_mask 0 is for
lili_window_evaluate and lili_window_marginalize only).  Measured: 15 iterations, 15 successful, max_iterations on both sides; end states d_cost 1.2e-16, 1.1e-16 m,
1.1e-16 rad, speed-bias 3.9e-16."""
import numpy as np
import pytest

import lili_om_amd as L
from tests import test_window_solve_gpu as S
from tests import window_factor_cases as F
from tests import window_harness as H

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ws(gpu_ctx):
    return L.WindowSolver(gpu_ctx, L.ScanToMapMatcher(gpu_ctx, L.make_params("livox")))


def set_case(ws, c):
    return ws.set_problem(None, 0, imu=[F.window_imu(r) for r in c["imu"]] if c["imu"] else None, prior=c["prior"], sb_prior=c["sb_prior"], n_kf=c["n_kf"])


@pytest.mark.parametrize("family", F.FAMILIES)
def test_evaluate_against_the_model(ws, family):
    allow = F.DEVICE_FACTOR * F.K[family]
    worst, worst_sym = 0.0, 0.0
    for c in F.by_family(family):
        m = F.model(c)
        set_case(ws, c)
        cost, g, H = ws.evaluate(c["state"])
        cost2, g2, H2 = ws.evaluate(c["state"])
        assert cost == cost2 and g.tobytes() == g2.tobytes() and H.tobytes() == H2.tobytes(), c["name"]
        assert np.isfinite(cost) and np.isfinite(g).all() and np.isfinite(H).all(), c["name"]
        rc, rg, rh = F.ratios(cost, m["cost"]), F.ratios(g, m["g"]), F.ratios(H, m["H"])
        r = float(max(rc.max(), rg.max(), rh.max()))
        print(f"{c['name']}: cost {float(rc):.3g}  g {rg.max():.3g}  H {rh.max():.3g}  (allowance {allow:g})")
        assert (H[m["H"][2] == 0] == 0).all() and (g[m["g"][2] == 0] == 0).all(), c["name"]          # structural zeros
        with np.errstate(divide="ignore", invalid="ignore"):
            sym = np.where(m["H"][2] > 0, np.abs(H - H.T) / (F.U * np.where(m["H"][2] > 0, m["H"][2], 1.0)), 0.0).max()
        worst, worst_sym = max(worst, r), max(worst_sym, float(sym))
        bad = np.argwhere(rh > allow)
        assert r <= allow, (c["name"], r, "cost" if rc.max() > allow else "", np.argwhere(rg > allow).ravel()[:8], bad[:8])
        assert sym <= allow, (c["name"], sym)
    print(f"evaluate [{family}]: worst |device - model| / (2^-53 magnitude) = {worst:.3g}, asymmetry of H {worst_sym:.3g}, allowance 8 K = {allow:g}")


@pytest.mark.parametrize("family", F.IMU_FAMILIES)
def test_last_three_columns_against_the_model(ws, family):
    cs = [c for c in F.last3_cases() if c["family"] == family]
    usable = [c for c in cs if F.marg_usable(c)]
    print(f"last three columns [{family}]: {len(cs)} systems, {len(cs) - len(usable)} dropped by the input condition")
    assert 4 * (len(cs) - len(usable)) <= len(cs) and usable
    bound = 100.0 * np.array(F.MARG_NUMPY_WORST[family])
    worst = np.zeros(2)
    for c in usable:
        mm = F.marg_model(c)
        set_case(ws, c)
        p = ws.marginalize(c["state"])
        again = ws.marginalize(c["state"])
        assert p["J0"].tobytes() == again["J0"].tobytes() and p["r0"].tobytes() == again["r0"].tobytes(), c["name"]
        _, _, kept = F.marg_selection(c)
        assert list(zip(p["block_kind"], p["block_keyframe"])) == [(kind, kf - 1) for kind, kf in kept], c["name"]
        assert p["J0"].shape == (len(mm["bs"]), len(mm["bs"])) and p["rank"] == len(mm["bs"]), c["name"]
        d = F.marg_difference(p["J0"], p["r0"], mm)
        print(f"{c['name']}: J0^T J0 {d[0]:.3e}  J0^T r0 {d[1]:.3e}  sweeps {p['sweeps']}")
        worst = np.maximum(worst, d)
        assert (d <= bound).all(), (c["name"], d, bound)
    print(f"last three columns [{family}]: worst J0^T J0 {worst[0]:.3e}  J0^T r0 {worst[1]:.3e}  (allowance {bound[0]:.2e}, {bound[1]:.2e})")


def test_solve_on_a_tumbling_window(gpu_ctx, oracle, monkeypatch):
    monkeypatch.setattr(H, "trajectory", F.tumbling_trajectory)
    win = S.make_window_n(3)
    assert min(np.abs(kf["q_true"]).min() for kf in win["kfs"]) > 0.2          # no component of any attitude is small
    recs, block = S.oracle_side(oracle, win)
    ws = S.window_problem(L.WindowSolver(gpu_ctx, S.gpu_side(gpu_ctx, win, recs)), win, 3)
    S.compare_solve(ws, S.build_problem(win, block), S.state_of(win, 3), 3, "tumbling window, n_kf = 3, speed-bias priors")
