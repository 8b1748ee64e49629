"""IMU pre-integration on the device (lili_imu_preintegrate, lili_om_amd.ImuPreintegrator) against the reference's own header:
tests/golden/ref_preint.npz holds what oracle/_ref/libref_imu.so::ref_preintegrate (Preintegration.h compiled unmodified) gives for seeds 1..3 of
tests/test_window_cpu.py::_samples and n in {0, 1, 2, 40, 63, 64, 65, 127, 128, 129, 400} — the kernel prepares 64 samples at a time.

Bounds.  delta_p, delta_q, delta_v and sum_dt: the reference's bits — the chain has no fused operation and no transcendental, the kernel keeps the reference's
operation order, division and square root are correctly rounded on both sides.  Jacobian and covariance: every entry equal as a number (==) and every exact
zero of the reference an exact zero — the kernel leaves out only terms with a structurally-zero factor, and x + 0 y = x; the comparison is
tests/preint_hard_cases.py::compare, shared with tests/test_imu_preint_hard_gpu.py (designed hard streams), and tests/test_preint_hard_cases_cpu.py shows which
faults it notices.  (Against the ORACLE's numpy object, whose `@` sums in another order, test_device_records_in_the_window keeps 1e-11 of the largest entry, the
tolerance tests/test_window_cpu.py applies between that restatement and the reference.)  Prediction: the bits of tests/preint_model.py::predict (+, -, x and a halving).
Determinism: bits.  Into the window: evaluate with the device's records against evaluate with the oracle's records of the same samples within EVAL_BOUND
of tests/test_window_solve_gpu.py (its evaluate-against-oracle tolerance); one solve from each ends the same way.

Measured on an MI355X (33 cases): state bit-equal in every case; Jacobian and covariance equal too (largest difference 0: the referee's stand-in for Eigen
multiplies with textbook loops, the kernel's order); window evaluation d_cost 0, d_gradient 2.3e-21, d_JtJ 9.6e-18 of the largest entry."""
import ctypes as C

import numpy as np
import pytest

import lili_om_amd as L
from oracle import lo_window as W
from tests import preint_hard_cases as HC
from tests import preint_model as M
from tests import window_harness as H
from tests.test_window_solve_gpu import EVAL_BOUND, MASK, gpu_side, state_of

pytestmark = pytest.mark.gpu

G_VEC = (0.0, 0.0, -9.805)


def _rec(w):
    """a lili_window_imu as (state (11), jacobian, covariance, raw bytes)"""
    state = np.array(list(w.delta_p) + list(w.delta_q) + list(w.delta_v) + [w.sum_dt])
    return state, np.array(w.jacobian[:]).reshape(15, 15), np.array(w.covariance[:]).reshape(15, 15), bytes(w)


@pytest.fixture(scope="module")
def cases():
    return M.golden_cases()


@pytest.fixture(scope="module")
def pre(gpu_ctx):
    return L.ImuPreintegrator(gpu_ctx)


@pytest.fixture(scope="module")
def singles(pre, cases):
    """every case in a call of its own: the records everything else is compared with (computed once, never modified)"""
    return [_rec(pre.preintegrate([M.segment_of(c)])[0]) for c in cases]


def test_every_case_against_the_reference_fixture(cases, singles):
    unequal, worst = 0, 0.0
    bad = []
    for c, (state, jac, cov, raw) in zip(cases, singles):
        r = HC.compare(state, jac, cov, c)
        print(HC.line(f"seed {c['seed']} n {c['n']:3d}", r))
        unequal += r["jacobian"]["unequal"] + r["covariance"]["unequal"]
        worst = max(worst, r["jacobian"]["worst"], r["covariance"]["worst"])
        if not HC.equal(r):
            bad.append((c["seed"], c["n"], r))
    print(f"attained: {unequal} unequal entries, worst {worst:.3g} units of 2^-53 x block maximum")
    assert not bad, bad
    for c, (state, jac, cov, raw) in zip(cases, singles):      # what else the record carries
        w = L.api.WindowImu.from_buffer_copy(raw)
        assert tuple(w.g) == G_VEC and np.array_equal(w.lin_ba, c["ba"]) and np.array_equal(w.lin_bg, c["bg"])


def test_results_do_not_depend_on_the_call(pre, cases, singles):
    # two calls
    i400 = next(i for i, c in enumerate(cases) if c["n"] == 400)
    assert _rec(pre.preintegrate([M.segment_of(cases[i400])])[0])[3] == singles[i400][3]
    # the three n = 40 segments in one batch, and in reversed order
    i40 = [i for i, c in enumerate(cases) if c["n"] == 40]
    assert len(i40) == 3
    out = pre.preintegrate([M.segment_of(cases[i]) for i in i40])
    assert [_rec(out[k])[3] for k in range(3)] == [singles[i][3] for i in i40]
    out = pre.preintegrate([M.segment_of(cases[i]) for i in reversed(i40)])
    assert [_rec(out[k])[3] for k in range(3)] == [singles[i][3] for i in reversed(i40)]
    # 64 segments of mixed length (every case, most of them twice: n = 0 and n = 400 included)
    idx = [(7 * k) % len(cases) for k in range(L.api.IMU_MAX_SEGMENTS)]
    assert {cases[i]["n"] for i in idx} == set(M.NS)
    out = pre.preintegrate([M.segment_of(cases[i]) for i in idx])
    for k, i in enumerate(idx):
        assert _rec(out[k])[3] == singles[i][3], (k, cases[i]["seed"], cases[i]["n"])


def test_kernel_time_option(gpu_ctx, pre, cases, singles):
    """option "imu_time": two events around the launch, read by lili_imu_kernel_ms (tools/preint_time.py); the records do not depend on it"""
    i = next(i for i, c in enumerate(cases) if c["n"] == 129)
    pre.preintegrate([M.segment_of(cases[i])])
    with pytest.raises(L.LiliError):
        pre.kernel_ms()                                                  # the last call was not timed
    gpu_ctx.set_option("imu_time", 1)
    try:
        assert _rec(pre.preintegrate([M.segment_of(cases[i])])[0])[3] == singles[i][3]
        assert 0.0 < pre.kernel_ms() < 1e3
    finally:
        gpu_ctx.set_option("imu_time", 0)


def _start_state(seed):
    rng = np.random.default_rng(50 + seed)
    q = W.qnormalized(np.array([1.0, 0, 0, 0]) + rng.normal(0, 0.3, 4))
    return rng.normal(0, 2.0, 3), W.qmat(q) * 1.0003, rng.normal(0, 1.0, 3)      # (R is used as it is: not quite orthonormal on purpose)


def test_prediction_against_the_plain_restatement(pre, cases, singles):
    picked = [i for i, c in enumerate(cases) if c["seed"] == 1 and c["n"] in (0, 1, 65, 400)]
    assert len(picked) == 4
    for i in picked:
        c = cases[i]
        P0, R0, V0 = _start_state(c["n"])
        out, preds = pre.preintegrate([M.segment_of(c, P0=P0, R0=R0, V0=V0, g=G_VEC)], predict=True)
        P1, R1, V1 = M.predict(P0, R0, V0, c["ba"], c["bg"], G_VEC, c["acc0"], c["gyr0"], c["dt"], c["acc"], c["gyr"])
        print(f"prediction n {c['n']}: dP {np.abs(preds[0][0] - P1).max():.3e} dR {np.abs(preds[0][1] - R1).max():.3e} dV {np.abs(preds[0][2] - V1).max():.3e}")
        assert preds[0][0].tobytes() == P1.tobytes() and preds[0][1].tobytes() == R1.tobytes() and preds[0][2].tobytes() == V1.tobytes(), c["n"]
        assert _rec(out[0])[3] == singles[i][3]                      # the factor's record does not depend on the prediction
        if c["n"] == 0:
            assert np.array_equal(preds[0][0], P0) and np.array_equal(preds[0][1], R0) and np.array_equal(preds[0][2], V0)
    # predict = 0 and predict = 1 in one batch: entries of the segments that do not predict stay as they were
    segs, want = [], []
    for k, i in enumerate(picked):
        c = cases[i]
        P0, R0, V0 = _start_state(c["n"])
        segs.append(M.segment_of(c, P0=P0, R0=R0, V0=V0, g=G_VEC, predict=k % 2 == 1))
        want.append(M.predict(P0, R0, V0, c["ba"], c["bg"], G_VEC, c["acc0"], c["gyr0"], c["dt"], c["acc"], c["gyr"]) if k % 2 == 1 else None)
    packed, keep, flags = pre._pack(segs)
    out = (L.api.WindowImu * 4)()
    pred = (L.api.ImuPrediction * 4)()
    C.memset(pred, 0x5A, C.sizeof(pred))
    assert pre.lib.lili_imu_preintegrate(pre.ctx.h, packed, 4, out, pred) == 0
    for k, i in enumerate(picked):
        assert _rec(out[k])[3] == singles[i][3]
        if want[k] is None:
            assert bytes(pred[k]) == b"\x5A" * C.sizeof(L.api.ImuPrediction)
        else:
            assert np.array(pred[k].P1[:]).tobytes() == want[k][0].tobytes() and np.array(pred[k].R1[:]).tobytes() == want[k][1].tobytes() and np.array(pred[k].V1[:]).tobytes() == want[k][2].tobytes()


def test_refusals_write_nothing(pre, cases):
    c = next(c for c in cases if c["n"] == 40)
    lib, h = pre.lib, pre.ctx.h
    out = (L.api.WindowImu * 2)()
    pred = (L.api.ImuPrediction * 2)()

    def refused(segments, n_seg=None, with_out=True, with_pred=True, null_seg=False, patch=None):
        packed, keep, flags = pre._pack(segments)
        if patch:
            patch(packed)
        C.memset(out, 0x5A, C.sizeof(out)); C.memset(pred, 0x5A, C.sizeof(pred))
        rc = lib.lili_imu_preintegrate(h, None if null_seg else packed, len(segments) if n_seg is None else n_seg, out if with_out else None, pred if with_pred else None)
        assert rc == -1, rc                                              # LILI_E_ARG
        assert bytes(out) == b"\x5A" * C.sizeof(out) and bytes(pred) == b"\x5A" * C.sizeof(pred)

    good = M.segment_of(c)
    refused([good], null_seg=True)
    refused([good], with_out=False)
    refused([M.segment_of(c, predict=True)], with_pred=False)           # a predicting segment needs somewhere to write
    refused([good], patch=lambda s: setattr(s[0], "acc", None))          # a null sample array with n > 0
    refused([good], n_seg=0)
    many = [good] * (L.api.IMU_MAX_SEGMENTS + 1)
    refused(many)
    refused([good], patch=lambda s: setattr(s[0], "n", -1))
    long = dict(good, dt=np.full(L.api.IMU_MAX_SAMPLES + 1, 0.005), acc=np.zeros((L.api.IMU_MAX_SAMPLES + 1, 3)), gyr=np.zeros((L.api.IMU_MAX_SAMPLES + 1, 3)))
    refused([long])
    for key, bad in (("acc", np.nan), ("gyr", np.inf), ("dt", np.nan), ("dt", np.inf)):
        a = np.array(good[key], np.float64)
        a[(17,) + (1,) * (a.ndim - 1)] = bad
        refused([good, dict(good, **{key: a})])                         # in the second segment of a batch
    for key in ("ba", "bg", "acc0", "gyr0", "g"):
        v = np.array(good.get(key, G_VEC), np.float64)
        v[2] = np.nan
        refused([dict(good, **{key: v})])
    refused([M.segment_of(c, predict=True, V0=[0.0, np.inf, 0.0])])
    d = c["dt"].copy()
    d[5] = -1e-9
    refused([dict(good, dt=d)])
    # the largest call the interface takes still works
    ok = dict(good, dt=np.full(L.api.IMU_MAX_SAMPLES, 0.0025), acc=np.tile(c["acc"][:1], (L.api.IMU_MAX_SAMPLES, 1)), gyr=np.tile(c["gyr"][:1], (L.api.IMU_MAX_SAMPLES, 1)))
    w = pre.preintegrate([ok])[0]
    assert abs(w.sum_dt - L.api.IMU_MAX_SAMPLES * 0.0025) < 1e-9 and np.isfinite(np.array(w.covariance[:])).all()


@pytest.fixture(scope="module")
def window(gpu_ctx):
    win = H.make_window(n_surf=2500, n_edge=200)
    return win, gpu_side(gpu_ctx, win)


def _window_segments(win):
    segs = []
    for p in win["pres"]:
        s = p["samples"]
        segs.append(dict(dt=[x[0] for x in s[1:]], acc=[x[1] for x in s[1:]], gyr=[x[2] for x in s[1:]], acc0=s[0][1], gyr0=s[0][2], ba=p["ba"], bg=p["bg"]))
    return segs


def _sb_prior(win):
    sb = np.full((H.N_KF, 9), np.nan)
    for k in range(H.N_KF - 1):
        sb[k] = win["init"][k]["sb"]
    return sb


def _compare_in_the_window(gpu_ctx, win, m, imu_oracle, imu_device, what):
    ws = L.WindowSolver(gpu_ctx, m)
    s0 = state_of(win, H.N_KF)
    results = []
    for imu in (imu_oracle, imu_device):
        ws.set_problem(list(range(H.N_KF)), MASK, imu=imu, sb_prior=_sb_prior(win))
        c, g, Hm = ws.evaluate(s0)
        for k in range(H.N_KF):
            m.pose_set(k, win["init"][k]["t"], win["init"][k]["q"])
        final, info = ws.solve(s0)
        results.append((c, g, Hm, final, info))
    (c0, g0, H0, f0, i0), (c1, g1, H1, f1, i1) = results
    scale = max(np.abs(H0).max(), np.abs(g0).max())
    dc, dg, dh = abs(c1 - c0) / abs(c0), np.abs(g1 - g0).max() / scale, np.abs(H1 - H0).max() / scale
    print(f"window [{what}]: d_cost {dc:.3e}  d_gradient {dg:.3e}  d_JtJ {dh:.3e} (relative to the largest entry {scale:.3e}); solves: {i0['termination']} after {i0['iterations']} "
          f"/ {i1['termination']} after {i1['iterations']}, final states differ by {np.abs(f1 - f0).max():.3e}")
    assert dc <= EVAL_BOUND and dg <= EVAL_BOUND and dh <= EVAL_BOUND, (dc, dg, dh)
    assert i1["termination"] == i0["termination"] and i1["iterations"] == i0["iterations"]
    return results


def test_device_records_in_the_window(gpu_ctx, pre, window):
    win, m = window
    device = pre.preintegrate(_window_segments(win))
    for k, p in enumerate(win["pres"]):      # the same samples: the oracle's object and the device's record agree as the fixture's cases do
        o = p["pre"]
        state, jac, cov, _ = _rec(device[k])
        assert state.tobytes() == np.concatenate([o.delta_p, o.delta_q, o.delta_v, [o.sum_dt]]).tobytes()
        assert np.abs(jac - o.jacobian).max() <= 1e-11 * np.abs(o.jacobian).max() and np.abs(cov - o.covariance).max() <= 1e-11 * np.abs(o.covariance).max()
    _compare_in_the_window(gpu_ctx, win, m, [p["pre"] for p in win["pres"]], device, "records of lili_imu_preintegrate against pack_preintegration(oracle)")


def test_python_surface_round_trip(gpu_ctx, window):
    """keyframe_samples -> preintegrate -> WindowSolver: the window's IMU stream as ONE buffer of stamped samples, sliced at the keyframes' stamps"""
    win, m = window
    ba, bg = win["pres"][0]["ba"], win["pres"][0]["bg"]
    true_ba, true_bg = win["kfs"][0]["sb_true"][3:6], win["kfs"][0]["sb_true"][6:9]
    n = int(round((H.N_KF - 1) * H.DT_KF * H.IMU_HZ)) + 3
    stamps = np.arange(n) / H.IMU_HZ
    s = H.imu_between(0.0, stamps[-1], true_ba, true_bg)
    acc, gyr = np.array([x[1] for x in s]), np.array([x[2] for x in s])
    pi = L.ImuPreintegrator(gpu_ctx)
    segs, objs = [], []
    for k in range(1, H.N_KF):
        seg = pi.keyframe_samples(stamps, acc, gyr, stamps[int(round(k * H.DT_KF * H.IMU_HZ))])
        assert seg["dt"].shape[0] == 41 and abs(seg["dt"].sum() - H.DT_KF) < 1e-12
        segs.append(dict(seg, ba=ba, bg=bg))
        o = W.Preintegration(seg["acc0"], seg["gyr0"], ba, bg)
        for j in range(seg["dt"].shape[0]):
            o.push_back(seg["dt"][j], seg["acc"][j], seg["gyr"][j])
        objs.append(o)
    device = pi.preintegrate(segs)
    assert isinstance(device[0], L.api.WindowImu) and len(device) == H.N_KF - 1
    res = _compare_in_the_window(gpu_ctx, win, m, objs, device, "keyframe_samples -> preintegrate -> WindowSolver")
    final, info = res[1][3], res[1][4]
    assert info["successful_steps"] >= 1 and info["final_cost"] < info["initial_cost"]
    for k, kf in enumerate(win["kfs"]):      # the solve with the device's factors pulls every keyframe towards the truth
        assert np.linalg.norm(final[k, 0:3] - kf["t_true"]) < np.linalg.norm(win["init"][k]["t"] - kf["t_true"])
