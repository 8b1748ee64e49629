"""IMU pre-integration, the parts that need no GPU:
  * tests/golden/ref_preint.npz is what the reference's own header gives now (oracle/_ref/libref_imu.so, where it is built) and what the oracle's
    restatement gives within the tolerances tests/test_window_cpu.py applies between the two (state 1e-13, Jacobian / covariance 1e-11 of the largest entry:
    numpy's `@` sums in another order; per 3 x 3 block and at 5e-14 on the hard streams in tests/test_preint_hard_cases_cpu.py).  That tolerance is the
    ORACLE's: the device is held to equality entry by entry (tests/preint_hard_cases.py::compare, tests/test_imu_preint_gpu.py);
  * lili_imu_keyframe_samples against the plain-float restatement of L/src/BackendFusion.cpp:1700-1771 (tests/preint_model.py): bit for bit — the
    arithmetic is a handful of IEEE operations in a fixed order;
  * the new structs' sizes and offsets against the header compiled as plain C."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import lili_om_amd as L
from oracle import lo_window as W
from tests import preint_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def cases():
    return M.golden_cases()


def test_fixture_covers_the_cases(cases):
    assert [(c["seed"], c["n"]) for c in cases] == [(s, n) for s in M.SEEDS for n in M.NS]
    assert os.path.getsize(M.GOLDEN) < 200 * 1000
    for c in cases:
        assert c["dt"].shape == (c["n"],) and c["acc"].shape == (c["n"], 3) and c["gyr"].shape == (c["n"], 3)
        if c["n"] >= 40:
            assert c["dt"][0] == 0.0
        if c["n"] == 0:                      # the constructor's state
            assert np.array_equal(c["state"], [0, 0, 0, 1, 0, 0, 0, 0, 0, 0, 0])
            assert np.array_equal(c["jacobian"], np.eye(15)) and np.array_equal(c["covariance"], 0.0001 * np.eye(15))
        else:
            assert np.linalg.eigvalsh(0.5 * (c["covariance"] + c["covariance"].T)).min() > 0


def test_fixture_equals_the_live_reference(cases):
    lib = M.ref_library()
    if lib is None:
        pytest.skip("oracle/_ref/libref_imu.so not built (needs the reference's sources: oracle/refshim/Makefile)")
    streams = M.generate_streams()
    for c in cases:
        dt, acc, gyr, acc0, gyr0 = M.case_inputs(streams[c["seed"]]["stream"], c["n"])       # the generator gives the recorded inputs ...
        for a, b in ((dt, c["dt"]), (acc, c["acc"]), (gyr, c["gyr"]), (acc0, c["acc0"]), (gyr0, c["gyr0"]), (streams[c["seed"]]["ba"], c["ba"]), (streams[c["seed"]]["bg"], c["bg"])):
            assert np.allclose(a, b, rtol=0, atol=1e-12)      # (sin / cos of the generator may differ in the last bit between C libraries)
        state, jac, cov = M.ref_preintegrate(lib, c["dt"], c["acc"], c["gyr"], c["acc0"], c["gyr0"], c["ba"], c["bg"])      # ... and the reference the recorded outputs
        assert state.tobytes() == c["state"].tobytes(), (c["seed"], c["n"])
        assert jac.tobytes() == c["jacobian"].tobytes() and cov.tobytes() == c["covariance"].tobytes(), (c["seed"], c["n"])


def test_fixture_equals_the_oracle_restatement(cases):
    worst = [0.0, 0.0, 0.0]
    for c in cases:
        pre = W.Preintegration(c["acc0"], c["gyr0"], c["ba"], c["bg"])
        for k in range(c["n"]):
            pre.push_back(c["dt"][k], c["acc"][k], c["gyr"][k])
        mine = np.concatenate([pre.delta_p, pre.delta_q, pre.delta_v, [pre.sum_dt]])
        worst[0] = max(worst[0], np.abs(mine - c["state"]).max())
        worst[1] = max(worst[1], np.abs(pre.jacobian - c["jacobian"]).max() / np.abs(c["jacobian"]).max())
        worst[2] = max(worst[2], np.abs(pre.covariance - c["covariance"]).max() / np.abs(c["covariance"]).max())
        assert np.abs(mine - c["state"]).max() < 1e-13, (c["seed"], c["n"])
        assert np.abs(pre.jacobian - c["jacobian"]).max() <= 1e-11 * np.abs(c["jacobian"]).max(), (c["seed"], c["n"])
        assert np.abs(pre.covariance - c["covariance"]).max() <= 1e-11 * np.abs(c["covariance"]).max(), (c["seed"], c["n"])
    print(f"oracle against the fixture: state {worst[0]:.3e}, jacobian {worst[1]:.3e}, covariance {worst[2]:.3e}")


# ---------------------------------------------------------------- lili_imu_keyframe_samples
def _buffer(seed=7, n=60, hz=200.0, t0=100.0):
    rng = np.random.default_rng(seed)
    stamps = t0 + np.arange(n) / hz + rng.uniform(-4e-4, 4e-4, n)
    acc = rng.normal(0, 3.0, (n, 3)) + np.array([0.0, 0.0, 9.8])
    gyr = rng.normal(0, 0.3, (n, 3))
    return stamps, acc, gyr


def _same(rows, seg):
    assert len(rows) == seg["dt"].shape[0]
    for k, (dt, a, g) in enumerate(rows):
        assert np.float64(dt).tobytes() == seg["dt"][k].tobytes(), k
        assert np.array(a).tobytes() == seg["acc"][k].tobytes() and np.array(g).tobytes() == seg["gyr"][k].tobytes(), k


def _state_same(st, pi):
    assert st["idx"] == pi.state.idx and np.float64(st["t_cur"]).tobytes() == np.float64(pi.state.t_cur).tobytes()
    assert np.array(st["acc0"]).tobytes() == np.array(pi.state.acc0[:]).tobytes() and np.array(st["gyr0"]).tobytes() == np.array(pi.state.gyr0[:]).tobytes()


def _both(stamps, acc, gyr, t_kfs):
    st, pi = M.new_kf_state(), L.ImuPreintegrator()
    out = []
    for t_kf in t_kfs:
        acc0 = list(st["acc0"]) if st["first"] else [float(v) for v in acc[0]]
        gyr0 = list(st["gyr0"]) if st["first"] else [float(v) for v in gyr[0]]
        rows = M.keyframe_samples(st, stamps, acc, gyr, t_kf)
        seg = pi.keyframe_samples(stamps, acc, gyr, t_kf)
        _same(rows, seg)
        _state_same(st, pi)
        assert np.array(acc0).tobytes() == seg["acc0"].tobytes() and np.array(gyr0).tobytes() == seg["gyr0"].tobytes()      # the segment's constructor pair
        out.append((rows, seg))
    return out, st, pi


def test_keyframe_samples_two_keyframes_share_the_state():
    stamps, acc, gyr = _buffer()
    out, st, pi = _both(stamps, acc, gyr, [stamps[20] + 0.0011, stamps[41] + 0.0027])
    (r0, s0), (r1, s1) = out
    assert len(r0) == 22 and len(r1) == 22              # 21 consumed + the boundary sample; then samples 21 .. 41 + boundary
    assert s0["dt"][0] == 0.0 and s1["dt"][0] > 0.0     # the first dt of a run is 0; the second segment starts from t_kf of the first
    assert np.float64(s1["dt"][0]).tobytes() == np.float64(stamps[21] - (stamps[20] + 0.0011)).tobytes()
    assert st["idx"] == 42 and s1["acc0"].tobytes() == s0["acc"][-1].tobytes() and s1["gyr0"].tobytes() == s0["gyr"][-1].tobytes()


def test_keyframe_samples_no_sample_before_the_keyframe():
    stamps, acc, gyr = _buffer()
    out, st, pi = _both(stamps, acc, gyr, [stamps[0] - 0.01])
    rows, seg = out[0]
    # nothing consumed: one boundary sample interpolated from zeros (dx .. rz start at 0, L:1700) over dt1 = t_kf - (-1): the reference's arithmetic, kept
    assert len(rows) == 1 and st["idx"] == 0 and seg["dt"][0] == (stamps[0] - 0.01) + 1.0
    out, st, pi = _both(stamps, acc, gyr, [stamps[10] + 0.001, stamps[10] + 0.002])      # second keyframe before the next sample
    assert len(out[1][0]) == 1 and st["idx"] == 11


def test_keyframe_samples_sample_exactly_at_the_keyframe():
    stamps, acc, gyr = _buffer()
    out, st, pi = _both(stamps, acc, gyr, [float(stamps[30])])
    rows, seg = out[0]
    assert len(rows) == 31 and st["idx"] == 30          # stamp < t_kf is strict: sample 30 is the boundary sample, with dt2 = 0 -> w1 = 0, w2 = 1
    assert seg["acc"][-1].tobytes() == np.clip(acc[30], [-15, -15, -18], [15, 15, 18]).tobytes() and seg["gyr"][-1].tobytes() == gyr[30].tobytes()


def test_keyframe_samples_buffer_ends_before_the_keyframe():
    stamps, acc, gyr = _buffer(n=25)
    out, st, pi = _both(stamps, acc, gyr, [stamps[-1] + 0.5, stamps[-1] + 0.7])
    assert len(out[0][0]) == 25 and st["idx"] == 25     # every sample consumed, no boundary sample
    assert len(out[1][0]) == 0 and st["t_cur"] == stamps[-1] + 0.7


def test_keyframe_samples_clamps_every_axis_and_sign():
    stamps, acc, gyr = _buffer(n=16)
    big = [(0, 15.5), (0, -15.5), (1, 17.0), (1, -17.0), (2, 18.5), (2, -18.5)]
    for k, (ax, v) in enumerate(big):
        acc[2 + k] = [1.0, -2.0, 9.0]
        acc[2 + k, ax] = v
    acc[10] = [40.0, -40.0, 40.0]                      # the boundary sample: interpolated, then clamped again
    acc[9] = [14.9, -14.9, 17.9]
    out, st, pi = _both(stamps, acc, gyr, [0.25 * stamps[9] + 0.75 * stamps[10]])
    seg = out[0][1]
    lim = np.array([15.0, 15.0, 18.0])
    for k, (ax, v) in enumerate(big):
        assert seg["acc"][2 + k, ax] == np.sign(v) * lim[ax]
    assert np.array_equal(seg["acc"][-1], [15.0, -15.0, 18.0]) and len(out[0][0]) == 11
    assert (np.abs(seg["acc"]) <= lim).all()


def test_keyframe_samples_cap_one_too_small():
    stamps, acc, gyr = _buffer()
    pi = L.ImuPreintegrator()
    pi.keyframe_samples(stamps, acc, gyr, stamps[5] + 0.001)
    before = bytes(pi.state)
    t_kf = stamps[20] + 0.001                           # 15 samples + the boundary sample
    dt_o, a_o, g_o = np.full(15, 7.0), np.full((15, 3), 7.0), np.full((15, 3), 7.0)
    n_out = C.c_size_t(99)
    p = lambda a: C.c_void_p(a.ctypes.data)
    rc = pi.lib.lili_imu_keyframe_samples(C.byref(pi.state), p(stamps), p(acc), p(gyr), len(stamps), float(t_kf), p(dt_o), p(a_o), p(g_o), 15, C.byref(n_out))
    assert rc == -1 and bytes(pi.state) == before and n_out.value == 99
    assert (dt_o == 7.0).all() and (a_o == 7.0).all() and (g_o == 7.0).all()
    with pytest.raises(L.LiliError):
        pi.keyframe_samples(stamps, acc, gyr, t_kf, cap=15)
    assert bytes(pi.state) == before
    assert pi.keyframe_samples(stamps, acc, gyr, t_kf, cap=16)["dt"].shape[0] == 16


def test_new_structs_match_the_header(tmp_path):
    pairs = [("lili_imu_segment", L.api.ImuSegment), ("lili_imu_prediction", L.api.ImuPrediction), ("lili_imu_kf_state", L.api.ImuKfState), ("lili_window_imu", L.api.WindowImu)]
    lines, expect = [], []
    for cname, T in pairs:
        lines.append(f'printf("%zu\\n", sizeof({cname}));')
        expect.append(C.sizeof(T))
        for fname, _ in T._fields_:
            lines.append(f'printf("%zu\\n", offsetof({cname}, {fname}));')
            expect.append(getattr(T, fname).offset)
    lines.append('printf("%d\\n%d\\n", LILI_IMU_MAX_SAMPLES, LILI_IMU_MAX_SEGMENTS);')
    expect += [L.api.IMU_MAX_SAMPLES, L.api.IMU_MAX_SEGMENTS]
    src = tmp_path / "lay_imu.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "lili_hip.h"\nint main(void){' + "".join(lines) + "return 0;}")
    exe = tmp_path / "lay_imu"
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    assert got == expect, [(i, a, b) for i, (a, b) in enumerate(zip(got, expect)) if a != b]
    lib = L.load_library()
    assert hasattr(lib, "lili_imu_preintegrate") and hasattr(lib, "lili_imu_keyframe_samples")
