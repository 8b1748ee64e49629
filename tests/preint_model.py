"""Helpers of tests/test_imu_preint_cpu.py and tests/test_imu_preint_gpu.py (IMU pre-integration on the device):
  * the cases of tests/golden/ref_preint.npz — recorded inputs and outputs of the reference's own Preintegration.h
    (oracle/_ref/libref_imu.so::ref_preintegrate), written by tests/golden/make_ref_preint_golden.py;
  * plain-Python restatements, explicit scalar sums on Python floats (IEEE doubles, no contraction, no `@`), of
      keyframe_samples   the sample slicing of saveKeyFramesAndFactors, L/src/BackendFusion.cpp:1700-1771 (+ imuHandler's first sample, L:636-662)
      predict            the state propagation of processIMU, L/src/BackendFusion.cpp:815-821 (deltaQ: utils/math_tools.h:125-138;
                         toRotationMatrix and the 3 x 3 products: Eigen 3.3's formulas, sums from left to right).
The sample generator is tests/test_window_cpu.py::_samples.  A seed's cases share ONE stream, _samples(seed, 400): the case of n samples takes its
first n (acc0 / gyr0 = row 0, push_back k = row k + 1), with dt[0] = 0 when n >= 40 — the reference's first sample of a run has dt 0."""
import ctypes as C
import os

import numpy as np

from tests.test_window_cpu import _samples

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "ref_preint.npz")
REF = os.path.join(ROOT, "oracle", "_ref", "libref_imu.so")
SEEDS = (1, 2, 3)
NS = (0, 1, 2, 40, 63, 64, 65, 127, 128, 129, 400)      # the kernel's chunk is 64: 63 / 64 / 65 and 127 / 128 / 129 straddle one and two chunks
N_MAX = 400


def case_inputs(seed_stream, n):
    """(dt (n), acc (n, 3), gyr (n, 3), acc0, gyr0) of the case with n samples from a seed's stream (dt (400), acc (401, 3), gyr (401, 3))."""
    dt, acc, gyr = seed_stream
    d = np.array(dt[:n], np.float64)
    if n >= 40:
        d[0] = 0.0
    return d, np.ascontiguousarray(acc[1:n + 1]), np.ascontiguousarray(gyr[1:n + 1]), acc[0].copy(), gyr[0].copy()


def generate_streams():
    out = {}
    for seed in SEEDS:
        dt, acc, gyr, ba, bg = _samples(seed, N_MAX)
        out[seed] = dict(stream=(dt, acc, gyr), ba=ba, bg=bg)
    return out


def ref_library():
    """oracle/_ref/libref_imu.so, or None where it is not built"""
    if not os.path.exists(REF):
        return None
    lib = C.CDLL(REF)
    lib.ref_preintegrate.restype = C.c_int
    return lib


def ref_preintegrate(lib, dt, acc, gyr, acc0, gyr0, ba, bg):
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    dt, acc, gyr = (np.ascontiguousarray(x, np.float64) for x in (dt, acc, gyr))
    acc0, gyr0, ba, bg = (np.ascontiguousarray(x, np.float64).copy() for x in (acc0, gyr0, ba, bg))
    state, jac, cov = np.zeros(11), np.zeros(225), np.zeros(225)
    assert lib.ref_preintegrate(len(dt), p(dt), p(acc), p(gyr), p(acc0), p(gyr0), p(ba), p(bg), p(state), p(jac), p(cov)) == 0
    return state, jac.reshape(15, 15), cov.reshape(15, 15)


def golden_cases():
    """list of dict(seed, n, dt, acc, gyr, acc0, gyr0, ba, bg, state (11: delta_p, delta_q wxyz, delta_v, sum_dt), jacobian, covariance)"""
    z = np.load(GOLDEN)
    cases, k = [], 0
    for si, seed in enumerate(z["seeds"]):
        stream = (z["dt"][si], z["acc"][si], z["gyr"][si])
        for n in z["ns"]:
            dt, acc, gyr, acc0, gyr0 = case_inputs(stream, int(n))
            cases.append(dict(seed=int(seed), n=int(n), dt=dt, acc=acc, gyr=gyr, acc0=acc0, gyr0=gyr0, ba=z["ba"][si].copy(), bg=z["bg"][si].copy(),
                              state=z["state"][k].copy(), jacobian=z["jacobian"][k].reshape(15, 15).copy(), covariance=z["covariance"][k].reshape(15, 15).copy()))
            k += 1
    return cases


def segment_of(case, **extra):
    d = dict(dt=case["dt"], acc=case["acc"], gyr=case["gyr"], acc0=case["acc0"], gyr0=case["gyr0"], ba=case["ba"], bg=case["bg"])
    d.update(extra)
    return d


# ---------------------------------------------------------------- saveKeyFramesAndFactors' sample slicing, L:1700-1771
def _clamp(a):
    if a[0] > 15.0: a[0] = 15.0
    if a[1] > 15.0: a[1] = 15.0
    if a[2] > 18.0: a[2] = 18.0
    if a[0] < -15.0: a[0] = -15.0
    if a[1] < -15.0: a[1] = -15.0
    if a[2] < -18.0: a[2] = -18.0


def new_kf_state():
    return dict(idx=0, t_cur=-1.0, acc0=[0.0] * 3, gyr0=[0.0] * 3, first=False)


def keyframe_samples(st, stamps, acc, gyr, t_kf):
    """Advances the state dict; returns the rows [(dt, [ax, ay, az], [gx, gy, gz]), ...] processIMU is called with for this keyframe."""
    stamps = [float(v) for v in stamps]
    acc = [[float(v) for v in r] for r in acc]
    gyr = [[float(v) for v in r] for r in gyr]
    n = len(stamps)
    rows = []
    if n > 0 and not st["first"]:                    # imuHandler: acc_0 / gyr_0 = the first message, as it is
        st["first"] = True
        st["acc0"], st["gyr0"] = list(acc[0]), list(gyr[0])
    a, r = [0.0, 0.0, 0.0], [0.0, 0.0, 0.0]
    i = st["idx"]
    t_cur = st["t_cur"]
    if i < n:
        while stamps[i] < t_kf:
            t = stamps[i]
            if t_cur < 0:
                t_cur = t
            dt = t - t_cur
            t_cur = stamps[i]
            a, r = list(acc[i]), list(gyr[i])
            _clamp(a)
            rows.append((dt, list(a), list(r)))
            i += 1
            if i >= n:
                break
        if i < n:
            dt1 = t_kf - t_cur
            dt2 = stamps[i] - t_kf
            w1 = dt2 / (dt1 + dt2)
            w2 = dt1 / (dt1 + dt2)
            a = [w1 * a[k] + w2 * acc[i][k] for k in range(3)]
            _clamp(a)
            r = [w1 * r[k] + w2 * gyr[i][k] for k in range(3)]
            rows.append((dt1, list(a), list(r)))
    if rows:
        st["acc0"], st["gyr0"] = list(rows[-1][1]), list(rows[-1][2])
    st["t_cur"] = float(t_kf)
    st["idx"] = i
    return rows


# ---------------------------------------------------------------- processIMU's state propagation, L:815-821
def _mat_of_quat(w, x, y, z):                        # QuaternionBase::toRotationMatrix, no normalisation
    tx, ty, tz = 2.0 * x, 2.0 * y, 2.0 * z
    twx, twy, twz = tx * w, ty * w, tz * w
    txx, txy, txz = tx * x, ty * x, tz * x
    tyy, tyz, tzz = ty * y, tz * y, tz * z
    return [1.0 - (tyy + tzz), txy - twz, txz + twy,
            txy + twz, 1.0 - (txx + tzz), tyz - twx,
            txz - twy, tyz + twx, 1.0 - (txx + tyy)]


def predict(P0, R0, V0, ba, bg, g, acc0, gyr0, dt, acc, gyr):
    """(P1 (3), R1 (3, 3), V1 (3)) after the samples; R is multiplied on and never re-normalised.  g is the FACTOR's gravity g_vec_ (e.g. (0, 0, -9.805)):
    processIMU subtracts its own g, and g_vec_ = -g (L:807)."""
    P, V = [float(v) for v in P0], [float(v) for v in V0]
    R = [float(v) for v in np.asarray(R0, np.float64).reshape(-1)]
    ba, bg = ([float(v) for v in x] for x in (ba, bg))
    g = [-float(v) for v in g]
    a0, g0 = [float(v) for v in acc0], [float(v) for v in gyr0]
    for k in range(len(dt)):
        h = float(dt[k])
        a1, g1 = [float(v) for v in acc[k]], [float(v) for v in gyr[k]]
        v = [a0[i] - ba[i] for i in range(3)]
        u0 = [((R[3 * i] * v[0] + R[3 * i + 1] * v[1]) + R[3 * i + 2] * v[2]) - g[i] for i in range(3)]
        ug = [0.5 * (g0[i] + g1[i]) - bg[i] for i in range(3)]
        half = [(ug[i] * h) / 2.0 for i in range(3)]                       # deltaQ(un_gyr * dt)
        M = _mat_of_quat(1.0, half[0], half[1], half[2])
        Rn = [0.0] * 9
        for i in range(3):
            for j in range(3):
                s = R[3 * i] * M[j]
                s = s + R[3 * i + 1] * M[3 + j]
                s = s + R[3 * i + 2] * M[6 + j]
                Rn[3 * i + j] = s
        R = Rn
        v = [a1[i] - ba[i] for i in range(3)]
        u1 = [((R[3 * i] * v[0] + R[3 * i + 1] * v[1]) + R[3 * i + 2] * v[2]) - g[i] for i in range(3)]
        hdd = 0.5 * h * h
        for i in range(3):
            ua = 0.5 * (u0[i] + u1[i])
            P[i] = P[i] + (h * V[i] + hdd * ua)
            V[i] = V[i] + h * ua
        a0, g0 = a1, g1
    return np.array(P), np.array(R).reshape(3, 3), np.array(V)
