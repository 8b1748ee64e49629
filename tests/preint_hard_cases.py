"""Hard sample streams for the IMU pre-integration (lili_imu_preintegrate, lili_om_amd/csrc/lili_imu.hip), the comparison the device's records
are held to, and a restatement with switches for the faults that comparison has to notice.

Shared by tests/test_preint_hard_cases_cpu.py (the conditions on the inputs, the fixture against the live reference and the oracle, the sensitivity of the
comparison), tests/test_imu_preint_hard_gpu.py and tests/test_imu_preint_gpu.py (the device against the fixtures) and tests/golden/make_ref_preint_golden.py
(which writes tests/golden/ref_preint_hard.npz).

Inputs.  Every stream comes from numpy.random.Generator.uniform / integers with a fixed seed and +, -, x, / alone — no sin, cos, normal — so that every machine
regenerates the same bits; the fixture holds OUTPUTS only (state (11), Jacobian (225), covariance (225) of the reference's own Preintegration.h through
oracle/_ref/libref_imu.so::ref_preintegrate), the exact-zero masks of the two matrices, and a SHA-256 of each case's input bytes, which `cases()` asserts.
A case has n + 1 sample rows: row 0 is the constructor's (acc0, gyr0), row k + 1 is push_back k.  The kernel prepares 64 samples at a time.

Families (each at the smallest n at which its hazard exists):
  rates          rate (9, -6, 30) rad/s + uniform noise of +-RATES_NOISE per axis and sample, dt 5 ms; n = 1, 65, 200.  The un-normalised result quaternion
                 (1, un_gyr dt / 2) * delta_q, which the kernel keeps for Rr, is >= 1 % off unit length in every case (|q| - 1; the constant rate alone gives
                 0.32 % at this dt, the noise amplitude is what carries a sample pair past |un_gyr| = 56.7 rad/s); delta_q.w < 0 at the end of n = 200
  rates_long_dt  the same rates at dt 20 ms, n = 100: the result quaternion is up to 16 % off unit, the Jacobian grows to 2e7 and the covariance to 6e10 (the reference's own numbers), all finite
  long_dt        dt 0.1 s, about 2 rad/s, n = 60
  dt_mixed       dt = m x 10^-e, m in [1, 5), e in 1 .. 6 (1e-6 .. 0.5 s); every 7th dt exactly 0 and samples 64, 65 and the last as well, so samples 0, 63, 64, 65
                 and 128 have dt = 0: F = I, V = 0 on both sides of a chunk boundary; n = 129
  tiny_dt        every dt 1e-6, n = 65: the increments are 1e-12 of the entries they are added to
  bias_large     ba up to +-2, bg up to +-0.5, n = 129
  acc_big        accelerations up to +-60 (neither the header nor the kernel clamps; lili_imu_keyframe_samples does), n = 129
  still          all-zero samples and biases, n = 1, 65: delta_q exactly (1, 0, 0, 0), most entries of both matrices exactly 0
  gravity_only   acc exactly (0, 0, 9.8), gyr 0, biases 0, n = 1, 65: delta_q exactly (1, 0, 0, 0)
  one_axis       six cases, one non-zero component among acc x, y, z, gyr x, y, z (the same value in all three rows), biases 0, n = 2: exact zeros beyond the structural ones
  turns          about 4 rad/s about a fixed axis for 4 s at dt 10 ms, n = 400: delta_q.w changes sign at least twice
  max            dt 2.5 ms, about 1 rad/s, n = 4095 and 4096 (the interface's maximum)

Comparison (`compare`).  State: the reference's bits.  Jacobian and covariance entry by entry: the kernel claims the reference's operation order with only
structurally-zero terms left out, and x + 0 * y = x for finite y, so every entry is expected EQUAL as a number (==: -0 equals +0), and an entry that is exactly 0
in the reference exactly 0 on the device.  Reported per record: the count of unequal entries and the worst difference in units of 2^-53 x the largest reference
entry of the entry's 3 x 3 block (a reordered sum of these lengths sits at tens of such units; one rounding is <= 1).
"""
import hashlib
import os

import numpy as np

from oracle import lo_window as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "ref_preint_hard.npz")
U = 2.0 ** -53
RATES_NOISE = 30.0

# (name, family, n, seed)
SPEC = (
    ("rates_1", "rates", 1, 4), ("rates_65", "rates", 65, 1), ("rates_200", "rates", 200, 1),
    ("rates_long_dt", "rates_long_dt", 100, 1),
    ("long_dt", "long_dt", 60, 1),
    ("dt_mixed", "dt_mixed", 129, 1),
    ("tiny_dt", "tiny_dt", 65, 1),
    ("bias_large", "bias_large", 129, 1),
    ("acc_big", "acc_big", 129, 1),
    ("still_1", "still", 1, 0), ("still_65", "still", 65, 0),
    ("gravity_only_1", "gravity_only", 1, 0), ("gravity_only_65", "gravity_only", 65, 0),
    ("one_axis_ax", "one_axis", 2, 0), ("one_axis_ay", "one_axis", 2, 1), ("one_axis_az", "one_axis", 2, 2),
    ("one_axis_gx", "one_axis", 2, 3), ("one_axis_gy", "one_axis", 2, 4), ("one_axis_gz", "one_axis", 2, 5),
    ("turns", "turns", 400, 1),
    ("max_4095", "max", 4095, 1), ("max_4096", "max", 4096, 2),
)
NAMES = tuple(s[0] for s in SPEC)
FAMILIES = tuple(dict.fromkeys(s[1] for s in SPEC))


def _inputs(family, n, seed):
    rng = np.random.default_rng(7000 + seed)
    z3 = np.zeros(3)
    gravity = np.array([0.0, 0.0, 9.8])
    small_ba, small_bg = lambda: rng.uniform(-0.02, 0.02, 3), lambda: rng.uniform(-0.003, 0.003, 3)
    acc_gentle = lambda: gravity + rng.uniform(-0.5, 0.5, (n + 1, 3))
    if family in ("rates", "rates_long_dt"):
        gyr = np.array([9.0, -6.0, 30.0]) + rng.uniform(-RATES_NOISE, RATES_NOISE, (n + 1, 3))
        return np.full(n, 0.005 if family == "rates" else 0.02), acc_gentle(), gyr, small_ba(), small_bg()
    if family == "long_dt":
        return np.full(n, 0.1), acc_gentle(), np.array([1.2, -0.9, 1.3]) + rng.uniform(-0.3, 0.3, (n + 1, 3)), small_ba(), small_bg()
    if family == "dt_mixed":
        scale = np.array([1e-1, 1e-2, 1e-3, 1e-4, 1e-5, 1e-6])
        dt = rng.uniform(1.0, 5.0, n) * scale[rng.integers(0, 6, n)]
        for k in list(range(0, n, 7)) + [64, 65, n - 1]:
            dt[k] = 0.0
        return dt, acc_gentle(), np.array([0.4, -0.3, 0.6]) + rng.uniform(-0.4, 0.4, (n + 1, 3)), small_ba(), small_bg()
    if family == "tiny_dt":
        return np.full(n, 1e-6), acc_gentle(), np.array([0.4, -0.3, 0.6]) + rng.uniform(-0.4, 0.4, (n + 1, 3)), small_ba(), small_bg()
    if family == "bias_large":
        return np.full(n, 0.005), acc_gentle(), np.array([0.4, -0.3, 0.6]) + rng.uniform(-0.4, 0.4, (n + 1, 3)), rng.uniform(-2.0, 2.0, 3), rng.uniform(-0.5, 0.5, 3)
    if family == "acc_big":
        return np.full(n, 0.005), rng.uniform(-60.0, 60.0, (n + 1, 3)), np.array([0.4, -0.3, 0.6]) + rng.uniform(-0.4, 0.4, (n + 1, 3)), small_ba(), small_bg()
    if family == "still":
        return np.full(n, 0.005), np.zeros((n + 1, 3)), np.zeros((n + 1, 3)), z3, z3
    if family == "gravity_only":
        return np.full(n, 0.005), np.tile(gravity, (n + 1, 1)), np.zeros((n + 1, 3)), z3, z3
    if family == "one_axis":      # seed = which of acc x, y, z, gyr x, y, z
        acc, gyr = np.zeros((n + 1, 3)), np.zeros((n + 1, 3))
        if seed < 3:
            acc[:, seed] = 3.0
        else:
            gyr[:, seed - 3] = 0.7
        return np.full(n, 0.005), acc, gyr, z3, z3
    if family == "turns":
        return np.full(n, 0.01), acc_gentle(), np.array([2.0, -2.0, 2.8]) + rng.uniform(-0.05, 0.05, (n + 1, 3)), small_ba(), small_bg()
    if family == "max":
        return np.full(n, 0.0025), acc_gentle(), np.array([0.5, -0.6, 0.6]) + rng.uniform(-0.2, 0.2, (n + 1, 3)), small_ba(), small_bg()
    raise KeyError(family)


def input_bytes(c):
    return b"".join(np.ascontiguousarray(c[k], "<f8").tobytes() for k in ("dt", "acc", "gyr", "acc0", "gyr0", "ba", "bg"))


def generate():
    """the cases' inputs: list of dict(name, family, n, dt (n), acc (n, 3), gyr (n, 3), acc0, gyr0, ba, bg, sha256)"""
    out = []
    for name, family, n, seed in SPEC:
        dt, acc, gyr, ba, bg = (np.array(a, np.float64) for a in _inputs(family, n, seed))
        c = dict(name=name, family=family, n=n, dt=dt, acc=np.ascontiguousarray(acc[1:]), gyr=np.ascontiguousarray(gyr[1:]), acc0=acc[0].copy(), gyr0=gyr[0].copy(), ba=ba, bg=bg)
        c["sha256"] = hashlib.sha256(input_bytes(c)).hexdigest()
        out.append(c)
    return out


def cases():
    """generate() joined with the fixture: adds state (11: delta_p, delta_q wxyz, delta_v, sum_dt), jacobian, covariance (15 x 15), zero_j, zero_p (bool 15 x 15)"""
    z = np.load(GOLDEN)
    names = [str(s) for s in z["names"]]
    assert names == list(NAMES), names
    out = generate()
    for k, c in enumerate(out):
        assert c["sha256"] == str(z["sha256"][k]), f"{c['name']}: the generator does not give the inputs the fixture was recorded from"
        c.update(state=z["state"][k].copy(), jacobian=z["jacobian"][k].reshape(15, 15).copy(), covariance=z["covariance"][k].reshape(15, 15).copy(),
                 zero_j=z["zero_j"][k].reshape(15, 15).copy(), zero_p=z["zero_p"][k].reshape(15, 15).copy())
    return out


# ---------------------------------------------------------------- the comparison
def block_max(ref):
    """(15, 15): the largest |entry| of the 3 x 3 block an entry lies in"""
    a = np.abs(np.asarray(ref, np.float64)).reshape(5, 3, 5, 3).max(axis=(1, 3))
    return np.repeat(np.repeat(a, 3, axis=0), 3, axis=1)


def _matrix(got, ref):
    got, ref = np.asarray(got, np.float64).reshape(15, 15), np.asarray(ref, np.float64).reshape(15, 15)
    d = np.abs(got - ref)
    bad = ~(got == ref)                                       # (a NaN on either side is unequal)
    with np.errstate(divide="ignore", invalid="ignore"):
        units = np.where(bad, d / (U * block_max(ref)), 0.0)  # a difference in a block whose reference entries are all 0: inf units
    units = np.where(np.isnan(units), np.inf, units)
    at = np.unravel_index(int(np.argmax(units)), units.shape) if bad.any() else None
    return dict(unequal=int(bad.sum()), worst=float(units.max()), at=None if at is None else (int(at[0]), int(at[1])), zeros_lost=int(((ref == 0.0) & ~(got == 0.0)).sum()))


def compare(state, jac, cov, ref):
    """a record against a case of a fixture: dict(state_bits, jacobian, covariance), the latter two dict(unequal, worst [2^-53 x block maximum], at, zeros_lost)"""
    state = np.asarray(state, np.float64)
    differ = [i for i in range(11) if state[i].tobytes() != ref["state"][i].tobytes()]
    return dict(state_bits=differ, jacobian=_matrix(jac, ref["jacobian"]), covariance=_matrix(cov, ref["covariance"]))


def line(label, r):
    j, p = r["jacobian"], r["covariance"]
    return (f"{label:>18}: state {'bits equal' if not r['state_bits'] else 'BITS DIFFER at ' + str(r['state_bits'])}  jacobian {j['unequal']:3d} unequal, worst {j['worst']:.3g} u"
            f"{'' if j['at'] is None else ' at ' + str(j['at'])}  covariance {p['unequal']:3d} unequal, worst {p['worst']:.3g} u{'' if p['at'] is None else ' at ' + str(p['at'])}")


def equal(r):
    """what the device is held to: the state's bits, every entry of both matrices equal as a number, every exact zero of the reference an exact zero"""
    return not r["state_bits"] and all(r[m]["unequal"] == 0 and r[m]["zeros_lost"] == 0 for m in ("jacobian", "covariance"))


def old_measure(jac, cov, ref):
    """what tests/test_imu_preint_gpu.py asserted before: the largest difference over the largest entry, bound 1e-11"""
    return max(np.abs(jac - ref["jacobian"]).max() / np.abs(ref["jacobian"]).max(), np.abs(cov - ref["covariance"]).max() / np.abs(ref["covariance"]).max())


# ---------------------------------------------------------------- restatement in the reference's operation order, with switches for faults
MUTANTS = ("gyr_w_removed", "gyr_w_doubled", "acc_w_removed", "rr_normalised", "f012_sixth", "v09_zeroed", "v69_zeroed", "f312_plus_dt")


def _mm(a, b):
    """textbook product: every entry is the sum over k in ascending order, no fused operation (numpy's `@` may reorder or fuse)"""
    s = a[:, 0:1] * b[0:1, :]
    for k in range(1, a.shape[1]):
        s = s + a[:, k:k + 1] * b[k:k + 1, :]
    return s


def restate(c, mutant=None, snapshots=()):
    """Preintegration.h:27-173 as it is written there, dense, every product a textbook loop: (state (11), jacobian, covariance) after the case's samples;
    with `snapshots` (sample counts) a dict n -> that triple after n samples instead.  mutant: one of MUTANTS."""
    assert mutant is None or mutant in MUTANTS
    acc_n, gyr_n, acc_w, gyr_w = 0.00059, 0.000061, 0.000011, 0.000001
    nz = np.zeros(18)
    nz[0:3] = nz[6:9] = acc_n * acc_n
    nz[3:6] = nz[9:12] = gyr_n * gyr_n
    nz[12:15] = 0.0 if mutant == "acc_w_removed" else acc_w * acc_w
    nz[15:18] = 0.0 if mutant == "gyr_w_removed" else (gyr_w * gyr_w) * (2.0 if mutant == "gyr_w_doubled" else 1.0)
    ba, bg = c["ba"], c["bg"]
    acc0, gyr0 = c["acc0"], c["gyr0"]
    dp, dq, dv, sum_dt = np.zeros(3), np.array([1.0, 0.0, 0.0, 0.0]), np.zeros(3), 0.0
    J, P, I3 = np.eye(15), 0.0001 * np.eye(15), np.eye(3)
    c6 = 1.0 / 6.0 if mutant == "f012_sixth" else 0.1667
    out = {}

    def result():
        return np.concatenate([dp, dq, dv, [sum_dt]]), J.copy(), P.copy()

    if 0 in snapshots:
        out[0] = result()
    for k in range(c["n"]):
        dt, acc1, gyr1 = float(c["dt"][k]), c["acc"][k], c["gyr"][k]
        un_acc_0 = W.qrot(dq, acc0 - ba)
        un_gyr = 0.5 * (gyr0 + gyr1) - bg
        rq = W.qmul(dq, np.array([1.0, un_gyr[0] * dt / 2, un_gyr[1] * dt / 2, un_gyr[2] * dt / 2]))
        un_acc_1 = W.qrot(rq, acc1 - ba)
        un_acc = 0.5 * (un_acc_0 + un_acc_1)
        rp = dp + dv * dt + 0.5 * un_acc * dt * dt
        rv = dv + un_acc * dt
        Rw, A0, A1 = W.skew(un_gyr), W.skew(acc0 - ba), W.skew(acc1 - ba)
        Rd, Rr = W.qmat(dq), W.qmat(W.qnormalized(rq) if mutant == "rr_normalised" else rq)
        IW = I3 - Rw * dt
        F = np.zeros((15, 15))
        F[0:3, 0:3] = I3
        F[0:3, 3:6] = _mm(-0.25 * Rd, A0) * dt * dt + _mm(_mm(-0.25 * Rr, A1), IW) * dt * dt
        F[0:3, 6:9] = I3 * dt
        F[0:3, 9:12] = -0.25 * (Rd + Rr) * dt * dt
        F[0:3, 12:15] = _mm(-c6 * Rr, A1) * dt * dt * -dt
        F[3:6, 3:6] = IW
        F[3:6, 12:15] = I3 * dt if mutant == "f312_plus_dt" else -I3 * dt
        F[6:9, 3:6] = _mm(-0.5 * Rd, A0) * dt + _mm(_mm(-0.5 * Rr, A1), IW) * dt
        F[6:9, 6:9] = I3
        F[6:9, 9:12] = -0.5 * (Rd + Rr) * dt
        F[6:9, 12:15] = _mm(-0.5 * Rr, A1) * dt * -dt
        F[9:12, 9:12] = I3
        F[12:15, 12:15] = I3
        V = np.zeros((15, 18))
        V[0:3, 0:3] = 0.5 * Rd * dt * dt
        V[0:3, 3:6] = _mm(-0.25 * Rr, A1) * dt * dt * 0.5 * dt
        V[0:3, 6:9] = 0.5 * Rr * dt * dt
        V[0:3, 9:12] = 0.0 if mutant == "v09_zeroed" else V[0:3, 3:6]
        V[3:6, 3:6] = 0.5 * I3 * dt
        V[3:6, 9:12] = 0.5 * I3 * dt
        V[6:9, 0:3] = 0.5 * Rd * dt
        V[6:9, 3:6] = _mm(0.5 * -Rr, A1) * dt * 0.5 * dt
        V[6:9, 6:9] = 0.5 * Rr * dt
        V[6:9, 9:12] = 0.0 if mutant == "v69_zeroed" else V[6:9, 3:6]
        V[9:12, 12:15] = I3 * dt
        V[12:15, 15:18] = I3 * dt
        J = _mm(F, J)
        P = _mm(_mm(F, P), F.T) + _mm(V * nz[None, :], V.T)      # (V noise)(i, c) = V(i, c) n_c: the other terms of that sum are zeros
        dp, dq, dv = rp, W.qnormalized(rq), rv
        sum_dt += dt
        acc0, gyr0 = acc1, gyr1
        if k + 1 in snapshots:
            out[k + 1] = result()
    return out if snapshots else result()


def result_quaternions(c):
    """(n, 4) the un-normalised result quaternion of every sample, and (n + 1, 4) delta_q before every sample and after the last — what the families' properties speak of"""
    dq, gyr0 = np.array([1.0, 0.0, 0.0, 0.0]), c["gyr0"]
    rqs, dqs = [], [dq]
    for k in range(c["n"]):
        dt = float(c["dt"][k])
        un_gyr = 0.5 * (gyr0 + c["gyr"][k]) - c["bg"]
        rq = W.qmul(dq, np.array([1.0, un_gyr[0] * dt / 2, un_gyr[1] * dt / 2, un_gyr[2] * dt / 2]))
        dq, gyr0 = W.qnormalized(rq), c["gyr"][k]
        rqs.append(rq); dqs.append(dq)
    return np.array(rqs).reshape(-1, 4), np.array(dqs)
