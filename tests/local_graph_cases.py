"""Cases of the local pose graph (lili_local_graph*), generated from fixed seeds: chains for the solve, sample buffers for the IMU walk.
The seeds were chosen on the CPU with tests/local_graph_model.py so that each family reaches the branches named next to it and no decision of the loop sits
on a threshold (tests/test_local_graph_model_cpu.py asserts both for every case)."""
import numpy as np

from oracle.lo_window import qmul, qinv, qrot

MAX_FRAMES = 16
MEAS_NOISE = (0.01, 0.005)      # m, rad on every measurement but family e's: the minimum has a cost, so the function tolerance can end a solve


def _rotvec_quat(v):
    a = float(np.linalg.norm(v))
    if a == 0.0:
        return np.array([1.0, 0.0, 0.0, 0.0])
    return np.concatenate([[np.cos(a / 2.0)], np.sin(a / 2.0) * np.asarray(v) / a])


def _perturb(pose, rng, sig_p, sig_r):
    q = qmul(pose[3:7], _rotvec_quat(rng.normal(size=3) * sig_r / np.sqrt(3.0)))
    return np.concatenate([pose[0:3] + rng.normal(size=3) * sig_p / np.sqrt(3.0), q / np.linalg.norm(q)])


def chain_case(name, seed, n, noise_p, noise_r, meas_noise=MEAS_NOISE, options=None, expect=None):
    """Truth: n + 2 poses, steps of about 0.5 m / 0.05 rad.  Anchors = the two ends; measurements = the true relative poses, perturbed by meas_noise;
    initial state = the truth perturbed by (noise_p m, noise_r rad)."""
    rng = np.random.default_rng(seed)
    start = np.concatenate([rng.uniform(-20, 20, 3), _rotvec_quat(rng.normal(size=3))])
    truth = [start]
    for _ in range(n + 1):
        a = truth[-1]
        dq = _rotvec_quat(0.05 * (np.array([0.0, 0.0, 1.0]) + 0.3 * rng.normal(size=3)))
        dp = 0.5 * (np.array([1.0, 0.0, 0.0]) + 0.2 * rng.normal(size=3))
        q = qmul(a[3:7], dq)
        truth.append(np.concatenate([a[0:3] + qrot(a[3:7], dp), q / np.linalg.norm(q)]))
    meas = []
    for k in range(n + 1):
        a, b = truth[k], truth[k + 1]
        m = np.concatenate([qrot(qinv(a[3:7]), b[0:3] - a[0:3]), qmul(qinv(a[3:7]), b[3:7])])
        if meas_noise is not None:
            m = _perturb(m, rng, *meas_noise)
        meas.append(m)
    x0 = np.array([_perturb(truth[k + 1], rng, noise_p, noise_r) if (noise_p or noise_r) else truth[k + 1] for k in range(n)], np.float64).reshape(n, 7)
    return dict(name=name, n=n, left=truth[0], right=truth[-1], meas=np.array(meas), x0=x0, options=dict(options or {}), expect=dict(expect or {}))


# expect: termination, iterations, and `cases` = the dogleg case of every logged candidate where the family fixes it
SOLVE_SPECS = [
    dict(name="a1", seed=101, n=1, noise_p=0.02, noise_r=0.01),
    dict(name="a2", seed=102, n=2, noise_p=0.02, noise_r=0.01),
    dict(name="b", seed=213, n=4, noise_p=0.5, noise_r=0.3, options=dict(initial_radius=0.1)),
    dict(name="c", seed=389, n=8, noise_p=3.0, noise_r=2.5, options=dict(initial_radius=1.0)),
    dict(name="d", seed=401, n=16, noise_p=2.0, noise_r=1.5),
    dict(name="e", seed=501, n=3, noise_p=0.0, noise_r=0.0, meas_noise=None),
    dict(name="f", seed=601, n=0, noise_p=0.0, noise_r=0.0),
    dict(name="g", seed=701, n=MAX_FRAMES, noise_p=0.05, noise_r=0.02),
]


def solve_cases():
    return [chain_case(**s) for s in SOLVE_SPECS]


def hard_states(case, seed=9):
    """states with rotation errors up to 3 rad around a case's initial state, and quaternions off the unit sphere by 1e-3 (the walk hands such ones over)"""
    rng = np.random.default_rng(seed)
    out = []
    for ang in (0.5, 1.5, 3.0):
        x = np.array([_perturb(p, rng, 1.0, 0.0) for p in case["x0"]]).reshape(-1, 7)
        for k in range(x.shape[0]):
            ax = rng.normal(size=3)
            x[k, 3:7] = qmul(x[k, 3:7], _rotvec_quat(ang * ax / np.linalg.norm(ax))) * (1.0 + 1e-3 * rng.normal())
        out.append(x)
    return out


# ---------------------------------------------------------------- the walk
def _imu_buffer(rng, t0, t1, rate, acc_amp=2.0, gyr_amp=0.3, jitter=0.0):
    n = int(round((t1 - t0) * rate)) + 1
    st = t0 + np.arange(n) / rate
    if jitter:
        st = st + rng.uniform(-jitter, jitter, n) / rate
    ph = rng.uniform(0, 2 * np.pi, 6)
    acc = np.stack([acc_amp * np.sin(3.0 * st + ph[i]) for i in range(3)], 1) + np.array([0.0, 0.0, 9.8]) + 0.05 * rng.normal(size=(n, 3))
    gyr = np.stack([gyr_amp * np.sin(2.0 * st + ph[3 + i]) for i in range(3)], 1) + 0.005 * rng.normal(size=(n, 3))
    return st, acc, gyr


def _walk_case(name, seed, n, rate=200.0, scan_dt=0.1, R0=None, f32_positions=False, **kw):
    rng = np.random.default_rng(seed)
    t_first = 100.0 + 0.0137
    T = t_first + scan_dt * np.arange(n + 2)
    st, acc, gyr = _imu_buffer(rng, 100.0 - 0.05, T[-1] + 0.05, rate, **kw)
    ii0 = int(np.searchsorted(st, T[0], side="left")) - 1        # imu_idx_in_kf: the last sample in front of the left keyframe's stamp
    if R0 is None:
        from oracle.lo_window import qmat
        R0 = qmat(_rotvec_quat(rng.normal(size=3)))
    left = np.concatenate([rng.uniform(-50, 50, 3), _rotvec_quat(rng.normal(size=3))])
    return dict(name=name, n=n, stamps=st, acc=acc, gyr=gyr, ii0=ii0, T=T, P0=left[0:3] + 0.01 * rng.normal(size=3), R0=np.array(R0, np.float64), V0=rng.normal(size=3),
                g=np.array([0.0, 0.0, 9.805]), left=left, f32_positions=f32_positions)


def walk_cases():
    from oracle.lo_window import qmat
    out = [_walk_case("200hz_n2", 11, 2), _walk_case("200hz_n0", 12, 0), _walk_case("200hz_n5_jitter", 13, 5, jitter=0.3),
           _walk_case("200hz_n16", 14, MAX_FRAMES), _walk_case("f32_positions", 15, 3, f32_positions=True)]
    # an interval that holds no sample: 10 Hz samples under 0.04 s scans
    out.append(_walk_case("empty_interval", 21, 4, rate=10.0, scan_dt=0.04))
    # a sample stamped exactly at a scan stamp (the comparison is a strict <)
    c = _walk_case("sample_at_scan_stamp", 22, 3)
    for f in (1, 2, 4):
        c["stamps"][int(np.searchsorted(c["stamps"], c["T"][f]))] = c["T"][f]
    out.append(c)
    # accelerations beyond the clamps, every axis and sign, also at the (unclamped) opening interpolation of a frame and the (clamped) one of the closing interval
    c = _walk_case("clamps", 23, 3)
    k = 0
    for f in range(4):
        i0 = int(np.searchsorted(c["stamps"], c["T"][f], side="left")) - 1
        for j in (i0, i0 + 1, i0 + 5, i0 + 6, i0 + 11, i0 + 12):
            c["acc"][j, k % 3] = (25.0 + k) * (1.0 if (k // 3) % 2 == 0 else -1.0)
            k += 1
    out.append(c)
    # a start rotation that is not orthonormal to 1e-3, and near half turns (the other branches of the matrix-to-quaternion conversion)
    rng = np.random.default_rng(24)
    out.append(_walk_case("r0_not_orthonormal", 24, 3, R0=qmat(_rotvec_quat(rng.normal(size=3))) + 1e-3 * rng.normal(size=(3, 3))))
    for i, axis in enumerate(np.eye(3)):
        out.append(_walk_case(f"r0_half_turn_{'xyz'[i]}", 25 + i, 2, R0=qmat(_rotvec_quat((np.pi - 1e-3) * (axis + 0.05 * rng.normal(size=3))))))
    # large rates: the un-normalised deltaQ matters
    out.append(_walk_case("rates_3rad_s", 31, 3, gyr_amp=3.0))
    # more samples than the kernel stages in LDS: 2 kHz
    out.append(_walk_case("2khz_n3", 32, 3, rate=2000.0))
    return out


def walk_kwargs(c):
    return dict(stamps=c["stamps"], acc=c["acc"], gyr=c["gyr"], ii0=c["ii0"], T=c["T"], P0=c["P0"], R0=c["R0"], V0=c["V0"], g=c["g"], left=c["left"], f32_positions=c["f32_positions"])
