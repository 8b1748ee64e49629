"""Test harness (not product code): numpy restatement of the odometry node's keyframe hand-over — undistortion (L/src/LidarOdometry.cpp:178-199) with Eigen 3.3's
slerp and q * v, the keyframe rule (L:565-585, 675-676) and computeRelative (L:444-480) — operation for operation in f64, so that fixtures of the reference's own node,
the C helpers and the HIP kernel can be compared with it bit for bit.  The keyword switches of undistort() are the MUTATIONS the tests prove the fixture tells apart."""
import numpy as np

KF_NO, KF_YES, KF_FIRST = 0, 1, 2
CLOUDS = ("edge", "surf", "full")
TOPICS = {"edge": "/laser_cloud_corner_last", "surf": "/laser_cloud_surf_last", "full": "/full_point_cloud"}
TIME_COL = {"livox": 8, "rot": 4}          # float index of `intensity` in a PointXYZINormal (48 B) / PointXYZI (32 B) row
ROW_FLOATS = {"livox": 12, "rot": 8}


def x86_int(i32):
    """(int) of a float as cvttss2si converts it: truncation; NaN and values outside int give INT_MIN."""
    f = np.asarray(i32, np.float32)
    ok = np.isfinite(f) & (f >= np.float32(-2147483648.0)) & (f < np.float32(2147483648.0))
    return np.where(ok, np.trunc(np.where(ok, f, 0)), -2147483648.0).astype(np.int64)


def ratio_of(intensity, clamp=True):
    f = np.asarray(intensity, np.float32)
    line = x86_int(f)
    with np.errstate(invalid="ignore"):
        dt = (f - line.astype(np.float32)).astype(np.float64)        # a FLOAT subtraction, widened afterwards
        r = dt / 0.1
        if clamp:
            r = np.where(r > 1, 1.0, r)                                # no lower bound; NaN passes through
    return r


def slerp_identity(ratio, q):
    """Eigen 3.3 Quaterniond::Identity().slerp(ratio, q), q = (w, x, y, z); returns (n, 4) rows w x y z."""
    w, x, y, z = (float(v) for v in q)
    one = 1.0 - 2.220446049250313e-16
    d = 0.0 * x + 0.0 * y + 0.0 * z + 1.0 * w
    if abs(d) >= one:
        s0, s1 = 1.0 - ratio, ratio + 0.0
    else:
        theta = np.arccos(abs(d))
        st = np.sin(theta)
        s0, s1 = np.sin((1.0 - ratio) * theta) / st, np.sin(ratio * theta) / st
    if d < 0:
        s1 = -s1
    return np.stack([s0 * 1.0 + s1 * w, s0 * 0.0 + s1 * x, s0 * 0.0 + s1 * y, s0 * 0.0 + s1 * z], 1)


def qrot_rows(q, v):
    """Eigen's q * v with one quaternion per row: v + w (2 u x v) + u x (2 u x v)."""
    w, ux, uy, uz = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    vx, vy, vz = v[:, 0], v[:, 1], v[:, 2]
    cx, cy, cz = uy * vz - uz * vy, uz * vx - ux * vz, ux * vy - uy * vx
    cx, cy, cz = cx + cx, cy + cy, cz + cz
    dx, dy, dz = uy * cz - uz * cy, uz * cx - ux * cz, ux * cy - uy * cx
    return np.stack([(vx + cx * w) + dx, (vy + cy * w) + dy, (vz + cz * w) + dz], 1)


def undistort(xyz, intensity, t_rel, q_rel=None, clamp=True, t_f32=False, sum_f32=False):
    """undistortion(cloud, t_rel, q_rel): xyz (n, 3) float32, intensity (n,) float32 -> (n, 3) float32.  q_rel None = (1, 0, 0, 0)."""
    xyz = np.asarray(xyz, np.float32).reshape(-1, 3)
    t = np.asarray(t_rel, np.float64)
    q = np.array([1.0, 0, 0, 0]) if q_rel is None else np.asarray(q_rel, np.float64)
    r = ratio_of(intensity, clamp)
    if t_f32:
        t = t.astype(np.float32).astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        ts = r[:, None] * t[None, :]
        if sum_f32:
            return xyz + ts.astype(np.float32)
        return (qrot_rows(slerp_identity(r, q), xyz.astype(np.float64)) + ts).astype(np.float32)


def qinv(q):
    w, x, y, z = (float(v) for v in q)
    n2 = x * x + y * y + z * z + w * w
    return np.array([w / n2, -x / n2, -y / n2, -z / n2]) if n2 > 0 else np.zeros(4)


def qmul(a, b):
    aw, ax, ay, az = (float(v) for v in a)
    bw, bx, by, bz = (float(v) for v in b)
    return np.array([aw * bw - ax * bx - ay * by - az * bz, aw * bx + ax * bw + ay * bz - az * by,
                     aw * by + ay * bw + az * bx - ax * bz, aw * bz + az * bw + ax * by - ay * bx])


def pose_relative(t_prev, q_prev, t_cur, q_cur):
    qi = qinv(q_prev)
    dv = (np.asarray(t_cur, np.float64) - np.asarray(t_prev, np.float64))[None, :]
    return qrot_rows(qi[None, :], dv)[0], qmul(qi, q_cur)


class Rule:
    """LidarOdometry's keyframe flag, statement for statement."""

    def __init__(self):
        self.kf, self.kf_num, self.n = True, 0, 0
        self.t_last, self.q_last = np.zeros(3), np.array([1.0, 0, 0, 0])

    def step(self, t, q, matched=True):
        if self.n == 0:                               # savePoses + checkInitialization
            self.n = 1
            return KF_FIRST
        if matched:
            t, q = np.asarray(t, np.float64), np.asarray(q, np.float64)
            d = t - self.t_last
            dis = np.sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2])
            with np.errstate(invalid="ignore"):
                ang = 2 * np.arccos(qmul(qinv(self.q_last), q)[0])
            since = self.n - self.kf_num
            if (((dis > 0.2 or ang > 0.1) and since > 1) or since > 2) or self.n <= 1:
                self.kf, self.t_last, self.q_last = True, t.copy(), q.copy()
            else:
                self.kf = False
        self.n += 1
        if self.kf:
            self.kf_num = self.n
        return KF_YES if self.kf else KF_NO


def f32_ulp(mag):
    """one unit in the last place of a float32 of magnitude `mag` (at least the smallest normal's)"""
    return float(np.spacing(np.float32(max(float(mag), 1.1754944e-38))))
