"""Numpy restatement of the levelled submap descriptors (include/lili_hip.h "levelled submap descriptors"): the frame and the relative placement in
f64 statement by statement, a row's placement as transform_point does it (f64, rounded to f32 once), and a VECTORISED descriptor that is f32-exact — every product
and sum an elementwise f32 operation, the decisions table comparisons, the maximum np.maximum.at — checked bit for bit against place_model.describe's plain loops in
tests/test_place_submap_model_cpu.py.  The referee of tests/test_place_submap_gpu.py."""
import numpy as np

from tests import place_model as PM

F = np.float32


def _norm(q):
    return np.sqrt(((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]) + q[3] * q[3])


def frame(pose, level):
    """F of a LiDAR map pose (p, then q w x y z), 7 doubles"""
    pose = np.asarray(pose, np.float64)
    out = pose.copy()
    if not level:
        return out
    w, x, y, z = pose[3:7] / _norm(pose[3:7])
    r00, r10 = 1.0 - 2.0 * (y * y + z * z), 2.0 * (x * y + w * z)
    h = np.sqrt(r00 * r00 + r10 * r10)
    c, s = (1.0, 0.0) if h < 1e-9 else (r00 / h, r10 / h)
    c = min(1.0, max(-1.0, c))
    qz = np.sqrt((1.0 - c) / 2.0)
    out[3:7] = [np.sqrt((1.0 + c) / 2.0), 0.0, 0.0, -qz if s < 0.0 else qz]      # (s = -0.0 is not < 0: a half turn is (0, 0, 0, +1))
    return out


def _cross(a, b):
    return np.array([a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]])


def relative(frm, pose):
    """(q_rel, t_rel): f' (x) p and f' . (t_k - t_i), f' the unit frame quaternion's conjugate, p the member's unit quaternion"""
    frm, pose = np.asarray(frm, np.float64), np.asarray(pose, np.float64)
    f = frm[3:7] / _norm(frm[3:7])
    a = np.array([f[0], -f[1], -f[2], -f[3]])
    b = pose[3:7] / _norm(pose[3:7])
    q = np.array([((a[0] * b[0] - a[1] * b[1]) - a[2] * b[2]) - a[3] * b[3],
                  ((a[0] * b[1] + a[1] * b[0]) + a[2] * b[3]) - a[3] * b[2],
                  ((a[0] * b[2] + a[2] * b[0]) + a[3] * b[1]) - a[1] * b[3],
                  ((a[0] * b[3] + a[3] * b[0]) + a[1] * b[2]) - a[2] * b[1]])
    v, u = pose[:3] - frm[:3], a[1:]
    uv = _cross(u, v)
    uv = uv + uv
    return q, (v + a[0] * uv) + _cross(u, uv)


def place_row(pts, q, t):
    """transform_point of lili_device_math.h on every row of pts (n, >= 3) f32: (float)((v + w (2 u x v)) + u x (2 u x v) + t), every operation in f64"""
    p = np.asarray(pts, F)[:, :3].astype(np.float64)
    q, t = np.asarray(q, np.float64), np.asarray(t, np.float64)
    vx, vy, vz = p[:, 0], p[:, 1], p[:, 2]
    w, ux, uy, uz = q
    with np.errstate(all="ignore"):
        ax, ay, az = uy * vz - uz * vy, uz * vx - ux * vz, ux * vy - uy * vx
        ax, ay, az = ax + ax, ay + ay, az + az
        cx, cy, cz = uy * az - uz * ay, uz * ax - ux * az, ux * ay - uy * ax
        r = np.stack([((vx + w * ax) + cx) + t[0], ((vy + w * ay) + cy) + t[1], ((vz + w * az) + cz) + t[2]], 1)
        return r.astype(F)


def describe(pts, n_ring=20, n_sector=60, max_radius=80.0, lidar_height=2.0):
    """place_model.describe, vectorised and f32-exact"""
    ring_r2, C, S = PM.tables(n_ring, n_sector, max_radius)
    d = np.zeros((n_sector, n_ring), F)
    pts = np.asarray(pts, F)
    if pts.shape[0] == 0:
        return d
    with np.errstate(all="ignore"):
        x, y, z = pts[:, 0], pts[:, 1], pts[:, 2]
        r2 = x * x + y * y
        keep = np.isfinite(x) & np.isfinite(y) & np.isfinite(z) & ~(r2 > F(max_radius) * F(max_radius))
        x, y, z, r2 = x[keep], y[keep], z[keep], r2[keep]
        ring = (r2[:, None] > ring_r2[None, 1:]).sum(1)
        q = np.where(y >= 0, np.where(x >= 0, 0, 1), np.where(x < 0, 2, 3))
        u = np.choose(q, [x, y, -x, -y])
        v = np.choose(q, [y, -x, -y, x])
        j = ((v[:, None] * C[None, 1:]) >= (u[:, None] * S[None, 1:])).sum(1)
        val = z + F(lidar_height)
    assert r2.dtype == F and val.dtype == F and u.dtype == F and (v[:, None] * C[None, 1:]).dtype == F
    best = np.full(n_sector * n_ring, -np.inf, F)
    np.maximum.at(best, (q * (n_sector // 4) + j) * n_ring + ring, val)
    return np.where(best > -np.inf, best, F(0)).astype(F).reshape(n_sector, n_ring)


def submap_describe(clouds, q_rel, t_rel, **params):
    """the descriptor of the clouds' rows, cloud i placed by (q_rel[i], t_rel[i]); q_rel None or q_rel[i] None: read untransformed"""
    rows = []
    for i, c in enumerate(clouds):
        c = np.asarray(c, F).reshape(-1, np.asarray(c).shape[1] if len(c) else 3)[:, :3]
        rows.append(c if q_rel is None or q_rel[i] is None else place_row(c, q_rel[i], t_rel[i]))
    return describe(np.concatenate(rows) if rows else np.zeros((0, 3), F), **params)


def windows(n, back, fwd):
    """[(first, last)] of every keyframe of an archive of n"""
    return [(max(0, i - back), min(n - 1, i + fwd)) for i in range(n)]


def keys(poses, back, fwd, level, rel=relative, frm=frame):
    """every keyframe's build key: ((member id, identity flag, q_rel bytes, t_rel bytes), ...) from the LiDAR map poses (n, 7).  rel / frm: the functions that give
    the relative placement and the frame (the model's, or the library's own)"""
    out = []
    for i, (a, b) in enumerate(windows(len(poses), back, fwd)):
        f = frm(poses[i], level)
        key = []
        for k in range(a, b + 1):
            if k == i and not level:
                key.append((k, 1, np.zeros(4).tobytes(), np.zeros(3).tobytes()))
            else:
                q, t = rel(f, poses[k])
                key.append((k, 0, np.asarray(q, np.float64).tobytes(), np.asarray(t, np.float64).tobytes()))
        out.append(tuple(key))
    return out


def expected_rebuilds(old_keys, new_keys):
    """the ids lili_place_update builds: no key yet, or another key"""
    return [i for i, k in enumerate(new_keys) if i >= len(old_keys) or old_keys[i] != k]


def archive_describe(clouds, poses, back, fwd, level, rel=relative, frm=frame, **params):
    """every keyframe's submap descriptor; clouds[k] None: the kind is absent"""
    out = []
    for key in keys(poses, back, fwd, level, rel, frm):
        cs, qs, ts = [], [], []
        for k, ident, q, t in key:
            if clouds[k] is None:
                continue
            cs.append(clouds[k])
            qs.append(None if ident else np.frombuffer(q))
            ts.append(None if ident else np.frombuffer(t))
        out.append(submap_describe(cs, qs, ts, **params))
    return out
