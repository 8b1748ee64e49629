"""Inputs shared by tests/test_place_submap_model_cpu.py and tests/test_place_submap_gpu.py: the 5 000-row hard cloud of tests/test_place_gpu.py, rebuilt here, and the
wedge scene — a street driven down and back by a sensor that sees 81.7 x 25.1 degrees, pitched down, with an odometry that is 25 m and 20 degrees off on the way back."""
import math

import numpy as np

from tests import place_model as PM
from tests import place_submap_model as SM

F = np.float32


def _r2(x, y):
    x, y = F(x), F(y)
    return F(F(x * x) + F(y * y))


def hard_cloud(n_ring, n_sector, max_radius, lidar_height, rng, n=5000):
    """5 000 rows (x, y, z, aux) with every edge the descriptor's definition names (tests/test_place_gpu.py's _hard_cloud, statement by statement)"""
    ring_r2, _, _ = PM.tables(n_ring, n_sector, max_radius)
    R = F(max_radius)
    rows = []
    for r in (0.5, 3.0, 17.25, 41.0, 63.5):
        for x, y in ((r, 0), (0, r), (-r, 0), (0, -r), (r, r), (-r, r), (-r, -r), (r, -r), (r, -0.0), (-0.0, r)):
            rows.append([x, y, rng.uniform(-1, 5)])
    for k in range(1, n_ring):
        b = F(F(R * F(k)) / F(n_ring))
        assert _r2(b, 0) == ring_r2[k]
        rows += [[b, 0.0, 1.0 + 0.1 * k], [0.0, -b, 2.0 + 0.1 * k], [np.nextafter(b, F(np.inf)), 0.0, 3.0], [-np.nextafter(b, F(0)), 0.0, 0.5]]
    rows += [[0.0, 0.0, 4.0], [0.0, 0.0, -0.5], [-0.0, -0.0, 1.0]]
    max_r2 = F(R * R)
    found = {}
    for target, x in ((np.nextafter(max_r2, F(np.inf)), R), (np.nextafter(max_r2, F(0)), np.nextafter(R, F(0))), (max_r2, R)):
        for y in np.arange(0, 0.2, 1e-4, dtype=np.float64):
            if _r2(x, y) == target:
                found[float(target)] = (float(x), float(F(y)))
                break
    assert len(found) == 3, found
    for x, y in found.values():
        rows += [[x, y, 9.0], [-y, x, 9.5]]
    rows += [[np.nan, 1, 1], [1, np.nan, 1], [1, 1, np.nan], [np.inf, 1, 1], [1, -np.inf, 1], [1, 1, np.inf], [1, 1, -np.inf]]
    for _ in range(40):
        a, r = rng.uniform(0, math.pi), rng.uniform(0.93, 0.96) * max_radius
        rows.append([r * math.cos(a), r * math.sin(a), -lidar_height - rng.uniform(0.5, 4)])
    a0, r0 = math.radians(33.0), 0.41 * max_radius
    for _ in range(600):
        rows.append([r0 * math.cos(a0) + rng.uniform(-0.05, 0.05), r0 * math.sin(a0) + rng.uniform(-0.05, 0.05), rng.uniform(-3, 7)])
    rows.append([0.985 * max_radius * math.cos(math.radians(200.5)), 0.985 * max_radius * math.sin(math.radians(200.5)), 6.25])
    while len(rows) < n:
        a, r = rng.uniform(0, 2 * math.pi), max_radius * math.sqrt(rng.uniform(0, 0.81))
        rows.append([r * math.cos(a), r * math.sin(a), rng.normal(0.5, 2.0)])
    out = np.zeros((n, 4), F)
    with np.errstate(all="ignore"):
        out[:, :3] = np.array(rows[:n], np.float64).astype(F)
    out[:, 3] = rng.uniform(0, 255, n)
    rng.shuffle(out)
    return out


# ---- the wedge scene ---------------------------------------------------------------------------------------------------------------------------------------------

def rz(deg):
    a = math.radians(deg)
    return np.array([[math.cos(a), -math.sin(a), 0], [math.sin(a), math.cos(a), 0], [0, 0, 1.0]])


def ry(deg):
    a = math.radians(deg)
    return np.array([[math.cos(a), 0, math.sin(a)], [0, 1.0, 0], [-math.sin(a), 0, math.cos(a)]])      # (positive: the x axis dips below the horizon)


def quat_of(R):
    """unit quaternion (w, x, y, z) of a rotation matrix whose w is not small (every rotation of this scene)"""
    w = math.sqrt(max(0.0, 1.0 + R[0, 0] + R[1, 1] + R[2, 2])) / 2.0
    if w > 1e-3:
        return np.array([w, (R[2, 1] - R[1, 2]) / (4 * w), (R[0, 2] - R[2, 0]) / (4 * w), (R[1, 0] - R[0, 1]) / (4 * w)])
    i = int(np.argmax(np.diag(R)))      # near a half turn: the largest diagonal entry's branch
    j, k = (i + 1) % 3, (i + 2) % 3
    s = math.sqrt(max(0.0, 1.0 + R[i, i] - R[j, j] - R[k, k])) * 2.0
    q = np.zeros(4)
    q[0], q[1 + i], q[1 + j], q[1 + k] = (R[k, j] - R[j, k]) / s, s / 4.0, (R[j, i] + R[i, j]) / s, (R[k, i] + R[i, k]) / s
    return q


def street(rng, x_lo=-40.0, x_hi=140.0):
    """tests/test_place_gpu.py's street — walls of various lengths and heights and poles on both sides — over x_lo .. x_hi"""
    walls, poles = [], []
    x = x_lo
    while x < x_hi:
        for side in (-1, 1):
            length, height, off = rng.uniform(3, 9), rng.uniform(2.5, 9), rng.uniform(7, 16)
            if rng.uniform() < 0.75:
                walls.append((x, side * off, x + length, side * off + rng.uniform(-1.5, 1.5), height))
            if rng.uniform() < 0.6:
                poles.append((x + length + 1.0 + rng.uniform(0, 1), side * (off - 3.0 - rng.uniform(0, 2)), rng.uniform(3, 10)))
        x += 12.0
    return walls, poles


def sample_street(st, rng, spacing=0.3, gx=(-70.0, 170.0), gy=(-40.0, 40.0)):
    walls, poles = st
    out = []
    for x0, y0, x1, y1, h in walls:
        n_u, n_v = int(math.hypot(x1 - x0, y1 - y0) / spacing), int(h / spacing)
        u, v = np.meshgrid((np.arange(n_u) + 0.5) / n_u, (np.arange(n_v) + 0.5) / n_v, indexing="ij")
        u, v = u.ravel() + rng.uniform(-0.3, 0.3, u.size) / n_u, v.ravel() + rng.uniform(-0.3, 0.3, v.size) / n_v
        out.append(np.stack([x0 + u * (x1 - x0), y0 + u * (y1 - y0), v * h], 1))
    for px, py, h in poles:
        n = int(h / 0.1) * 6
        a, z = rng.uniform(0, 2 * math.pi, n), rng.uniform(0, h, n)
        out.append(np.stack([px + 0.15 * np.cos(a), py + 0.15 * np.sin(a), z], 1))
    ax, ay = np.meshgrid(np.arange(gx[0], gx[1], 0.8), np.arange(gy[0], gy[1], 0.8), indexing="ij")
    out.append(np.stack([ax.ravel() + rng.uniform(-0.25, 0.25, ax.size), ay.ravel() + rng.uniform(-0.25, 0.25, ax.size), np.zeros(ax.size)], 1))
    return np.concatenate(out)


H_FOV, V_FOV, RANGE = 40.85, 12.55, 50.0      # half angles in degrees (a Livox Horizon's 81.7 x 25.1 degree field), metres


def wedge_scan(world, t, R, seed=0):
    """the world's points the sensor at (t, R) sees, in its frame: rows (x, y, z, aux)"""
    near = world[np.linalg.norm(world[:, :2] - t[:2], axis=1) < RANGE + 1.0]
    loc = (near - t) @ R
    rho = np.hypot(loc[:, 0], loc[:, 1])
    see = (np.linalg.norm(loc, axis=1) <= RANGE) & (np.abs(np.degrees(np.arctan2(loc[:, 1], loc[:, 0]))) <= H_FOV) & (np.abs(np.degrees(np.arctan2(loc[:, 2], rho))) <= V_FOV)
    loc = loc[see].astype(F)
    return np.concatenate([loc, np.random.default_rng(seed).uniform(0, 1, (loc.shape[0], 1)).astype(F)], 1)


N1, N2, QUERY, MATCH = 60, 26, 83, 37      # keyframes of pass 1 / pass 2, the query (third from last, at x = 34), the keyframe of pass 1 that stood there


def wedge_scene(seed=77, pitch=12.0):
    """dict: rows[k] (the scan, LiDAR frame), true[k] / odo[k] = (t, R) LiDAR poses as they were / as the odometry believes, times[k], poses (n, 7) = odo as p, q,
    D = (D_R, D_t): the odometry's error on pass 2 (odo = D true)"""
    st = street(np.random.default_rng(seed))
    w1, w2 = sample_street(st, np.random.default_rng(1)), sample_street(st, np.random.default_rng(2))      # a revisit never sees the same points
    true = [(np.array([-40.0 + 2.0 * k, 0.0, 1.8]), ry(pitch)) for k in range(N1)]
    true += [(np.array([80.0 - 2.0 * j, 0.5, 1.8]), rz(180.0) @ ry(pitch)) for j in range(N2)]
    pivot = true[QUERY][0]
    D_R = rz(20.0)
    D_t = pivot + np.array([0.0, -25.0, 0.0]) - D_R @ pivot
    odo = true[:N1] + [(D_R @ t + D_t, D_R @ R) for t, R in true[N1:]]
    rows = [wedge_scan(w1 if k < N1 else w2, t, R, seed=k) for k, (t, R) in enumerate(true)]
    times = [2.0 * k if k < N1 else 200.0 + 2.0 * k for k in range(N1 + N2)]
    poses = np.array([np.concatenate([t, quat_of(R)]) for t, R in odo])
    return dict(rows=rows, true=true, odo=odo, times=times, poses=poses, D=(D_R, D_t))


PARAMS = dict(n_ring=20, n_sector=60, max_radius=30.0, lidar_height=2.0)
BACK, FWD = 20, 2
