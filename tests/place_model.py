"""Numpy restatement of the place-recognition descriptor and search (include/lili_hip.h "place recognition"): f32 where the definition says
f32, f64 for the distance.  Plain loops: clarity over speed.  The referee of tests/test_place_gpu.py; not in the reference, so there is no reference fixture."""
import math

import numpy as np

F = np.float32


def tables(n_ring, n_sector, max_radius):
    """(ring_r2[k] = b_k b_k, k < n_ring; cos / sin of 2 pi m / n_sector, m < n_sector / 4) in f32 (the angles in f64, libm's cos / sin)"""
    R = F(max_radius)
    ring_r2 = np.zeros(n_ring, F)
    for k in range(n_ring):
        b = F(F(R * F(k)) / F(n_ring))
        ring_r2[k] = F(b * b)
    c, s = np.zeros(n_sector // 4, F), np.zeros(n_sector // 4, F)
    for m in range(n_sector // 4):
        a = 2.0 * math.pi * m / n_sector
        c[m], s[m] = F(math.cos(a)), F(math.sin(a))
    return ring_r2, c, s


def cell_of(x, y, z, n_ring, n_sector, max_radius, tab):
    """(sector, ring) of a point, or None: skipped"""
    ring_r2, C, S = tab
    x, y, z = F(x), F(y), F(z)
    if not (np.isfinite(x) and np.isfinite(y) and np.isfinite(z)):
        return None
    r2 = F(F(x * x) + F(y * y))
    if r2 > F(F(max_radius) * F(max_radius)):
        return None
    ring = sum(1 for k in range(1, n_ring) if r2 > ring_r2[k])
    if y >= 0:
        q = 0 if x >= 0 else 1
    else:
        q = 2 if x < 0 else 3
    u, v = [(x, y), (y, F(-x)), (F(-x), F(-y)), (F(-y), x)][q]
    j = sum(1 for m in range(1, n_sector // 4) if F(v * C[m]) >= F(u * S[m]))
    return q * (n_sector // 4) + j, ring


def describe(pts, n_ring=20, n_sector=60, max_radius=80.0, lidar_height=2.0):
    """(n_sector, n_ring) f32: the maximum of z + lidar_height per cell, 0 without a point"""
    tab = tables(n_ring, n_sector, max_radius)
    best = {}
    with np.errstate(all="ignore"):
        for p in np.asarray(pts, F).reshape(-1, pts.shape[1] if len(pts) else 3):
            c = cell_of(p[0], p[1], p[2], n_ring, n_sector, max_radius, tab)
            if c is None:
                continue
            v = F(F(p[2]) + F(lidar_height))
            if c not in best or v > best[c]:
                best[c] = v
    d = np.zeros((n_sector, n_ring), F)
    for (s, r), v in best.items():
        d[s, r] = v
    return d


def describe_atan(pts, n_ring, n_sector, max_radius, lidar_height):
    """the paper's form: ring = ceil(r / max_radius * n_ring), sector = ceil(theta / 2 pi * n_sector), both 1-based, in f64"""
    d = np.zeros((n_sector, n_ring), F)
    seen = np.zeros((n_sector, n_ring), bool)
    for x, y, z in np.asarray(pts, np.float64)[:, :3]:
        r = math.hypot(x, y)
        if r > max_radius:
            continue
        th = math.atan2(y, x) % (2 * math.pi)
        ring = max(1, min(n_ring, math.ceil(r / max_radius * n_ring))) - 1
        sec = max(1, min(n_sector, math.ceil(th / (2 * math.pi) * n_sector))) - 1
        v = F(F(z) + F(lidar_height))
        if not seen[sec, ring] or v > d[sec, ring]:
            d[sec, ring], seen[sec, ring] = v, True
    return d


def shift_distances(A, B):
    """d(s) for every s (f64; +inf where no sector pair is occupied): column j of A against column j + s of B"""
    A, B = np.asarray(A, np.float64), np.asarray(B, np.float64)
    ns = A.shape[0]
    na, nb = np.sqrt((A * A).sum(1)), np.sqrt((B * B).sum(1))
    valid = np.outer(na > 0, nb > 0)
    with np.errstate(all="ignore"):
        cos = np.where(valid, (A @ B.T) / np.outer(na, nb), 0.0)      # cos[j, l] = A_j . B_l / (|A_j| |B_l|)
    j = np.arange(ns)
    l = (j[None, :] + j[:, None]) % ns                                # l[s, j] = (j + s) mod n_sector
    total, count = cos[j[None, :], l].sum(1), valid[j[None, :], l].sum(1)
    out = np.full(ns, np.inf)
    out[count > 0] = 1.0 - total[count > 0] / count[count > 0]
    return out


def shift_distances_loops(A, B):
    """the same, statement by statement as the header words it (the vectorised form is checked against this one in tests/test_place_model_cpu.py)"""
    A, B = np.asarray(A, np.float64), np.asarray(B, np.float64)
    ns = A.shape[0]
    na, nb = np.sqrt((A * A).sum(1)), np.sqrt((B * B).sum(1))
    out = np.full(ns, np.inf)
    for s in range(ns):
        cs = [float(A[j] @ B[(j + s) % ns]) / (na[j] * nb[(j + s) % ns]) for j in range(ns) if na[j] > 0 and nb[(j + s) % ns] > 0]
        if cs:
            out[s] = 1.0 - sum(cs) / len(cs)
    return out


def pair(A, B):
    """(distance, shift): the minimum over the shifts, the smallest shift that attains it"""
    d = shift_distances(A, B)
    s = int(np.argmin(d))
    return float(d[s]), s


def search(descs, times, query, k, q_id=-1, q_time=0.0, min_time_gap=-1.0, max_id=2 ** 31 - 1, cache=None):
    """[(id, shift, distance)] ascending by (distance, id), at most k; descs: the archive's descriptors (None: the keyframe has none).  cache: {(key of the query,
    candidate): pair}, filled here"""
    rows = []
    for c, B in enumerate(descs):
        if B is None or c > max_id or c == q_id or not abs(times[c] - q_time) > min_time_gap:
            continue
        key = (query.tobytes(), c)
        if cache is not None and key in cache:
            d, s = cache[key]
        else:
            d, s = pair(query, B)
            if cache is not None:
                cache[key] = (d, s)
        if np.isfinite(d):
            rows.append((d, c, s))
    rows.sort()
    return [(c, s, d) for d, c, s in rows[:k]]


def guess(pose_src, pose_dst, shift, n_sector):
    """M_dst Rz(2 pi shift / n_sector) M_src^-1; poses: p then q w x y z"""
    def M(p):
        w, x, y, z = np.asarray(p[3:7], np.float64) / np.linalg.norm(p[3:7])
        T = np.eye(4)
        T[:3, :3] = [[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)], [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]]
        T[:3, 3] = p[:3]
        return T
    a = 2.0 * math.pi * shift / n_sector
    Rz = np.eye(4)
    Rz[:2, :2] = [[math.cos(a), -math.sin(a)], [math.sin(a), math.cos(a)]]
    Ms, Mi = M(pose_src), np.eye(4)
    Mi[:3, :3], Mi[:3, 3] = Ms[:3, :3].T, -Ms[:3, :3].T @ Ms[:3, 3]      # a rigid transform's inverse
    return M(pose_dst) @ Rz @ Mi


def bin_centre_points(cells, n_ring, n_sector, max_radius, rng, z_lo=-1.5, z_hi=6.0):
    """one point at the polar centre of each (sector, ring) of `cells`, random height: a scene whose rotation by whole sectors shifts its descriptor exactly"""
    pts = []
    for s, r in cells:
        th = 2 * math.pi * (s + 0.5) / n_sector
        rad = max_radius * (r + 0.5) / n_ring
        pts.append([rad * math.cos(th), rad * math.sin(th), rng.uniform(z_lo, z_hi)])
    return np.array(pts, F).reshape(-1, 3)
