"""Hard neighbourhoods for the line fit of the association kernels (edge_fit, lili_s2m_dev.h: centroid, covariance, eig3_sym, the
ev[2] > 3 ev[1] gate, canon_sign, ROT's dist < edge_dist_max gate) and an independent model of it.

Shared by tests/test_edge_fit_cases_cpu.py (the conditions on the inputs, on the oracle alone) and tests/test_edge_fit_gpu.py (every launcher
against the oracle and the model).

Scene.  Clusters of exactly five map points stand on a cubic lattice of pitch 4 m, cluster k owning map rows 5 k .. 5 k + 4; the points lie
within 0.4 m of the lattice node and the one query of the cluster within 0.05 m of it (0.65 m for the gate cases), so the five nearest
neighbours of a query are its own cluster without doubt: every other point is more than 2.9 m away, the gate is 1 m.  Every case is built
twice: the lattice starting at the origin — there one f32 ulp of A and B is ~1e-8 m and 0.2 u resolves the direction to ~1e-7 rad, an
unconverged eigen-solver shows — and starting at (500, -480, 15), where the f32 coordinates quantise the spread at 3e-5 .. 6e-5 m.
Queries are handed over in a local frame and reach the map through the association pose (Q_ASSOC, T_ASSOC), which is not the identity.

Kinds (one string per cluster):
  line     random direction, lateral noise 1e-6 .. 1e-2 of the extent
  exact    exactly collinear in f32 in a general direction: k (a, b, c) g with small integers — rank one, ev[1] is rounding noise of either sign
  graded   eigenvalues about 1 : 1e-8 : 1e-16 of the largest
  tiny     a line cluster of 1e-4 m extent;   huge: one that spans the full 0.4 m either way
  band     the pattern of exact-3 stretched by 1 + d, d = +-1e-1 .. +-1e-6, in a random orientation: ratios either side of 3
  iso      isotropic clouds, planar isotropic patches (the largest eigenvalue repeats, exactly for the f32-exact square), rejected
  prolate  f32-exact clusters whose two SMALL eigenvalues are exactly equal (diagonal covariance)
  dup      five coincident points; four coincident points and one other
  axis     +-x, +-y, +-z with zero lateral spread: the covariance is diagonal, no Jacobi sweep runs, the sort alone decides
  box      f32-exact (+-a, 0, 0), (0, +-b, 0), 0 in the six axis assignments: diagonal covariance diag(2 a^2, 2 b^2, 0), a^2 / b^2 either side of 3
  diag     (1, +-1, 0), (1, 0, +-1), (0, 1, +-1), (+-1, +-1, 1): f32-exact multiples (the two leading |components| are EQUAL: canon_sign decides on the
           rounding of two different algorithms) and normalised ones with lateral noise
  exact3   f32-exact, ratio exactly 3: with g a power of two x = 3 g (-2, -1, 0, 1, 2), y = g (-3, 2, 2, 2, -3), z = 0 — sums x^2 = 90 g^2, y^2 = 30 g^2,
           xy = 0, zero means — in the six axis assignments.  The gate is strict: rejected
  ulp      exact3 with ONE coordinate moved by one f32 ulp either way: decided cases of both outcomes (a point of |x| = 6 g moved outwards changes the
           ratio by 2e-7 relative, three orders above the margin)
  rot345   exact3 turned by the 3-4-5 rotation (times 5, so still f32-exact): off-diagonals are non-zero, rounding enters, the margin rule decides
  lateral  lines along an axis, the query 0.1 + {0, +-1e-7, +-1e-4, +-1e-2} m beside the line: ROT's gate
  egate    the fifth neighbour's d^2 either side of edge_gate = 1

Model (plain numpy f64, vectorised, no transcription of either solver): centroid = sum / 5 and covariance of the centred points in the order of the
neighbour list it is given, numpy.linalg.eigh, r = ev[2] / (3 ev[1]), the leading vector under the same canonical sign rule and the gap between its two
largest |components|, A, B = c +- 0.1 u rounded to f32, ROT's distance of the transformed query from the line.

Margin rule (derived, not measured).  A backward-stable 3 x 3 solver errs by a few eps ||A|| in each eigenvalue; at the threshold ev[1] = ev[2] / 3, so r is
uncertain by ~1e-15 relative; differences in how the covariance sums are rounded add about the same.  A cluster is UNDECIDED if |ev[2] - 3 ev[1]| < 1e-10 ev[2]
(that is |r - 1| < 1e-10), a query's ROT distance if |dist - 0.1| < 1e-9 m, and a sign is TIED if the gap is below 1e-9.

One f32 ulp (ulp_close): |x - y| <= the f32 spacing at max(|x|, |y|) — with a floor of 1e-15 m.  A = c + 0.1 u carries the solver's error in u, a few f64 eps
(||u|| = 1 and an accepted cluster has an eigen-gap of at least two thirds of its spectrum), i.e. ~1e-16 m absolute; where a component of A is below ~1e-8 m
(the cluster at the origin itself, exact patterns with zero means) that exceeds its f32 spacing.  The floor is nine orders below what an unconverged sweep leaves."""
import functools

import numpy as np

PITCH = 4.0
OFFSETS = {"origin": (0.0, 0.0, 0.0), "far": (500.0, -480.0, 15.0)}
CASES = ("generic", "aligned", "exact3", "gates")
VARIANTS = ("livox", "rot")
EDGE_GATE, EDGE_DIST_MAX = 1.0, {"livox": 0.0, "rot": 0.1}          # L/src/BackendFusion.cpp:1543, R/src/BackendFusion.cpp:1443

_ang = np.radians(21.0)
_ax = np.array([0.3, -0.5, 0.81]) / np.linalg.norm([0.3, -0.5, 0.81])
Q_ASSOC = np.r_[np.cos(_ang / 2), np.sin(_ang / 2) * _ax]
T_ASSOC = np.array([1.5, -0.7, 0.3])

M_RATIO, M_DIST, M_TIE = 1e-10, 1e-9, 1e-9

PERMS = ((0, 1, 2), (0, 2, 1), (1, 0, 2), (1, 2, 0), (2, 0, 1), (2, 1, 0))
X3 = 3.0 * np.array([-2.0, -1.0, 0.0, 1.0, 2.0])
Y3 = np.array([-3.0, 2.0, 2.0, 2.0, -3.0])
DIAGS = np.array([(1, 1, 0), (1, -1, 0), (1, 0, 1), (1, 0, -1), (0, 1, 1), (0, 1, -1), (1, 1, 1), (-1, 1, 1), (1, -1, 1), (-1, -1, 1)], np.float64)


# ------------------------------------------------------------------------------------------------
# poses
# ------------------------------------------------------------------------------------------------
def _qrot(q, v):
    """q * v as Eigen evaluates it (v + w (2 u x v) + u x (2 u x v)), f64."""
    u = np.asarray(q[1:4], np.float64)
    uv = np.cross(u, v)
    uv = uv + uv
    return (v + uv * q[0]) + np.cross(u, uv)


def to_map(q_local, Q=Q_ASSOC, T=T_ASSOC):
    """transformPoint (L/src/BackendFusion.cpp:695-711): the f32 query, rotated and moved in f64, stored f32 — what both sides search and gate with."""
    return (_qrot(Q, np.asarray(q_local, np.float32).astype(np.float64)) + T).astype(np.float32)


def _to_local(p_map):
    Qi = np.r_[Q_ASSOC[0], -Q_ASSOC[1:]]
    return _qrot(Qi, np.asarray(p_map, np.float64) - T_ASSOC).astype(np.float32)


# ------------------------------------------------------------------------------------------------
# clusters: every builder returns (offsets (n, 5, 3) f64 from the lattice node, query offsets (n, 3) or None, kind)
# ------------------------------------------------------------------------------------------------
def _unit(rng, n):
    v = rng.normal(size=(n, 3))
    return v / np.linalg.norm(v, axis=1, keepdims=True)


def _frame(rng, n):
    d = _unit(rng, n)
    e1 = np.cross(d, _unit(rng, n)); e1 /= np.linalg.norm(e1, axis=1, keepdims=True)
    return d, e1, np.cross(d, e1)


def _line(rng, n, extent=0.4, noise=(-6, -2)):
    d = _unit(rng, n)
    t = rng.uniform(-extent, extent, (n, 5))
    sig = extent * 10.0 ** rng.uniform(noise[0], noise[1], n)
    return t[:, :, None] * d[:, None, :] + rng.normal(size=(n, 5, 3)) * sig[:, None, None]


def _k5(rng, n, hi=4):
    """five distinct integers in [-hi, hi] per cluster"""
    return np.stack([rng.permutation(np.arange(-hi, hi + 1))[:5] for _ in range(n)]).astype(np.float64)


def _exact(rng, n):
    abc = rng.integers(-7, 8, (n, 3)).astype(np.float64)
    abc[(abc == 0).all(1)] = (3, -5, 7)
    return _k5(rng, n)[:, :, None] * abc[:, None, :] * 2.0 ** -7


def _graded(rng, n):
    d, e1, e2 = _frame(rng, n)
    t, s, r = rng.uniform(-0.4, 0.4, (n, 5)), rng.uniform(-1, 1, (n, 5)), rng.uniform(-1, 1, (n, 5))
    return t[:, :, None] * d[:, None] + 0.4e-4 * s[:, :, None] * e1[:, None] + 0.4e-8 * r[:, :, None] * e2[:, None]


def _huge(rng, n):
    d = _unit(rng, n)
    t = np.tile(np.array([-0.4, -0.17, 0.03, 0.21, 0.4]), (n, 1))
    return t[:, :, None] * d[:, None, :] + rng.normal(size=(n, 5, 3)) * 1e-5


def _band(rng, n):
    d, e1, _ = _frame(rng, n)
    delta = np.resize(np.r_[10.0 ** -np.arange(1, 7), -(10.0 ** -np.arange(1, 7))], n)
    h = 0.03
    return h * X3[None, :, None] * d[:, None] + h * (1.0 + delta)[:, None, None] * Y3[None, :, None] * e1[:, None]


TETRA = np.array([(1, 1, 1), (1, -1, -1), (-1, 1, -1), (-1, -1, 1), (0, 0, 0)], np.float64)          # covariance 4 I
SQUARE = np.array([(1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 0)], np.float64)              # covariance diag(2, 2, 0)


def _iso(rng, n):
    """a third each: the tetrahedron with its centre (isotropic) and the square with its centre (planar isotropic), turned at random with 5 % noise; and the
    two f32-exact along the axes — the largest eigenvalue repeats exactly, three times for the tetrahedron"""
    third = n // 3
    d, e1, e2 = _frame(rng, 2 * third)
    R = np.stack([d, e1, e2], 1)
    pat = np.where((np.arange(2 * third) < third)[:, None, None], TETRA[None], SQUARE[None])
    size = rng.uniform(0.02, 0.2, 2 * third)
    out = np.zeros((n, 5, 3))
    out[:2 * third] = (np.einsum("nki,nij->nkj", pat, R) + rng.normal(0, 0.05, (2 * third, 5, 3))) * size[:, None, None]
    for k in range(2 * third, n):
        out[k] = (SQUARE[:, PERMS[k % 6]] if k % 2 else TETRA) * 2.0 ** -(3 + k % 5)
    return out


def _prolate(rng, n):
    t = np.array([1.0, 1, -1, -1, 0]); y = np.array([1.0, -1, 0, 0, 0]); z = np.array([0.0, 0, 1, -1, 0])
    out = np.zeros((n, 5, 3))
    for k in range(n):
        p, b = (2, 1, 3, 1, 1, 5)[k % 6], (1, 1, 2, 2, 3, 4)[k % 6]             # ratio 2 (p / b)^2: 8, 2, 4.5, 0.5, 2/9, 3.125
        g = 2.0 ** -(4 + (k // 6) % 4)
        out[k] = (np.stack([p * t, b * y, b * z], 1) * g)[:, PERMS[(k // 3) % 6]]
    return out


def _dup(rng, n):
    out = np.zeros((n, 5, 3))
    base = rng.integers(-40, 41, (n, 3)) * 2.0 ** -8
    out[:] = base[:, None, :]
    other = rng.integers(-40, 41, (n, 3)) * 2.0 ** -8
    other[(other == base).all(1)] += 2.0 ** -6
    out[n // 3:, 4] = other[n // 3:]                                             # four coincident points and one other
    return out


def _axis(rng, n):
    out = np.zeros((n, 5, 3))
    k5 = _k5(rng, n, 6)
    for k in range(n):
        out[k, :, k % 3] = (1 - 2 * ((k // 3) % 2)) * k5[k] * 2.0 ** -(4 + (k // 6) % 6)
    return out


def _box(rng, n):
    out = np.zeros((n, 5, 3))
    ab = ((7, 4), (5, 3), (12, 7), (26, 15), (1, 1), (3, 1), (2, 1), (19, 11), (97, 56), (4, 3), (9, 5), (7, 5))      # a^2 / b^2 from 1 to 9, several within 1e-3 of 3
    for k in range(n):
        a, b = ab[k % len(ab)]
        g = 2.0 ** -((9 if a > 20 else 5) + (k // 12) % 3)
        p = np.array([(a, 0, 0), (-a, 0, 0), (0, b, 0), (0, -b, 0), (0, 0, 0)], np.float64) * g
        out[k] = p[:, PERMS[(k // 2) % 6]]
    return out


def _diag_exact(rng, n):
    """f32-exact multiples of the diagonal: the two (or three) leading |components| of the direction are EQUAL"""
    k5 = _k5(rng, n, 6)
    return np.stack([k5[k][:, None] * DIAGS[k % 10][None, :] * 2.0 ** -(5 + (k // 10) % 4) for k in range(n)])


def _diag_noisy(rng, n):
    d = DIAGS[np.arange(n) % 10]; d = d / np.linalg.norm(d, axis=1, keepdims=True)
    t = rng.uniform(-0.35, 0.35, (n, 5))
    sig = 0.35 * 10.0 ** rng.uniform(-6, -3, n)
    return t[:, :, None] * d[:, None, :] + rng.normal(size=(n, 5, 3)) * sig[:, None, None]


def _exact3(g, perm):
    return (np.stack([X3, Y3, np.zeros(5)], 1) * g)[:, perm]


def _exact3_all():
    return np.stack([_exact3(2.0 ** -e, p) for e in range(5, 10) for p in PERMS])                  # 30 clusters


def _rot345_all():
    out = []
    for e in range(7, 11):
        g = 2.0 ** -e
        for p in PERMS:
            for sgn in (1.0, -1.0):
                x, y = 3.0 * X3 - sgn * 4.0 * Y3, sgn * 4.0 * X3 + 3.0 * Y3                         # 5 R(3-4-5) (x, y): small integers times g
                out.append((np.stack([x, y, np.zeros(5)], 1) * g)[:, p])
    return np.stack(out)                                                                             # 48 clusters


def _lateral(rng, n):
    """axis lines; the query 0.1 + delta beside them"""
    pts = np.zeros((n, 5, 3)); q = np.zeros((n, 3))
    deltas = (0.0, 1e-7, -1e-7, 1e-4, -1e-4, 1e-2, -1e-2)
    k5 = _k5(rng, n, 6)
    for k in range(n):
        ax = k % 3
        pts[k, :, ax] = k5[k] * 2.0 ** -5
        phi = (0.0, 0.5 * np.pi, np.pi, 1.5 * np.pi, 0.7, 2.9)[(k // 21) % 6]
        lat = np.zeros(3); lat[(ax + 1) % 3], lat[(ax + 2) % 3] = np.cos(phi), np.sin(phi)
        q[k] = lat * (0.1 + deltas[(k // 3) % 7])
        q[k, ax] = rng.uniform(-0.02, 0.02)
    return pts, q


def _egate(rng, n):
    """the farthest of the five points at d^2 = 1 + delta from the query"""
    d = _unit(rng, n)
    t = np.array([-0.4, -0.2, 0.0, 0.2, 0.4])
    pts = t[None, :, None] * d[:, None, :]
    delta = np.resize(np.r_[10.0 ** -np.arange(1.0, 7.0), -(10.0 ** -np.arange(1.0, 7.0))], n)
    return pts, (np.sqrt(1.0 + delta) - 0.4)[:, None] * d


ULP_MOVES = [(j, 0) for j in (0, 1, 3, 4)] + [(j, 1) for j in range(5)]      # (point, pattern column): every move changes the ratio at first order (x_j, y_j != 0)


def _ulp_neighbours(centres_f32):
    """exact3 with ONE in-plane coordinate of one point moved by one f32 ulp either way, as absolute f32 rows (n, 5, 3); n = 30 x 9 x 2"""
    out = []
    k = 0
    for e in range(5, 10):
        for perm in PERMS:
            for j, col in ULP_MOVES:
                for up in (False, True):
                    p = (centres_f32[k].astype(np.float64)[None, :] + _exact3(2.0 ** -e, perm)).astype(np.float32)
                    ax = perm.index(col)
                    p[j, ax] = np.nextafter(p[j, ax], np.float32(np.inf if up else -np.inf))
                    out.append(p)
                    k += 1
    assert k == centres_f32.shape[0]
    return np.stack(out)


N_ULP = 30 * len(ULP_MOVES) * 2


def _parts(case, rng):
    """[(kind, offsets (n, 5, 3), query offsets (n, 3) or None, claims to be f32-exact at both offsets)]"""
    if case == "generic":
        return [("line", _line(rng, 160), None, False), ("exact", _exact(rng, 60), None, True), ("graded", _graded(rng, 60), None, False),
                ("tiny", _line(rng, 40, extent=1e-4), None, False), ("huge", _huge(rng, 40), None, False), ("band", _band(rng, 120), None, False),
                ("iso", _iso(rng, 120), None, False), ("prolate", _prolate(rng, 48), None, True), ("dup", _dup(rng, 30), None, True)]
    if case == "aligned":
        return [("axis", _axis(rng, 144), None, True), ("box", _box(rng, 144), None, True), ("diag", _diag_exact(rng, 200), None, True),
                ("diag", _diag_noisy(rng, 200), None, False)]
    if case == "exact3":
        return [("exact3", _exact3_all(), None, True), ("ulp", np.zeros((N_ULP, 5, 3)), None, False), ("rot345", _rot345_all(), None, True)]
    if case == "gates":
        lp, lq = _lateral(rng, 378)
        ep, eq = _egate(rng, 120)
        return [("lateral", lp, lq, True), ("egate", ep, eq, False), ("line", _line(rng, 60), None, False), ("iso", _iso(rng, 42), None, False)]
    raise ValueError(case)


@functools.lru_cache(maxsize=None)
def build(case, offset):
    """-> dict(map_xyz (5 n, 3) f32, q_local (n, 3) f32, q_map (n, 3) f32 = to_map(q_local), kind (n,) str, centre (n, 3) f64, n)"""
    rng = np.random.default_rng({"generic": 101, "aligned": 202, "exact3": 303, "gates": 404}[case] + (7 if offset == "far" else 0))
    parts = _parts(case, rng)
    n = sum(p[1].shape[0] for p in parts)
    assert n <= 1500
    side = int(np.ceil(n ** (1 / 3)))
    ijk = np.stack(np.meshgrid(np.arange(side), np.arange(side), np.arange(side), indexing="ij"), -1).reshape(-1, 3)
    ijk = ijk[rng.permutation(ijk.shape[0])[:n]]                                   # the kinds spread over the lattice
    centre = np.asarray(OFFSETS[offset]) + PITCH * ijk.astype(np.float64)
    kind = np.concatenate([np.full(p[1].shape[0], p[0]) for p in parts])
    off = np.concatenate([p[1] for p in parts])
    assert np.abs(off).max() <= 0.4 * np.sqrt(3) + 1e-9
    pts = (centre[:, None, :] + off).astype(np.float32)
    ulp = kind == "ulp"
    if ulp.any():
        pts[ulp] = _ulp_neighbours(centre[ulp].astype(np.float32))
    exact = np.concatenate([np.full(p[1].shape[0], p[3]) for p in parts])
    assert np.array_equal(pts[exact].astype(np.float64), (centre[:, None, :] + off)[exact])          # what claims to be f32-exact is
    qoff = np.clip(rng.normal(0, 0.02, (n, 3)), -0.05, 0.05)
    at = 0
    for p in parts:
        if p[2] is not None:
            qoff[at:at + p[1].shape[0]] = p[2]
        at += p[1].shape[0]
    q_local = _to_local(centre + qoff)
    out = dict(map_xyz=np.ascontiguousarray(pts.reshape(-1, 3)), q_local=q_local, q_map=to_map(q_local), kind=kind, centre=centre, n=n, side=side, offset=offset)
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def short_map():
    """four map points: fewer than five neighbours, every query is refused"""
    rng = np.random.default_rng(5)
    mp = (np.array([0.0, 0, 0]) + rng.normal(0, 0.1, (4, 3))).astype(np.float32)
    return dict(map_xyz=mp, q_local=_to_local(rng.normal(0, 0.05, (50, 3))), n=50)


@functools.lru_cache(maxsize=None)
def dense_filler(case, offset):
    """Points that make the map of a case dense enough for the fine index (point-weighted mean occupancy of the gate-sized cells > 12, lili_map.hip) and stay
    outside every query's gate: 40 points within 0.15 m of the CENTRE of every lattice cell, 2 sqrt(3) = 3.46 m from the nearest nodes — no query is within 2.8 m.
    Appended BEHIND the clusters, so the cluster points keep their indices."""
    s = build(case, offset)
    side = s["side"]
    ijk = np.stack(np.meshgrid(np.arange(side - 1), np.arange(side - 1), np.arange(side - 1), indexing="ij"), -1).reshape(-1, 3)
    rng = np.random.default_rng(11)
    c = np.asarray(OFFSETS[offset]) + PITCH * (ijk.astype(np.float64) + 0.5)
    f = (c[:, None, :] + rng.uniform(-0.15, 0.15, (c.shape[0], 40, 3))).reshape(-1, 3).astype(np.float32)
    d = np.linalg.norm(f.astype(np.float64)[:, None, :] - s["q_map"].astype(np.float64)[None, ::7, :], axis=2).min()
    assert d > 2.5
    f.setflags(write=False)
    return f


def occupancy(points, cell=1.01 * 0.65):
    """point-weighted mean number of points per gate-sized cell (origin at the box minimum), as lili_map_density reports it"""
    p = np.asarray(points, np.float64)
    key = np.floor((p - p.min(0)) / cell).astype(np.int64)
    _, inv, cnt = np.unique(key, axis=0, return_inverse=True, return_counts=True)
    return float(cnt[inv.reshape(-1)].mean())


# ------------------------------------------------------------------------------------------------
# the model
# ------------------------------------------------------------------------------------------------
def d2_f32(q_map, pts):
    """squared distances as both sides compute them: f32 differences, squares added in f32 in x, y, z order"""
    d = q_map.astype(np.float32)[:, None, :] - pts.astype(np.float32)
    r = d[..., 0] * d[..., 0]
    r = r + d[..., 1] * d[..., 1]
    return r + d[..., 2] * d[..., 2]


def canon(u):
    """largest-|component| positive, the first one on ties; also the gap between the two largest |components|"""
    a = np.abs(u)
    lead = np.argmax(a, axis=1)                                                    # first maximum
    s = np.where(u[np.arange(u.shape[0]), lead] < 0, -1.0, 1.0)
    srt = np.sort(a, axis=1)
    return u * s[:, None], srt[:, 2] - srt[:, 1]


def model(map_xyz, q_map, idx, variant):
    """idx (n, 5): the neighbour list of every query (map rows, nearest first).  Everything f64 unless said otherwise."""
    n = idx.shape[0]
    dist_max = EDGE_DIST_MAX[variant]
    p32 = np.asarray(map_xyz, np.float32)[idx]                                     # (n, 5, 3)
    p = p32.astype(np.float64)
    d2 = d2_f32(q_map, p32)
    c = p[:, 0]
    for k in range(1, 5):
        c = c + p[:, k]
    c = c / 5.0
    z = p - c[:, None, :]
    cov = np.einsum("nki,nkj->nij", z, z)
    ev, vec = np.linalg.eigh(cov)
    u, gap = canon(vec[:, :, 2])
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = ev[:, 2] / (3.0 * ev[:, 1])
    A64, B64 = c + 0.1 * u, c - 0.1 * u
    lp = q_map.astype(np.float64)
    dist = np.linalg.norm(np.cross(lp - A64, lp - B64), axis=1) / np.linalg.norm(A64 - B64, axis=1)
    in_gate = d2[:, 4].astype(np.float64) < EDGE_GATE
    line = ev[:, 2] > 3.0 * ev[:, 1]
    # an exactly diagonal covariance (f32-exact patterns along the axes) leaves no solver arithmetic to disagree on: the eigenvalues ARE the diagonal, decided
    # whatever the ratio — exact3 (ratio exactly 3, refused by the strict gate) lives here
    diagonal = (cov[:, 0, 1] == 0) & (cov[:, 0, 2] == 0) & (cov[:, 1, 2] == 0)
    und_ratio = (np.abs(ev[:, 2] - 3.0 * ev[:, 1]) < M_RATIO * ev[:, 2]) & ~diagonal
    near = (dist < dist_max) if dist_max > 0 else np.ones(n, bool)
    und_dist = (np.abs(dist - dist_max) < M_DIST) if dist_max > 0 else np.zeros(n, bool)
    # a gate that refuses for certain decides the query whatever the later ones say
    undecided = in_gate & (und_ratio | (line & und_dist))
    return dict(d2=d2, c=c, ev=ev, ratio=ratio, u=u, gap=gap, tied=gap < M_TIE, diagonal=diagonal, A=A64.astype(np.float32), B=B64.astype(np.float32), dist=dist,
                in_gate=in_gate, valid=in_gate & line & near, undecided=undecided, decided=~undecided)


def ulp_close(x, y):
    """per component: |x - y| <= one f32 ulp at the larger magnitude (floor 1e-15, see the module docstring)"""
    x, y = np.asarray(x, np.float32), np.asarray(y, np.float32)
    tol = np.maximum(np.spacing(np.maximum(np.abs(x), np.abs(y))).astype(np.float64), 1e-15)
    return np.abs(x.astype(np.float64) - y.astype(np.float64)) <= tol


def pair_close(a, b, a2, b2, tied):
    """(n,) bool: (a, b) is (a2, b2) within one ulp per component — on tied rows as an unordered pair"""
    same = ulp_close(a, a2).all(1) & ulp_close(b, b2).all(1)
    swapped = ulp_close(a, b2).all(1) & ulp_close(b, a2).all(1)
    return same | (tied & swapped)


@functools.lru_cache(maxsize=None)
def reference(case, offset, variant):
    """(scene, oracle records over ALL queries, model) — computed once per session and shared, never written to"""
    from oracle import oracle as O
    s = build(case, offset)
    tree = O.KdTree(s["map_xyz"])
    rec = O.associate_edge(tree, s["q_local"], Q_ASSOC, T_ASSOC, O.params(variant))
    mdl = model(s["map_xyz"], s["q_map"], rec["nn_idx"], variant)
    for d in (rec, mdl):
        for v in d.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
    return s, rec, mdl


def summary(case, offset, variant):
    """the counts both tests print: decided / undecided / tied clusters and the accepted / rejected split of the decided ones (model)"""
    s, rec, m = reference(case, offset, variant)
    dec = m["decided"]
    return dict(n=s["n"], decided=int(dec.sum()), undecided=int((~dec).sum()), undecided_rot345=int((~dec & (s["kind"] == "rot345")).sum()),
                tied=int((m["tied"] & m["valid"]).sum()), accepted=int((dec & m["valid"]).sum()), rejected=int((dec & ~m["valid"]).sum()))
