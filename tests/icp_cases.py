"""Hard cases for the loop-closure registration (lili_loop.hip) and exact models of its three parts.

Shared by tests/test_icp_cases_cpu.py (the models and the numpy restatement tests/icp_model.py held to each other, the mutations that the cases must catch)
and tests/test_loop_icp_hard_gpu.py (the device held to the models).  Expected values never come from the code under test.

Models.
  nn_brute       exact 1-NN over the WHOLE target with the library's f32 expression (dx*dx + dy*dy) + dz*dz, dx = p - q; the smallest index among equal d2;
                 non-finite target points are never chosen, a non-finite query gets index -1 and d2 = inf.  No candidate is cut to a reach.
  exact_rotation H = sum (p - pm)(q - qm)^T of the f32 pairs in fractions.Fraction (exact), its rank by exact minors, the SVD by Jacobi on H^T H in decimal at
                 PREC digits, R = v1 u1^T + v2 u2^T + (v1 x v2)(u1 x u2)^T — which is V diag(1, 1, det U det V) U^T with singular values descending — the singular
                 values, det H, the optimum tr(R H) = s1 + s2 + sign(det H) s3 and t = qm - R pm.  Standard library only.
  BruteTree      nn_brute behind the interface icp_model.step / align / fitness expect of the oracle's kd-tree: the model of one step and of a whole align is
                 the numpy restatement driven by the brute-force neighbour, so ties are defined; it runs on its own, not as a replay of a device log.

Allowance for R (measured, not chosen).  The polar factor errs by the rounding of the sums over the gap: with S the largest entry of the UNCENTRED sums
sum (p - o)(q - o)^T about the target's centroid o (where the device cancels: H = S - n pm qm^T) and g = s2 + s3 (det H >= 0) or s2 - s3 (det H < 0), the
allowance is K 2^-52 S / g on the largest entry of R.  K is the worst ratio of `restated_rotation` (plain numpy f64 in the device's formulation) over all
unique-R cases: K_MEASURED below, K_IN_USE for the restatement, 8 K_IN_USE for the device.  The translation gets the same allowance times |pm| plus one ulp
of |qm|.  Cases whose allowance exceeds CAP = 1e-3 are not evidence and are counted, at most 5 %.
Where R is not unique (rank 1; reflected with s2 = s3) every solution is orthonormal with det +1 and attains the optimum of tr(R H): that is asserted,
within the allowance without the gap, K 2^-52 S (tr(R H) moves by no more than three times the error of H's entries); for rank 1 the source line
is mapped onto the target line, R u1 = v1, within K 2^-52 S / s1 (the line's gap is s1 itself).

Forcing a chosen H through the public API: max_iterations = 1, no guess, and a sparse target whose points are far apart next to the distance from a source
point to its partner, so NN(p_i) = q_i — `partner` in every case, asserted with nn_brute before anything is compared.

Scales.  Every family is built at scale 1, 1e-3 and 1e3 (coordinates and gate), and at scale 1 with as many decoy target points 7.8 km away as the set has
points, which puts the target's centroid — the device's origin — 4.9 km from the pairs.  The families whose point is an EXACT structure (rank 1, rank 0,
equal singular values) take 2^-10 for 1e-3: a factor that is no power of two rounds them into general position, where the 5 % cap would be spent on them.

The lower clamp of the cell (0.05) cannot be reached by a target of 4096 points: the extents enter the volume floored at 1 m, so the cell is at least
(1 / 4096)^(1/3) = 0.0625.  The `dense` shape therefore has 12000 points in half a metre; every other target stays within 4096.
"""
import decimal
from fractions import Fraction

import numpy as np

from tests import icp_model as M

PREC = 120
CAP = 1e-3
K_MEASURED = 5.11     # re-measured and printed by tests/test_icp_cases_cpu.py, which fails above K_IN_USE; made by cube_turned (S / g = 1 / 2: the SVD's own few ulps)
K_IN_USE = 5.5
DEVICE_FACTOR = 8.0
U52 = 2.0 ** -52
MAX_CELLS = 1 << 27
DMAX = np.finfo(np.float64).max


# ------------------------------------------------------------------------------------------------------------------------------------------------------------
# nearest neighbour
# ------------------------------------------------------------------------------------------------------------------------------------------------------------
def _d2_all(tx, ty, tz, q):
    with np.errstate(all="ignore"):
        dx, dy, dz = tx - q[0], ty - q[1], tz - q[2]
        return (dx * dx + dy * dy) + dz * dz


def nn_brute(tgt, q, multiplicity=False):
    """(index (-1: none), f32 d2 (inf: none)[, how many target points share the least d2]) of every row of q"""
    tgt = np.ascontiguousarray(np.asarray(tgt, np.float32)[:, :3])
    q = np.ascontiguousarray(np.asarray(q, np.float32)[:, :3])
    bad = ~np.isfinite(tgt).all(1)
    tx, ty, tz = (np.ascontiguousarray(tgt[:, k]) for k in range(3))
    idx = np.full(q.shape[0], -1, np.int64)
    d2 = np.full(q.shape[0], np.inf, np.float32)
    mult = np.zeros(q.shape[0], np.int64)
    for i in range(q.shape[0]):
        if not np.isfinite(q[i]).all():
            continue
        d = _d2_all(tx, ty, tz, q[i])
        d[bad] = np.inf
        d[np.isnan(d)] = np.inf
        j = int(np.argmin(d))      # the first of the least: the smallest index
        if d[j] < np.inf:
            idx[i], d2[i] = j, d[j]
            mult[i] = int((d == d[j]).sum())
    return (idx, d2, mult) if multiplicity else (idx, d2)


class BruteTree:
    """nn_brute where icp_model expects the oracle's kd-tree (only column 0 of knn5 is read)"""

    def __init__(self, tgt, nn=nn_brute):
        self.tgt, self.nn = np.asarray(tgt, np.float32), nn

    def knn5(self, q):
        idx, d2 = self.nn(self.tgt, q)
        return idx[:, None], d2[:, None]


def fitness_brute(tgt, src, T, max_range=DMAX):
    return M.fitness(BruteTree(tgt), tgt, src, T, max_range)


# ------------------------------------------------------------------------------------------------------------------------------------------------------------
# the host's grid (index_target in lili_loop.hip, build_grid in lili_map.hip) — used ONLY to place inputs and by the small walk of the mutation test
# ------------------------------------------------------------------------------------------------------------------------------------------------------------
def grid_restate(tgt, max_cells=MAX_CELLS):
    t = np.asarray(tgt, np.float32)[:, :3]
    t = t[np.isfinite(t).all(1)].astype(np.float64)
    n = max(t.shape[0], 1)
    mn, mx = (t.min(0), t.max(0)) if t.shape[0] else (np.zeros(3), np.zeros(3))
    cell = float(np.cbrt(np.prod(np.maximum(mx - mn, 1.0)) / n))
    cell = min(max(cell, 0.05), 50.0)
    while True:
        dims = np.floor((mx - mn) / cell).astype(np.int64) + 1
        total = float(dims[0]) * float(dims[1]) * float(dims[2])
        if total <= max_cells:
            break
        cell *= float(np.cbrt(total / max_cells)) * 1.02
    inv = 1.0 / cell
    return dict(o=mn, dims=dims, inv_cell=inv, cell=1.0 / inv)


def walk_nn(g, tgt, q, gate=-1.0, bound_shift=1):
    """icp_nn restated plainly for small targets: Chebyshev shells around the query's cell, the stop rule best d2 < ((r - bound_shift + f) cell (1 - 4e-6))^2.
    bound_shift = 0 is the mutation `r + f`."""
    tgt = np.asarray(tgt, np.float32)[:, :3]
    q = np.asarray(q, np.float32)[:, :3]
    dims = g["dims"]
    cells = {}
    for j, p in enumerate(tgt):
        c = np.zeros(3, np.int64) if not np.isfinite(p).all() else np.clip(np.floor((p.astype(np.float64) - g["o"]) * g["inv_cell"]).astype(np.int64), 0, dims - 1)
        cells.setdefault(tuple(int(v) for v in c), []).append(j)
    idx = np.full(q.shape[0], -1, np.int64)
    d2 = np.full(q.shape[0], np.inf, np.float32)
    for i, qq in enumerate(q):
        if not np.isfinite(qq).all():
            continue
        u = (qq.astype(np.float64) - g["o"]) * g["inv_cell"]
        c = np.floor(u).astype(np.int64)
        fr = u - c
        f = max(min(0.5, float(np.minimum(fr, 1.0 - fr).min())), 0.0)
        r0 = int(max(0, np.max(np.maximum(-c, c - (dims - 1)))))
        rmax = int(np.max(np.maximum(c, dims - 1 - c)))
        bd, bi = np.float32(np.inf), -1
        for r in range(r0, rmax + 1):
            if r >= 1:
                lb = ((r - bound_shift) + f) * g["cell"] * (1.0 - 4e-6)
                if gate >= 0.0 and lb > gate:
                    break
                if float(bd) < lb * lb:
                    break
            lo, hi = np.maximum(c - r, 0), np.minimum(c + r, dims - 1)
            for z in range(int(lo[2]), int(hi[2]) + 1):
                for y in range(int(lo[1]), int(hi[1]) + 1):
                    for x in range(int(lo[0]), int(hi[0]) + 1):
                        if max(abs(x - c[0]), abs(y - c[1]), abs(z - c[2])) != r:
                            continue
                        for j in cells.get((x, y, z), ()):
                            d = tgt[j] - qq
                            dd = (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]
                            if dd < bd or (dd == bd and j < bi):
                                bd, bi = dd, j
        idx[i], d2[i] = bi, bd
    return idx, d2


# ------------------------------------------------------------------------------------------------------------------------------------------------------------
# the exact rotation
# ------------------------------------------------------------------------------------------------------------------------------------------------------------
def _dec(fr):
    return decimal.Decimal(fr.numerator) / decimal.Decimal(fr.denominator)


def _frac_rows(A):
    return [[Fraction(float(v)) for v in row[:3]] for row in np.asarray(A, np.float32)]


def _exact_rank(H):
    det = (H[0][0] * (H[1][1] * H[2][2] - H[1][2] * H[2][1]) - H[0][1] * (H[1][0] * H[2][2] - H[1][2] * H[2][0]) + H[0][2] * (H[1][0] * H[2][1] - H[1][1] * H[2][0]))
    if det != 0:
        return 3, det
    for r in range(3):
        for s in range(3):
            a, b = [k for k in range(3) if k != r], [k for k in range(3) if k != s]
            if H[a[0]][b[0]] * H[a[1]][b[1]] - H[a[0]][b[1]] * H[a[1]][b[0]] != 0:
                return 2, det
    return (1 if any(v != 0 for row in H for v in row) else 0), det


def _jacobi_sym3(A):
    """eigen-decomposition of a symmetric 3x3 of Decimals: (eigenvalues, V with the eigenvectors as columns)"""
    one, zero = decimal.Decimal(1), decimal.Decimal(0)
    A = [row[:] for row in A]
    V = [[one if r == s else zero for s in range(3)] for r in range(3)]
    tiny = decimal.Decimal(10) ** (-2 * (PREC - 8))
    for _ in range(200):
        off = A[0][1] ** 2 + A[0][2] ** 2 + A[1][2] ** 2
        tr = A[0][0] + A[1][1] + A[2][2]
        if off <= tiny * tr * tr:
            break
        for p, q in ((0, 1), (0, 2), (1, 2)):
            if A[p][q] == 0:
                continue
            theta = (A[q][q] - A[p][p]) / (2 * A[p][q])
            t = (one if theta >= 0 else -one) / (abs(theta) + (theta * theta + one).sqrt())
            c = one / (t * t + one).sqrt()
            s = t * c
            for k in range(3):      # columns p, q of A and of V
                akp, akq = A[k][p], A[k][q]
                A[k][p], A[k][q] = c * akp - s * akq, s * akp + c * akq
                vkp, vkq = V[k][p], V[k][q]
                V[k][p], V[k][q] = c * vkp - s * vkq, s * vkp + c * vkq
            for k in range(3):      # rows p, q of A
                apk, aqk = A[p][k], A[q][k]
                A[p][k], A[q][k] = c * apk - s * aqk, s * apk + c * aqk
    else:
        raise RuntimeError("Jacobi did not converge")
    return [A[k][k] for k in range(3)], V


def _cross(a, b):
    return [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]


def exact_rotation(P, Q):
    """The model of TransformationEstimationSVD without scale for the f32 pairs (P[i], Q[i]).  A dict: rank, det_sign, sigma (3 floats, descending), opt, unique,
    R (3x3 f64, None where not unique — rank 0: the identity), t, u1 / v1 (the leading source / target directions), H (Fractions), pm, qm (Fractions)."""
    with decimal.localcontext() as ctx:
        ctx.prec = PREC
        Pf, Qf = _frac_rows(P), _frac_rows(Q)
        n = len(Pf)
        pm = [sum(r[k] for r in Pf) / n for k in range(3)]
        qm = [sum(r[k] for r in Qf) / n for k in range(3)]
        H = [[sum((Pf[i][r] - pm[r]) * (Qf[i][s] - qm[s]) for i in range(n)) for s in range(3)] for r in range(3)]
        rank, det = _exact_rank(H)
        det_sign = (det > 0) - (det < 0)
        out = dict(rank=rank, det_sign=det_sign, det=float(det), H=H, pm=pm, qm=qm, n=n)
        zero = decimal.Decimal(0)
        if rank == 0:
            R = [[decimal.Decimal(int(r == s)) for s in range(3)] for r in range(3)]
            out.update(sigma=[0.0, 0.0, 0.0], opt=0.0, unique=True, gap=0.0, u1=None, v1=None)
        else:
            HtH = [[_dec(sum(H[k][r] * H[k][s] for k in range(3))) for s in range(3)] for r in range(3)]
            lam, V = _jacobi_sym3(HtH)
            order = sorted(range(3), key=lambda k: -lam[k])
            sig = [(lam[k] if lam[k] > 0 else zero).sqrt() if j < rank else zero for j, k in enumerate(order)]
            v = [[V[r][k] for r in range(3)] for k in order]
            Hd = [[_dec(x) for x in row] for row in H]
            u = [[sum(Hd[r][s] * v[j][s] for s in range(3)) / sig[j] for r in range(3)] for j in range(min(rank, 2))]
            equal23 = abs(sig[1] - sig[2]) <= decimal.Decimal(10) ** -60 * sig[0]
            unique = rank == 2 or (rank == 3 and (det_sign > 0 or not equal23))
            gap = sig[1] + sig[2] if det_sign >= 0 else sig[1] - sig[2]
            out.update(sigma=[float(s) for s in sig], opt=float(sig[0] + sig[1] + det_sign * sig[2]), unique=unique, gap=float(gap),
                       u1=np.array([float(x) for x in u[0]]), v1=np.array([float(x) for x in v[0]]))
            R = None
            if unique:
                u3, v3 = _cross(u[0], u[1]), _cross(v[0], v[1])
                R = [[v[0][r] * u[0][s] + v[1][r] * u[1][s] + v3[r] * u3[s] for s in range(3)] for r in range(3)]
        if R is None:
            out.update(R=None, t=None)
        else:
            pd, qd = [_dec(x) for x in pm], [_dec(x) for x in qm]
            out["R"] = np.array([[float(x) for x in row] for row in R])
            out["t"] = np.array([float(qd[r] - sum(R[r][s] * pd[s] for s in range(3))) for r in range(3)])
        return out


def trace_RH(R, H):
    """tr(R H) = sum (R p') . q' exactly, for a float R and the Fraction H"""
    return float(sum(Fraction(float(R[r][s])) * H[s][r] for r in range(3) for s in range(3)))


def target_origin(tgt):
    t = np.asarray(tgt, np.float32)[:, :3]
    return t[np.isfinite(t).all(1)].astype(np.float64).mean(0)


def uncentred_scale(P, Q, o):
    """S: the largest entry of sum (p - o)(q - o)^T"""
    Pc, Qc = np.asarray(P, np.float32)[:, :3].astype(np.float64) - o, np.asarray(Q, np.float32)[:, :3].astype(np.float64) - o
    return float(np.abs(Pc.T @ Qc).max())


def restated_rotation(P, Q, o, det_sign=True):
    """plain numpy f64 in the device's formulation: uncentred sums about o, H = S - n pm qm^T, numpy.linalg.svd, V's third column negated when det U det V < 0
    (det_sign = False is the mutation that drops it).  (R, t)"""
    Pc, Qc = np.asarray(P, np.float32)[:, :3].astype(np.float64) - o, np.asarray(Q, np.float32)[:, :3].astype(np.float64) - o
    n = Pc.shape[0]
    pm, qm = Pc.sum(0) / n, Qc.sum(0) / n
    H = Pc.T @ Qc - n * np.outer(pm, qm)
    U, _, Vt = np.linalg.svd(H)
    V = Vt.T.copy()
    if det_sign and np.linalg.det(U) * np.linalg.det(V) < 0:
        V[:, 2] *= -1
    R = V @ U.T
    return R, (qm + o) - R @ (pm + o)


def allowance(P, Q, o, model, K):
    """(allowance on R's entries, allowance on t's, S)"""
    S = uncentred_scale(P, Q, o)
    aR = K * U52 * S / model["gap"] if model["gap"] > 0 else np.inf
    pm = np.array([float(x) for x in model["pm"]])
    qm = np.array([float(x) for x in model["qm"]])
    at = aR * np.linalg.norm(pm) + float(np.spacing(np.linalg.norm(qm)))
    return aR, at, S


# ------------------------------------------------------------------------------------------------------------------------------------------------------------
# cases that force a chosen H
# ------------------------------------------------------------------------------------------------------------------------------------------------------------
def rot(axis, deg):
    a = np.deg2rad(deg)
    axis = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    Kx = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    return np.eye(3) + np.sin(a) * Kx + (1 - np.cos(a)) * Kx @ Kx


AXES = dict(z=(0.0, 0.0, 1.0), x=(1.0, 0.0, 0.0), y=(0.0, 1.0, 0.0), skew=(1.0, 2.0, 3.0))
ANGLES = (30.0, 90.0, 150.0, 179.0, 180.0)
DECOY_OFFSET = np.array([6000.0, -6000.0, 5000.0])


def _frame(axis):
    a = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    e = np.eye(3)[int(np.argmin(np.abs(a)))]
    b = np.cross(a, e)
    b /= np.linalg.norm(b)
    return np.stack([b, np.cross(a, b), a], 1)      # columns: two normals, the axis


def _lattice(rng, z):
    xy = np.array([[10.0 * i, 10.0 * j] for i in range(4) for j in range(8)])
    return np.concatenate([xy, z(rng, 32)[:, None]], 1)


def _raw_h_cases():
    """(name, target f64, source f64, exact structure) at scale 1; the partner of source row i is target row i"""
    out = []
    rng = np.random.default_rng(2024)

    def zs(r, n):
        return r.uniform(0.3, 1.5, n) * r.choice([-1.0, 1.0], n)

    t = _lattice(rng, zs)
    out.append(("reflect", t, t * [1, 1, -1], False))
    for an, ax in AXES.items():
        F = _frame(ax)
        rad, ph = rng.uniform(0.2, 0.5, 24), rng.uniform(0, 2 * np.pi, 24)
        loc = np.stack([rad * np.cos(ph), rad * np.sin(ph), 3.0 * np.arange(24) - 34.5], 1)
        t = loc @ F.T
        for deg in ANGLES:
            out.append((f"rot_{an}_{deg:g}", t, t @ rot(ax, deg).T, False))
    t = _lattice(rng, lambda r, n: np.zeros(n))
    out.append(("zerocol", t, t + np.concatenate([rng.uniform(-0.3, 0.3, (32, 2)), rng.uniform(-1, 1, (32, 1))], 1), False))
    t = _lattice(rng, zs)
    s = t + np.concatenate([rng.uniform(-0.3, 0.3, (32, 2)), np.zeros((32, 1))], 1)
    s[:, 2] = 0.0
    out.append(("zerorow", t, s, False))
    for an, d in dict(x=(10, 0, 0), y=(0, 10, 0), z=(0, 0, 10), skew=(9, 6, 3)).items():
        t = np.arange(12)[:, None] * np.array(d, np.float64)
        out.append((f"rank1_{an}", t, t + [0.25, -0.5, 0.25], True))
    t = np.array([[0, 0, 0], [10, 0, 0], [0, 10, 0], [10, 10, 4], [-10, 3, 8]], np.float64)
    for n in (3, 4, 5, 7):
        out.append((f"rank0_{n}", t, np.repeat(t[2:3] + [0.25, 0.5, -0.25], n, 0), True))
    cube = np.array([[i, j, k] for i in (-1, 1) for j in (-1, 1) for k in (-1, 1)], np.float64)
    out.append(("cube_equal", cube * 4, cube * 4 + [0.25, -0.5, 0.125], True))
    out.append(("cube_turned", cube * 4, (cube * 4) @ rot(AXES["skew"], 20.0).T, False))
    out.append(("box_s1_eq_s2", cube * [4, 4, 2], cube * [4, 4, 2] + [0.25, -0.5, 0.125], True))
    out.append(("box_s2_eq_s3", cube * [4, 2, 2], cube * [4, 2, 2] + [0.25, -0.5, 0.125], True))
    sg = np.array([[1, 1], [1, -1], [-1, 1], [-1, -1], [-1, -1], [-1, 1], [1, -1], [1, 1]], np.float64)
    t = np.concatenate([10.0 * np.arange(8)[:, None], 0.5 * sg], 1)
    out.append(("reflect_s2_eq_s3", t, t * [1, 1, -1], True))
    t = np.stack([np.linspace(-50, 50, 32), rng.uniform(-0.005, 0.005, 32), rng.uniform(-0.0005, 0.0005, 32)], 1)
    out.append(("needle", t, t @ (rot(AXES["z"], 0.3) @ rot(AXES["x"], 20.0)).T + [0.02, -0.01, 0.003], False))
    t = np.array([[0, 0, 0], [10, 0, 1], [2, 9, -1]], np.float64)
    out.append(("three", t, t @ rot(AXES["skew"], 10.0).T + [0.1, -0.2, 0.05], False))
    return out


VARIANTS = ("unit", "milli", "kilo", "decoy")


def h_cases(variant):
    """dicts: name, tgt (m, 3) f32, src (n, 3) f32, partner (n,), gate"""
    scale = dict(unit=1.0, milli=1e-3, kilo=1e3, decoy=1.0)[variant]
    out = []
    for name, t, s, exact in _raw_h_cases():
        k = 2.0 ** -10 if (exact and variant == "milli") else scale
        tgt, src = (t * k).astype(np.float32), (s * k).astype(np.float32)
        partner = np.arange(src.shape[0]) if not name.startswith("rank0") else np.full(src.shape[0], 2)
        if variant == "decoy":
            rng = np.random.default_rng(len(name))
            decoy = (DECOY_OFFSET + rng.uniform(-20, 20, (tgt.shape[0], 3))).astype(np.float32)
            tgt, partner = np.concatenate([decoy, tgt], 0), partner + decoy.shape[0]
        out.append(dict(name=f"{variant}/{name}", tgt=tgt, src=src, partner=partner, gate=30.0 * k))
    return out


# ------------------------------------------------------------------------------------------------------------------------------------------------------------
# nearest-neighbour cases: dicts with name, tgt, src, gates (max_corr_dist values), fit (max_range values), guess (4x4 or None)
# ------------------------------------------------------------------------------------------------------------------------------------------------------------
def lattice_target():
    g = np.array([[i, j, k] for i in range(6) for j in range(6) for k in range(6)], np.float32)
    return g[np.random.default_rng(7).permutation(g.shape[0])]


def lattice_queries(n=200):
    rng = np.random.default_rng(8)
    return (rng.integers(0, 5, (n, 3)) + 0.5 * rng.integers(0, 2, (n, 3))).astype(np.float32)


def blob_halo_target():
    rng = np.random.default_rng(9)
    return np.concatenate([rng.uniform(-0.005, 0.005, (3686, 3)), rng.uniform(-100, 100, (410, 3))], 0)[rng.permutation(4096)].astype(np.float32)


def blob_halo_queries(n=600):
    rng = np.random.default_rng(10)
    return np.concatenate([rng.uniform(-0.02, 0.02, (n // 2, 3)), rng.uniform(-110, 110, (n - n // 2, 3))], 0).astype(np.float32)


def _ulps(x, k):
    x = np.float32(x)
    for _ in range(abs(k)):
        x = np.nextafter(x, np.float32(np.inf if k > 0 else -np.inf))
    return x


def _cellface_case():
    """targets and queries within a few f32 ulps of cell faces, and queries whose best distance is within 1e-5 of the next shell's lower bound"""
    rng = np.random.default_rng(11)
    n, ext = 2048, 12.0
    cell = float(np.cbrt(ext ** 3 / n))
    cell = 1.0 / (1.0 / cell)

    def face(k):
        return k * cell      # the grid's origin is the box's corner (0, 0, 0)

    def near_faces(m):
        p = rng.uniform(0.5, ext - 0.5, (m, 3)).astype(np.float32)
        for i in range(m):
            for ax in rng.permutation(3)[:rng.integers(1, 4)]:
                p[i, ax] = _ulps(face(int(rng.integers(1, int(ext / cell)))), int(rng.integers(-2, 3)))
        return p
    nb = 64
    body = rng.uniform(0, ext, (n - 2 - 400 - 2 * nb, 3)).astype(np.float32)
    tf = near_faces(400)
    # the bound: a query at distance dl from the lower x face of its cell, a point of its own cell at dl (1 + e1) on the far side, a point across the face at dl (1 + e2)
    qb, inside, across = [], [], []
    for _ in range(nb):
        kx = int(rng.integers(2, int(ext / cell) - 1))
        y, z = ((rng.integers(2, int(ext / cell) - 1, 2) + rng.uniform(0.45, 0.55, 2)) * cell)
        dl = rng.uniform(0.05, 0.3) * cell
        e1, e2 = rng.uniform(-1e-5, 1e-5, 2)
        x = face(kx) + dl
        qb.append([x, y, z])
        inside.append([x + dl * (1 + e1), y, z])
        across.append([x - dl * (1 + e2), y, z])
    tgt = np.concatenate([np.float32([[0, 0, 0], [ext, ext, ext]]), body, tf, np.float32(inside), np.float32(across)], 0)
    assert tgt.shape[0] == n
    src = np.concatenate([near_faces(400), np.float32(qb), tf[:100] + np.float32([0.0, 0.0, 1e-4])], 0)
    return dict(name="cellfaces", tgt=tgt[rng.permutation(n)], src=src, gates=(30.0, 0.3), fit=(DMAX,), guess=None)


def _outside_case():
    rng = np.random.default_rng(12)
    tgt = np.concatenate([np.float32([[0, 0, 0], [20, 20, 20]]), rng.uniform(0, 20, (1998, 3)).astype(np.float32)], 0)
    cell = grid_restate(tgt)["cell"]
    q = []
    for cells in (0.5, 3.0, 40.0, 1000.0):
        for d in [(i, j, k) for i in (-1, 0, 1) for j in (-1, 0, 1) for k in (-1, 0, 1) if (i, j, k) != (0, 0, 0)]:      # 6 faces, 12 edges, 8 corners
            p = rng.uniform(1, 19, 3)
            for ax in range(3):
                if d[ax]:
                    p[ax] = (20.0 if d[ax] > 0 else 0.0) + d[ax] * cells * cell * rng.uniform(1.0, 1.1)
            q.append(p)
    q += list(rng.uniform(0, 20, (96, 3)))      # and inside the box
    return dict(name="outside", tgt=tgt, src=np.float32(q), gates=(30.0, 0.3), fit=(DMAX, 100.0), guess=None)


def nn_cases():
    rng = np.random.default_rng(13)
    out = [dict(name="lattice_ties", tgt=lattice_target(), src=lattice_queries(), gates=(30.0, 0.6), fit=(DMAX,), guess=None)]
    base = rng.uniform(-8, 8, (1000, 3)).astype(np.float32)
    out.append(dict(name="duplicates", tgt=np.repeat(base, 3, 0)[rng.permutation(3000)], src=(base[::2] + rng.normal(0, 0.3, (500, 3))).astype(np.float32),
                    gates=(30.0, 0.3), fit=(DMAX,), guess=None))
    out.append(_outside_case())
    out.append(_cellface_case())
    q = rng.uniform(-3, 3, (300, 3)).astype(np.float32)
    out.append(dict(name="one_point", tgt=np.float32([[0.5, -0.25, 1.0]]), src=q, gates=(30.0, 2.0), fit=(DMAX, 4.0), guess=None))
    out.append(dict(name="two_points", tgt=np.float32([[0.5, -0.25, 1.0], [-1.5, 0.25, -1.0]]), src=q, gates=(30.0, 2.0), fit=(DMAX,), guess=None))
    out.append(dict(name="all_equal", tgt=np.tile(np.float32([[0.5, -0.25, 1.0]]), (100, 1)), src=q, gates=(30.0, 2.0), fit=(DMAX,), guess=None))
    plane = np.concatenate([rng.uniform(-10, 10, (1000, 2)), np.zeros((1000, 1))], 1).astype(np.float32)
    qp = np.concatenate([rng.uniform(-12, 12, (400, 2)), rng.uniform(-3, 3, (400, 1))], 1).astype(np.float32)
    out.append(dict(name="plane_nz1", tgt=plane, src=qp, gates=(30.0, 0.5), fit=(DMAX,), guess=None))
    line = np.concatenate([rng.uniform(-10, 10, (500, 1)), np.zeros((500, 2))], 1).astype(np.float32)
    out.append(dict(name="line_ny1_nz1", tgt=line, src=qp, gates=(30.0, 0.5), fit=(DMAX,), guess=None))
    out.append(dict(name="blob_halo", tgt=blob_halo_target(), src=blob_halo_queries(), gates=(30.0, 0.004), fit=(DMAX,), guess=None))
    dense = rng.uniform(0, 0.5, (12000, 3)).astype(np.float32)
    out.append(dict(name="dense_clamp_005", tgt=dense, src=rng.uniform(-0.1, 0.6, (500, 3)).astype(np.float32), gates=(30.0, 0.02), fit=(DMAX,), guess=None))
    far = np.float32([[i, j, k] for i in (0, 5000) for j in (0, 5000) for k in (0, 5000)])
    qs = (far[rng.integers(0, 8, 64)] + rng.uniform(-1, 1, (64, 3)) * np.where(np.arange(64) % 2, 150.0, 15.0)[:, None]).astype(np.float32)
    out.append(dict(name="sparse8_clamp_50", tgt=far, src=qs, gates=(300.0, 30.0), fit=(DMAX,), guess=None))
    out.append(dict(name="sparse8_max_cells", tgt=far, src=qs, gates=(300.0, 30.0), fit=(DMAX,), guess=None, max_cells=20000))
    G = np.eye(4)
    G[0, 3] = 3.0e8
    out.append(dict(name="full_scan", tgt=lattice_target(), src=lattice_queries(), gates=(1.0e9,), fit=(DMAX,), guess=G))
    t = rng.uniform(-5, 5, (500, 3)).astype(np.float32)
    t[[0, 1, 2, 250, 499]] = np.float32([[np.nan, 0, 0], [np.inf, 0, 0], [0, -np.inf, 1], [1, 1, np.nan], [np.inf, np.nan, 0]])
    s = rng.uniform(-5, 5, (300, 3)).astype(np.float32)
    s[[0, 7, 150, 299]] = np.float32([[np.nan, 1, 1], [np.inf, 0, 0], [0, -np.inf, 0], [2, np.nan, np.inf]])
    out.append(dict(name="non_finite", tgt=t, src=s, gates=(30.0, 0.3), fit=(DMAX, 1.0), guess=None))
    # the gate boundary: 3-4-5 offsets, d2 = 25 exactly
    t = np.float32([[40 * i, 40 * j, 40 * k] for i in range(3) for j in range(3) for k in range(3)])
    offs = np.float32([[3, 4, 0], [0, -3, 4], [-4, 0, 3], [0, 0, 5], [3, -4, 0], [1, 2, 2], [0, 0, 0], [2, 2, 1]])
    s = np.concatenate([t[i:i + 1] + offs[i % 8] for i in range(27)], 0)
    out.append(dict(name="gate_boundary", tgt=t, src=s, gates=(5.0, float(np.nextafter(5.0, 0.0))), fit=(25.0, float(np.nextafter(25.0, 0.0))), guess=None))
    return out


# ------------------------------------------------------------------------------------------------------------------------------------------------------------
# exits: dicts with name, tgt, src, and the arguments of icp_model.align
# ------------------------------------------------------------------------------------------------------------------------------------------------------------
def exit_cases():
    rng = np.random.default_rng(14)
    t = rng.uniform(-5, 5, (600, 3)).astype(np.float32)
    out = [dict(name="transform_at_1", tgt=t, src=t[::2].copy(), kw=dict(), want=(M.TRANSFORM, 1)),
           dict(name="abs_mse_at_2", tgt=t, src=t[::2].copy(), kw=dict(teps=-1.0), want=(M.ABS_MSE, 2)),
           dict(name="rel_mse", tgt=t, src=(t[::2].astype(np.float64) @ rot((1, 1, 2), 2.0).T + [0.05, 0.02, -0.03] + rng.normal(0, 0.05, (300, 3))).astype(np.float32),
                kw=dict(teps=-1.0, feps=0.5),
                want=(M.REL_MSE, None)),
           dict(name="no_corr_at_0", tgt=t, src=np.concatenate([t[:2], t[2:40] + np.float32([100, 0, 0])], 0), kw=dict(max_corr_dist=0.5),
                want=(M.NO_CORRESPONDENCES, 0))]
    # both mse tests hold at once: a source a few f32 ulps off the target, mse ~3e-12 twice -> ABS_MSE, which the rule asks first
    out.append(dict(name="abs_before_rel", tgt=t, src=(t[::2] + rng.normal(0, 1e-6, (300, 3))).astype(np.float32), kw=dict(teps=-1.0, feps=0.5), want=(M.ABS_MSE, 2)))
    # a gate the increments carry the pairs out of: four sparse pairs 0.085 .. 0.098 m apart under a gate of 0.1 m (found by a random search over such sets with
    # the numpy restatement; every distance stays 2 % of the gate or more from it): 4 pairs, then 3, then 2 -> two completed iterations
    t4 = np.float32([[2.5426965, -7.8300686, -0.9536108], [0.9070234, -3.9019666, -6.720755], [-9.441073, 9.575517, -1.8354708], [-5.8120675, 2.9084916, -8.154446]])
    s4 = np.float32([[2.5127459, -7.8261557, -0.8630778], [0.9831838, -3.9594324, -6.7309775], [-9.429619, 9.619976, -1.7511482], [-5.8277197, 2.9525194, -8.239424]])
    out.append(dict(name="no_corr_later", tgt=t4, src=s4, kw=dict(max_corr_dist=0.1, teps=-1.0, feps=-1.0), want=(M.NO_CORRESPONDENCES, 2)))
    return out
