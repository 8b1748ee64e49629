"""Referee of the global pose graph (include/lili_hip.h: lili_pose_graph*, lili_loop_measurement, lili_correct_poses), numpy / scipy.

Conventions (the header's): a pose is p (3) then q (w, x, y, z); the tangent is (omega, v), rotation first; X (+) xi = (p + R v, normalise(q Exp(omega)));
between-factor e = (Log(R_Z^T R_A^T R_B), R_Z^T (R_A^T (p_B - p_A) - t_Z)), r = e / s; the prior is the same factor with A = the identity.  Factor f of a graph
with N nodes: 0 = the prior, 1 .. N - 1 = the chain factor (f - 1, f), N + l = loop l.  Everything that touches every node is vectorised."""
import math

import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spla

SMALL_ANGLE = 0.1          # LILI_PG_SMALL_ANGLE
PRIOR_VAR = np.array([1e-6] * 3 + [1e-8] * 3)      # L/src/BackendFusion.cpp:552-557
ODOM_VAR = np.array([1e-6] * 3 + [1e-4] * 3)
MAX_ITERATIONS, GRADIENT_TOLERANCE, PARAMETER_TOLERANCE, FUNCTION_TOLERANCE, NUMERICAL_FAILURE, COST_INCREASED = 0, 1, 2, 3, 5, 7
CONVERGED = (GRADIENT_TOLERANCE, PARAMETER_TOLERANCE, FUNCTION_TOLERANCE)


# ---- quaternion algebra on (..., 4) arrays -------------------------------------------------------------------------
def qmul(a, b):
    aw, ax, ay, az = np.moveaxis(np.asarray(a, np.float64), -1, 0)
    bw, bx, by, bz = np.moveaxis(np.asarray(b, np.float64), -1, 0)
    return np.stack([aw * bw - ax * bx - ay * by - az * bz, aw * bx + ax * bw + ay * bz - az * by,
                     aw * by + ay * bw + az * bx - ax * bz, aw * bz + az * bw + ax * by - ay * bx], -1)


def qconj(q):
    return np.asarray(q, np.float64) * np.array([1.0, -1.0, -1.0, -1.0])


def qrot(q, v):
    q, v = np.asarray(q, np.float64), np.asarray(v, np.float64)
    u = q[..., 1:4]
    uv = np.cross(u, v)
    uv = uv + uv
    return (v + q[..., 0:1] * uv) + np.cross(u, uv)


def qmat(q):
    w, x, y, z = np.moveaxis(np.asarray(q, np.float64), -1, 0)
    R = np.empty(w.shape + (3, 3))
    R[..., 0, 0] = 1 - 2 * (y * y + z * z); R[..., 0, 1] = 2 * (x * y - w * z); R[..., 0, 2] = 2 * (x * z + w * y)
    R[..., 1, 0] = 2 * (x * y + w * z); R[..., 1, 1] = 1 - 2 * (x * x + z * z); R[..., 1, 2] = 2 * (y * z - w * x)
    R[..., 2, 0] = 2 * (x * z - w * y); R[..., 2, 1] = 2 * (y * z + w * x); R[..., 2, 2] = 1 - 2 * (x * x + y * y)
    return R


def qnormalize(q):
    q = np.asarray(q, np.float64)
    return q / np.linalg.norm(q, axis=-1, keepdims=True)


def qlog(q):
    """rotation vector of a unit quaternion, angle in [0, pi]"""
    q = np.asarray(q, np.float64)
    q = np.where(q[..., 0:1] < 0, -q, q)
    n = np.linalg.norm(q[..., 1:4], axis=-1, keepdims=True)
    with np.errstate(invalid="ignore", divide="ignore"):
        k = np.where(n > 0, 2.0 * np.arctan2(n, q[..., 0:1]) / np.where(n > 0, n, 1.0), 2.0)
    return k * q[..., 1:4]


def qexp(w):
    w = np.asarray(w, np.float64)
    th = np.linalg.norm(w, axis=-1, keepdims=True)
    s = np.where(th > 0, np.sin(0.5 * th) / np.where(th > 0, th, 1.0), 0.5)
    return np.concatenate([np.cos(0.5 * th), s * w], -1)


def skew(v):
    v = np.asarray(v, np.float64)
    S = np.zeros(v.shape[:-1] + (3, 3))
    S[..., 0, 1] = -v[..., 2]; S[..., 0, 2] = v[..., 1]
    S[..., 1, 0] = v[..., 2]; S[..., 1, 2] = -v[..., 0]
    S[..., 2, 0] = -v[..., 1]; S[..., 2, 1] = v[..., 0]
    return S


def jr_inv_coefficient(t2):
    t2 = np.asarray(t2, np.float64)
    series = 1.0 / 12.0 + t2 * (1.0 / 720.0 + t2 * (1.0 / 30240.0 + t2 * (1.0 / 1209600.0)))
    t = np.sqrt(np.where(t2 > 0, t2, 1.0))
    with np.errstate(invalid="ignore", divide="ignore"):
        closed = 1.0 / (t * t) - (1.0 + np.cos(t)) / (2.0 * t * np.sin(t))
    return np.where(t2 < SMALL_ANGLE * SMALL_ANGLE, series, closed)


def jr_inv(phi):
    """inverse of SO(3)'s right Jacobian: I + [phi]x / 2 + c [phi]x^2"""
    phi = np.asarray(phi, np.float64)
    t2 = np.sum(phi * phi, -1)
    c = jr_inv_coefficient(t2)[..., None, None]
    S = skew(phi)
    return np.eye(3) + 0.5 * S + c * (phi[..., :, None] * phi[..., None, :] - t2[..., None, None] * np.eye(3))


def retract(X, xi):
    X, xi = np.asarray(X, np.float64), np.asarray(xi, np.float64)
    out = np.empty_like(X)
    out[..., 0:3] = X[..., 0:3] + qrot(X[..., 3:7], xi[..., 3:6])
    out[..., 3:7] = qnormalize(qmul(X[..., 3:7], qexp(xi[..., 0:3])))
    return out


def between(A, B):
    A, B = np.asarray(A, np.float64), np.asarray(B, np.float64)
    ia = qconj(A[..., 3:7])
    return np.concatenate([qrot(ia, B[..., 0:3] - A[..., 0:3]), qmul(ia, B[..., 3:7])], -1)


def normalize_poses(P):
    P = np.array(P, np.float64).reshape(-1, 7)
    P[:, 3:7] = qnormalize(P[:, 3:7])
    return P


IDENTITY = np.array([0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0])


def factor_error(A, B, Z):
    """e (…, 6) and the pieces the Jacobians reuse: qab, d, qe"""
    ia, iz = qconj(A[..., 3:7]), qconj(Z[..., 3:7])
    d = qrot(ia, B[..., 0:3] - A[..., 0:3])
    ev = qrot(iz, d - Z[..., 0:3])
    qab = qmul(ia, B[..., 3:7])
    qe = qmul(iz, qab)
    return np.concatenate([qlog(qe), ev], -1), qab, d, qe


def factor_jacobians(A, B, Z):
    """e, d e / d xi_A, d e / d xi_B (unweighted), the issue's blocks"""
    e, qab, d, qe = factor_error(A, B, Z)
    Jri = jr_inv(e[..., 0:3])
    Rz = qmat(qconj(Z[..., 3:7]))
    Ja = np.zeros(e.shape[:-1] + (6, 6))
    Jb = np.zeros_like(Ja)
    Ja[..., 0:3, 0:3] = -Jri @ np.swapaxes(qmat(qab), -1, -2)
    Ja[..., 3:6, 0:3] = Rz @ skew(d)
    Ja[..., 3:6, 3:6] = -Rz
    Jb[..., 0:3, 0:3] = Jri
    Jb[..., 3:6, 3:6] = qmat(qe)
    return e, Ja, Jb


class Graph:
    """estimates X (N, 7), frozen measurements meas (N, 7; 0: the prior's), loops [(from, to, meas (7), var (6))]"""

    def __init__(self, prior_var=PRIOR_VAR, odom_var=ODOM_VAR):
        self.X, self.meas, self.loops = np.zeros((0, 7)), np.zeros((0, 7)), []
        self.prior_var, self.odom_var = np.asarray(prior_var, np.float64), np.asarray(odom_var, np.float64)

    @property
    def n(self):
        return self.X.shape[0]

    def copy(self):
        g = Graph(self.prior_var, self.odom_var)
        g.X, g.meas, g.loops = self.X.copy(), self.meas.copy(), list(self.loops)
        return g

    def append(self, prev, poses):
        poses = normalize_poses(poses)
        if self.n == 0:
            assert prev is None
            m = np.vstack([poses[0:1], between(poses[:-1], poses[1:])])
        else:
            chain = np.vstack([normalize_poses(prev), poses])
            m = between(chain[:-1], chain[1:])
        first = self.n
        self.X, self.meas = np.vstack([self.X, poses]), np.vstack([self.meas, m])
        return first

    def add_loop(self, a, b, meas, var):
        self.loops.append((int(a), int(b), normalize_poses(meas)[0], np.asarray(var, np.float64).reshape(6).copy()))

    def factors(self, X):
        """A, B, Z, w, a, b over all factors (a = -1: the prior)"""
        n, L = self.n, len(self.loops)
        a = np.concatenate([[-1], np.arange(0, n - 1), [l[0] for l in self.loops]]).astype(np.int64)
        b = np.concatenate([[0], np.arange(1, n), [l[1] for l in self.loops]]).astype(np.int64)
        Z = np.vstack([self.meas] + [l[2][None] for l in self.loops])
        w = np.vstack([1.0 / np.sqrt(self.prior_var)[None], np.repeat(1.0 / np.sqrt(self.odom_var)[None], n - 1, 0)] + [1.0 / np.sqrt(l[3])[None] for l in self.loops])
        A = np.where((a >= 0)[:, None], X[np.maximum(a, 0)], IDENTITY[None])
        assert Z.shape[0] == n + L
        return A, X[b], Z, w, a, b

    def cost(self, X):
        A, B, Z, w, _, _ = self.factors(X)
        e = factor_error(A, B, Z)[0]
        return 0.5 * float(np.sum((e * w) ** 2))

    def linearize(self, X):
        A, B, Z, w, a, b = self.factors(X)
        e, Ja, Jb = factor_jacobians(A, B, Z)
        return e * w, Ja * w[:, :, None], Jb * w[:, :, None], a, b

    def evaluate(self, X=None):
        """cost, g (N, 6), diagonal blocks (N, 6, 6), sub (N - 1, 6, 6): chain block (i + 1, i), loop blocks (L, 6, 6): block (from, to)"""
        X = self.X if X is None else X
        n, L = self.n, len(self.loops)
        r, Ja, Jb, a, b = self.linearize(X)
        JaT, JbT = np.swapaxes(Ja, -1, -2), np.swapaxes(Jb, -1, -2)
        D, g = np.zeros((n, 6, 6)), np.zeros((n, 6))
        D[:] = (JbT[:n] @ Jb[:n])
        g[:] = (JbT[:n] @ r[:n, :, None])[..., 0]
        D[:n - 1] += JaT[1:n] @ Ja[1:n]
        g[:n - 1] += (JaT[1:n] @ r[1:n, :, None])[..., 0]
        for l in range(L):
            f = n + l
            D[a[f]] += JaT[f] @ Ja[f]; g[a[f]] += JaT[f] @ r[f]
            D[b[f]] += JbT[f] @ Jb[f]; g[b[f]] += JbT[f] @ r[f]
        S = JbT[1:n] @ Ja[1:n]
        LB = JaT[n:] @ Jb[n:]
        return 0.5 * float(np.sum(r * r)), g, D, S, LB

    def jacobian(self, X):
        """r (6 F) and the sparse J (6 F x 6 N)"""
        r, Ja, Jb, a, b = self.linearize(X)
        F = r.shape[0]
        rows = (6 * np.arange(F)[:, None, None] + np.arange(6)[None, :, None]) + np.zeros((1, 1, 6), np.int64)
        cb = (6 * b[:, None, None] + np.arange(6)[None, None, :]) + np.zeros((1, 6, 1), np.int64)
        ca = (6 * a[:, None, None] + np.arange(6)[None, None, :]) + np.zeros((1, 6, 1), np.int64)
        has = a >= 0
        J = sp.coo_matrix((np.concatenate([Jb.ravel(), Ja[has].ravel()]), (np.concatenate([rows.ravel(), rows[has].ravel()]), np.concatenate([cb.ravel(), ca[has].ravel()]))),
                          shape=(6 * F, 6 * self.n)).tocsc()
        return r.ravel(), J


def linear_step(J, r, solver):
    """delta of H delta = -g; None on a matrix that is not positive definite.  dense: numpy.linalg.solve; sparse: SuperLU on J^T J (COLAMD order); natural: SuperLU
    in the natural order (the second opinion where the dense matrix would not fit)"""
    H = (J.T @ J).tocsc()
    g = J.T @ r
    if solver == "dense":
        Hd = H.toarray()
        try:
            np.linalg.cholesky(Hd)
        except np.linalg.LinAlgError:
            return None, g
        return np.linalg.solve(Hd, -g), g
    d = spla.spsolve(H, -g, permc_spec="NATURAL" if solver == "natural" else "COLAMD")
    if not np.all(np.isfinite(d)) or float(d @ (H @ d)) <= 0:
        return None, g
    return d, g


def gauss_newton(graph, X0=None, max_iterations=10, function_tolerance=1e-6, gradient_tolerance=1e-10, parameter_tolerance=1e-8, solver="sparse"):
    """The header's loop.  -> X, summary: iterations, termination, initial_cost, final_cost, cost / step_inf / grad_inf per iteration, and `margins`: for every stop
    decision taken, (name, value, threshold)."""
    X = (graph.X if X0 is None else np.asarray(X0, np.float64)).copy()
    cost = graph.cost(X)
    s = dict(iterations=0, termination=MAX_ITERATIONS, initial_cost=cost, final_cost=cost, cost=[], step_inf=[], grad_inf=[], margins=[])
    for it in range(max_iterations):
        r, J = graph.jacobian(X)
        delta, g = linear_step(J, r, solver)
        gmax = float(np.abs(g).max())
        s["grad_inf"].append(gmax)
        s["margins"].append(("gradient", gmax, gradient_tolerance))
        if gmax <= gradient_tolerance:
            s["termination"] = GRADIENT_TOLERANCE
            break
        if delta is None:
            s["termination"] = NUMERICAL_FAILURE
            break
        Xn = retract(X, delta.reshape(-1, 6))
        new_cost = graph.cost(Xn)
        smax = float(np.abs(delta).max())
        s["cost"].append(new_cost); s["step_inf"].append(smax)
        s["iterations"] = it + 1
        s["margins"].append(("increase", new_cost, cost))
        if not new_cost <= cost:
            s["termination"] = COST_INCREASED
            break
        X, old, cost = Xn, cost, new_cost
        s["final_cost"] = cost
        s["margins"].append(("parameter", smax, parameter_tolerance))
        if smax <= parameter_tolerance:
            s["termination"] = PARAMETER_TOLERANCE
            break
        s["margins"].append(("function", abs(old - new_cost), function_tolerance * old))
        if abs(old - new_cost) <= function_tolerance * old:
            s["termination"] = FUNCTION_TOLERANCE
            break
        if it + 1 >= max_iterations:
            s["termination"] = MAX_ITERATIONS
            break
    return X, s


def pose_difference(Xa, Xb):
    """largest position difference and largest rotation angle between two pose arrays (q and -q are the same rotation)"""
    Xa, Xb = np.asarray(Xa, np.float64).reshape(-1, 7), np.asarray(Xb, np.float64).reshape(-1, 7)
    dp = float(np.abs(Xa[:, 0:3] - Xb[:, 0:3]).max())
    qd = qmul(qconj(Xa[:, 3:7]), Xb[:, 3:7])
    ang = 2.0 * np.arctan2(np.linalg.norm(qd[:, 1:4], axis=1), np.abs(qd[:, 0]))
    return dp, float(ang.max())


# ---- host restatements, scalar arithmetic in the library's order (bit for bit) -------------------------------------
def _mul(a, b):
    return (a[0] * b[0] - a[1] * b[1] - a[2] * b[2] - a[3] * b[3], a[0] * b[1] + a[1] * b[0] + a[2] * b[3] - a[3] * b[2],
            a[0] * b[2] + a[2] * b[0] + a[3] * b[1] - a[1] * b[3], a[0] * b[3] + a[3] * b[0] + a[1] * b[2] - a[2] * b[1])


def _inv(q):
    n2 = q[1] * q[1] + q[2] * q[2] + q[3] * q[3] + q[0] * q[0]
    return (q[0] / n2, -q[1] / n2, -q[2] / n2, -q[3] / n2)


def _cross(a, b):
    return (a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0])


def _rot(q, v):
    u = (q[1], q[2], q[3])
    uv = _cross(u, v)
    uv = (uv[0] + uv[0], uv[1] + uv[1], uv[2] + uv[2])
    c = _cross(u, uv)
    return ((v[0] + q[0] * uv[0]) + c[0], (v[1] + q[0] * uv[1]) + c[1], (v[2] + q[0] * uv[2]) + c[2])


def _normalized(q):
    n = math.sqrt(q[1] * q[1] + q[2] * q[2] + q[3] * q[3] + q[0] * q[0])
    return (q[0] / n, q[1] / n, q[2] / n, q[3] / n)


def _from_matrix(m):
    """Eigen::Quaterniond(const Matrix3d&)"""
    t = m[0][0] + m[1][1] + m[2][2]
    q = [0.0] * 4
    if t > 0.0:
        t = math.sqrt(t + 1.0)
        q[0] = 0.5 * t
        t = 0.5 / t
        q[1] = (m[2][1] - m[1][2]) * t; q[2] = (m[0][2] - m[2][0]) * t; q[3] = (m[1][0] - m[0][1]) * t
    else:
        i = 0
        if m[1][1] > m[0][0]:
            i = 1
        if m[2][2] > m[i][i]:
            i = 2
        j = (i + 1) % 3
        k = (j + 1) % 3
        t = math.sqrt(m[i][i] - m[j][j] - m[k][k] + 1.0)
        q[1 + i] = 0.5 * t
        t = 0.5 / t
        q[0] = (m[k][j] - m[j][k]) * t
        q[1 + j] = (m[j][i] + m[i][j]) * t
        q[1 + k] = (m[k][i] + m[i][k]) * t
    return tuple(q)


def loop_measurement(T_icp, pose_latest, pose_closest):
    """L/src/BackendFusion.cpp:2587-2622: the ICP transform corrects the latest keyframe's pose; poseFrom.between(poseTo) of the two unit-quaternion poses"""
    T = [[float(v) for v in row] for row in np.asarray(T_icp, np.float64).reshape(4, 4)]
    pl, pc = [float(v) for v in pose_latest], [float(v) for v in pose_closest]
    q_inc = _from_matrix(T)                                                    # L:2589
    q_cor = _mul(q_inc, (pl[3], pl[4], pl[5], pl[6]))                          # L:2599
    r = _rot(q_inc, (pl[0], pl[1], pl[2]))
    t_cor = (r[0] + T[0][3], r[1] + T[1][3], r[2] + T[2][3])                   # L:2600
    qf, qt = _normalized(q_cor), _normalized((pc[3], pc[4], pc[5], pc[6]))     # L:2602-2612 (Rot3::Quaternion)
    fi = (qf[0], -qf[1], -qf[2], -qf[3])
    t = _rot(fi, (pc[0] - t_cor[0], pc[1] - t_cor[1], pc[2] - t_cor[2]))       # L:2622 between
    q = _normalized(_mul(fi, qt))
    return np.array([t[0], t[1], t[2], q[0], q[1], q[2], q[3]])


def correct_poses(solution, keyframe_id_in_frame, slide_window_width, abs_poses, keyframe_poses, f32_positions=False):
    """L/src/BackendFusion.cpp:2177-2311 on copies -> dict(abs_poses, frame_poses, keyframe_poses, last_pose, select_pose).  abs_poses rows are (q wxyz, p);
    the other pose rows (p, q)."""
    sol = np.asarray(solution, np.float64).reshape(-1, 7)
    ab = [[float(v) for v in row] for row in np.asarray(abs_poses, np.float64).reshape(-1, 7)]
    kf = [[float(v) for v in row] for row in np.asarray(keyframe_poses, np.float64).reshape(-1, 7)]
    w, n_abs = int(slide_window_width), len(ab)
    pos = (lambda v: float(np.float32(v))) if f32_positions else (lambda v: float(v))
    qrel, trel = [], []
    for i in range(n_abs - w, n_abs - 1):                                      # L:2189-2209
        qf, qt = tuple(ab[i][0:4]), tuple(ab[i + 1][0:4])
        tf, tt = ab[i][4:7], ab[i + 1][4:7]
        qrel.append(_mul(_inv(qf), qt))
        trel.append(_rot(_inv(qf), (tt[0] - tf[0], tt[1] - tf[1], tt[2] - tf[2])))
    frames = [[pos(s[0]), pos(s[1]), pos(s[2]), float(s[3]), float(s[4]), float(s[5]), float(s[6])] for s in sol]      # L:2211-2225
    for i in range(0, len(kf) - w + 1):                                        # L:2227-2258
        kf[i] = list(frames[int(keyframe_id_in_frame[i])])
        ab[i + 1] = [kf[i][3], kf[i][4], kf[i][5], kf[i][6], kf[i][0], kf[i][1], kf[i][2]]
    for i in range(n_abs - w, n_abs - 1):                                      # L:2260-2298
        iq, it = tuple(ab[i][0:4]), ab[i][4:7]
        r = _rot(iq, trel[i - n_abs + w])
        it = (it[0] + r[0], it[1] + r[1], it[2] + r[2])
        iq = _mul(iq, qrel[i - n_abs + w])
        ab[i + 1] = [iq[0], iq[1], iq[2], iq[3], it[0], it[1], it[2]]
        kf[i] = [pos(it[0]), pos(it[1]), pos(it[2]), iq[0], iq[1], iq[2], iq[3]]
    last = list(ab[n_abs - w])                                                 # L:2300-2308
    return dict(abs_poses=np.array(ab), frame_poses=np.array(frames), keyframe_poses=np.array(kf), last_pose=np.array(last),
                select_pose=np.array([pos(last[4]), pos(last[5]), pos(last[6])]))
