"""REFEREE — TEST INFRASTRUCTURE ONLY.  Plain numpy / Python-float f64 restatement of the per-frame trajectory of the reference back end and of the
trust-region rules the device solve is pinned to:

  walk        buildLocalPoseGraph's IMU propagation through the non-keyframe scans, L/src/BackendFusion.cpp:1897-2108, statement by statement, and
  measurements the relative poses it is turned into, L:2110-2170.  Every sum is written out term by term in the order the text's expressions evaluate
              (Eigen 3.3 without vectorisation, no contraction): the device kernel has the same expression trees, so the two agree bit for bit.
  factor      LidarPoseFactor.h's residual (the Left / Right variants are the same expression with a constant node) and its ANALYTIC Jacobians in the
              local coordinates of ceres::QuaternionParameterization (delta on the left, full angle).
  dogleg      Ceres 2.0 TrustRegionMinimizer + DoglegStrategy (TRADITIONAL_DOGLEG, DENSE_QR, Jacobi scaling) as the issue that introduced it restates
              them — pinned to those semantics, not to a Ceres binary.  The Gauss-Newton step is computed as Ceres does, by QR on the augmented
              Jacobian (numpy lstsq); the device uses a banded Cholesky factorisation of the same regularised normal equations.

(L/ = the reference's LiLi-OM package.)  Poses are 7 doubles: p (3), q (w, x, y, z)."""
import numpy as np

from oracle.lo_window import qmul, qinv, qrot, qmat, quat_plus, plus_jacobian

MAX_FRAMES = 16
TERMINATION = {0: "max_iterations", 1: "gradient_tolerance", 2: "parameter_tolerance", 3: "function_tolerance", 4: "stalled", 5: "numerical_failure", 6: "min_radius"}


# ---------------------------------------------------------------- the walk
def _clamp(d):
    if d[0] > 15.0: d[0] = 15.0
    if d[1] > 15.0: d[1] = 15.0
    if d[2] > 18.0: d[2] = 18.0
    if d[0] < -15.0: d[0] = -15.0
    if d[1] < -15.0: d[1] = -15.0
    if d[2] < -18.0: d[2] = -18.0


def _matvec(R, v):
    return [(R[i][0] * v[0] + R[i][1] * v[1]) + R[i][2] * v[2] for i in range(3)]


def _matmul(A, B):
    return [[(A[i][0] * B[0][j] + A[i][1] * B[1][j]) + A[i][2] * B[2][j] for j in range(3)] for i in range(3)]


def mat_to_quat(m):
    """Eigen 3.3 quaternion from a 3 x 3 matrix (internal::quaternionbase_assign_impl), the matrix taken as it is"""
    t = (m[0][0] + m[1][1]) + m[2][2]
    q = [0.0, 0.0, 0.0, 0.0]      # w, x, y, z
    if t > 0.0:
        t = float(np.sqrt(t + 1.0))
        q[0] = 0.5 * t
        t = 0.5 / t
        q[1] = (m[2][1] - m[1][2]) * t
        q[2] = (m[0][2] - m[2][0]) * t
        q[3] = (m[1][0] - m[0][1]) * t
    else:
        i = 0
        if m[1][1] > m[0][0]: i = 1
        if m[2][2] > m[i][i]: i = 2
        j = (i + 1) % 3
        k = (j + 1) % 3
        t = float(np.sqrt(m[i][i] - m[j][j] - m[k][k] + 1.0))
        q[1 + i] = 0.5 * t
        t = 0.5 / t
        q[0] = (m[k][j] - m[j][k]) * t
        q[1 + j] = (m[j][i] + m[i][j]) * t
        q[1 + k] = (m[k][i] + m[i][k]) * t
    return q


def walk_indices(stamps, ii0, T):
    """The sample indices the walk reads, from the stamps alone: (lowest, highest) index, or None where the text would read at or beyond len(stamps), below 0,
    or divide by dt1 + dt2 == 0 — what the library refuses with LILI_E_ARG."""
    n_imu, ii, hi = len(stamps), int(ii0), int(ii0)
    if ii < 0:
        return None
    for f in range(1, len(T)):
        if ii + 1 >= n_imu:
            return None
        if (T[f - 1] - stamps[ii]) + (stamps[ii + 1] - T[f - 1]) == 0.0:
            return None
        ii += 1
        while True:
            if ii >= n_imu:
                return None
            if not (stamps[ii] < T[f]):
                break
            ii += 1
        if (T[f] - stamps[ii - 1]) + (stamps[ii] - T[f]) == 0.0:
            return None
        hi = max(hi, ii)
        if f != len(T) - 1:
            ii -= 1
    return int(ii0), hi


def walk(stamps, acc, gyr, ii0, T, P0, R0, V0, g, left, f32_positions=False):
    """L:1897-2170.  T = the n + 2 scan stamps (left keyframe, the n frames, right keyframe); (P0, R0 3 x 3, V0) = the start state; left = the left anchor's pose.
    Returns poses (n, 7), end state (P (3), R (3, 3), V (3)), measurements (n + 1, 7) = (delta p, delta q).  f32_positions: the frames' positions go through the
    float members of pcl::PointXYZI as in the text (pose_each_frame), their quaternions (PointPoseInfo) stay doubles."""
    st = [float(s) for s in stamps]
    A = [[float(v) for v in row] for row in np.asarray(acc, np.float64).reshape(-1, 3)]
    G = [[float(v) for v in row] for row in np.asarray(gyr, np.float64).reshape(-1, 3)]
    T = [float(t) for t in T]
    n = len(T) - 2
    P, V = [float(v) for v in P0], [float(v) for v in V0]
    R = [[float(v) for v in row] for row in np.asarray(R0, np.float64).reshape(3, 3)]
    g = [float(v) for v in g]
    ii = int(ii0)
    d, r = [0.0, 0.0, 0.0], [0.0, 0.0, 0.0]
    poses = []

    def step(a0, gy0, a1, gy1, dt):
        nonlocal R
        u0 = _matvec(R, [a0[i] - 0.0 for i in range(3)])
        un_acc_0 = [u0[i] - g[i] for i in range(3)]
        un_gyr = [0.5 * (gy0[i] + gy1[i]) - 0.0 for i in range(3)]
        dq = [1.0] + [un_gyr[i] * dt / 2.0 for i in range(3)]                  # deltaQ(un_gyr * dt): not normalised
        R = _matmul(R, qmat(dq).tolist())
        u1 = _matvec(R, [a1[i] - 0.0 for i in range(3)])
        un_acc_1 = [u1[i] - g[i] for i in range(3)]
        hdd = 0.5 * dt * dt
        for i in range(3):
            un_acc = 0.5 * (un_acc_0[i] + un_acc_1[i])
            P[i] = P[i] + (dt * V[i] + hdd * un_acc)
            V[i] = V[i] + dt * un_acc

    for f in range(1, n + 2):
        last = f == n + 1
        dt1 = T[f - 1] - st[ii]
        dt2 = st[ii + 1] - T[f - 1]
        w1 = dt2 / (dt1 + dt2)
        w2 = dt1 / (dt1 + dt2)
        d = [w1 * A[ii][i] + w2 * A[ii + 1][i] for i in range(3)]
        r = [w1 * G[ii][i] + w2 * G[ii + 1][i] for i in range(3)]
        if last:
            _clamp(d)                                                          # L:2029-2035; the frames' opening interpolation (L:1912-1918) is not clamped
        a0, gy0 = list(d), list(r)
        ii += 1
        t_start = T[f - 1]
        while st[ii] < T[f]:
            dt = st[ii] - t_start
            t_start = st[ii]
            d, r = list(A[ii]), list(G[ii])
            _clamp(d)
            step(a0, gy0, d, r, dt)
            a0, gy0 = list(d), list(r)
            ii += 1
        dt1 = T[f] - st[ii - 1]
        dt2 = st[ii] - T[f]
        w1 = dt2 / (dt1 + dt2)
        w2 = dt1 / (dt1 + dt2)
        d = [w1 * d[i] + w2 * A[ii][i] for i in range(3)]
        r = [w1 * r[i] + w2 * G[ii][i] for i in range(3)]
        _clamp(d)
        step(a0, gy0, d, r, dt1)
        if not last:
            ii -= 1
            p = [float(np.float32(v)) for v in P] if f32_positions else list(P)
            poses.append(p + mat_to_quat(R))
    end_q = mat_to_quat(R)
    nodes = [[float(v) for v in left]] + poses
    meas = []
    for k in range(n + 1):
        a = nodes[k]
        pb, qb = (nodes[k + 1][:3], nodes[k + 1][3:]) if k < n else (P, end_q)
        ia = qinv(np.array(a[3:]))
        dp = qrot(ia, np.array([pb[i] - a[i] for i in range(3)]))
        dq = qmul(ia, np.array(qb))
        meas.append(list(dp) + list(dq))
    return np.array(poses, np.float64).reshape(n, 7), (np.array(P), np.array(R), np.array(V)), np.array(meas, np.float64).reshape(n + 1, 7)


# ---------------------------------------------------------------- the factor
def _lmat(q):      # q * p = L(q) p
    w, x, y, z = q
    return np.array([[w, -x, -y, -z], [x, w, -z, y], [y, z, w, -x], [z, -y, x, w]])


def _rmat(p):      # q * p = R(p) q
    w, x, y, z = p
    return np.array([[w, -x, -y, -z], [x, w, z, -y], [y, -z, w, x], [z, y, -x, w]])


def _skew(v):
    return np.array([[0.0, -v[2], v[1]], [v[2], 0.0, -v[0]], [-v[1], v[0], 0.0]])


def factor_residual(a, b, m):
    """2 vec(dq^-1 qa^-1 qb), then qa^-1 (pb - pa) - dp; a, b = poses of the two nodes, m = (dp, dq); no quaternion is normalised (Eigen's inverse())"""
    ia, di = qinv(a[3:7]), qinv(m[3:7])
    e = qmul(qmul(di, ia), b[3:7])
    return np.concatenate([2.0 * e[1:4], qrot(ia, b[0:3] - a[0:3]) - m[0:3]])


def factor_jacobians(a, b, m):
    """(6 x 6, 6 x 6): d residual / d local coordinates (translation block, then rotation block) of node a and of node b"""
    qa, qb = a[3:7], b[3:7]
    n2 = qa[1] * qa[1] + qa[2] * qa[2] + qa[3] * qa[3] + qa[0] * qa[0]
    ia, di = qinv(qa), qinv(m[3:7])
    v = b[0:3] - a[0:3]
    w, u = ia[0], ia[1:4]
    dia = (np.diag([1.0, -1.0, -1.0, -1.0]) - 2.0 * np.outer(ia, qa)) / n2                   # d qa^-1 / d qa
    M = np.eye(3) + 2.0 * w * _skew(u) + 2.0 * (np.outer(u, u) - u.dot(u) * np.eye(3))       # d (q v) / d v at q = qa^-1 (Eigen's formula, q not unit)
    Dq = np.zeros((3, 4))                                                                    # d (q v) / d q
    Dq[:, 0] = 2.0 * np.cross(u, v)
    Dq[:, 1:] = -2.0 * w * _skew(v) + 2.0 * (u.dot(v) * np.eye(3) + np.outer(u, v) - 2.0 * np.outer(v, u))
    Ja, Jb = np.zeros((6, 6)), np.zeros((6, 6))
    Ja[0:3, 3:6] = 2.0 * ((_lmat(di) @ _rmat(qb))[1:4, :] @ dia) @ plus_jacobian(qa)
    Ja[3:6, 0:3] = -M
    Ja[3:6, 3:6] = (Dq @ dia) @ plus_jacobian(qa)
    Jb[0:3, 3:6] = 2.0 * _lmat(qmul(di, ia))[1:4, :] @ plus_jacobian(qb)
    Jb[3:6, 0:3] = M
    return Ja, Jb


class Chain:
    """n unknown poses between two anchors, n + 1 measurements; local dimension 6 n"""

    def __init__(self, left, right, meas):
        self.left, self.right = np.array(left, np.float64), np.array(right, np.float64)
        self.meas = np.array(meas, np.float64).reshape(-1, 7)
        self.n = self.meas.shape[0] - 1

    def nodes(self, x):
        return [self.left] + [x[k] for k in range(self.n)] + [self.right]

    def residuals(self, x):
        nd = self.nodes(x)
        return np.concatenate([factor_residual(nd[k], nd[k + 1], self.meas[k]) for k in range(self.n + 1)])

    def evaluate(self, x, want_jac=True):
        n, nd = self.n, self.nodes(x)
        r = self.residuals(x)
        cost = 0.5 * float(r @ r)
        if not want_jac:
            return cost, r, None
        J = np.zeros((6 * (n + 1), 6 * n))
        for k in range(n + 1):
            Ja, Jb = factor_jacobians(nd[k], nd[k + 1], self.meas[k])
            if k >= 1:
                J[6 * k:6 * k + 6, 6 * (k - 1):6 * k] = Ja
            if k < n:
                J[6 * k:6 * k + 6, 6 * k:6 * k + 6] = Jb
        return cost, r, J

    def plus(self, x, delta):
        out = np.array(x, np.float64).copy()
        for k in range(self.n):
            out[k, 0:3] = x[k, 0:3] + delta[6 * k:6 * k + 3]
            out[k, 3:7] = quat_plus(x[k, 3:7], delta[6 * k + 3:6 * k + 6])
        return out


# ---------------------------------------------------------------- the loop
def dogleg(chain, x0, max_num_iterations=15, function_tolerance=1e-6, gradient_tolerance=1e-10, parameter_tolerance=1e-8, initial_radius=1e4, max_radius=1e16,
           min_radius=1e-32, min_relative_decrease=1e-3, min_lm_diagonal=1e-6, max_lm_diagonal=1e32):
    """-> x, info(cost, initial_cost, iterations, successful_steps, termination, radius, mu), log (one entry per evaluated candidate)"""
    x = np.array(x0, np.float64).reshape(-1, 7).copy()
    n = chain.n
    log = []
    if n == 0:
        c = chain.evaluate(x, want_jac=False)[0]
        return x, dict(cost=c, initial_cost=c, iterations=0, successful_steps=0, termination="gradient_tolerance", radius=initial_radius, mu=1e-8), log
    cost, r, J = chain.evaluate(x)
    cost0 = cost
    scale = 1.0 / (1.0 + np.sqrt((J * J).sum(0)))
    radius, mu, reuse = initial_radius, 1e-8, False
    it, n_ok, n_invalid, termination = 0, 0, 0, "max_iterations"
    diag = g = gn = None
    alpha = 0.0
    while True:
        if it >= max_num_iterations:
            termination = "max_iterations"
            break
        if np.abs(J.T @ r).max() <= gradient_tolerance:
            termination = "gradient_tolerance"
            it += 1
            break
        if not (radius > min_radius):
            termination = "min_radius"
            break
        valid = True
        if not reuse:
            Js = J * scale
            diag = np.sqrt(np.clip((Js * Js).sum(0), min_lm_diagonal, max_lm_diagonal))
            g = (Js.T @ r) / diag
            jg = Js @ (g / diag)
            alpha = float(g @ g) / float(jg @ jg)
            valid = False
            for _ in range(9):
                if not (mu < 1.0):
                    break
                A = np.vstack([Js, np.diag(diag * np.sqrt(mu))])
                xs = np.linalg.lstsq(A, np.concatenate([r, np.zeros(6 * n)]), rcond=None)[0]
                if np.isfinite(xs).all():
                    valid = True
                    break
                mu *= 10.0
            if valid:
                gn = -xs * diag
                mu = max(1e-8, 2.0 * mu / 10.0)
        case = 0
        if valid:
            gn_norm, g_norm = float(np.sqrt(gn @ gn)), float(np.sqrt(g @ g))
            if gn_norm <= radius:
                case, step = 1, gn.copy()
            elif alpha * g_norm >= radius:
                case, step = 2, -(radius / g_norm) * g
            else:
                case = 3
                b_dot_a = -alpha * float(g @ gn)
                a2 = (alpha * g_norm) ** 2
                bma2 = a2 - 2.0 * b_dot_a + gn_norm * gn_norm
                c = b_dot_a - a2
                d = float(np.sqrt(c * c + bma2 * (radius * radius - a2)))
                beta = (d - c) / bma2 if c <= 0.0 else (radius * radius - a2) / (d + c)
                step = (-alpha * (1.0 - beta)) * g + beta * gn
            dogleg_norm = float(np.sqrt(step @ step))
            delta = step / diag * scale
            jd = J @ delta
            model_change = -float(jd @ (r + 0.5 * jd))
            valid = model_change > 0.0
        if not valid:
            mu *= 10.0
            reuse = False
            it += 1
            n_invalid += 1
            if n_invalid >= 5:
                termination = "numerical_failure"
                break
            continue
        n_invalid = 0
        x_new = chain.plus(x, delta)
        new_cost = chain.evaluate(x_new, want_jac=False)[0]
        rho = (cost - new_cost) / model_change
        step_norm = float(np.sqrt(delta @ delta))
        entry = dict(it=it, cost=cost, new_cost=new_cost, rho=rho, radius=radius, step=step_norm, case=case, reused=reuse, gn_norm=gn_norm, cauchy_norm=alpha * g_norm,
                     dogleg_norm=dogleg_norm, accepted=False)
        log.append(entry)
        xnorm = float(np.sqrt((x * x).sum()))
        entry["xnorm"] = xnorm
        stop = False
        if step_norm <= parameter_tolerance * (xnorm + parameter_tolerance):
            termination, stop = "parameter_tolerance", True
        elif abs(cost - new_cost) <= function_tolerance * cost:
            termination, stop = "function_tolerance", True
        elif rho > min_relative_decrease:
            entry["accepted"] = True
            x = x_new
            cost, r, J = chain.evaluate(x)
            if rho < 0.25:
                radius *= 0.5
            if rho > 0.75:
                radius = max(radius, 3.0 * dogleg_norm)
            reuse = False
            n_ok += 1
        else:
            radius *= 0.5
            reuse = True
            if not (radius > min_radius):
                termination, stop = ("max_iterations" if it + 1 >= max_num_iterations else "min_radius"), True
        it += 1
        if stop:
            break
    return x, dict(cost=cost, initial_cost=cost0, iterations=it, successful_steps=n_ok, termination=termination, radius=radius, mu=mu), log
