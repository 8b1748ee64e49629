"""Multi-precision referee of the pose graph's factor arithmetic (include/lili_hip.h, "Global pose graph", Conventions), mpmath at DPS digits.

Written from the header's conventions, not from the kernel or from tests/pose_graph_model.py:
  a pose is p (3) then q (w, x, y, z); the tangent is xi = (omega, v), rotation first; X (+) xi = (p + R v, normalise(q Exp(omega)));
  between(A, B) = (R_A^T (p_B - p_A), q_A^-1 q_B);
  between-factor on (a, b), measurement Z = (t_Z, q_Z), variances s^2:  e = (Log(R_Z^T R_A^T R_B), R_Z^T (R_A^T (p_B - p_A) - t_Z)),  r = e / s;
  the prior is the same factor with A the identity; node 0's prior sits at its pose as given; the chain measurement of node i is between(pose[i - 1], pose[i]) of
  the poses as given (the first node of a later append: between(prev, poses[0])); quaternions are normalised on entry (here: in mp);
  a robust loop is linearised as sqrt(w) r, sqrt(w) J and adds rho to the cost (Huber, Cauchy, Geman-McClure as the header writes them).
Its Jacobians follow from those lines: with E = R_Z^T R_A^T R_B, phi = Log(E) and X (+) xi on either node,
  Log(E Exp(w)) = phi + Jr^-1(phi) w + ...                       -> d e_rot / d omega_B = Jr^-1
  R_A -> R_A Exp(w) turns E into E Exp(-R_AB^T w)                -> d e_rot / d omega_A = -Jr^-1 R_AB^T,  R_AB = R_A^T R_B
  p_B -> p_B + R_B v                                             -> d e_v / d v_B = R_Z^T R_A^T R_B
  p_A -> p_A + R_A v,  R_A^T -> (I - [w]x) R_A^T                 -> d e_v / d v_A = -R_Z^T,  d e_v / d omega_A = R_Z^T [d]x,  d = R_A^T (p_B - p_A)
and tests/test_pose_graph_factor_cases_cpu.py checks every block against central differences of `error` through `retract` at 50 digits.
No series and no threshold: Jr^-1 = I + [phi]x / 2 + c [phi]x^2, c = 1 / t^2 - (1 + cos t) / (2 t sin t) in mp at every t > 0; the limits c = 1 / 12 and Log's factor 2
at t = 0 exactly.  Log's sign convention (w < 0 negates q) is applied to the mp value of q_e.

Every gradient and block entry comes with its magnitude sum A: the same sum with every term replaced by its absolute value.  Stopped at the products
J[k][i] J[k][j] that sum is too short: an entry of a rotation matrix built from a generic quaternion, 1 - 2 (y^2 + z^2) say, can be 1e-17 and still round like 1.  So
the sum is followed down to the inputs, to first order and without compounding: a number here is a pair (value, magnitude) with
  an input          m = |x|
  a + b, a - b      m = m_a + m_b                                   (the terms' absolute values add)
  a b               m = max(|a| m_b, m_a |b|)                       (a product of accurate numbers has the magnitude |a b|, nothing more)
  a / b             m = max(m_a / |b|, |a| m_b / b^2)
  f(a)              m = max(|f(a)|, |f'(a)| m_a)                    (sqrt, sin, cos, atan2, log1p, and the coefficient c as a function of t)
so m is the entry's value wherever no sum cancels, and the size of the cancelling terms where one does.  At generic states A is within 64 times the largest value
of the entry's 3 x 3 quadrant (tests/test_pose_graph_factor_cases_cpu.py asserts it, and that the f64 model's error is of the order of eps in units of A); in a
frame whose quaternions are exact units every product has one non-zero term, and the magnitude of a 1e-12 residual is 1e-12.  How many roundings meet in an entry is
not in A: that is what the 64 of the tests' 64 eps is for.  c(t) is smooth up to pi (its limit is 1 / pi^2), so A holds nothing of the cancellation that the f64
closed form meets there."""
import mpmath as mp
import numpy as np

DPS = 50
NONE, HUBER, CAUCHY, GEMAN_MCCLURE = 0, 1, 2, 3


def hp(fn):
    """run at DPS digits whatever the caller's precision is"""
    def wrapped(*a, **kw):
        with mp.workdps(DPS):
            return fn(*a, **kw)
    wrapped.__name__, wrapped.__doc__ = fn.__name__, fn.__doc__
    return wrapped


class V:
    """a value and its magnitude (see the module's text)"""
    __slots__ = ("v", "m")

    def __init__(self, v, m=None):
        self.v = v.v if isinstance(v, V) else mp.mpf(v)
        self.m = abs(self.v) if m is None else m

    def __add__(self, o):
        o = o if isinstance(o, V) else V(o)
        return V(self.v + o.v, self.m + o.m)
    __radd__ = __add__

    def __sub__(self, o):
        o = o if isinstance(o, V) else V(o)
        return V(self.v - o.v, self.m + o.m)

    def __rsub__(self, o):
        return V(o) - self

    def __neg__(self):
        return V(-self.v, self.m)

    def __mul__(self, o):
        o = o if isinstance(o, V) else V(o)
        return V(self.v * o.v, max(abs(self.v) * o.m, self.m * abs(o.v)))
    __rmul__ = __mul__

    def __truediv__(self, o):
        o = o if isinstance(o, V) else V(o)
        return V(self.v / o.v, max(self.m / abs(o.v), abs(self.v) * o.m / (o.v * o.v)))

    def __rtruediv__(self, o):
        return V(o) / self

    def __abs__(self):
        return V(abs(self.v), self.m)

    def __float__(self):
        return float(self.v)

    def __lt__(self, o):
        return self.v < val(o)

    def __le__(self, o):
        return self.v <= val(o)

    def __gt__(self, o):
        return self.v > val(o)

    def __ge__(self, o):
        return self.v >= val(o)

    def __eq__(self, o):
        return self.v == val(o)
    __hash__ = None


def val(x):
    return x.v if isinstance(x, V) else x


def vals(x):
    """the plain mpf values of a (nested) list of pairs"""
    return [vals(y) for y in x] if isinstance(x, list) else val(x)


def _fun(f, df, a):
    y = f(a.v)
    return V(y, max(abs(y), abs(df(a.v)) * a.m))


def vsqrt(a):
    if a.v == 0:
        return V(0, mp.sqrt(a.m))
    return _fun(mp.sqrt, lambda x: 1 / (2 * mp.sqrt(x)), a)


def vsin(a):
    return _fun(mp.sin, mp.cos, a)


def vcos(a):
    return _fun(mp.cos, mp.sin, a)


def vlog1p(a):
    return _fun(mp.log1p, lambda x: 1 / (1 + x), a)


def vatan2(n, w):
    y, h = mp.atan2(n.v, w.v), n.v * n.v + w.v * w.v
    return V(y, max(abs(y), (abs(w.v) * n.m + abs(n.v) * w.m) / h))


def _c_of_t(t):
    return 1 / (t * t) - (1 + mp.cos(t)) / (2 * t * mp.sin(t))


# ---- small algebra on lists of pairs -----------------------------------------------------------------------------------
def vec(v):
    """f64 inputs (or mpf values) as exact pairs"""
    return [x if isinstance(x, V) else V(x if isinstance(x, mp.mpf) else mp.mpf(float(x))) for x in v]


def qmul(a, b):
    return [a[0] * b[0] - a[1] * b[1] - a[2] * b[2] - a[3] * b[3], a[0] * b[1] + a[1] * b[0] + a[2] * b[3] - a[3] * b[2],
            a[0] * b[2] + a[2] * b[0] + a[3] * b[1] - a[1] * b[3], a[0] * b[3] + a[3] * b[0] + a[1] * b[2] - a[2] * b[1]]


def qconj(q):
    return [q[0], -q[1], -q[2], -q[3]]


def qnormalize(q):
    n = vsqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3])
    return [x / n for x in q]


def qmat(q):
    """rotation matrix of a unit quaternion"""
    w, x, y, z = q
    return [[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
            [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
            [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]]


def mT(M):
    return [[M[j][i] for j in range(len(M))] for i in range(len(M[0]))]


def mm(A, B):
    return [[sum(A[i][k] * B[k][j] for k in range(len(B))) for j in range(len(B[0]))] for i in range(len(A))]


def mv(M, v):
    return [sum(M[i][k] * v[k] for k in range(len(v))) for i in range(len(M))]


def skew(v):
    return [[0, -v[2], v[1]], [v[2], 0, -v[0]], [-v[1], v[0], 0]]


def qexp(w):
    w = vec(w)
    t2 = w[0] * w[0] + w[1] * w[1] + w[2] * w[2]
    if t2 == 0:
        return vec([1, 0, 0, 0])
    t = vsqrt(t2)
    s = vsin(t / 2) / t
    return [vcos(t / 2), s * w[0], s * w[1], s * w[2]]


def qlog(q):
    """rotation vector of a unit quaternion, angle in [0, pi]: w < 0 negates q"""
    if q[0] < 0:
        q = [-x for x in q]
    n2 = q[1] * q[1] + q[2] * q[2] + q[3] * q[3]
    if n2 == 0:
        return [2 * q[1], 2 * q[2], 2 * q[3]]
    n = vsqrt(n2)
    k = 2 * vatan2(n, q[0]) / n
    return [k * q[1], k * q[2], k * q[3]]


def jr_inv(phi):
    t2 = phi[0] * phi[0] + phi[1] * phi[1] + phi[2] * phi[2]
    if t2 == 0:
        c = V(mp.mpf(1) / 12)
    else:
        c = _fun(_c_of_t, lambda x: mp.diff(_c_of_t, x), vsqrt(t2))
    S = skew(phi)
    S2 = mm(S, S)
    return [[(1 if i == j else 0) + S[i][j] / 2 + c * S2[i][j] for j in range(3)] for i in range(3)]


def pose(P):
    """7 numbers -> (p, q) in mp, q normalised: what the library does on entry"""
    P = vec(P)
    return P[0:3], qnormalize(P[3:7])


IDENTITY = (vec([0, 0, 0]), vec([1, 0, 0, 0]))


def retract(X, xi):
    p, q = X
    R = qmat(q)
    dv = mv(R, xi[3:6])
    return [p[i] + dv[i] for i in range(3)], qnormalize(qmul(q, qexp(xi[0:3])))


def between(A, B):
    (pa, qa), (pb, qb) = A, B
    return mv(mT(qmat(qa)), [pb[i] - pa[i] for i in range(3)]), qmul(qconj(qa), qb)


def error(A, B, Z):
    """e (6) of the between factor (A = IDENTITY: the prior), and q_e"""
    (pa, qa), (pb, qb), (tz, qz) = A, B, Z
    RzT = mT(qmat(qz))
    d = mv(mT(qmat(qa)), [pb[i] - pa[i] for i in range(3)])
    qe = qmul(qconj(qz), qmul(qconj(qa), qb))
    return qlog(qe) + mv(RzT, [d[i] - tz[i] for i in range(3)]), qe


def jacobians(A, B, Z):
    """e, d e / d xi_A, d e / d xi_B (6 x 6 each, unweighted), q_e"""
    (pa, qa), (pb, qb), (tz, qz) = A, B, Z
    e, qe = error(A, B, Z)
    Ra, Rb, RzT = qmat(qa), qmat(qb), mT(qmat(qz))
    Rab = mm(mT(Ra), Rb)
    d = mv(mT(Ra), [pb[i] - pa[i] for i in range(3)])
    Jri = jr_inv(e[0:3])
    zero = V(0)
    Ja = [[zero] * 6 for _ in range(6)]
    Jb = [[zero] * 6 for _ in range(6)]
    JA = mm(Jri, mT(Rab))
    VA = mm(RzT, skew(d))
    Re = mm(RzT, Rab)
    for i in range(3):
        for j in range(3):
            Ja[i][j] = -JA[i][j]
            Ja[3 + i][j] = VA[i][j]
            Ja[3 + i][3 + j] = -RzT[i][j]
            Jb[i][j] = Jri[i][j]
            Jb[3 + i][3 + j] = Re[i][j]
    return e, Ja, Jb, qe


def loss_weight(kind, k, d2):
    if kind == NONE:
        return V(1)
    if kind == HUBER:
        d = vsqrt(d2)
        return V(1) if d <= k else k / d
    u = k * k / (k * k + d2)
    return u if kind == CAUCHY else u * u


def loss_rho(kind, k, d2):
    if kind == NONE:
        return d2 / 2
    if kind == HUBER:
        d = vsqrt(d2)
        return d2 / 2 if d <= k else k * (d - k / 2)
    if kind == CAUCHY:
        return k * k / 2 * vlog1p(d2 / (k * k))
    return k * k / 2 * d2 / (k * k + d2)


# ---- a graph ---------------------------------------------------------------------------------------------------------
class Graph:
    """given (N, 7): the poses at append time; prev: None, or the pose handed to a second append that starts at node `split` (the measurement of node `split` is
    between(prev, given[split])); estimates (N, 7); loops [(from, to, meas (7), var (6), loss, scale)]; prior_var, odom_var (6).  All as the f64 numbers the
    library is given: they are exact inputs here."""

    @hp
    def __init__(self, given, estimates, loops, prior_var, odom_var, prev=None, split=1):
        self.n = len(given)
        G = [pose(P) for P in given]
        self.meas = [G[0]]
        for i in range(1, self.n):
            self.meas.append(between(pose(prev) if prev is not None and i == split else G[i - 1], G[i]))
        self.X = [pose(P) for P in estimates]
        self.loops = [(int(a), int(b), pose(m), [1 / vsqrt(V(float(v))) for v in var], int(kind), V(float(k))) for a, b, m, var, kind, k in loops]
        self.w_prior = [1 / vsqrt(V(float(v))) for v in prior_var]
        self.w_odom = [1 / vsqrt(V(float(v))) for v in odom_var]

    def factor_inputs(self, X, f):
        """a (-1: the prior), b, A, B, Z, whitening weights, loss, scale"""
        if f == 0:
            return -1, 0, IDENTITY, X[0], self.meas[0], self.w_prior, NONE, V(0)
        if f < self.n:
            return f - 1, f, X[f - 1], X[f], self.meas[f], self.w_odom, NONE, V(0)
        a, b, Z, w, kind, k = self.loops[f - self.n]
        return a, b, X[a], X[b], Z, w, kind, k

    def factor(self, X, f):
        """dict: a, b; plain mpf values r0, Ja0, Jb0 (whitened, before the loss), d2, w, rho, qe, e; pairs r, Ja, Jb (scaled by sqrt(w)) and d2V, wV, rhoV"""
        a, b, A, B, Z, w, kind, k = self.factor_inputs(X, f)
        e, Ja, Jb, qe = jacobians(A, B, Z)
        r0 = [e[i] * w[i] for i in range(6)]
        Ja0 = [[Ja[i][j] * w[i] for j in range(6)] for i in range(6)]
        Jb0 = [[Jb[i][j] * w[i] for j in range(6)] for i in range(6)]
        d2 = sum(x * x for x in r0)
        wl = loss_weight(kind, k, d2)
        sw = vsqrt(wl)
        rho = loss_rho(kind, k, d2)
        return dict(a=a, b=b, r0=vals(r0), Ja0=vals(Ja0), Jb0=vals(Jb0), d2=d2.v, w=wl.v, rho=rho.v, qe=vals(qe), e=vals(e),
                    r=[x * sw for x in r0], Ja=[[x * sw for x in row] for row in Ja0], Jb=[[x * sw for x in row] for row in Jb0])

    def cost(self, X):
        return sum(self.factor(X, f)["rho"] for f in range(self.n + len(self.loops)))

    def normal_equations(self, X):
        """dense H (6 N x 6 N) and g (6 N) as pairs, and the factors"""
        n6 = 6 * self.n
        H = [[V(0)] * n6 for _ in range(n6)]
        g = [V(0)] * n6
        F = [self.factor(X, f) for f in range(self.n + len(self.loops))]
        for fac in F:
            cols = ([(fac["a"], fac["Ja"])] if fac["a"] >= 0 else []) + [(fac["b"], fac["Jb"])]
            for ni, Ji in cols:
                for i in range(6):
                    for k in range(6):
                        g[6 * ni + i] = g[6 * ni + i] + Ji[k][i] * fac["r"][k]
                    for nj, Jj in cols:
                        for j in range(6):
                            for k in range(6):
                                H[6 * ni + i][6 * nj + j] = H[6 * ni + i][6 * nj + j] + Ji[k][i] * Jj[k][j]
        return H, g, F


def _blocks(H, pairs, what):
    return np.array([[[float(getattr(H[6 * a + i][6 * b + j], what)) for j in range(6)] for i in range(6)] for a, b in pairs], dtype=np.float64).reshape(-1, 6, 6)


def _chain_sub(F, n):
    """H block (i + 1, i) of the chain factor alone, and its magnitude sums"""
    S, AS = np.zeros((n - 1, 6, 6)), np.zeros((n - 1, 6, 6))
    for f in range(1, n):
        Ja, Jb = F[f]["Ja"], F[f]["Jb"]
        for i in range(6):
            for j in range(6):
                t = sum(Jb[k][i] * Ja[k][j] for k in range(6))
                S[f - 1, i, j], AS[f - 1, i, j] = float(t.v), float(t.m)
    return S, AS


def _loop_blocks(F, n):
    """H block (from, to) of every loop alone, and its magnitude sums"""
    L = len(F) - n
    B, AB = np.zeros((L, 6, 6)), np.zeros((L, 6, 6))
    for l in range(L):
        Ja, Jb = F[n + l]["Ja"], F[n + l]["Jb"]
        for i in range(6):
            for j in range(6):
                t = sum(Ja[k][i] * Jb[k][j] for k in range(6))
                B[l, i, j], AB[l, i, j] = float(t.v), float(t.m)
    return B, AB


@hp
def evaluate(graph, X=None):
    """What lili_pose_graph_evaluate and lili_pose_graph_loop_status document, in the former's layout, rounded to f64 at the end.
    -> dict: cost, gradient (N, 6), diag (N, 6, 6), sub (N - 1, 6, 6), loop (L, 6, 6), d2 (L), w (L), and A_<name> for each (for the scalars: the value)."""
    X = graph.X if X is None else X
    n = graph.n
    H, g, F = graph.normal_equations(X)
    out = dict(cost=float(sum(f["rho"] for f in F)))
    out["gradient"] = np.array([float(x.v) for x in g]).reshape(n, 6)
    out["A_gradient"] = np.array([float(x.m) for x in g]).reshape(n, 6)
    out["diag"], out["A_diag"] = _blocks(H, [(i, i) for i in range(n)], "v"), _blocks(H, [(i, i) for i in range(n)], "m")
    out["sub"], out["A_sub"] = _chain_sub(F, n)
    out["loop"], out["A_loop"] = _loop_blocks(F, n)
    out["d2"] = np.array([float(f["d2"]) for f in F[n:]])
    out["w"] = np.array([float(f["w"]) for f in F[n:]])
    out["A_cost"], out["A_d2"], out["A_w"] = abs(out["cost"]), np.abs(out["d2"]), np.abs(out["w"])
    return out


def poses_f64(X):
    return np.array([[float(v) for v in p] + [float(v) for v in q] for p, q in X])


@hp
def gauss_newton_step(graph, X=None):
    """One Gauss-Newton iteration in mp: the dense 6 N system H delta = -g, the retraction, the candidate's cost.
    -> dict: cost (at X), new_cost, step_inf, poses (N, 7, rounded to f64), X (the mp candidate)"""
    X = graph.X if X is None else X
    H, g, F = graph.normal_equations(X)
    n6 = 6 * graph.n
    delta = mp.lu_solve(mp.matrix(vals(H)), mp.matrix([-x.v for x in g]))
    delta = [delta[i] for i in range(n6)]
    Xn = [retract(X[i], delta[6 * i:6 * i + 6]) for i in range(graph.n)]
    return dict(cost=float(sum(f["rho"] for f in F)), new_cost=float(graph.cost(Xn)), step_inf=float(max(abs(x) for x in delta)), poses=poses_f64(Xn), X=Xn)


@hp
def numeric_jacobians(graph, f, X=None, h="1e-20"):
    """central differences of factor f's whitened error through retract -> Ja (None for the prior), Jb as 6 x 6 lists of mpf"""
    X = graph.X if X is None else X
    h = mp.mpf(h)
    a, b, A, B, Z, w, _, _ = graph.factor_inputs(X, f)

    def column(which, j):
        xi, mi = vec([0] * 6), vec([0] * 6)
        xi[j], mi[j] = V(h), V(-h)
        if which == 0:
            ep, em = error(retract(A, xi), B, Z)[0], error(retract(A, mi), B, Z)[0]
        else:
            ep, em = error(A, retract(B, xi), Z)[0], error(A, retract(B, mi), Z)[0]
        return [((ep[i] - em[i]) / (2 * h) * w[i]).v for i in range(6)]

    Jb = mT([column(1, j) for j in range(6)])
    Ja = mT([column(0, j) for j in range(6)]) if a >= 0 else None
    return Ja, Jb


@hp
def compose_rotation(q, theta, axis):
    """q Exp(theta axis / |axis|) as plain mpf values (q normalised first); theta an mpf or a string, axis strings or numbers"""
    ax = [mp.mpf(x) for x in axis]
    n = mp.sqrt(sum(x * x for x in ax))
    th = mp.mpf(theta)
    return vals(qmul(qnormalize(vec(q)), qexp([th * x / n for x in ax])))
