"""Designed cases and an exact model for the window's closed-form factors (win_imu_raw, win_prior_block and the assembly of win_build in
lili_om_amd/csrc/lili_window.hip), shared by tests/test_window_factor_cases_cpu.py and tests/test_window_factors_gpu.py.

THE MODEL restates, in mpmath at 60 digits,
  ImuFactor::Evaluate + Preintegration::evaluate   L/include/factors/ImuFactor.h:18-144, Preintegration.h:186-211 (math_tools.h: Qleft, Qright,
                                                   LeftQuatMatrix, deltaQ), with sqrt_info = LLT(covariance^-1).matrixL()^T exact,
  MarginalizationFactor::Evaluate                  L/src/MarginalizationFactor.cpp:233-283 (held to those lines by reading them: the shim's Eigen
                                                   stand-in has no run-time sizes, so that function is not compiled),
  the speed-bias prior                             r = 15 (sb - mean), J = 15 I (PriorFactor.h:13-23),
  Ceres' plus-Jacobian (QuaternionParameterization::ComputeJacobian) and the assembly to (cost, g, H) in local coordinates, n_kf = 2 .. 4,
  and the last-three-columns variant (MarginalizationFactor.cpp:9-17; win_build<true>: of the IMU factors only the one between keyframes 0 and 1).
Quaternion expressions have Eigen 3.3's shape (inverse = conjugate / squared norm, q * v = v + w (2 u x v) + u x (2 u x v), toRotationMatrix).

MAGNITUDES.  Every number of the model is a pair (value, magnitude): the magnitude is the same expression with every term of a sum or difference
replaced by its absolute value and every product by the product of the magnitudes (f64 is enough for it).  An entry of cost, g or H is judged
against ITS OWN magnitude — where Pj - Pi - Vi s cancels from 1e4 m to 0.2 m the magnitude says 1e4 — never against the largest entry of the
matrix.  A magnitude of 0 means a structural zero: only exact zeros were added.

CASES.  `cases()` lists them by family; each has a one-line claim (`claim`, `check_claim`) about what it reaches, asserted on the model by the CPU
file.  State quaternions are unit up to rounding throughout (what an un-normalised state should give is pinned nowhere).

COST.  The model of all cases of the GPU file, cached per session, takes about 12 s of one CPU (5 s for the 132 evaluations, 6 s for the 75 last-three-columns
systems and their Schur complements).  Structural zeros are skipped (sparse rows).  Only the bias steps are thin (one direction for dbg and dba); the
families are complete.
"""
import functools

import mpmath as mp
import numpy as np

import lili_om_amd as L
from oracle import lo_window as W

mp.mp.dps = 60
U = 2.0 ** -53
MUTATIONS = ("cq_conjugate", "qleft_sign", "qright_sign", "dq_swap", "rq_unified", "dw_strict", "dq_dbg_transposed", "jraw_18", "prior_T_one_side")


# ---------------------------------------------------------------- numbers with magnitudes
class N:
    __slots__ = ("v", "m")

    def __init__(self, v, m=None):
        self.v = v if isinstance(v, mp.mpf) else mp.mpf(float(v))
        self.m = abs(float(v)) if m is None else m

    def __add__(self, o):
        if not isinstance(o, N):
            o = N(o)
        return N(self.v + o.v, self.m + o.m)
    __radd__ = __add__

    def __sub__(self, o):
        if not isinstance(o, N):
            o = N(o)
        return N(self.v - o.v, self.m + o.m)

    def __rsub__(self, o):
        return N(o) - self

    def __mul__(self, o):
        if not isinstance(o, N):
            o = N(o)
        return N(self.v * o.v, self.m * o.m)
    __rmul__ = __mul__

    def __truediv__(self, o):
        if not isinstance(o, N):
            o = N(o)
        return N(self.v / o.v, self.m / abs(float(o.v)))

    def __neg__(self):
        return N(-self.v, self.m)

    def sqrt(self):
        return N(mp.sqrt(self.v), float(np.sqrt(self.m)))


ZERO, ONE = N(0.0), N(1.0)


def nv(a):
    return [N(float(x)) for x in np.asarray(a, np.float64).reshape(-1)]


def sumn(terms):
    terms = list(terms)
    if not terms:
        return ZERO
    return N(mp.fsum(t.v for t in terms), float(sum(t.m for t in terms)))


def dot(a, b):
    return sumn(x * y for x, y in zip(a, b) if x.m != 0.0 and y.m != 0.0)


def cross(a, b):
    return [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]


def qmul(a, b):
    return [a[0] * b[0] - a[1] * b[1] - a[2] * b[2] - a[3] * b[3], a[0] * b[1] + a[1] * b[0] + a[2] * b[3] - a[3] * b[2],
            a[0] * b[2] + a[2] * b[0] + a[3] * b[1] - a[1] * b[3], a[0] * b[3] + a[3] * b[0] + a[1] * b[2] - a[2] * b[1]]


def qn2(q):
    return q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]


def qinv(q, conjugate=False):
    if conjugate:
        return [q[0], -q[1], -q[2], -q[3]]
    n2 = qn2(q)
    return [q[0] / n2, -(q[1] / n2), -(q[2] / n2), -(q[3] / n2)]


def qnormalized(q):
    n = qn2(q).sqrt()
    return [c / n for c in q]


def qrot(q, v):
    u = q[1:]
    uv = cross(u, v)
    uv = [c + c for c in uv]
    w = cross(u, uv)
    return [v[i] + q[0] * uv[i] + w[i] for i in range(3)]


def qmat(q):
    w, x, y, z = q
    tx, ty, tz = 2.0 * x, 2.0 * y, 2.0 * z
    twx, twy, twz, txx, txy, txz, tyy, tyz, tzz = tx * w, ty * w, tz * w, tx * x, ty * x, tz * x, ty * y, tz * y, tz * z
    return [[1.0 - (tyy + tzz), txy - twz, txz + twy], [txy + twz, 1.0 - (txx + tzz), tyz - twx], [txz - twy, tyz + twx, 1.0 - (txx + tyy)]]


def skew(v):
    return [[ZERO, -v[2], v[1]], [v[2], ZERO, -v[0]], [-v[1], v[0], ZERO]]


def q_left(q, mut=None):       # math_tools.h Qleft: [w, -v^T; v, w I + [v]x]
    sk = skew(q[1:])
    m = [[q[0], -q[1], -q[2], -q[3]]] + [[q[1 + i]] + [(q[0] if i == c else ZERO) + sk[i][c] for c in range(3)] for i in range(3)]
    if mut == "qleft_sign":
        m[2][1] = -m[2][1]       # row 2 (of rows 1..3), the +z of the skew part
    return m


def q_right(p, mut=None):      # math_tools.h Qright: [w, -v^T; v, w I - [v]x]
    sk = skew(p[1:])
    m = [[p[0], -p[1], -p[2], -p[3]]] + [[p[1 + i]] + [(p[0] if i == c else ZERO) - sk[i][c] for c in range(3)] for i in range(3)]
    if mut == "qright_sign":
        m[1][3] = -m[1][3]
    return m


def plus_jacobian(q):          # ceres::QuaternionParameterization::ComputeJacobian, 4 x 3, of the RAW state quaternion
    w, x, y, z = q
    return [[-x, -y, -z], [w, z, -y], [-z, w, x], [y, -x, w]]


def matmul(A, B):
    cols = list(zip(*B))
    return [[dot(r, c) for c in cols] for r in A]


# ---------------------------------------------------------------- sqrt_info = LLT(cov^-1).matrixL()^T, exact
@functools.lru_cache(maxsize=None)
def _sqrt_info_cached(key):
    cov = np.frombuffer(key, np.float64).reshape(15, 15)
    A = mp.matrix(15, 15)
    for i in range(15):
        for j in range(15):
            A[i, j] = (mp.mpf(float(cov[i, j])) + mp.mpf(float(cov[j, i]))) / 2
    Li = mp.cholesky(mp.inverse(A))
    return [{j: N(Li[j, i]) for j in range(i, 15) if Li[j, i] != 0} for i in range(15)]      # rows of L^T, sparse


def sqrt_info(cov):
    return _sqrt_info_cached(np.ascontiguousarray(cov, np.float64).tobytes())


def host_sqrt_info(cov):
    """lili_window_sqrt_info's f64 result (host code of the product, no GPU), and the same as the model's sparse rows: its entries taken as exact"""
    S = L.api.window_sqrt_info(cov)
    return S, [{j: N(float(S[i, j])) for j in range(15) if S[i, j] != 0.0} for i in range(15)]


# ---------------------------------------------------------------- ImuFactor::Evaluate, un-whitened
def imu_factor_global(rec, xi, xj, mut=None):
    """residual[15] and the six GLOBAL Jacobian blocks (15x3, 15x4, 15x9, 15x3, 15x4, 15x9) as sparse {(row, col): N}, un-whitened; aux: rq, cq."""
    xi, xj = nv(xi), nv(xj)
    Pi, Pj = xi[0:3], xj[0:3]
    Qi, Qj = qnormalized(xi[3:7]), qnormalized(xj[3:7])
    Vi, Bai, Bgi, Vj, Baj, Bgj = xi[7:10], xi[10:13], xi[13:16], xj[7:10], xj[10:13], xj[13:16]
    g, s = nv(rec["g"]), N(float(rec["sum_dt"]))
    Jp = np.asarray(rec["jacobian"], np.float64).reshape(15, 15)
    blk = lambda r, c: [nv(Jp[r + i, c:c + 3]) for i in range(3)]
    dp_dba, dp_dbg, dq_dbg, dv_dba, dv_dbg = blk(0, 9), blk(0, 12), blk(3, 12), blk(6, 9), blk(6, 12)
    if mut == "dq_dbg_transposed":
        dq_dbg = [list(r) for r in zip(*dq_dbg)]
    dba = [a - b for a, b in zip(Bai, nv(rec["lin_ba"]))]
    dbg = [a - b for a, b in zip(Bgi, nv(rec["lin_bg"]))]
    th = [dot(r, dbg) for r in dq_dbg]
    cq = qmul(nv(rec["delta_q"]), [ONE] + [t / 2.0 for t in th])
    cv = [a + dot(r1, dba) + dot(r2, dbg) for a, r1, r2 in zip(nv(rec["delta_v"]), dv_dba, dv_dbg)]
    cp = [a + dot(r1, dba) + dot(r2, dbg) for a, r1, r2 in zip(nv(rec["delta_p"]), dp_dba, dp_dbg)]
    Qi_inv = qinv(Qi)
    cq_inv = qinv(cq, conjugate=(mut == "cq_conjugate"))
    tmp = [(-0.5) * g[i] * s * s + Pj[i] - Pi[i] - Vi[i] * s for i in range(3)]
    tmp1 = [-(g[i] * s) + Vj[i] - Vi[i] for i in range(3)]
    rp = [a - b for a, b in zip(qrot(Qi_inv, tmp), cp)]
    rq = qnormalized(qmul(cq_inv, qmul(Qi_inv, Qj)))
    if mut == "rq_unified" and rq[0].v < 0:
        rq = [-c for c in rq]
    rv = [a - b for a, b in zip(qrot(Qi_inv, tmp1), cv)]
    r = rp + [2.0 * c for c in rq[1:]] + rv + [a - b for a, b in zip(Baj, Bai)] + [a - b for a, b in zip(Bgj, Bgi)]
    Ri = qmat(Qi_inv)
    u = Qi[1:]
    J = [dict() for _ in range(6)]

    def put(b, r0, c0, M, sign=1.0):
        for i, row in enumerate(M):
            for c, v in enumerate(row):
                if v.m != 0.0:
                    J[b][(r0 + i, c0 + c)] = v if sign == 1.0 else -v

    def dq_block(v, r0):          # :63-64, :71-72
        uxv, uv, sk = cross(u, v), dot(u, v), skew(v)
        c0 = [2.0 * (Qi[0] * v[i] + uxv[i]) for i in range(3)]
        a, b = (v, u) if mut == "dq_swap" else (u, v)
        c1 = [[2.0 * ((uv if i == c else ZERO) + a[i] * b[c] - b[i] * a[c] - Qi[0] * sk[i][c]) for c in range(3)] for i in range(3)]
        put(1, r0, 0, [[c0[i]] + c1[i] for i in range(3)])

    put(0, 0, 0, Ri, -1.0)
    dq_block(tmp, 0)
    put(1, 3, 0, [[-2.0 * v for v in row] for row in matmul(q_left(qinv(Qj), mut), q_right(cq, mut))[1:4]])
    dq_block(tmp1, 6)
    put(2, 0, 0, [[-(v * s) for v in row] for row in Ri])
    put(2, 0, 3, dp_dba, -1.0)
    put(2, 0, 6, dp_dbg, -1.0)
    a = qmul(qmul(qinv(Qj), Qi), cq)
    ska = skew(a[1:])
    M = [[(a[0] if i == c else ZERO) + ska[i][c] for c in range(3)] for i in range(3)]      # LeftQuatMatrix(.)[0:3, 0:3]
    put(2, 3, 6, matmul(M, dq_dbg), -1.0)
    put(2, 6, 0, Ri, -1.0)
    put(2, 6, 3, dv_dba, -1.0)
    put(2, 6, 6, dv_dbg, -1.0)
    for i in range(3):
        J[2][(9 + i, 3 + i)] = -ONE
        J[2][(12 + i, 6 + i)] = -ONE
        J[5][(9 + i, 3 + i)] = ONE
        J[5][(12 + i, 6 + i)] = ONE
    put(3, 0, 0, Ri)
    put(4, 3, 0, [[2.0 * v for v in row] for row in q_left(qmul(cq_inv, Qi_inv), mut)[1:4]])
    put(5, 6, 0, Ri)
    return r, J, dict(rq=rq, cq=cq, xi_q=xi[3:7], xj_q=xj[3:7])


def imu_factor_local(rec, xi, xj, last3=False, mut=None):
    """rows[15] of {col: N}: 30 local columns (keyframe i, keyframe j), column 30 = the residual; un-whitened.  last3: quaternion blocks by the last
    three of their four global columns instead of through the plus-Jacobian."""
    r, J, aux = imu_factor_global(rec, xi, xj, mut)
    rows = [dict() for _ in range(15)]
    for i in range(15):
        if r[i].m != 0.0:
            rows[i][30] = r[i]
    offs = (0, 3, 6, 15, 18, 21)
    if mut == "jraw_18":
        offs = (0, 3, 6, 18, 18, 21)
    for b in range(6):
        if b in (1, 4):
            Pq = plus_jacobian(aux["xi_q"] if b == 1 else aux["xj_q"])
            for i in range(15):
                g4 = [J[b].get((i, c)) for c in range(4)]
                if all(v is None for v in g4):
                    continue
                for c in range(3):
                    if last3:
                        v = g4[1 + c] if g4[1 + c] is not None else ZERO
                    else:
                        v = sumn(g4[k] * Pq[k][c] for k in range(4) if g4[k] is not None)
                    if v.m != 0.0:
                        rows[i][offs[b] + c] = rows[i][offs[b] + c] + v if offs[b] + c in rows[i] else v
        else:
            for (i, c), v in J[b].items():
                rows[i][offs[b] + c] = rows[i][offs[b] + c] + v if offs[b] + c in rows[i] else v
    return rows, aux


def whiten(S, rows):
    out = []
    for i in range(15):
        acc = {}
        for j, sij in S[i].items():
            for c, v in rows[j].items():
                acc.setdefault(c, []).append(sij * v)
        out.append({c: (t[0] if len(t) == 1 else sumn(t)) for c, t in acc.items()})
    return out


# ---------------------------------------------------------------- the window: (cost, g, H) in local coordinates
class Acc:
    def __init__(self, n):
        self.n, self.H, self.g, self.cost = n, {}, {}, []

    def add_rows(self, rows, cols, rcol):
        """+= J^T J, J^T r, 1/2 r^T r of sparse rows {col: N}; cols maps a row's column to the window's, rcol = the residual's column"""
        for row in rows:
            items = [(cols[c], v) for c, v in row.items() if c != rcol]
            rr = row.get(rcol)
            for ia, (a, va) in enumerate(items):
                for b, vb in items[ia:]:
                    p = va * vb
                    self.H.setdefault((a, b) if a <= b else (b, a), []).append(p)
                if rr is not None:
                    self.g.setdefault(a, []).append(va * rr)
            if rr is not None:
                self.cost.append(rr * rr)

    def result(self):
        n = self.n
        out = {}
        for name, shape in (("H", (n, n)), ("g", (n,)), ("cost", ())):
            out[name] = [np.zeros(shape), np.zeros(shape), np.zeros(shape)]          # hi, lo, magnitude

        def put(name, idx, v):
            hi = float(v.v)
            out[name][0][idx], out[name][1][idx], out[name][2][idx] = hi, float(v.v - mp.mpf(hi)), v.m
        for (a, b), t in self.H.items():
            v = sumn(t)
            put("H", (a, b), v)
            put("H", (b, a), v)
        for a, t in self.g.items():
            put("g", (a,), sumn(t))
        put("cost", (), 0.5 * sumn(self.cost))
        return out


def block_local(kf, kind):
    return 15 * kf + (0, 3, 6)[kind]


@functools.lru_cache(maxsize=None)
def _prior_gram(key, n_rows, n_cols):
    J0 = np.frombuffer(key, np.float64).reshape(n_rows, n_cols)
    cols = [nv(J0[:, c]) for c in range(n_cols)]
    A = {}
    for a in range(n_cols):
        for b in range(a, n_cols):
            A[(a, b)] = A[(b, a)] = dot(cols[a], cols[b])
    return A


def prior_terms(prior, state, acc, last3=False, mut=None):
    """MarginalizationFactor::Evaluate on the kept blocks: r = r0 + J0 dx, J = J0 blockdiag(I, T_q ...) -> acc (through A0 = J0^T J0 as the device goes)"""
    J0 = np.ascontiguousarray(prior["J0"], np.float64)
    n_rows, n_cols = J0.shape
    dx, T, col_of = [], {}, []          # T: first column of a q block -> 3x3;  col_of: J0 column -> (local column, q block's first column or None, index)
    col = 0
    for kind, kf, x0 in zip(prior["block_kind"], prior["block_keyframe"], prior["x0"]):
        x0n, loc = nv(x0), block_local(kf, kind)
        if kind == 1:
            x = nv(state[kf, 3:7])
            q0i = qinv(x0n)
            d = qmul(q0i, x)
            pos = d[0].v > 0 if mut == "dw_strict" else d[0].v >= 0
            sg = 2.0 if pos else -2.0
            dx += [sg * c for c in qnormalized(d)[1:]]
            Lr = q_left(q0i, mut)[1:4]
            T[col] = [[sg * v for v in row[1:4]] for row in Lr] if last3 else [[sg * v for v in row] for row in matmul(Lr, plus_jacobian(x))]
            col_of += [(loc + i, col, i) for i in range(3)]
            col += 3
        else:
            x = nv(state[kf, 0:3] if kind == 0 else state[kf, 7:16])
            dx += [a - b for a, b in zip(x, x0n)]
            col_of += [(loc + i, None, i) for i in range(len(x0n))]
            col += len(x0n)
    assert col == n_cols
    r = [N(float(prior["r0"][i])) + dot(nv(J0[i]), dx) for i in range(n_rows)]
    pv = [dot(nv(J0[:, c]), r) for c in range(n_cols)]
    A0 = _prior_gram(J0.tobytes(), n_rows, n_cols)

    def expand(c):          # J0 column combination giving local column c's: list of (J0 column, weight)
        loc, q0, i = col_of[c]
        return [(c, ONE)] if q0 is None else [(q0 + k, T[q0][k][i]) for k in range(3)]
    for ca in range(n_cols):
        ea = expand(ca)
        v = sumn(w * pv[k] for k, w in ea if w.m != 0.0 and pv[k].m != 0.0)
        if v.m != 0.0:
            acc.g.setdefault(col_of[ca][0], []).append(v)
        if mut == "prior_T_one_side":
            ea = [(ca, ONE)]
        for cb in range(n_cols):
            a, b = col_of[ca][0], col_of[cb][0]
            if a > b:
                continue
            v = sumn(wa * sumn(A0[(ka, kb)] * wb for kb, wb in expand(cb)) for ka, wa in ea)
            if v.m != 0.0:
                acc.H.setdefault((a, b), []).append(v)
    acc.cost += [x * x for x in r]


def window(case, last3=False, mut=None):
    """(cost, g, H): each [hi, lo, magnitude] with value = hi + lo.  last3 = the system win_build<true> forms (IMU factor 0 only, no cost meaning)."""
    state, n_kf = case["state"], case["n_kf"]
    acc = Acc(15 * n_kf)
    aux_all = []
    sb = case.get("sb_prior")
    if sb is not None:
        for k in range(n_kf):
            if np.isnan(sb[k, 0]):
                continue
            rows = [{0: N(15.0), 1: 15.0 * (N(float(state[k, 7 + i])) - N(float(sb[k, i])))} for i in range(9)]
            for i, row in enumerate(rows):
                if row[1].m == 0.0:
                    del row[1]
                acc.add_rows([row], {0: 15 * k + 6 + i}, 1)
    imu = case.get("imu") or []
    for f, rec in enumerate(imu[:1] if last3 else imu):
        rows, aux = imu_factor_local(rec, state[f], state[f + 1], last3, mut)
        aux_all.append(aux)
        S = host_sqrt_info(rec["covariance"])[1] if case.get("given_sqrt_info") else sqrt_info(rec["covariance"])
        acc.add_rows(whiten(S, rows), {c: 15 * f + c for c in range(30)}, 30)
    if case.get("prior") is not None:
        prior_terms(case["prior"], state, acc, last3, mut)
    out = acc.result()
    out["aux"] = aux_all
    return out


_CACHE = {}


def model(case, last3=False):
    """the model of a case, computed once per session"""
    key = (case["name"], last3)
    if key not in _CACHE:
        _CACHE[key] = window(case, last3)
    return _CACHE[key]


def ratios(dev, ref):
    """|dev - model| / (2^-53 magnitude) per entry (0 where both the difference and the magnitude are 0, inf where only the magnitude is)"""
    hi, lo, mag = ref
    d = np.abs((np.asarray(dev, np.float64) - hi) - lo)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(mag > 0, d / (U * np.where(mag > 0, mag, 1.0)), np.where(d == 0, 0.0, np.inf))


def worst_ratio(cost, g, H, m):
    return float(max(ratios(cost, m["cost"]).max(), ratios(g, m["g"]).max(), ratios(H, m["H"]).max()))


# ---------------------------------------------------------------- the last-three-columns system and its Schur complement
def marg_selection(case):
    """columns win_build<true> fills, as lili_window_marginalize picks them (window_marg_table): (sel, m, kept blocks [(kind, kf)])"""
    n_kf = case["n_kf"]
    touched = np.zeros((n_kf, 3), bool)
    if case.get("prior") is not None:
        for kind, kf in zip(case["prior"]["block_kind"], case["prior"]["block_keyframe"]):
            touched[kf, kind] = True
    if case.get("sb_prior") is not None:
        touched[:, 2] |= ~np.isnan(case["sb_prior"][:, 0])
    if case.get("imu"):
        touched[0:2, :] = True
    sel, m, kept = [], 0, []
    for k in range(n_kf):
        for kind in range(3):
            if touched[k, kind]:
                sel += [block_local(k, kind) + i for i in range(9 if kind == 2 else 3)]
                if k == 0:
                    m = len(sel)
                else:
                    kept.append((kind, k))
    return sel, m, kept


def marg_model(case):
    """(S, bs, eig(Amm), eig(S)) of the last-three-columns system in mpmath (values as f64 arrays), or None when Amm is singular"""
    key = (case["name"], "schur")
    if key in _CACHE:
        return _CACHE[key]
    mdl = model(case, last3=True)
    sel, m, _ = marg_selection(case)
    n = len(sel)
    A, b = mp.matrix(n, n), mp.matrix(n, 1)
    for i, a in enumerate(sel):
        b[i] = mp.mpf(mdl["g"][0][a]) + mp.mpf(mdl["g"][1][a])
        for j, c in enumerate(sel):
            A[i, j] = mp.mpf(mdl["H"][0][a, c]) + mp.mpf(mdl["H"][1][a, c])
    Af = np.array(A.tolist(), np.float64)
    w_mm = np.linalg.eigvalsh(Af[:m, :m])
    out = None
    if w_mm.min() > 0:
        Ai = mp.inverse(A[:m, :m])
        S = A[m:, m:] - A[m:, :m] * Ai * A[:m, m:]
        bs = b[m:, 0] - A[m:, :m] * Ai * b[:m, 0]
        Sf = np.array(S.tolist(), np.float64)
        out = dict(S=Sf, bs=np.array(bs.tolist(), np.float64).reshape(-1), w_mm=w_mm, w_s=np.linalg.eigvalsh(0.5 * (Sf + Sf.T)), A=Af,
                   b=np.array(b.tolist(), np.float64).reshape(-1), m=m)
    _CACHE[key] = out
    return out


def marg_difference(J0, r0, mm):
    """(J0^T J0 - S, J0^T r0 - bs), each relative to the largest entry of the model's quantity (tests/test_marg_gpu.py's measure)"""
    J0, r0 = np.asarray(J0, np.float64), np.asarray(r0, np.float64)
    return np.array([np.abs(J0.T @ J0 - mm["S"]).max() / np.abs(mm["S"]).max(), np.abs(J0.T @ r0 - mm["bs"]).max() / np.abs(mm["bs"]).max()])


def marg_usable(case):
    """tests/test_marg_cpu.py's input condition on the model: every eigenvalue of Amm and S >= 1e-3 (none in between that and the 1e-8 threshold)"""
    mm = marg_model(case)
    return mm is not None and mm["w_mm"].min() >= 1e-3 and mm["w_s"].min() >= 1e-3


# ---------------------------------------------------------------- records and states
G = np.array([0.0, 0.0, -9.805])


def quat(axis, angle):
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    return np.concatenate([[np.cos(angle / 2)], np.sin(angle / 2) * a])


def unit(q):          # unit up to rounding: one normalisation in f64, and again (a fixed point)
    q = np.asarray(q, np.float64)
    q = q / np.sqrt(q @ q)
    return q / np.sqrt(q @ q)


SKEW_AXIS = np.array([0.48, -0.6, 0.64])


def hand_record(seed, sum_dt=0.2, g=G, cov=None, dq=None):
    """a WindowImu record built field by field: nothing in it comes from an integration"""
    rng = np.random.default_rng(seed)
    s = float(sum_dt)
    jac = np.eye(15)
    jac[0:3, 9:12] = -0.5 * s * s * np.eye(3) + 0.1 * s * s * rng.normal(size=(3, 3))
    jac[0:3, 12:15] = 0.3 * s * s * rng.normal(size=(3, 3))
    jac[3:6, 12:15] = -s * np.eye(3) + 0.4 * s * rng.normal(size=(3, 3))
    jac[6:9, 9:12] = -s * np.eye(3) + 0.2 * s * rng.normal(size=(3, 3))
    jac[6:9, 12:15] = 0.5 * s * rng.normal(size=(3, 3))
    return dict(sum_dt=s, g=np.array(g, np.float64), delta_p=s * s * rng.normal(size=3), delta_q=unit(quat(rng.normal(size=3), 0.9 + rng.uniform())) if dq is None else np.array(dq, np.float64),
                delta_v=s * rng.normal(size=3), lin_ba=0.05 * rng.normal(size=3), lin_bg=0.01 * rng.normal(size=3), jacobian=jac,
                covariance=np.eye(15) if cov is None else np.array(cov, np.float64))


def tumbling(n_seg, seed=5, dt_kf=0.2, hz=200.0):
    """keyframe states and W.Preintegration records on a trajectory that tumbles about all three axes (body rate (0.9 sin 2t + 0.8, -1.1 cos 1.5t, 0.8 + 0.5 sin t) rad/s)"""
    rng = np.random.default_rng(seed)
    ba, bg = np.array([0.02, -0.01, 0.015]), np.array([0.002, -0.001, 0.0015])
    p0, v0, a = np.array([0.8, -0.5, 1.5]), np.array([0.9, 0.4, 0.05]), np.array([0.6, -0.8, 0.3])
    rate = lambda t: np.array([0.9 * np.sin(2 * t) + 0.8, -1.1 * np.cos(1.5 * t), 0.8 + 0.5 * np.sin(t)])
    n = int(round(dt_kf * hz))
    q, h = unit(quat([0.3, -0.5, 0.8], 2.2)), 1.0 / hz
    states, recs = [], []
    for k in range(n_seg + 1):
        t0 = k * dt_kf
        states.append(np.concatenate([p0 + v0 * t0 + 0.5 * a * t0 * t0, q, v0 + a * t0, ba, bg]))
        if k == n_seg:
            break
        pre = None
        for i in range(n + 1):
            t = t0 + i * h
            acc, gyr = W.qrot(W.qinv(q), a - G) + ba, rate(t) + bg
            if pre is None:
                pre = W.Preintegration(acc, gyr, ba + 0.003, bg - 0.0004)
            else:
                pre.push_back(h, acc, gyr)
            if i < n:
                w = rate(t + 0.5 * h)
                q = unit(W.qmul(q, quat(w, np.linalg.norm(w) * h)))
        recs.append(dict(sum_dt=pre.sum_dt, g=G.copy(), delta_p=pre.delta_p.copy(), delta_q=pre.delta_q.copy(), delta_v=pre.delta_v.copy(), lin_ba=pre.ba.copy(),
                         lin_bg=pre.bg.copy(), jacobian=pre.jacobian.copy(), covariance=pre.covariance.copy()))
    states = np.array(states)
    for k in range(n_seg + 1):          # the window the front end would hand over: a few cm, a few degrees, a little speed and bias off
        states[k, 0:3] += rng.normal(0, 0.03, 3)
        states[k, 3:7] = unit(W.qmul(states[k, 3:7], quat(rng.normal(size=3), 0.05)))
        states[k, 7:16] += np.concatenate([rng.normal(0, 0.05, 3), rng.normal(0, 0.004, 3), rng.normal(0, 0.0005, 3)])
    return states, recs


def window_imu(rec):
    """the lili_window_imu structure of a record"""
    w = L.api.WindowImu()
    w.sum_dt = float(rec["sum_dt"])
    for name, n in (("g", 3), ("delta_p", 3), ("delta_q", 4), ("delta_v", 3), ("lin_ba", 3), ("lin_bg", 3), ("jacobian", 225), ("covariance", 225)):
        a = np.asarray(rec[name], np.float64).reshape(-1)
        assert a.size == n
        getattr(w, name)[:] = a.tolist()
    return w


class _Pre:          # what W.imu_factor reads of a Preintegration
    def __init__(self, rec):
        self.sum_dt, self.g_vec, self.jacobian, self.covariance = rec["sum_dt"], rec["g"], np.asarray(rec["jacobian"]).reshape(15, 15), np.asarray(rec["covariance"]).reshape(15, 15)
        self.delta_p, self.delta_q, self.delta_v, self.ba, self.bg = rec["delta_p"], rec["delta_q"], rec["delta_v"], rec["lin_ba"], rec["lin_bg"]
        self.evaluate = lambda *a: W.Preintegration.evaluate(self, *a)


def oracle_problem(case):
    """the case on oracle/lo_window.py's blocks (imu_factor, Marginalization.factor, speed_bias_prior) as a W.Problem"""
    pb = W.Problem()
    n_kf, state = case["n_kf"], case["state"]
    for k in range(n_kf):
        pb.add_parameter(f"t{k}", state[k, 0:3])
        pb.add_parameter(f"q{k}", state[k, 3:7], quat=True)
        pb.add_parameter(f"sb{k}", state[k, 7:16])
    if case.get("sb_prior") is not None:
        for k in range(n_kf):
            if not np.isnan(case["sb_prior"][k, 0]):
                pb.add_residual(lambda sb, mean=case["sb_prior"][k].copy(): W.speed_bias_prior(mean, sb), [f"sb{k}"])
    for f, rec in enumerate(case.get("imu") or []):
        S = host_sqrt_info(rec["covariance"])[0] if case.get("given_sqrt_info") else None
        pb.add_residual(lambda ti, qi, sbi, tj, qj, sbj, pre=_Pre(rec), S=S: W.imu_factor(pre, ti, qi, sbi, tj, qj, sbj, sqrt_info=S), [f"t{f}", f"q{f}", f"sb{f}", f"t{f + 1}", f"q{f + 1}", f"sb{f + 1}"])
    pr = case.get("prior")
    if pr is not None:
        M = W.Marginalization.__new__(W.Marginalization)
        M.linearized_jacobians, M.linearized_residuals, M.n = np.asarray(pr["J0"], np.float64), np.asarray(pr["r0"], np.float64), pr["J0"].shape[1]
        M.kept = [(f"{'tqs'[kind]}{kf}", np.asarray(x0, np.float64), kind == 1) for kind, kf, x0 in zip(pr["block_kind"], pr["block_keyframe"], pr["x0"])]
        names = [("t", "q", "sb")[kind] + str(kf) for kind, kf in zip(pr["block_kind"], pr["block_keyframe"])]
        pb.add_residual(M.factor(), names)
    return pb


def oracle_evaluate(case):
    cost, r, J = oracle_problem(case).evaluate()
    return cost, J.T @ r, J.T @ J


# ---------------------------------------------------------------- case builders
def consistent_next(rec, xi, rng, delta=None, dpos=0.05, dvel=0.05):
    """keyframe j of a factor: Qj = Qi cq delta (delta = (axis, angle), default a small one), Pj / Vj so that r_p, r_v are about dpos, dvel"""
    Qi, Vi = xi[3:7], xi[7:10]
    s, g = rec["sum_dt"], rec["g"]
    J = np.asarray(rec["jacobian"]).reshape(15, 15)
    th = J[3:6, 12:15] @ (xi[13:16] - rec["lin_bg"])
    cq = W.qmul(rec["delta_q"], np.array([1.0, th[0] / 2, th[1] / 2, th[2] / 2]))
    d = quat(*delta) if delta is not None else quat(rng.normal(size=3), 0.02)
    Qj = unit(W.qmul(W.qmul(Qi, unit(cq)), d))
    Pj = xi[0:3] + Vi * s + 0.5 * g * s * s + W.qrot(Qi, rec["delta_p"] + dpos * rng.normal(size=3))
    Vj = Vi + g * s + W.qrot(Qi, rec["delta_v"] + dvel * rng.normal(size=3))
    return np.concatenate([Pj, Qj, Vj, xi[10:13] + 0.002 * rng.normal(size=3), xi[13:16] + 0.0003 * rng.normal(size=3)])


def first_state(rng, Qi, rec, P=None, V=None, dba=0.01, dbg=0.001):
    P = rng.normal(size=3) if P is None else np.asarray(P, np.float64)
    V = rng.normal(size=3) if V is None else np.asarray(V, np.float64)
    ba = rec["lin_ba"] + (dba * rng.normal(size=3) if np.isscalar(dba) else np.asarray(dba))
    bg = rec["lin_bg"] + (dbg * rng.normal(size=3) if np.isscalar(dbg) else np.asarray(dbg))
    return np.concatenate([P, Qi, V, ba, bg])


def pair_case(name, family, claim, rec, xi, xj, **kw):
    return dict(name=name, family=family, claim=claim, n_kf=2, state=np.array([xi, xj]), imu=[rec], sb_prior=kw.get("sb_prior"), prior=kw.get("prior"))


ATTITUDES = [("identity", np.array([1.0, 0, 0, 0]))] + [(f"{deg}{ax}", np.array([np.cos(np.radians(deg) / 2) if deg != 180 else 0.0] + [np.sin(np.radians(deg) / 2) if i == k else 0.0 for i in range(3)]))
                                                          for deg in (90, 180) for k, ax in enumerate("xyz")] + \
    [(f"random{k}", unit(quat(np.random.default_rng(70 + k).normal(size=3), 1.5 + k))) for k in range(3)]


def random_prior(rng, blocks, state, n_rows=None, x0_off=0.02, scale=1.0):
    """a hand-built marginalisation prior over blocks [(kind, kf)] linearised near `state`"""
    n_cols = sum(9 if k == 2 else 3 for k, _ in blocks)
    n_rows = n_cols if n_rows is None else n_rows
    x0 = []
    for kind, kf in blocks:
        if kind == 1:
            x0.append(unit(W.qmul(state[kf, 3:7], quat(rng.normal(size=3), x0_off * 3))))
        else:
            x0.append((state[kf, 0:3] if kind == 0 else state[kf, 7:16]) + x0_off * rng.normal(size=3 if kind == 0 else 9))
    Jm = rng.normal(size=(n_rows, n_cols))
    if n_rows == n_cols:          # well conditioned: singular values 1 .. 3
        Uo, _, Vo = np.linalg.svd(Jm)
        Jm = Uo @ np.diag(np.linspace(1.0, 3.0, n_cols)) @ Vo
    return dict(block_kind=[k for k, _ in blocks], block_keyframe=[f for _, f in blocks], x0=x0, J0=scale * Jm, r0=0.3 * rng.normal(size=n_rows))


TABLE_30 = [(kind, kf) for kf in (0, 1) for kind in (0, 1, 2)]
TABLE_21 = [(0, 0), (1, 0), (2, 0), (0, 1), (1, 1)]
TABLE_36 = TABLE_30 + [(0, 2), (1, 2)]


@functools.lru_cache(maxsize=None)
def cases():
    """every case, in family order"""
    out = []
    rng = np.random.default_rng(2024)
    I15 = np.eye(15)
    # ---- attitude x signs
    for k, (aname, Qi) in enumerate(ATTITUDES):
        rec = hand_record(100 + k)
        xi = first_state(rng, Qi, rec)
        xj = consistent_next(rec, xi, rng, delta=(SKEW_AXIS, 0.3))
        for sname, si, sj in (("", 1, 1), ("-Qi", -1, 1), ("-Qj", 1, -1), ("-Qi-Qj", -1, -1)):
            a, b = xi.copy(), xj.copy()
            a[3:7] *= si
            b[3:7] *= sj
            out.append(pair_case(f"attitude/{aname}{sname}", "attitude", ("rq_w", 0, si * sj * np.cos(0.15), 1e-12), rec, a, b))
    # ---- residual angle
    for k, ang in enumerate((0.0, 1e-9, 1e-3, 1.0, np.pi - 1e-6, np.pi, np.pi + 0.5)):
        rec = hand_record(130 + k)
        xi = first_state(rng, ATTITUDES[7 + k % 3][1], rec)
        xj = consistent_next(rec, xi, rng, delta=(SKEW_AXIS, ang))
        out.append(pair_case(f"angle/{k}:{ang:.10g}", "residual angle", ("rq_w", 0, np.cos(ang / 2), 1e-12), rec, xi, xj))
    # ---- bias step
    for k, dbg in enumerate((0.0, 1e-6, 1e-2, 0.5)):
        for dba in (0.0, 0.5):
            rec = hand_record(140 + k)
            d = np.array([0.6, -0.64, 0.48])
            xi = first_state(rng, ATTITUDES[8][1], rec, dba=dba * d, dbg=dbg * d)
            if dbg == 0.0:
                xi[13:16] = rec["lin_bg"]
            xj = consistent_next(rec, xi, rng)
            claim = ("cq_is_delta_q", 0) if dbg == 0.0 else ("cq_norm_excess", 0, 1e-3) if dbg == 0.5 else ("cq_norm_excess", 0, 0.0)
            out.append(pair_case(f"bias/dbg{dbg:g}_dba{dba:g}", "bias step", claim, rec, xi, xj))
    # ---- magnitudes
    for k, s in enumerate((0.005, 0.2, 2.0, 10.0)):
        rec = hand_record(150 + k, sum_dt=s)
        xi = first_state(rng, ATTITUDES[9][1], rec, P=[1.0e4, -0.7e4, 1.2e4] if k % 2 == 1 else None, V=[30.0, -5.0, 2.0] if k >= 1 else None)
        xj = consistent_next(rec, xi, rng)
        claim = ("cancellation", 0, 1e4 if k == 1 else 1.0)
        out.append(pair_case(f"magnitudes/sum_dt{s:g}", "magnitudes", claim, rec, xi, xj))
    rec = hand_record(155, sum_dt=0.2, dq=unit([1.0, 1e-3, -1e-3, 5e-4]))          # P about 1e4 m, Pj - Pi about 0.2 m
    xi = first_state(rng, ATTITUDES[7][1], rec, P=[1.0e4, 0.9e4, -1.1e4], V=[0.6, -0.5, 0.4])
    rec["delta_p"] = 0.02 * rng.normal(size=3)
    xj = consistent_next(rec, xi, rng, dpos=0.01)
    out.append(pair_case("magnitudes/far_origin", "magnitudes", ("cancellation", 0, 1e4), rec, xi, xj))
    # ---- gravity
    for gname, g in (("tilted", [3.1, -4.2, -8.3]), ("zero", [0.0, 0.0, 0.0])):
        rec = hand_record(160, g=g)
        xi = first_state(rng, ATTITUDES[8][1], rec)
        out.append(pair_case(f"gravity/{gname}", "gravity", ("gravity", 0), rec, xi, consistent_next(rec, xi, rng)))
    # ---- covariance
    st, trecs = tumbling(3)
    covs = [("identity", I15)]
    for gi, gname in enumerate(("p", "q", "v", "ba", "bg")):
        d = np.full(15, 1e6)
        d[3 * gi:3 * gi + 3] = 1.0
        covs.append((f"rows_{gname}", np.diag(d)))
    covs.append(("preintegrated", trecs[0]["covariance"]))
    Uo = np.linalg.qr(np.random.default_rng(9).normal(size=(15, 15)))[0]
    dense = Uo @ np.diag(np.logspace(-4, 4, 15)) @ Uo.T
    covs += [("dense_1e8", 0.5 * (dense + dense.T)), ("1e-12", 1e-12 * I15), ("1e6", 1e6 * I15)]
    for cname, cov in covs:
        rec = dict(trecs[0], covariance=np.array(cov))
        family = {"preintegrated": "covariance preintegrated", "dense_1e8": "covariance conditioned", "1e-12": "covariance scale"}.get(cname, "covariance")
        out.append(pair_case(f"covariance/{cname}", family, ("covariance", 0), rec, st[0], st[1]))
        if family in ("covariance preintegrated", "covariance conditioned"):          # the same case with the host's own f64 sqrt_info taken as given, in the model and in the oracle: the device's
            # arithmetic on a dense, realistic sqrt_info is then held to a few units, apart from how exact that sqrt_info is (the claim bounds that)
            out.append(dict(out[-1], name=f"covariance_given/{cname}", family="covariance given", claim=("host_sqrt_info", 0), given_sqrt_info=True))
    # ---- position in the window: the hard record (w = 0 attitude, negated Qj, large bias step) at factor f, tumbling records beside it; every position with every
    # speed-bias-prior pattern (all rows, none, all but keyframe f's — a NaN row)
    count = 0
    for n_kf in (2, 3, 4):
        for f in range(n_kf - 1):
            state, recs_ = st[:n_kf].copy(), [dict(r, covariance=I15 * (1.0 + 0.5 * i)) for i, r in enumerate(trecs[:n_kf - 1])]
            hard = hand_record(170 + count)
            recs_[f] = hard
            state[f, 3:7] = ATTITUDES[5][1]          # 180 deg about y: w = 0
            state[f, 13:16] = hard["lin_bg"] + 0.3 * np.array([0.6, -0.64, 0.48])
            nxt = consistent_next(hard, state[f], rng, delta=(SKEW_AXIS, 0.4))
            state[f + 1, 0:10] = nxt[0:10]
            state[f + 1, 3:7] *= -1.0
            means = state[:, 7:16] + 0.01 * rng.normal(size=(n_kf, 9))
            for pat in ("all", "none", "subset"):
                sb = None if pat == "none" else means.copy()
                if pat == "subset":
                    sb[f] = np.nan
                    sb[f, 1:] = 1.0          # a NaN row: only its first entry says so
                out.append(dict(name=f"position/n{n_kf}_f{f}_{pat}", family="position", claim=("rq_w", f, -np.cos(0.2), 1e-12), n_kf=n_kf, state=state, imu=recs_, sb_prior=sb, prior=None))
            count += 1
    # ---- prior: block tables
    st4, trecs4 = tumbling(3, seed=6)
    tables = [("30", TABLE_30, 3), ("21", TABLE_21, 3), ("36", TABLE_36, 3), ("lone_q", [(1, 1)], 2), ("lone_t", [(0, 0)], 2), ("kf0_kf2", [(0, 0), (1, 0), (2, 0), (0, 2), (1, 2), (2, 2)], 3),
              ("60", [(kind, kf) for kf in range(4) for kind in (0, 1, 2)], 4)]          # the full table: 12 blocks, 60 columns, 60 rows at n_kf = 4
    for tname, blocks, n_kf in tables:
        pr = random_prior(rng, blocks, st4[:n_kf])
        out.append(dict(name=f"prior_table/{tname}", family="prior tables", claim=("prior_cols", pr["J0"].shape[1]), n_kf=n_kf, state=st4[:n_kf].copy(), imu=None, sb_prior=None, prior=pr))
    # ---- prior: rows
    for rname, n_rows in (("square", None), ("rows5", 5), ("rows1", 1), ("zero_rows", None), ("rows40", 40), ("rows60", 60)):          # more rows than columns, up to the limit of 60
        pr = random_prior(rng, TABLE_21, st4[:3], n_rows=n_rows)
        if rname == "zero_rows":
            pr["J0"][[2, 7, 20]] = 0.0
        out.append(dict(name=f"prior_rows/{rname}", family="prior rows", claim=("prior_rows", pr["J0"].shape[0]), n_kf=3, state=st4[:3].copy(), imu=None, sb_prior=None, prior=pr))
    # ---- prior: the kept quaternion, d = q0^-1 q
    kept = [("w_pos", None, None, 1), ("w_neg", None, None, -1), ("w_zero", np.array([1.0, 0, 0, 0]), np.array([0.0, 1.0, 0, 0]), 0),
            ("skew180", unit(quat([0.2, 0.5, -0.3], 1.1)), None, None)]
    for kname, q0, q, sgn in kept:
        state = st4[:3].copy()
        pr = random_prior(rng, TABLE_21, state)
        if kname == "w_neg":
            state[1, 3:7] *= -1.0
        if kname == "w_zero":
            pr["x0"][4], state[1, 3:7] = q0, q
        if kname == "skew180":
            pr["x0"][4] = q0
            state[1, 3:7] = unit(W.qmul(q0, np.concatenate([[0.0], SKEW_AXIS])))
        claim = ("prior_dw", 4, sgn) if sgn is not None else ("prior_dw_small", 4, 1e-15)
        out.append(dict(name=f"prior_q/{kname}", family="prior quaternion", claim=claim, n_kf=3, state=state, imu=None, sb_prior=None, prior=pr))
    # ---- prior: x0 quaternion of norm 1 + 1e-3
    state = st4[:3].copy()
    pr = random_prior(rng, TABLE_21, state)
    pr["x0"][1], pr["x0"][4] = pr["x0"][1] * (1.0 + 1e-3), pr["x0"][4] * (1.0 - 1e-3)
    out.append(dict(name="prior_x0/norm_1e-3", family="prior x0 norm", claim=("prior_x0_norm", 1, 1e-3), n_kf=3, state=state, imu=None, sb_prior=None, prior=pr))
    # ---- combined: each of the above with IMU factors and speed-bias priors on the same window
    trecs4 = [dict(r, covariance=I15) for r in trecs4]
    for base in [c for c in list(out) if c["family"].startswith("prior")]:
        state, n_kf = base["state"].copy(), base["n_kf"]
        sb = state[:, 7:16] + 0.01 * rng.normal(size=(n_kf, 9))
        sb[n_kf - 1] = np.nan
        out.append(dict(name="combined/" + base["name"], family="combined", claim=base["claim"], n_kf=n_kf, state=state, imu=trecs4[:n_kf - 1], sb_prior=sb, prior=base["prior"]))
    # ---- two more tables window_prior_table accepts: blocks in no particular order, a lone speed-bias block; alone and combined (their own generator: the cases above keep their draws)
    rng2 = np.random.default_rng(2025)
    for tname, blocks, n_kf in (("shuffled", [(2, 1), (1, 0), (0, 2), (1, 1), (0, 0)], 3), ("lone_sb", [(2, 1)], 2)):
        pr = random_prior(rng2, blocks, st4[:n_kf])
        base = dict(name=f"prior_table/{tname}", family="prior tables", claim=("prior_cols", pr["J0"].shape[1]), n_kf=n_kf, state=st4[:n_kf].copy(), imu=None, sb_prior=None, prior=pr)
        sb = base["state"][:, 7:16] + 0.01 * rng2.normal(size=(n_kf, 9))
        sb[n_kf - 1] = np.nan
        out += [base, dict(base, name="combined/" + base["name"], family="combined", imu=trecs4[:n_kf - 1], sb_prior=sb)]
    names = [c["name"] for c in out]
    assert len(set(names)) == len(names)
    return tuple(out)


# the covariance family in groups, so that the exactly invertible covariances are not judged by the allowance of the others: "covariance" = I, the five one-row-group
# diagonals, 1e6 I;  "covariance scale" = 1e-12 I (an information of 1e12: the Schur complement cancels from 1e13 to 4e3);  "covariance preintegrated" = the pre-integration's
# own (dense, condition 38: numpy's f64 inverse + Cholesky cost 36 units);  "covariance conditioned" = the dense one of condition 1e8 (numpy loses that many digits: K says
# so);  "covariance given" = the last two again with the host's f64 sqrt_info taken as given by the model and by the oracle, so that the device's arithmetic on a dense
# sqrt_info is held to a few units whatever the inverse costs (how exact that sqrt_info is, is the cases' claim)
FAMILIES = ("attitude", "residual angle", "bias step", "magnitudes", "gravity", "covariance", "covariance scale", "covariance conditioned", "covariance preintegrated", "position", "covariance given", "prior tables", "prior rows",
            "prior quaternion", "prior x0 norm", "combined")
IMU_FAMILIES = FAMILIES[:10]
# K per family: the worst |oracle/lo_window.py - model| / (2^-53 magnitude) over cost, g and H, measured by tests/test_window_factor_cases_cpu.py (which asserts that the
# measurement stays below this table), written here rounded up in the third digit.
K = {"attitude": 2.59, "residual angle": 2.15, "bias step": 1.81, "magnitudes": 2.66, "gravity": 1.13, "covariance": 2.78, "covariance scale": 2.62, "covariance conditioned": 8.69e6,
     "covariance preintegrated": 36.6, "position": 2.78, "covariance given": 2.33, "prior tables": 6.24, "prior rows": 3.54, "prior quaternion": 4.49, "prior x0 norm": 2.19, "combined": 5.74}
DEVICE_FACTOR = 8          # the device sums the 15-term whitening and Gram sums, and expands the quaternion products, in another order than numpy (the plane-fit test's convention)
# numpy's Marginalization (oracle/lo_window.py) against the model's Schur complement of the last-three-columns systems, per family: the worst (J0^T J0, J0^T r0) difference
# relative to the largest entry of the model's quantity; measured by the CPU file (3.40e-15, 4.65e-15; 2.39e-15, 6.21e-15; 4.53e-15, 2.73e-15; 9.44e-15, 3.96e-13; 1.89e-15, 8.48e-15; 2.27e-15, 1.15e-15; 1.21e-5, 6.83e-6;
# 6.83e-13, 8.93e-13; 1.99e-13, 1.22e-13; 1.64e-15, 1.52e-15), written here rounded up to one digit.  The device gets 100 x (tests/test_marg_gpu.py's rule).
MARG_NUMPY_WORST = {"attitude": (4e-15, 5e-15), "residual angle": (3e-15, 7e-15), "bias step": (5e-15, 3e-15), "magnitudes": (1e-14, 4e-13), "gravity": (2e-15, 9e-15),
                    "covariance": (3e-15, 2e-15), "covariance scale": (2e-5, 7e-6), "covariance conditioned": (7e-13, 9e-13), "covariance preintegrated": (2e-13, 2e-13), "position": (2e-15, 2e-15)}


def by_family(family):
    return [c for c in cases() if c["family"] == family]


def last3_case(case):
    """the case as lili_window_marginalize is given it: speed-bias priors on every keyframe and a hand-built old prior on the poses of keyframes 0 and 1, so
    that nothing but the factor under test decides the conditioning"""
    rng = np.random.default_rng(sum(map(ord, case["name"])))
    state = case["state"]
    sb = state[:, 7:16] + 0.01 * rng.normal(size=(case["n_kf"], 9))
    pr = random_prior(rng, [(0, 0), (1, 0), (0, 1), (1, 1)], state)
    return dict(case, name="last3/" + case["name"], sb_prior=sb, prior=pr)


@functools.lru_cache(maxsize=None)
def last3_cases():
    return tuple(last3_case(c) for c in cases() if c["family"] in IMU_FAMILIES and c["n_kf"] <= 3 and not c["name"].endswith(("_none", "_subset")))          # (last3_case sets the speed-bias priors itself)


# ---------------------------------------------------------------- claims
def check_claim(case, mdl=None):
    """asserts the case's claim on the model; returns the one-line statement"""
    mdl = mdl or model(case)
    c = case["claim"]
    kind = c[0]
    if kind == "rq_w":
        w = float(mdl["aux"][c[1]]["rq"][0].v)
        assert abs(w - c[2]) <= c[3], (case["name"], w, c[2])
        return f"r_q.w of factor {c[1]} is {c[2]:+.6f}"
    if kind == "cq_is_delta_q":
        cq = [float(v.v) for v in mdl["aux"][c[1]]["cq"]]
        assert cq == list(case["imu"][c[1]]["delta_q"]), case["name"]
        return "dbg = 0 bit for bit: cq is delta_q"
    if kind == "cq_norm_excess":
        n2 = float(qn2(mdl["aux"][c[1]]["cq"]).v)
        dq_n2 = float(np.sum(np.asarray(case["imu"][c[1]]["delta_q"]) ** 2))
        assert n2 - 1.0 >= c[2] - 1e-12 and abs(dq_n2 - 1.0) < 1e-15, (case["name"], n2)
        return f"|cq|^2 - 1 = {n2 - 1.0:.3e} >= {c[2]:g}"
    if kind == "cancellation":
        f = c[1]
        r, _, _ = imu_factor_global(case["imu"][f], case["state"][f], case["state"][f + 1])
        ratio = max(r[i].m for i in range(3)) / max(max(abs(float(r[i].v)) for i in range(3)), 1e-300)
        assert ratio >= 0.5 * c[2], (case["name"], ratio)
        return f"magnitude / |r_p| = {ratio:.3g} >= {0.5 * c[2]:g}"
    if kind == "gravity":
        g = np.asarray(case["imu"][c[1]]["g"])
        assert (g == 0).all() or (abs(g[0]) > 1 and abs(g[1]) > 1)
        return "g = 0" if (g == 0).all() else "g has x and y components above 1 m/s^2"
    if kind == "covariance":
        cov = np.asarray(case["imu"][c[1]]["covariance"])
        S = sqrt_info(cov)
        M = np.array([[float(S[i][j].v) if j in S[i] else 0.0 for j in range(15)] for i in range(15)])
        err = np.abs(M.T @ M @ cov - np.eye(15)).max()
        assert err <= 1e-6, (case["name"], err)
        return f"sqrt_info^T sqrt_info covariance = I to {err:.1e}"
    if kind == "host_sqrt_info":
        Sh, _ = host_sqrt_info(case["imu"][c[1]]["covariance"])
        Se = sqrt_info(case["imu"][c[1]]["covariance"])
        M = np.array([[float(Se[i][j].v) if j in Se[i] else 0.0 for j in range(15)] for i in range(15)])
        err = np.abs(Sh - M).max() / np.abs(M).max()
        cond = np.linalg.cond(np.asarray(case["imu"][c[1]]["covariance"]))
        bound = 2.0 ** -53 + 15 * cond * 2.0 ** -64          # the rounding to f64, and the long-double Cholesky route: n x condition x 2^-64 at most
        assert err <= bound, (case["name"], cond, err)
        assert (np.abs(Sh) > 0).sum() > 60          # dense: the 15-term whitening sums are all at work
        return f"host sqrt_info is within {err:.2e} of the exact one (condition {cond:.2e}, bound {bound:.2e}), relative to its largest entry"
    if kind == "prior_cols":
        assert case["prior"]["J0"].shape[1] == c[1] == sum(9 if k == 2 else 3 for k in case["prior"]["block_kind"])
        return f"{c[1]} prior columns"
    if kind == "prior_rows":
        assert case["prior"]["J0"].shape[0] == c[1]
        return f"{c[1]} prior rows"
    if kind in ("prior_dw", "prior_dw_small"):
        pr = case["prior"]
        b = c[1]
        d = qmul(qinv(nv(pr["x0"][b])), nv(case["state"][pr["block_keyframe"][b], 3:7]))
        w = float(d[0].v)
        if kind == "prior_dw_small":
            assert abs(w) <= c[2], (case["name"], w)
        elif c[2] == 0:
            assert d[0].v == 0, (case["name"], w)
        else:
            assert w * c[2] > 0.5, (case["name"], w)
        return f"d.w = {w:+.3e}"
    if kind == "prior_x0_norm":
        n = float(np.linalg.norm(case["prior"]["x0"][c[1]]))
        assert abs(n - 1.0 - c[2]) < 1e-9
        return f"|x0| = {n:.6f}"
    raise AssertionError(kind)


# ---------------------------------------------------------------- a tumbling trajectory for tests/window_harness.py (the solve)
def tumbling_trajectory(t):
    """tests/window_harness.py::trajectory with a constant body rate of 1.29 rad/s about a skew axis from a large skew attitude: every quaternion component is
    large, gravity is not parallel to the rotation axis.  Body pose, velocity, world acceleration and body rate at time t."""
    p0, v0, a = np.array([0.8, -0.5, 1.5]), np.array([0.9, 0.4, 0.05]), np.array([0.6, -0.8, 0.1])
    w = np.array([0.9, -0.7, 0.6])
    q = W.qmul(quat([0.3, -0.5, 0.8], 2.2), quat(w, np.linalg.norm(w) * t))
    return p0 + v0 * t + 0.5 * a * t * t, q, v0 + a * t, a, w
