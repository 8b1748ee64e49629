"""Designed inputs for the linearisation (surf_lin_geom / surf_lin_scale / edge_lin_row / GramAcc / lin_surf_body / lin_edge_body, lili_s2m_dev.h; robustify /
loss_eval, lili_device_math.h) and an independent model of it in extended precision.

Shared by tests/test_linearize_cases_cpu.py (the conditions on the inputs, the oracle held to the model, the constant K, the sensitivity of the bounds) and
tests/test_linearize_hard_gpu.py (every launcher against the model and the oracle).

Scene.  The lattice of tests/plane_fit_cases.py / tests/edge_fit_cases.py (clusters of five map points on a 4 m lattice, queries handed over in a local frame
through (Q_ASSOC, T_ASSOC)), built at `origin` and at `far` = (500, -480, 15).  Surf records come from the healthy patches of the `generic` plane case (kinds
patch, huge, through0), edge records from the healthy lines of the `generic` edge case (kinds line, huge); every query used is DECIDED and valid in the model of
its fit (asserted in scene()): this file tests the linearisation, not the fit.  An invalid query is one placed in the centre of a lattice cell, 3.4 m from every
cluster.  The records a test linearises are the ones the side under test wrote itself (the device's, read back; the oracle's on the CPU); the model receives
exactly those f32 values.  The linearisation pose is chosen apart from the association pose: T is solved (in the model's arithmetic, rounded to f64 once) so that
the transformed point lands at a designed distance from its plane / line — that is how a designed residual is reached under any rotation.

Row families (one record, one pose, one parameter set per probe row; `w` is the weight that multiplies the geometry: 1 (front-end), the score (livox), the
count-scaled score (rot)):
  huber     front-end, and loss = 2, loss_a = 0.1 handed to livox: |r| = a (1 + d), d = +-1e-1 .. +-1e-6, and |r| = 1e-9, 1e-3, 1, 1e3
  cauchy    livox, rot: |r| = 1e-12 .. 1e6 in decades; rot with the count N = 1 (the slot's own), N = 2 and 1000 (imported) and with the numerators 1024 / 256, for
            which score * num / N is exact
  none      loss = 0 handed to both sides, the decades of cauchy
  zero      r == 0 exactly (the sq == 0 arm): an f32-exact plane z = 1 / 4, the query in it, the identity pose; front-end at `origin`
  cancel    surf at `far`: the records with the largest |d| (hundreds of metres), |n . pw + d| = 1e-1 .. 1e-9
  nearline  edge: the point 5e-2 .. 5e-8 m beside its line, |nu| / (|lp - A| |lp - B|) from 1 down to 1e-6
  pose      rotation by 0, 1e-8, 1, pi - 1e-6, pi in front of the default; -q; |q| = 1 +- 1e-3; the point moved 16, 256, 4096 m along its plane (surf) or 16, 256 m
            along its line (edge); rot carries its configured extrinsic (0.7071, 0, 0, 0.7071), which is not a unit quaternion
  onepoint  an edge query exactly on its line (f32-exact, identity pose): nu == 0.  Not a probe of accuracy: the factor's derivative does not exist there, the
            reference's jets give NaN, and so do the oracle and the device
Edge rows are kept only where the point is at least DMIN from the line: 2e-8 m at `origin` (on the clusters nearest to the origin) and 1e-4 m at `far`.  lp - A is
the difference of two numbers of size |lp| whose own rounding is eps |lp|; nu = (lp - A) x (lp - B) inherits 0.1 eps |lp| absolutely against |nu| = 0.2 dist, so
the DIRECTION of the row is known to ~eps |lp| / dist: 1.5e-13 / dist at `far`.  Closer than DMIN that exceeds 1e-6 and the row would test nothing (condition
below).  For the same reason the edge rows of `pose` stop at 256 m along the line.

Model.  Written from the factor definitions, not from lo_s2m.cpp or the kernel: the residual functors of LidarKeyframeFactor.h (:38-44 edge, :86-90 plane with
the extrinsic, :118-128 front-end) with Eigen's quaternion product v + w (2 u x v) + u x (2 u x v) and inverse conj / |q|^2, the corrector of
MarginalizationFactor.cpp:44-70 and the closed forms of ceres::CauchyLoss / HuberLoss.  Probe rows: mpmath at 400 bits, the Jacobian by CENTRAL DIFFERENCES of
the residual (step 2^-150: exact for the plane residual, which is quadratic in q, and ~2^-240 for the edge residual) — no hand-derived derivative enters.  ROT's
count scaling is applied as the reference writes it: (score * 1000.0) / N in double, (s * 200.f) / N in float.  Whole Grams: numpy.longdouble, vectorised, with
the derivative of Eigen's product written out; tests/test_linearize_cases_cpu.py holds that to an mpmath sum of the mpmath rows.

Allowance, per entry of a row.  The polynomial part (both rotations, pw, base, jq; lp of the edge factor) has exact f32 inputs; its evaluation error is bounded by
gamma_k times the same expression with every leaf replaced by its magnitude and every subtraction by an addition (Higham, Accuracy and Stability of Numerical
Algorithms, section 3.1) — `S` below, computed in f64.  For nu = (lp - A) x (lp - B) and g = (A - B) x nu that form is useless — (|lp| + |A|)^2 is eight orders above
|nu| although lp - A is a nearly exact difference — so from lp on the edge factor carries the bound step by step (the running error of section 3.3: what the operands
carry, times the other operand's magnitude, plus the result's own magnitude).  That is propagated to first order through the division and the square roots of the edge factor (d|nu| <= (|nu| . S_nu)
/ |nu|, relative errors add in s |nu| / |de| and s / (|nu| |de|)) and through the corrector (r' = f(r) r, J' = f(r) J with f = sqrt(rho'(r^2)): dr' = |(f r)'| dr,
dJ' = f dJ + |J f'| dr; cost: rho' |r| dr, plus b / 2 for the rounding of 1 + s / b inside ceres' b log(1 + s / b) and a |r| + b / 2 for 2 a |r| - b), each result adding its own magnitude once for its final rounding.  The allowance is K eps S with ONE constant K
measured on the CPU: the oracle's worst error / (eps S) over every probe row, offset and variant = 0.77 (in use: K_EVAL = 0.8; 0.5 of it is the model's own rounding to f64).  tests/test_linearize_cases_cpu.py
re-measures it, prints it and fails if it exceeds the value in use.  The oracle is held to 1 x, the device to DEVICE_FACTOR = 8 x, the factor
tests/plane_fit_cases.py uses (other summation order, fma, multiply by reciprocal).  A Gram entry of one row is a product: |x_a| dx_b + |x_b| dx_a + dx_a dx_b + eps |x_a x_b|.
Whole Gram, per entry (never relative to the largest entry): the sum of the rows' product allowances + 2 (64 trips + 16 + nb + 8) eps sum |x_a x_b|,
nb = min(ceil(n / 1024), 256), trips = ceil(n / (1024 nb)) — the depth of the kernel's summation tree (16 MFMA steps of four rows per trip, 16 waves, nb partials).

Conditions, asserted on the model alone by the CPU test: every huber row is decided (||r| - a| > 1e-9 a); every probe row's allowance (device factor included) is
at most 1e-6 of the row's norm (onepoint exempt); every partition case has the intended count of valid records."""
import functools
import math

import mpmath
import numpy as np

from tests import edge_fit_cases as E
from tests import plane_fit_cases as P
from tests.edge_fit_cases import OFFSETS, PITCH, Q_ASSOC, T_ASSOC  # noqa: F401  (re-exported)

EPS = 2.0 ** -52
K_EVAL, DEVICE_FACTOR = 0.8, 8.0            # K: the measured 0.77 rounded up (measure_K(); the CPU test re-measures and prints it)
PREC, H_EXP = 400, 150
LD = np.longdouble
BULK_OK = bool(np.finfo(LD).eps < 2e-19)
BULK_SKIP = "numpy.longdouble is no wider than 64 bits of mantissa here: no extended-precision referee for whole Grams"
VARIANTS = ("livox", "rot", "frontend")
LOSS_NONE, LOSS_CAUCHY, LOSS_HUBER = 0, 1, 2
DMIN = {"origin": 2e-8, "far": 1e-4}
NREC = 4                                     # probe records per kind
LIN_BLOCK, MAX_LIN_BLOCKS = 1024, 256

_CFG = {"livox": dict(variant="livox", loss=LOSS_CAUCHY, loss_a=1.0, q_lb=(0.0, 0.0, 0.0, 1.0), t_lb=(-0.0265, 0.0202, 0.05309), num_s=0.0, num_e=0.0),
        "rot": dict(variant="rot", loss=LOSS_CAUCHY, loss_a=1.0, q_lb=(0.7071, 0.0, 0.0, 0.7071), t_lb=(-0.18, 0.0, -0.095), num_s=1000.0, num_e=200.0),
        "frontend": dict(variant="frontend", loss=LOSS_HUBER, loss_a=0.1, q_lb=(1.0, 0.0, 0.0, 0.0), t_lb=(0.0, 0.0, 0.0), num_s=0.0, num_e=0.0)}


def params(variant, **over):
    """the parameter set of a variant (L/config, R/config, L/src/LidarOdometry.cpp:365) as a plain dict, with overrides"""
    return dict(_CFG[variant], **over)


def device_overrides(prm):
    """keywords for lili_om_amd.make_params(variant, ...)"""
    return dict(loss=int(prm["loss"]), loss_a=float(prm["loss_a"]), scale_surf_num=float(prm["num_s"]), scale_edge_num=float(prm["num_e"]))


def oracle_overrides(prm):
    return dict(loss=int(prm["loss"]), loss_a=float(prm["loss_a"]))


def oracle_scale(prm, kind, N):
    """the `scale` argument of oracle.linearize_surf / linearize_edge"""
    num = prm["num_s"] if kind == "s" else prm["num_e"]
    return (float(num), int(N)) if num > 0 and prm["variant"] != "frontend" else 1.0


def weight(prm, kind, score, N):
    """the weight in front of the geometry, as the reference writes it: R/src/BackendFusion.cpp:861 in double, :843 in float; (n,) f64"""
    score = np.atleast_1d(score)
    if kind == "s":
        if prm["variant"] == "frontend":
            return np.ones(score.shape[0])
        s = score.astype(np.float64)
        return (s * float(prm["num_s"])) / float(int(N)) if prm["num_s"] > 0 else s
    s = score.astype(np.float32)
    return ((s * np.float32(prm["num_e"])) / np.float32(int(N))).astype(np.float64) if prm["num_e"] > 0 else s.astype(np.float64)


# ------------------------------------------------------------------------------------------------
# quaternions, f64 (pose design only)
# ------------------------------------------------------------------------------------------------
def qmul(a, b):
    aw, ax, ay, az = a; bw, bx, by, bz = b
    return np.array([aw * bw - ax * bx - ay * by - az * bz, aw * bx + ax * bw + ay * bz - az * by, aw * by - ax * bz + ay * bw + az * bx, aw * bz + ax * by - ay * bx + az * bw])


def qaxis(angle, axis):
    axis = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    return np.r_[math.cos(0.5 * angle), math.sin(0.5 * angle) * axis]


def default_rotation(prm, kind):
    """the body rotation under which the factor sees the association's rotation: Q_ASSOC q_lb for the plane factor with extrinsic, Q_ASSOC otherwise"""
    if kind == "e" or prm["variant"] == "frontend":
        return np.array(Q_ASSOC)
    q = qmul(Q_ASSOC, np.asarray(prm["q_lb"]) / np.linalg.norm(prm["q_lb"]))
    return q / np.linalg.norm(q)


# ------------------------------------------------------------------------------------------------
# scenes
# ------------------------------------------------------------------------------------------------
def _frozen(d):
    for v in d.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return d


@functools.lru_cache(maxsize=None)
def scene(variant, offset):
    """-> dict(surf_map (m, 3 | 4) f32, surf_q (ns, 3 | 4) f32 healthy local queries, surf_d (ns,) the model's distance of each plane from the origin, surf_c (ns, 3),
    edge_map, edge_q, edge_c (absent rows for the front-end: no edge factors, L/src/LidarOdometry.cpp:513-526), invalid (3 | 4,) f32 a local query outside every gate)"""
    ps, pm = P.build("generic", offset, variant), P.model("generic", offset, variant)
    sel = np.isin(ps["kind"], ("patch", "huge", "through0")) & pm["valid"] & pm["decided"]          # (one or two through0 queries per scene are undecided: left out)
    assert pm["decided"][sel].all() and pm["valid"][sel].all() and sel.sum() > 300                   # no query may be undecided in its fit
    mp_, ql = P.clouds(ps, variant)
    out = dict(surf_map=mp_, surf_q=np.ascontiguousarray(ql[sel]), surf_d=pm["ninv"][sel].copy(), surf_c=ps["centre"][ps["cl"][sel]].copy(), offset=offset, variant=variant)
    cell = np.asarray(OFFSETS[offset]) + 0.5 * PITCH
    inv = E._to_local(cell[None])[0]
    for cloud in (ps["map_xyz"], E.build("generic", offset)["map_xyz"]):
        assert np.linalg.norm(cloud.astype(np.float64) - E.to_map(inv[None]).astype(np.float64), axis=1).min() > 2.5
    out["invalid"] = np.r_[inv, np.float32(100.0)][:ql.shape[1]].astype(np.float32)
    if variant != "frontend":
        es = E.build("generic", offset)
        own = 5 * np.arange(es["n"])[:, None] + np.arange(5)[None, :]
        d2 = E.d2_f32(es["q_map"], es["map_xyz"][own])
        idx = np.take_along_axis(own, np.stack([np.lexsort((own[i], d2[i])) for i in range(es["n"])]), 1)
        em = E.model(es["map_xyz"], es["q_map"], idx, variant)
        esel = np.isin(es["kind"], ("line", "huge")) & em["valid"] & em["decided"]
        assert em["decided"][esel].all() and em["valid"][esel].all() and esel.sum() > 100
        out.update(edge_map=es["map_xyz"], edge_q=np.ascontiguousarray(es["q_local"][esel]), edge_c=es["centre"][esel].copy())
    return _frozen(out)


def probe_queries(variant, offset):
    """indices into surf_q / edge_q of the NREC probe records per kind: at `origin` the clusters nearest to the origin (an f32 ulp of the record is smallest there,
    DMIN depends on it), at `far` the planes farthest from the origin (cancel) — and one through0 plane in either"""
    s = scene(variant, offset)
    key = np.linalg.norm(s["surf_c"], axis=1) if offset == "origin" else -s["surf_d"]
    si = list(np.argsort(key, kind="stable")[:NREC - 1]) + [int(np.argmin(s["surf_d"]))]
    ei = list(np.argsort(np.linalg.norm(s["edge_c"], axis=1), kind="stable")[:NREC]) if variant != "frontend" else []
    return [int(i) for i in si], [int(i) for i in ei]


EXACT = dict(surf_map=np.array([(-0.25, -0.25, 0.25), (0.25, -0.25, 0.25), (0.25, 0.25, 0.25), (-0.25, 0.25, 0.25), (0.0, 0.0, 0.25)], np.float32),
             surf_q=np.array([(0.0, 0.0, 0.25)], np.float32),          # (on the z axis: whatever rounding noise the fit leaves in n.x, n.y meets a zero)
             edge_map=np.array([(k / 32.0, 0.0, 0.0) for k in (-2, -1, 0, 1, 2)], np.float32), edge_q=np.array([(0.015625, 0.0, 0.0)], np.float32),
             invalid=np.array([10.0, 10.0, 10.0], np.float32))
IDENTITY = (np.zeros(3), np.array([1.0, 0.0, 0.0, 0.0]))


def exact_clouds(variant, kind):
    """(map, [invalid, probe, invalid]) of the f32-exact scene of `zero` (surf) / `onepoint` (edge), associated at the identity"""
    mp_, q = EXACT[kind + "_map"], np.stack([EXACT["invalid"], EXACT[kind + "_q"][0], EXACT["invalid"]])
    if variant == "livox" and kind == "surf":
        mp_ = np.c_[mp_, 100.0 + np.array([1, -2, 3, -1, 2])].astype(np.float32); q = np.c_[q, np.full(3, 100.0)].astype(np.float32)
    return np.ascontiguousarray(mp_), np.ascontiguousarray(q)


# ------------------------------------------------------------------------------------------------
# the model, vectorised: rows of n records at one pose, in dtype `dt` (numpy.longdouble for the referee, f64 works as well), and the magnitudes S in f64
# ------------------------------------------------------------------------------------------------
def _rot(q, v):
    """Eigen's q * v (Quaternion::_transformVector): v + w (2 u x v) + u x (2 u x v)"""
    uv = np.cross(q[1:][None, :], v)
    return v + 2 * q[0] * uv + 2 * np.cross(q[1:][None, :], uv)


def _drot(q, v):
    """its derivative by (w, x, y, z): (4, n, 3)"""
    u = q[1:][None, :]
    uv = np.cross(u, v)
    out = [2 * uv]
    for i in range(3):
        e = np.zeros((1, 3), v.dtype); e[0, i] = 1
        ev = np.cross(e, v)
        out.append(2 * q[0] * ev + 2 * (np.cross(e, uv) + np.cross(u, ev)))
    return np.stack(out)


def _ac(a, b):
    """|a| x |b| with every product positive"""
    a, b = np.abs(a), np.abs(b)
    return np.stack([a[..., 1] * b[..., 2] + a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] + a[..., 0] * b[..., 2], a[..., 0] * b[..., 1] + a[..., 1] * b[..., 0]], -1)


def _arot(q, v):
    u = np.abs(q[1:])[None, :]
    uv = _ac(u, v)
    return np.abs(v) + 2 * abs(q[0]) * uv + 2 * _ac(u, uv)


def _adrot(q, v):
    u = np.abs(q[1:])[None, :]
    uv = _ac(u, v)
    out = [2 * uv]
    for i in range(3):
        e = np.zeros((1, 3)); e[0, i] = 1
        ev = _ac(e, v)
        out.append(2 * abs(q[0]) * ev + 2 * (_ac(e, uv) + _ac(u, ev)))
    return np.stack(out)


def _dot(a, b):
    return (a * b).sum(-1)


def _corrector(prm, r, J, Sr, SJ, dt):
    """robustified (r', J', cost) and their magnitudes: f = sqrt(rho'(r^2)); the corrector of MarginalizationFactor.cpp:44-70 reduces to r' = f r, J' = f J because
    rho'' <= 0 for both losses (the general form is kept in the mpmath model, which the CPU test compares this with)"""
    a = dt(prm["loss_a"]); b = a * a
    s = r * r
    ar = np.abs(r)
    one = np.ones_like(r)
    with np.errstate(divide="ignore", invalid="ignore"):
        if prm["loss"] == LOSS_CAUCHY:
            f2 = 1 / (1 + s / b)
            f = np.sqrt(f2)
            rho0, df, dfr = b * np.log1p(s / b), ar / b * f2 * f, f2 * f
            crho = b + 0 * one                                                     # ceres evaluates b log(1 + s / b): the rounding of the sum alone is b eps
        elif prm["loss"] == LOSS_HUBER:
            out = s > b
            f2 = np.where(out, a / np.where(out, ar, one), one)
            f = np.sqrt(f2)
            rho0 = np.where(out, 2 * a * ar - b, s)
            df, dfr = np.where(out, f / (2 * np.where(out, ar, one)), 0 * one), np.where(out, f / 2, one)
            crho = np.where(out, 2 * a * ar + b, 0 * one)                          # 2 a |r| - b
        else:
            f2, f, rho0, df, dfr, crho = one, one, s, 0 * one, one, 0 * one
    r2, J2, cost = f * r, f[:, None] * J, rho0 / 2
    f64 = lambda x: np.asarray(x, np.float64)   # noqa: E731
    Sr2 = f64(dfr) * Sr + f64(np.abs(r2))
    SJ2 = f64(f)[:, None] * SJ + f64(np.abs(J) * df[:, None]) * Sr[:, None] + f64(np.abs(J2))
    Sc = f64(f2) * (f64(ar) + DEVICE_FACTOR * K_EVAL * EPS * Sr) * Sr + f64(np.abs(cost)) + f64(crho) / 2          # (second order kept: |r| may be below its own error)
    return r2, J2, cost, Sr2, SJ2, Sc


def rows(kind, prm, rec, w, t, q, dt=LD):
    """kind 's': rec = dict(cp, n (k, 3) f32, d (k,) f32); 'e': dict(cp, a, b (k, 3) f32); w (k,) f64 weights; pose t (3,), q (4,) f64.
    -> X (k, 8) = [J'(7) | r'], cost (k,) in dt; S (k, 8), Sc (k,) f64: the error of an evaluation in f64 is gamma S"""
    f64 = lambda x: np.asarray(x, np.float64)   # noqa: E731
    t, q, wd = np.asarray(t, np.float64).astype(dt), np.asarray(q, np.float64).astype(dt), np.asarray(w, np.float64).astype(dt)
    cp = np.asarray(rec["cp"], np.float32).astype(dt)
    at, aq, aw = f64(np.abs(t)), f64(np.abs(q)), f64(np.abs(wd))
    with np.errstate(divide="ignore", invalid="ignore"):
        if kind == "s":
            n, d = np.asarray(rec["n"], np.float32).astype(dt), np.asarray(rec["d"], np.float32).astype(dt)
            if prm["variant"] == "frontend":
                v, mv = cp, f64(np.abs(cp))
            else:
                qlb, tlb = np.asarray(prm["q_lb"], np.float64).astype(dt), np.asarray(prm["t_lb"], np.float64).astype(dt)
                qi = np.r_[qlb[0], -qlb[1:]] / _dot(qlb, qlb)                      # Eigen's inverse(): conjugate / squaredNorm  (:86)
                v, mv = _rot(qi, cp - tlb[None, :]), _arot(f64(qi), f64(np.abs(cp)) + f64(np.abs(tlb))[None, :])
            pw = _rot(q, v) + t[None, :]                                           # :87
            base = _dot(n, pw) + d                                                 # :90
            jq = _dot(n[None], _drot(q, v)).T                                      # (k, 4)
            an = f64(np.abs(n))
            mbase = _dot(an, _arot(aq, mv) + at[None, :]) + f64(np.abs(d))
            mjq = _dot(an[None], _adrot(aq, mv)).T
            r, J = wd * base, np.concatenate([wd[:, None] * n, wd[:, None] * jq], 1)
            Sr = aw * mbase + f64(np.abs(r))
            SJ = np.concatenate([aw[:, None] * an, aw[:, None] * mjq], 1) + f64(np.abs(J))
        else:
            A, B = np.asarray(rec["a"], np.float32).astype(dt), np.asarray(rec["b"], np.float32).astype(dt)
            lp = _rot(q, cp) + t[None, :]                                          # :38
            nu, de = np.cross(lp - A, lp - B), A - B                               # :40-41
            nn, dn = np.sqrt(_dot(nu, nu)), np.sqrt(_dot(de, de))
            r = wd * (nn / dn)                                                     # :43-44
            g = np.cross(de, nu) / nn[:, None]                                     # d|nu| / dlp: d nu = dlp x (A - B), so d|nu| = dlp . ((A - B) x nu) / |nu|
            jt = (wd / dn)[:, None] * g
            J = np.concatenate([jt, _dot(jt[None], _drot(q, cp)).T], 1)
            mlp = _arot(aq, f64(np.abs(cp))) + at[None, :]
            # lp - A is the difference of two numbers of size |lp| and nearly exact itself: the plain magnitude bound (|lp| + |A|)^2 for nu would be eight orders
            # above |nu|.  From lp on the bound is carried step by step (running error, Higham section 3.3): what the operands carry, plus the result's own rounding
            aa, ab, ade, anu = f64(np.abs(lp - A)), f64(np.abs(lp - B)), f64(np.abs(de)), f64(np.abs(nu))
            Sa, Sb = mlp + aa, mlp + ab
            mnu = _ac(Sa, ab) + _ac(aa, Sb) + _ac(aa, ab)
            mg = _ac(ade, mnu) + 2.0 * _ac(ade, anu)
            nn64, dn64 = f64(nn), f64(dn)
            Snn, Sdn = _dot(anu, mnu) / nn64 + nn64, 2.0 * dn64
            rel = Snn / nn64 + Sdn / dn64 + 1.0
            Sr = f64(np.abs(r)) * rel
            Sjt = (aw / (nn64 * dn64))[:, None] * mg + f64(np.abs(jt)) * rel[:, None]
            SJ = np.concatenate([Sjt, _dot(Sjt[None], _adrot(aq, f64(np.abs(cp)))).T], 1) + f64(np.abs(J))
    r2, J2, cost, Sr2, SJ2, Sc = _corrector(prm, r, J, Sr, SJ, dt)
    return np.concatenate([J2, r2[:, None]], 1), cost, np.concatenate([SJ2, Sr2[:, None]], 1), Sc


# ------------------------------------------------------------------------------------------------
# the model of ONE row in mpmath: the residual functor as the reference writes it, differentiated numerically
# ------------------------------------------------------------------------------------------------
def _mcross(a, b):
    return [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]


def _mrot(q, v):
    uv = _mcross(q[1:], v)
    uuv = _mcross(q[1:], uv)
    return [v[i] + 2 * q[0] * uv[i] + 2 * uuv[i] for i in range(3)]


def _mvec(x):
    return [mpmath.mpf(float(c)) for c in x]


def _mresidual(kind, prm, rec, w):
    """the unrobustified residual as a function of the 7 parameters (t, q), in the working precision"""
    cp = _mvec(rec["cp"])
    if kind == "s":
        n, d = _mvec(rec["n"]), mpmath.mpf(float(rec["d"]))
        if prm["variant"] == "frontend":
            v = cp
        else:
            qlb, tlb = _mvec(prm["q_lb"]), _mvec(prm["t_lb"])
            n2 = sum(c * c for c in qlb)
            v = _mrot([qlb[0] / n2, -qlb[1] / n2, -qlb[2] / n2, -qlb[3] / n2], [cp[i] - tlb[i] for i in range(3)])

        def F(x):
            pw = _mrot(x[3:], v)
            return w * (sum(n[i] * (pw[i] + x[i]) for i in range(3)) + d)
        return F
    A, B = _mvec(rec["a"]), _mvec(rec["b"])
    dn = mpmath.sqrt(sum((A[i] - B[i]) ** 2 for i in range(3)))

    def G(x):
        lp = _mrot(x[3:], cp)
        lp = [lp[i] + x[i] for i in range(3)]
        nu = _mcross([lp[i] - A[i] for i in range(3)], [lp[i] - B[i] for i in range(3)])
        return mpmath.sqrt(sum(c * c for c in nu)) / dn * w
    return G


def _mloss(prm, s):
    """rho, rho', rho'' of ceres::CauchyLoss(a) / HuberLoss(a) / no loss"""
    a = mpmath.mpf(float(prm["loss_a"])); b = a * a
    if prm["loss"] == LOSS_CAUCHY:
        u = 1 + s / b
        return b * mpmath.log(u), 1 / u, -1 / (b * u * u)
    if prm["loss"] == LOSS_HUBER and s > b:
        rt = mpmath.sqrt(s)
        return 2 * a * rt - b, a / rt, -(a / rt) / (2 * s)
    return s, mpmath.mpf(1), mpmath.mpf(0)


def row_mp(kind, prm, rec, w, t, q, as_mp=False):
    """-> (X (8,) f64 = [J'(7) | r'], cost f64, raw |r| f64) of one record (rec: the fields of ONE record); NaN Jacobian where the edge point is ON its line.
    as_mp: X and cost as mpmath numbers (valid in the caller's working precision)"""
    with mpmath.workprec(PREC):
        F = _mresidual(kind, prm, rec, mpmath.mpf(float(w)))
        x = _mvec(np.r_[t, q])
        r = F(x)
        if kind == "e" and r == 0:
            J = [mpmath.nan] * 7                                                   # |nu| is not differentiable at nu = 0: ceres' jets give 0 / 0
        else:
            h = mpmath.ldexp(1, -H_EXP)
            J = [(F(x[:k] + [x[k] + h] + x[k + 1:]) - F(x[:k] + [x[k] - h] + x[k + 1:])) / (2 * h) for k in range(7)]
        sq = r * r
        rho = _mloss(prm, sq)
        cost = rho[0] / 2
        if prm["loss"] != LOSS_NONE:                                               # MarginalizationFactor.cpp:44-70, one residual
            s1 = mpmath.sqrt(rho[1])
            if sq == 0 or rho[2] <= 0:
                scaling, alpha_sq = s1, mpmath.mpf(0)
            else:
                alpha = 1 - mpmath.sqrt(1 + 2 * sq * rho[2] / rho[1])
                scaling, alpha_sq = s1 / (1 - alpha), alpha / sq
            J = [s1 * (j - alpha_sq * r * (r * j)) for j in J]
            raw = r
            r = r * scaling
        else:
            raw = r
        if as_mp:
            return J + [r], cost, abs(float(raw))
        return np.array([float(j) for j in J] + [float(r)]), float(cost), abs(float(raw))


# ------------------------------------------------------------------------------------------------
# probe rows
# ------------------------------------------------------------------------------------------------
def _one(rec, i):
    return {k: np.asarray(v)[i] for k, v in rec.items() if k in ("cp", "n", "d", "a", "b", "score", "s")}


def _solve_T(kind, prm, rec, Qr, target, along):
    """T (f64) such that the transformed point lies `target` (signed metres) off its plane / beside its line and `along` metres along it, under the rotation Qr"""
    with mpmath.workprec(PREC):
        cp = _mvec(rec["cp"])
        pa = _mrot(_mvec(Q_ASSOC), cp)
        pa = [pa[i] + mpmath.mpf(float(T_ASSOC[i])) for i in range(3)]            # where the association saw the point
        if kind == "s":
            n, d = _mvec(rec["n"]), mpmath.mpf(float(rec["d"]))
            nn = mpmath.sqrt(sum(c * c for c in n))
            nh = [c / nn for c in n]
            off = (sum(n[i] * pa[i] for i in range(3)) + d) / nn
            k = int(np.argmin(np.abs(np.asarray(rec["n"], np.float64))))
            e = _mcross(nh, [mpmath.mpf(int(i == k)) for i in range(3)])
            en = mpmath.sqrt(sum(c * c for c in e))
            goal = [pa[i] + nh[i] * (mpmath.mpf(target) - off) + e[i] / en * mpmath.mpf(along) for i in range(3)]
            if prm["variant"] == "frontend":
                v = cp
            else:
                qlb, tlb = _mvec(prm["q_lb"]), _mvec(prm["t_lb"])
                n2 = sum(c * c for c in qlb)
                v = _mrot([qlb[0] / n2, -qlb[1] / n2, -qlb[2] / n2, -qlb[3] / n2], [cp[i] - tlb[i] for i in range(3)])
        else:
            A, B = _mvec(rec["a"]), _mvec(rec["b"])
            u = [A[i] - B[i] for i in range(3)]
            un = mpmath.sqrt(sum(c * c for c in u)); u = [c / un for c in u]
            s = sum((pa[i] - A[i]) * u[i] for i in range(3))
            foot = [A[i] + u[i] * s for i in range(3)]
            e = [pa[i] - foot[i] for i in range(3)]
            en = mpmath.sqrt(sum(c * c for c in e))
            if en < mpmath.mpf(10) ** -9:
                e = _mcross(u, [mpmath.mpf(int(i == 0)) for i in range(3)]); en = mpmath.sqrt(sum(c * c for c in e))
            goal = [foot[i] + e[i] / en * mpmath.mpf(target) + u[i] * mpmath.mpf(along) for i in range(3)]
            v = cp
        rv = _mrot(_mvec(Qr), v)
        return np.array([float(goal[i] - rv[i]) for i in range(3)])


DELTAS6 = [s * 10.0 ** -k for k in range(1, 7) for s in (1, -1)]
DECADES = [10.0 ** k for k in range(-12, 7)]


def probe_rows(variant, offset, srec, erec, n_own=1):
    """[dict(fam, kind, i, t, q, prm, N, w)] for the probe records srec / erec (the NREC records of probe_queries(), fields as read back from the side under test;
    erec None for the front-end).  N: the count the weight is scaled with (rot) — n_own is the slot's own, any other value is imported."""
    out = []

    def add(fam, kind, i, prm, target, Qr=None, along=0.0, N=None, signed=True):
        rec = _one(srec if kind == "s" else erec, i)
        N = n_own if N is None else N
        w = float(weight(prm, kind, rec["score"] if kind == "s" else rec["s"], N)[0])
        dist = target / w
        if kind == "e":
            dist = abs(dist)
            if not DMIN[offset] <= dist <= 1e5:
                return
        elif not signed:
            dist = abs(dist)
        Qr = default_rotation(prm, kind) if Qr is None else Qr
        out.append(dict(fam=fam, kind=kind, i=i, t=_solve_T(kind, prm, rec, Qr, dist, along), q=np.asarray(Qr, np.float64), prm=prm, N=N, w=w))

    kinds = ("s",) if variant == "frontend" else ("s", "e")
    c = 0
    for kind in kinds:
        if variant in ("frontend", "livox"):
            prm = params(variant, loss=LOSS_HUBER, loss_a=0.1)
            for d in DELTAS6:
                c += 1
                add("huber", kind, c % NREC, prm, (1 - 2 * (c % 2)) * 0.1 * (1.0 + d))
            for r in (1e-9, 1e-3, 1.0, 1e3):
                c += 1
                add("huber", kind, c % NREC, prm, -r if c % 2 else r)
        if variant in ("livox", "rot"):
            prm = params(variant)
            for r in DECADES:
                c += 1
                add("cauchy", kind, c % NREC, prm, -r if c % 2 else r)
            if variant == "rot":
                for N in (2, 1000):
                    for r in (1e-6, 1e-1, 1e2, 1e5):
                        c += 1
                        add("cauchy", kind, c % NREC, prm, r, N=N)
                prm2 = params(variant, num_s=1024.0, num_e=256.0)
                for N in (n_own, 2):
                    for r in (1e-3, 1.0, 1e3):
                        c += 1
                        add("cauchy", kind, c % NREC, prm2, -r, N=N)
        prm = params(variant, loss=LOSS_NONE)
        for r in DECADES[::2]:
            c += 1
            add("none", kind, c % NREC, prm, r if c % 2 else -r)
        prm = params(variant)
        if kind == "s" and offset == "far":
            for k in range(1, 10):
                rec = _one(srec, k % (NREC - 1))
                w = float(weight(prm, "s", rec["score"], n_own)[0])
                add("cancel", "s", k % (NREC - 1), prm, (1 - 2 * (k % 2)) * 10.0 ** -k * w)
        if kind == "e":
            for k in range(0, 7):
                rec = _one(erec, k % NREC)
                w = float(weight(prm, "e", rec["s"], n_own)[0])
                add("nearline", "e", k % NREC, prm, 5e-2 * 10.0 ** -k * w)
        # pose
        base = default_rotation(prm, kind)
        axis = (0.4, -0.3, 0.85)
        poses = [qmul(qaxis(a, axis), base) for a in (0.0, 1e-8, 1.0, math.pi - 1e-6, math.pi)]
        poses += [-qmul(qaxis(1.0, axis), base), 1.001 * base, 0.999 * qmul(qaxis(0.3, axis), base)]
        for j, Qr in enumerate(poses):
            rec = _one(srec if kind == "s" else erec, j % NREC)
            w = float(weight(prm, kind, rec["score"] if kind == "s" else rec["s"], n_own)[0])
            add("pose", kind, j % NREC, prm, 0.05 * w, Qr=Qr)
        for j, along in enumerate((16.0, 256.0, 4096.0) if kind == "s" else (16.0, 256.0)):
            rec = _one(srec if kind == "s" else erec, j % NREC)
            w = float(weight(prm, kind, rec["score"] if kind == "s" else rec["s"], n_own)[0])
            add("pose", kind, j % NREC, prm, 0.05 * w, Qr=poses[2], along=along)
    return out


def probe_model(row, srec, erec):
    """-> dict(X (8,), cost, raw, S (8,), Sc): the mpmath row and its magnitudes (allowance = factor K_EVAL eps S)"""
    rec = _one(srec if row["kind"] == "s" else erec, row["i"])
    X, cost, raw = row_mp(row["kind"], row["prm"], rec, row["w"], row["t"], row["q"])
    one = {k: np.asarray(v)[None] for k, v in rec.items()}
    _, _, S, Sc = rows(row["kind"], row["prm"], one, np.array([row["w"]]), row["t"], row["q"])
    return dict(X=X, cost=cost, raw=raw, S=S[0], Sc=float(Sc[0]))


def gram_of_row(m, factor):
    """the 8 x 8 Gram of one row (its outer product) and its per-entry allowance; cost allowance"""
    X, dX = m["X"], factor * K_EVAL * EPS * m["S"]
    ax = np.abs(X)
    G = np.outer(X, X)
    return G, np.outer(ax, dX) + np.outer(dX, ax) + np.outer(dX, dX) + EPS * np.abs(G), factor * K_EVAL * EPS * m["Sc"]          # (second order kept: |r| may be below its own error)


# ------------------------------------------------------------------------------------------------
# whole Grams
# ------------------------------------------------------------------------------------------------
def summation_depth(n):
    nb = min(-(-n // LIN_BLOCK), MAX_LIN_BLOCKS)
    trips = -(-n // (nb * LIN_BLOCK)) if n else 0
    return 64 * trips + 16 + nb + 8


def gram_model(kind, prm, rec, N, t, q, n_q, factor, depth=None):
    """rec: the compacted record list of ONE kind (fields (k, ...)), N the count its weights are scaled with, n_q the number of queries of the launch.
    depth: the depth of the summation tree if it is not k_linearize's.  -> (G (8, 8) longdouble, cost, allowance (8, 8) f64, cost allowance)"""
    depth = summation_depth(n_q) if depth is None else depth
    k = np.asarray(rec["cp"]).shape[0]
    if k == 0:
        return np.zeros((8, 8), LD), LD(0), np.zeros((8, 8)), 0.0
    w = weight(prm, kind, rec["score"] if kind == "s" else rec["s"], N)
    X, cost, S, Sc = rows(kind, prm, rec, w, t, q, dt=LD)
    G = X.T @ X
    ax = np.abs(X).astype(np.float64)
    dX = factor * K_EVAL * EPS * S
    absG = ax.T @ ax
    allow = ax.T @ dX + dX.T @ ax + dX.T @ dX + EPS * absG + 2.0 * depth * EPS * absG
    acost = float(factor * K_EVAL * EPS * Sc.sum() + 2.0 * depth * EPS * np.abs(cost).astype(np.float64).sum())
    return G, cost.sum(), allow, acost


SIZES = (1, 63, 64, 65, 1023, 1024, 1025, 262144, 262145, 263169, 524289)
EDGE_SIZES = (1, 63, 64, 65, 1023, 1024, 1025, 262145)
PATTERNS = ("all", "wave0_invalid", "block0_invalid", "last_only", "second_trip_only", "every_other")


def validity(n, pattern):
    """(n,) bool — which queries of a partition case are valid ones"""
    v = np.ones(n, bool)
    i = np.arange(n)
    if pattern == "wave0_invalid":
        v[:64] = False
    elif pattern == "block0_invalid":
        v[:1024] = False
    elif pattern == "last_only":
        v[:] = False; v[-1] = True
    elif pattern == "second_trip_only":
        v = i >= MAX_LIN_BLOCKS * LIN_BLOCK
    elif pattern == "every_other":
        v = i % 2 == 1
    elif pattern != "all":
        raise ValueError(pattern)
    return v


def partition_applies(n, pattern):
    if pattern == "second_trip_only":
        return n in (262145, 263169)
    return not ((pattern == "wave0_invalid" and n <= 64) or (pattern == "block0_invalid" and n <= 1024) or (pattern == "every_other" and n < 2))


def partition_queries(variant, offset, kind, n, pattern):
    """(queries (n, 3 | 4) f32, valid (n,) bool): the healthy queries of the scene cycled over the valid positions, the far-away query everywhere else"""
    s = scene(variant, offset)
    src = s["surf_q"] if kind == "s" else s["edge_q"]
    v = validity(n, pattern)
    q = np.empty((n, src.shape[1]), np.float32)
    q[:] = s["invalid"][:src.shape[1]]
    q[v] = src[np.arange(int(v.sum())) % src.shape[0]]
    return q, v


def partition_pose(variant, kind):
    """one linearisation pose per variant and kind, 0.1 m and 7e-5 rad (5 cm at 700 m) off the association's: unweighted residuals from 0 to 0.15 m, on both sides of
    the front-end's Huber threshold; still inside every gate when an iteration associates there"""
    prm = params(variant)
    Qr = qmul(qaxis(7e-5, (0.2, 0.9, -0.4)), default_rotation(prm, kind))
    if kind == "e" or variant == "frontend":
        t = np.array(T_ASSOC)
    else:   # body translation under which the plane factor sees the association's: T_ASSOC + R t_lb (unit extrinsic assumed: a design pose, nothing depends on it)
        t = np.array(T_ASSOC) + E._qrot(np.array(Q_ASSOC), np.asarray(prm["t_lb"]))
    return t + np.array([0.06, -0.05, 0.07]), Qr


def measure_K(cases):
    """cases: [(model dict of probe_model, X_oracle (8,), cost_oracle)] -> the worst |oracle - model| / (eps S) over every finite entry"""
    k = 0.0
    for m, Xo, co in cases:
        ok = np.isfinite(m["X"])
        k = max(k, float((np.abs(Xo - m["X"])[ok] / (EPS * m["S"][ok])).max()), abs(co - m["cost"]) / (EPS * m["Sc"]))
    return k


def plus_jacobian(q):
    """ceres::QuaternionParameterization::ComputeJacobian: d(q (+) delta) / d delta at 0, rows w, x, y, z"""
    w, x, y, z = q
    return np.array([[-x, -y, -z], [w, z, -y], [-z, w, x], [y, -x, w]], LD)


def gn_step_model(G, allow, q):
    """the Gauss-Newton step of the 6-dof local parameterisation from a Gram [J | r]^T [J | r] (longdouble): H = P^T G77 P, g = -P^T G7r, delta = H^-1 g.
    -> (delta (6,), cond(H), bound, componentwise (6,)).  bound: the first-order norm bound cond(H) (|dH| / |H| + |dg| / |g|) |delta| from the Gram's per-entry
    allowance, plus 64 eps cond(H) |delta| for the device's own 6 x 6 factorisation (backward stable: a few n eps).  componentwise: the same first-order statement
    without the norms, |H^-1| (|dg| + |dH| |delta|) + 64 eps |H^-1| |H| |delta| — H mixes metres and radians, so cond(H) overstates what a perturbation that is small
    entry by entry can do by orders of magnitude; this form does not"""
    Pm = np.zeros((7, 6), LD); Pm[:3, :3] = np.eye(3); Pm[3:, 3:] = plus_jacobian(np.asarray(q, np.float64).astype(LD))
    H, g = Pm.T @ G[:7, :7] @ Pm, -(Pm.T @ G[:7, 7])
    H64, g64 = H.astype(np.float64), g.astype(np.float64)
    delta = np.linalg.solve(H64, g64)
    delta = delta + np.linalg.solve(H64, (g - H @ delta.astype(LD)).astype(np.float64))           # one refinement with the residual in longdouble
    aP = np.abs(Pm).astype(np.float64)
    dH, dg = aP.T @ allow[:7, :7] @ aP, aP.T @ allow[:7, 7]
    cond = float(np.linalg.cond(H64))
    bound = cond * (np.linalg.norm(dH) / np.linalg.norm(H64) + np.linalg.norm(dg) / np.linalg.norm(g64) + 64 * EPS) * np.linalg.norm(delta)
    Hi = np.abs(np.linalg.inv(H64))
    cw = Hi @ (dg + dH @ np.abs(delta)) + 64 * EPS * (Hi @ (np.abs(H64) @ np.abs(delta)))
    return delta, cond, float(bound), cw
