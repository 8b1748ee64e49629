"""Hard neighbourhoods for the plane fit of the association kernels (surf_fit, lili_s2m_dev.h: the kd_max_radius gate, the Livox reflectivity weights and
their reflect_thres gate, plane_fit_centered / lstsq53, the normalisation, the surf_dist_thres loop, the float pd / weight chain, the surf_weight_min gate,
the record and the score) and an independent model of it.

Shared by tests/test_plane_fit_cases_cpu.py (the conditions on the inputs and the oracle held to the model) and tests/test_plane_fit_hard_gpu.py (every
launcher against the oracle and the model).

Scene.  The lattice of tests/edge_fit_cases.py: clusters of exactly five map points on a cubic lattice of pitch 4 m, cluster k owning map rows 5 k .. 5 k + 4,
the points within 0.4 m of their node, query k within 0.05 m of the patch of cluster k (up to 0.7 m from the node in the gate kinds), so the five nearest
neighbours of a query are its own cluster without doubt: every other point is more than 2.9 m away, kd_max_radius is 1.  Queries are handed over in a local
frame and reach the map through (Q_ASSOC, T_ASSOC) of the edge cases.  Every case is built at `origin` (lattice from (0, 0, 0)) and at `far`
(500, -480, 15).  The plane fit is NOT translation invariant — it solves A n = -1 with the raw coordinates as rows — so `far` is not a copy of `origin`:
|n| ~ 1 / 700 there and cond(A) is in the thousands for a healthy patch.  A few kinds need a node with a coordinate exactly 0: at `origin` those are
lattice nodes of the faces i = 0, j = 0, k = 0; at `far` only z = 0 is within reach (nodes (500 + 4 i, -480 + 4 j, 0), 15 m under the lattice — x = 0 or
y = 0 would stretch the map's box by 500 m, and a grid coarsened for its size gets no fine index, so the dense launch would not run).  One cluster may serve
more queries than its own: the wgate kind at `origin` hangs its queries on the cluster of the node (0, 0, 0), the only one near enough to the origin for the
configs' surf_weight_min to be reachable; `cl` maps queries to clusters.

Kinds (one string per query):
  patch     planar patches in random orientation, off-plane noise 1e-6 .. 1e-2 of the extent;   tiny: extent 1e-4 m;   huge: the full 0.4 m
  strip     nearly collinear patches, the second in-plane extent 1e-6 .. 1 of the first: rho = denom / scale of plane_fit_centered (exact, by the model)
            populates [1e-9, 1e-7) below the switch, [1e-7, 1e-6) just above it and [1e-6, 1e-4)
  through0  the plane passes the origin at distance h = +-1e-9 .. +-1e-2 m; away from the origin the normal is perpendicular to the node direction
  zerocol   f32-exact clusters in the coordinate planes: one column of A is exactly zero, nz = 2 without rounding — decided, both sides return the basic solution;
            three quarters are near a line of that plane (the fitted plane is valid), a quarter in general position (refused by surf_dist_thres)
  nearrank  zerocol with one point 1e-12 .. 1e-10 of the cluster's size out of the coordinate plane: sigma_3 / sigma_1 from 1.1e-12 up, full rank on both sides
  tilt0     f32-exact tilted planes through the origin (h = 0);   colgen / colaxis: f32-exact collinear clusters in a general direction / along the axes;
  dup       five coincident points, four coincident points and one other.  In these four the third (or second) pivot is rounding noise of either sign
            against eps max ||col||: rank_undecided by construction (unless exactly zero columns decide, which the model reads off the data)
  dgate     a square patch whose centre is lifted so that the largest |n^ . m + 1 / |n|| of the REFITTED plane is surf_dist_thres (1 + d), d = +-1e-1 .. +-1e-7
            (the lift is found by bisection on a plain f64 fit of the rounded points; the model classifies)
  wgate     queries whose weight 1 - 0.9 |pd| / |p|^(1/2) is surf_weight_min + d (1 - surf_weight_min); at `origin` on the origin cluster with the configs'
            value, and (kind wulp) pairs ONE f32 ulp of weight apart, on the two f32 neighbours of the threshold; at `far` (|p| ~ 700, weight > 0.96 for any query in reach)
            with surf_weight_min = 0.98 handed identically to both sides
  dexact    (case dexact, `origin` only: it needs a map point AT the origin) the largest residual equals surf_dist_thres exactly, see _dexact: accepted
  kgate     the fifth neighbour's d^2 = 1 + d either side of kd_max_radius, the query in the patch's plane
  refl_*    (livox) integer reflectivities 0 .. 255: sum_w 14 (lo), exactly 15 (eq: the gate is a strict >, accepted), 16 (hi); span: |differences| 1 : 11 in one
            cluster, the widest that sum_w <= 15 allows; zero1 / zero5: one / five zero differences; inf0: a zero difference on a point with a coordinate exactly
            0 (inf * 0).  The zero kinds are dropped through NaN by the reference, the oracle and the device.  Case `reflwide` hands reflect_thres = 300 to both
            sides: |differences| up to 1 : 255, the least-squares weights w^2 span up to 1 : 6.5e4 (1 : 1e3 cannot be had under sum_w <= 15)
Every livox cluster outside the refl kinds carries reflectivities 100 +- {1, 2, 3} (query 100): the weighted fit runs everywhere.

Model.  Transcribes neither solver.  From the neighbour list it is given: the f64 weights as one plain expression (1 / |D|) / sum |D|; the minimiser of
sum w_k^2 (p_k . n + 1)^2 EXACTLY — the 3 x 3 normal equations by Cramer in integer arithmetic on the f32 inputs scaled by their common power of two, every
quotient a fractions.Fraction rounded once; n^, 1 / |n|, the five residuals and pd from exact numerators (no cancellation at 700 m); the weight through
the documented float chain (float pd, float r2, sqrtf(sqrtf()), double division, float cast) and in exact arithmetic; cond(A_w) by numpy.linalg.svd;
rho = det(A^T A) / (tr S^2 tr(A^T A)) exactly.  An exactly zero column is dropped and the rest solved the same way (the basic solution).

Margins (derived, not measured).
  Solution bound.  A backward-stable least-squares solver differs from the exact x by ||dx|| <= B ||x||.  B = K eps cond(A_w) with K MEASURED on the CPU as the
  oracle's lstsq53's worst ||x - x_exact|| / (||x_exact|| eps cond) over every case, offset and variant: K = 146 (in use: 150).  That figure is made by
  through0 alone (every other kind stays below 4.4): there the rows' own f32 rounding leaves a residual that is large against the plane's distance from the
  origin, and least-squares perturbation theory (Wedin; Higham, Accuracy and Stability, thm 20.1) has a second term, cond^2 times the relative residual, that
  dominates.  Taken alone, 150 eps cond would allow every healthy patch a hundred times its true error, so the allowance is the SMALLER of the plain form and
  the full first-order one: B = min(K eps cond, K_ls eps cond (1 + cond theta)), theta = ||r_w|| / (sigma_1 ||x||), K_ls measured the same way = 1.50 (in
  use: 1.6) — never wider than the plain form.  Where the default build takes the centred fast path (rho >= 1e-7), B is the larger of that and K_c eps / rho (its
  denominator is a determinant computed with relative error ~eps / rho); K_c = worst err rho / eps of centred_f64 below (plain numpy f64, no fma) = 0.47 (in
  use: 0.5).  tests/test_plane_fit_cases_cpu.py re-measures the three, prints them and fails if one exceeds the value in use.  The oracle is held to 1 x,
  the device to 8 x (other summation order, explicit fma in the centred path, recomputed instead of down-dated column norms, multiply-by-reciprocal for
  division).  To first order n^ errs by B (normalising projects the error) and 1 / |n| by B relative.
  rank_decided_full: sigma_3 > 1e-12 sigma_1 (four orders above the eps-relative threshold and the Householder noise);  rank_decided_deficient: exactly zero
  columns and the remaining ones full rank by the same rule;  everything else rank_undecided.
  surf_dist_thres: |n^ . m + 1 / |n|| as evaluated differs from the exact residual by at most (2 B_dev + 8 eps) (|m| + 1 / |n|); UNDECIDED if the largest
  residual is within that of the threshold.   surf_weight_min: the float chain's roundings — pd (2^-24 of 1 - w), r2 (two f32 roundings, a quarter each after
  the two roots), two sqrtf, the final cast — are below 4 x 2^-24 absolute, plus 0.9 / |p|^(1/2) of pd's error; UNDECIDED within that.   kd_max_radius and
  reflect_thres: nothing, d^2 is bit-compared and the sum of integer differences is exact.  A gate that refuses for certain decides the query.
  Records: per component |rec - w n^| <= one f32 ulp at the larger magnitude (floor 1e-15, as the edge file) + B w; rec.d / ||rec.n|| against the exact 1 / |n|
  at 2^-23 + B relative.  Queries with B > 1e-3 have no meaningful direction: on the device compared against the oracle only, and only if rank-decided.

Undecided queries per case (default build's bounds; origin / far, the three variants alike within a few): generic 0 - 1 / 1 - 2 (through0); rank 257 - 263 / 262 -
264, of which 240 are the kinds that are rank_undecided by construction and the rest nearrank (cond ~1e12: decided in rank, not against a gate); gates 20 - 45 /
12 - 20 (wulp by construction, wgate and dgate at d <= 1e-6); refl, reflwide 0; dexact 12 by construction.  About 510 queries of a generic case take the fast path and
390 the QR; gates and refl are fast-path throughout, rank is QR but for its patches.

Measured on an MI355X, worst err / (one f32 ulp + 8 B) over all launchers' records: against the model 0.75 (default build), 0.75 (QR everywhere), 0.75 (fast
path everywhere) — the f32 rounding of the record itself, the 8 B share of the allowance is below 1 % of it on every query that set a maximum; against the
oracle 0.86.  Flags: no decided query differs; the device and the oracle toss the rank coin differently on 1 - 23 tilt0 / colgen / dup queries per case and agree on
every other undecided one, the ulp pairs of wulp included."""
import functools
import math
from fractions import Fraction

import numpy as np

from tests import edge_fit_cases as E
from tests.edge_fit_cases import OFFSETS, PITCH, Q_ASSOC, T_ASSOC, d2_f32, occupancy, to_map  # noqa: F401  (re-exported for the two tests)

EPS, U32 = 2.0 ** -52, 2.0 ** -24
K_QR, K_LS, K_C, DEVICE_FACTOR = 150.0, 1.6, 0.5, 8.0          # the measured 146, 1.50, 0.47 rounded up (measure_constants(); the CPU test re-measures and prints them)

VARIANTS = ("livox", "rot", "frontend")
CASES = ("generic", "rank", "gates", "refl", "reflwide", "dexact")
GRID = [(c, o, v) for c in CASES for o in OFFSETS for v in VARIANTS if (v == "livox" or not c.startswith("refl")) and (o == "origin" or c != "dexact")]
DEXACT = {"livox": (0.125, 0), "rot": (0.125, 1), "frontend": (0.0625, 2)}          # (z0, axis) of the exact-equality cluster
CONFIG = {"livox": dict(surf_dist_thres=0.12, surf_weight_min=0.2, reflect_thres=15.0), "rot": dict(surf_dist_thres=0.12, surf_weight_min=0.3, reflect_thres=0.0),
          "frontend": dict(surf_dist_thres=0.06, surf_weight_min=0.4, reflect_thres=0.0)}          # L/R config_fr_iosb.yaml, L/src/LidarOdometry.cpp:389,400
KD_MAX_RADIUS = 1.0
RHO_SWITCH, RANK_FULL, B_MEANINGLESS = 1e-7, 1e-12, 1e-3
RHO_BANDS = ((1e-9, 1e-7), (1e-7, 1e-6), (1e-6, 1e-4))
RANK_UNDECIDED_KINDS = ("tilt0", "colgen", "colaxis", "dup")
# (wulp: within one f32 ulp of surf_weight_min, inside the float chain's own roundings; dexact: ON surf_dist_thres — decided by exact arithmetic, which both tests assert by kind)
UNDECIDED_BY_CONSTRUCTION = RANK_UNDECIDED_KINDS + ("wulp", "dexact")
SQUARE = 0.25 * np.array([(-1.0, -1), (1, -1), (1, 1), (-1, 1), (0, 0)])
DELTAS7 = np.r_[10.0 ** -np.arange(1.0, 8.0), -(10.0 ** -np.arange(1.0, 8.0))]


def overrides(case, offset, variant):
    """parameters handed identically to L.make_params(variant, ...) and oracle.params(variant, ...)"""
    if case == "gates" and offset == "far":
        return dict(surf_weight_min=0.98)
    if case == "reflwide":
        return dict(reflect_thres=300.0)
    if case == "dexact":
        return dict(surf_dist_thres=DEXACT[variant][0])
    return {}


def thresholds(case, offset, variant):
    return dict(CONFIG[variant], kd_max_radius=KD_MAX_RADIUS, **overrides(case, offset, variant))


# ------------------------------------------------------------------------------------------------
# clusters: every builder returns dict(pts (n, 5, 3) f64 absolute, q (n, 3) f64 absolute map frame or None, exact, mrefl (n, 5) / qrefl (n,) or None,
#                                      xq (m, 3) / xcl (m,): further queries on the part's clusters)
# ------------------------------------------------------------------------------------------------
def _plane(c, nrm, e1, e2, uv, z=0.0):
    return c[:, None, :] + uv[..., 0:1] * e1[:, None, :] + uv[..., 1:2] * e2[:, None, :] + np.asarray(z)[..., None] * nrm[:, None, :]


def _near(rng, c, nrm, e1, e2, lift=0.05):
    n = c.shape[0]
    return c + rng.uniform(-0.03, 0.03, (n, 1)) * e1 + rng.uniform(-0.03, 0.03, (n, 1)) * e2 + rng.uniform(-lift, lift, (n, 1)) * nrm


def _patch(rng, c, extent=0.27, noise=(-6, -2), squeeze=None):
    n = c.shape[0]
    nrm, e1, e2 = E._frame(rng, n)
    uv = rng.uniform(-extent, extent, (n, 5, 2))
    if squeeze is not None:
        uv[:, :, 1] *= squeeze[:, None]
    sig = extent * (1.0 if squeeze is None else squeeze) * 10.0 ** rng.uniform(noise[0], noise[1], n)
    return dict(pts=_plane(c, nrm, e1, e2, uv, rng.normal(size=(n, 5)) * sig[:, None]), q=_near(rng, c, nrm, e1, e2))


def _tiny(rng, c):
    return _patch(rng, c, extent=1e-4)


def _huge(rng, c):
    n = c.shape[0]
    nrm, e1, e2 = E._frame(rng, n)
    uv = np.tile(np.array([(-0.28, -0.28), (0.28, -0.28), (0.28, 0.28), (-0.28, 0.28), (0.03, -0.02)]), (n, 1, 1))
    return dict(pts=_plane(c, nrm, e1, e2, uv, rng.normal(size=(n, 5)) * 1e-5), q=_near(rng, c, nrm, e1, e2))


def _strip(rng, c):
    return _patch(rng, c, noise=(-4, -1), squeeze=10.0 ** rng.uniform(-6, 0, c.shape[0]))


def _through0(rng, c):
    n = c.shape[0]
    nrm = np.cross(c, E._unit(rng, n))
    at0 = np.linalg.norm(nrm, axis=1) < 1e-9
    nrm[at0] = E._unit(rng, int(at0.sum()))
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    e1 = np.cross(nrm, E._unit(rng, n)); e1 /= np.linalg.norm(e1, axis=1, keepdims=True)
    e2 = np.cross(nrm, e1)
    h = np.resize(np.r_[10.0 ** -np.arange(2.0, 10.0), -(10.0 ** -np.arange(2.0, 10.0))], n)
    uv = rng.uniform(-0.27, 0.27, (n, 5, 2))
    return dict(pts=_plane(c, nrm, e1, e2, uv, h[:, None] * np.ones((1, 5))), q=_near(rng, c + h[:, None] * nrm, nrm, e1, e2))


def _zero_axis(c):
    ax = np.argmax(c == 0.0, axis=1)
    assert (c[np.arange(c.shape[0]), ax] == 0.0).all()
    return ax


def _zerocol(rng, c):
    """in the coordinate plane through the node: (a, b) k / 128 along a line of that plane with a small integer scatter across it; every fourth in general position"""
    n = c.shape[0]
    ax = _zero_axis(c)
    pts = np.repeat(c[:, None, :], 5, 1)
    q = c.copy()
    for k in range(n):
        o = [j for j in range(3) if j != ax[k]]
        if k % 4 == 3:
            d = rng.integers(-30, 31, (5, 2)).astype(np.float64)
        else:
            ab = rng.integers(-4, 5, 2); ab[0] = ab[0] if ab.any() else 3
            d = (2 * E._k5(rng, 1, 4)[0][:, None] * ab[None, :] + rng.integers(-1, 2, 5)[:, None] * np.array([-ab[1], ab[0]])[None, :]).astype(np.float64)
        pts[k][:, o] += d * 2.0 ** -7
        q[k, o] += rng.uniform(-0.03, 0.03, 2)
        q[k, ax[k]] += rng.uniform(-0.05, 0.05)
    return dict(pts=pts, q=q, exact=True)


NEARRANK = (1.1e-12, 1.2e-12, 1.3e-12, 1.5e-12, 2e-12, 3e-12, 1e-11, 1e-10)


def _nearrank(rng, c):
    """zerocol near a line, ONE point moved out of the coordinate plane by so little that sigma_3 / sigma_1 of A is NEARRANK[k]: full rank for Eigen's threshold
    (eps max ||col||, four orders below) and for the model's rule — the plane through all five points within 1e-12 m is the answer, not the basic solution"""
    n = c.shape[0]
    ax = _zero_axis(c)
    out = _zerocol(rng, np.repeat(c, 4, 0))                                        # (every fourth of _zerocol is in general position: the first of four is taken)
    pts, q = out["pts"].reshape(n, 4, 5, 3)[:, 0].copy(), out["q"].reshape(n, 4, 3)[:, 0].copy()
    for k in range(n):
        p = _f32(pts[k]); p[2, ax[k]] = 1e-6
        sv = np.linalg.svd(p, compute_uv=False)
        pts[k, 2, ax[k]] = float(np.float32(1e-6 * NEARRANK[k % len(NEARRANK)] / (sv[2] / sv[0])))
    return dict(pts=pts, q=q, exact=True, uniform_refl=True)


def _tilt0(rng, c):
    """span(c, d2) through the origin: c (1 + a 2^-s) + b d2 / 128 with small integers a, b (c = 0: (a d1 + b d2) / 128)"""
    n = c.shape[0]
    pts = np.zeros((n, 5, 3))
    for k in range(n):
        d2 = rng.integers(-4, 5, 3).astype(np.float64)
        while np.linalg.norm(np.cross(d2, c[k] if c[k].any() else np.array([1.0, 2, 3]))) == 0:
            d2 = rng.integers(-4, 5, 3).astype(np.float64)
        a = rng.permutation(np.arange(-2, 3)).astype(np.float64)
        b = rng.integers(-3, 4, 5).astype(np.float64)
        if np.unique(np.stack([a, b], 1), axis=0).shape[0] < 5 or np.linalg.matrix_rank(np.stack([a - a.mean(), b - b.mean()], 1)) < 2:
            b = np.array([-3.0, 2, 0, -1, 3])
        if c[k].any():
            s = int(np.ceil(np.log2(np.linalg.norm(c[k]) * 10.0)))
            pts[k] = c[k][None, :] * (1.0 + a[:, None] * 2.0 ** -s) + b[:, None] * d2[None, :] * 2.0 ** -7
        else:
            d1 = np.array([3.0, -2, 4])
            pts[k] = (a[:, None] * 2 * d1[None, :] + b[:, None] * d2[None, :]) * 2.0 ** -7
    return dict(pts=pts, exact=True)


def _from_edge(builder):
    return lambda rng, c: dict(pts=c[:, None, :] + builder(rng, c.shape[0]) * 0.5, exact=True)


def _fit64(p, w=None):
    """plain f64 least squares of the (weighted) rows, for placing the gate cases only: n^ (n, 3), 1 / |n| (n,)"""
    w = np.ones(p.shape[:2]) if w is None else w
    x = np.stack([np.linalg.lstsq(w[k][:, None] * p[k], -w[k], rcond=None)[0] for k in range(p.shape[0])])
    nn = np.linalg.norm(x, axis=1)
    return x / nn[:, None], 1.0 / nn


def _f32(a):
    return np.asarray(a, np.float32).astype(np.float64)


def _square(rng, c):
    nrm, e1, e2 = E._frame(rng, c.shape[0])
    return nrm, e1, e2, _plane(c, nrm, e1, e2, np.tile(SQUARE, (c.shape[0], 1, 1)))


def _dgate(thres):
    def build(rng, c):
        n = c.shape[0]
        nrm, e1, e2, base = _square(rng, c)
        target = thres * (1.0 + np.resize(DELTAS7, n))
        lo, hi = np.zeros(n), np.full(n, 0.39)
        for _ in range(48):                                                        # bisection on the lift of the centre point, the rounded points refitted each time
            mid = 0.5 * (lo + hi)
            p = base.copy(); p[:, 4] += mid[:, None] * nrm
            p = _f32(p)
            nh, ni = _fit64(p)
            big = np.abs(np.einsum("nkj,nj->nk", p, nh) + ni[:, None]).max(1) > target
            hi = np.where(big, mid, hi); lo = np.where(big, lo, mid)
        p = base.copy(); p[:, 4] += np.where(np.resize(DELTAS7, n) > 0, hi, lo)[:, None] * nrm
        return dict(pts=p, q=_near(rng, c, nrm, e1, e2, lift=0.02), uniform_refl=True)
    return build


def chain_weight(pd64, q32):
    """the documented float chain (L/src/BackendFusion.cpp:1661-1662): float pd, float r2, sqrt(sqrt()) in float, the quotient in double, stored float"""
    q = np.asarray(q32, np.float32)
    pd = np.abs(np.asarray(pd64, np.float64).astype(np.float32))
    r2 = q[..., 0] * q[..., 0] + q[..., 1] * q[..., 1] + q[..., 2] * q[..., 2]
    with np.errstate(divide="ignore", invalid="ignore"):
        return (1.0 - 0.9 * pd.astype(np.float64) / np.sqrt(np.sqrt(r2)).astype(np.float64)).astype(np.float32)


def f32_neighbours(x):
    """the largest f32 below and the smallest f32 above a double that is not an f32 itself"""
    r = np.float32(x)
    assert float(r) != x
    return (np.nextafter(r, np.float32(-np.inf)), r) if float(r) > x else (r, np.nextafter(r, np.float32(np.inf)))


def _weight64(nh, ni, q_abs):
    """f64 weight of a query placed at q_abs (through the local frame and back, as the sides will see it)"""
    qm = to_map(E._to_local(q_abs)).astype(np.float64)
    pd = np.einsum("nj,nj->n", qm, nh) + ni
    return 1.0 - 0.9 * np.abs(pd) / np.sqrt(np.linalg.norm(qm, axis=1))


def _wgate_far(wmin):
    def build(rng, c):
        n = c.shape[0]
        nrm, e1, e2, base = _square(rng, c)
        nh, ni = _fit64(_f32(base))
        side = np.where(np.arange(n) % 2 == 0, 1.0, -1.0)
        delta = np.resize(np.r_[DELTAS7[:6], DELTAS7[7:13]], n)                    # (one f32 step of a query 700 m out moves the weight by 1e-6: d = 1e-7 has no meaning here)
        target = wmin + delta * (1.0 - wmin)
        jit = rng.uniform(-0.03, 0.03, (n, 1)) * e1
        lo, hi = np.zeros(n), np.full(n, 0.68)
        for _ in range(48):                                                        # the weight falls as the query leaves the plane
            mid = 0.5 * (lo + hi)
            low = _weight64(nh, ni, c + jit + (side * mid)[:, None] * nrm) < target
            hi = np.where(low, mid, hi); lo = np.where(low, lo, mid)
        return dict(pts=base, q=c + jit + (side * np.where(delta > 0, lo, hi))[:, None] * nrm, uniform_refl=True)
    return build


def _wgate_origin(wmin):
    """one cluster in the plane nrm . x = 0.25 over the origin; its own query near the plane, the others between the plane and the origin, where
    0.9 |pd| / |p|^(1/2) crosses 1 - wmin"""
    def build(rng, c):
        assert c.shape[0] == 1 and not c.any()
        nrm, e1, e2 = (v[0] for v in E._frame(rng, 1))
        base = 0.25 * nrm[None, :] + 0.8 * (SQUARE[:, 0:1] * e1[None, :] + SQUARE[:, 1:2] * e2[None, :])
        nh, ni = _fit64(_f32(base)[None])
        nb = f32_neighbours(wmin)
        def crossing(jit, target):                                                 # the weight rises with s between 0.03 and 0.21
            lo, hi = 0.03, 0.21
            for _ in range(60):
                mid = 0.5 * (lo + hi)
                lo, hi = (mid, hi) if _weight64(nh, ni, (jit + mid * nrm)[None])[0] < target else (lo, mid)
            return lo, hi
        xq, xkind = [], []
        for j in range(49):
            jit = rng.uniform(-0.02, 0.02) * e1 + rng.uniform(-0.02, 0.02) * e2
            if j < 9:
                for delta in DELTAS7:
                    lo, hi = crossing(jit, wmin + delta * (1.0 - wmin))
                    xq.append(jit + (hi if delta >= 0 else lo) * nrm); xkind.append("wgate")
            # walk the query through the threshold in steps below its own f32 spacing: those whose float weight IS one of the two f32 neighbours of the threshold
            cand = jit[None, :] + (crossing(jit, wmin)[1] + np.arange(-300, 301) * 2e-9)[:, None] * nrm[None, :]
            qm = to_map(E._to_local(cand))
            w = chain_weight(np.einsum("nj,j->n", qm.astype(np.float64), nh[0]) + ni[0], qm)
            for v in nb:
                hit = cand[np.nonzero(w == v)[0][:2]]
                xq.extend(hit); xkind += ["wulp"] * hit.shape[0]
        return dict(pts=base[None], q=(0.26 * nrm + 0.01 * e1)[None], xq=np.stack(xq), xcl=np.zeros(len(xq), np.int64), xkind=xkind, uniform_refl=True)
    return build


def _kgate(rng, c):
    n = c.shape[0]
    nrm, e1, e2, base = _square(rng, c)
    delta = np.resize(np.r_[10.0 ** -np.arange(1.0, 7.0), -(10.0 ** -np.arange(1.0, 7.0))], n)
    diag = (e1 + e2) / np.sqrt(2.0)
    return dict(pts=base, q=c + (np.sqrt(1.0 + delta) - 0.25 * np.sqrt(2.0))[:, None] * diag, uniform_refl=True)


def _dexact(z0, axis):
    """The one neighbourhood whose largest residual EQUALS a threshold in every correct implementation: the origin itself and four coincident points z0 along an
    axis, z0 a power of two, the query nearest to the origin (row 0).  Two columns are exactly zero; the Householder step on (0, z0, z0, z0, z0) is exact
    (beta = -2 z0, essential part 1 / 2, tau = 1, b -> 2), so n = -1 / z0, n^ = -axis, 1 / |n| = z0 and the residuals are z0, 0, 0, 0, 0 without a rounding;
    with the reflectivity differences (4, 1, 1, 1, 1) the livox weights are 1 / 32 and 1 / 8 and everything stays a power of two.  surf_dist_thres = z0 is handed
    to both sides: the loop's strict > accepts."""
    def build(rng, c):
        assert c.shape[0] == 1 and not c.any()
        pts = np.zeros((1, 5, 3)); pts[0, 1:, axis] = z0
        m = 12
        q = rng.uniform(-0.1, 0.1, (m, 3)) * z0
        q[:, axis] = rng.uniform(0.3, 0.45, m) * z0
        return dict(pts=pts, q=q[:1], xq=q[1:], xcl=np.zeros(m - 1, np.int64), xkind=["dexact"] * (m - 1), exact=True, mrefl=100.0 + np.array([[4, 1, 1, 1, 1]]), qrefl=np.array([100.0]))
    return build


REFL_DIFFS = {"refl_lo": ((3, 3, 3, 3, 2), (1, 2, 3, 4, 4), (10, 1, 1, 1, 1), (1, 1, 1, 1, 1)), "refl_eq": ((3, 3, 3, 3, 3), (1, 2, 3, 4, 5), (7, 2, 2, 2, 2), (4, 4, 4, 2, 1)),
              "refl_hi": ((3, 3, 3, 3, 4), (1, 2, 3, 4, 6), (12, 1, 1, 1, 1), (40, 50, 60, 70, 80)), "refl_span": ((11, 1, 1, 1, 1), (1, 1, 11, 1, 1), (1, 1, 1, 1, 11), (10, 1, 1, 1, 2)),
              "refl_zero1": ((0, 3, 3, 3, 3), (1, 2, 0, 4, 5), (1, 1, 1, 1, 0), (0, 1, 1, 1, 1)), "refl_zero5": ((0, 0, 0, 0, 0),), "refl_inf0": ((0, 3, 3, 3, 3), (2, 2, 0, 2, 2), (1, 1, 1, 1, 0)),
              "refl_wide": ((1, 1, 1, 2, 40), (32, 1, 1, 1, 1), (2, 3, 1, 1, 255), (5, 7, 100, 3, 2), (1, 255, 1, 1, 1), (255, 255, 255, 255, 255), (100, 100, 50, 49, 1), (60, 60, 60, 60, 61))}


def _refl(kind, geometry):
    def build(rng, c):
        out = geometry(rng, c)
        n = c.shape[0]
        diffs = np.array([rng.permutation(REFL_DIFFS[kind][k % len(REFL_DIFFS[kind])]) for k in range(n)], np.int64)
        qr = np.where(diffs.max(1) > 100, np.where(np.arange(n) % 2 == 0, 0, 255), rng.integers(100, 156, n))
        sign = np.where(qr[:, None] == 0, 1, np.where(qr[:, None] == 255, -1, rng.choice([-1, 1], (n, 5))))
        out.update(mrefl=(qr[:, None] + sign * diffs).astype(np.float64), qrefl=qr.astype(np.float64))
        assert out["mrefl"].min() >= 0 and out["mrefl"].max() <= 255
        return out
    return build


def _parts(case, offset, variant):
    """[(kind, node class, builder, clusters)] — node classes: any; x0 / y0 / z0: a node with that coordinate exactly 0; o: the node (0, 0, 0)"""
    T = thresholds(case, offset, variant)
    zero = ("z0",) if offset == "far" else ("x0", "y0", "z0")
    if case == "generic":
        return [("patch", "any", _patch, 200), ("tiny", "any", _tiny, 60), ("huge", "any", _huge, 60), ("strip", "any", _strip, 420), ("through0", "any", _through0, 160)]
    if case == "rank":
        return [("zerocol", z, _zerocol, 120 // len(zero)) for z in zero] + [("nearrank", z, _nearrank, 24 // len(zero)) for z in zero] + [("tilt0", "any", _tilt0, 90), ("colgen", "any", _from_edge(E._exact), 60),
                ("colaxis", "any", _from_edge(E._axis), 60), ("dup", "any", _from_edge(E._dup), 30), ("patch", "any", _patch, 120)]
    if case == "gates":
        w = [("wgate", "any", _wgate_far(T["surf_weight_min"]), 140)] if offset == "far" else [("wgate", "o", _wgate_origin(T["surf_weight_min"]), 1)]
        return w + [("dgate", "any", _dgate(T["surf_dist_thres"]), 252), ("kgate", "any", _kgate, 120), ("patch", "any", _patch, 60)]
    if case == "refl":
        return [(k, "any", _refl(k, _patch), 48) for k in ("refl_lo", "refl_eq", "refl_hi", "refl_span", "refl_zero1", "refl_zero5")] + \
               [("refl_inf0", z, _refl("refl_inf0", _zerocol), 48 // len(zero)) for z in zero] + [("patch", "any", _patch, 48)]
    if case == "reflwide":
        return [("refl_wide", "any", _refl("refl_wide", _patch), 160), ("patch", "any", _patch, 40)]
    if case == "dexact":
        return [("dexact", "o", _dexact(*DEXACT[variant]), 1), ("patch", "any", _patch, 60)]
    raise ValueError(case)


def _alloc(offset, parts, rng):
    """lattice nodes per part: the special classes first"""
    total = sum(p[3] for p in parts)
    side = max(int(np.ceil((1.25 * total) ** (1 / 3))) + 1, int(np.ceil(np.sqrt(sum(p[3] for p in parts if p[1] != "any")))) + 1)
    ijk = np.stack(np.meshgrid(np.arange(side), np.arange(side), np.arange(side), indexing="ij"), -1).reshape(-1, 3)
    ijk = ijk[rng.permutation(ijk.shape[0])]
    org = np.asarray(OFFSETS[offset])
    used = np.zeros(ijk.shape[0], bool)
    used |= (ijk == 0).all(1) & any(p[1] == "o" for p in parts)                  # reserved for the part that asks for it
    out = [None] * len(parts)
    under = iter(rng.permutation(side * side))                                     # `far`: nodes of the plane z = 0 under the lattice
    for i in sorted(range(len(parts)), key=lambda i: parts[i][1] == "any"):
        cls, n = parts[i][1], parts[i][3]
        if cls == "o":
            assert offset == "origin" and n == 1
            out[i] = np.zeros((1, 3))
            continue
        if cls == "z0" and offset == "far":
            ij = np.array([divmod(int(next(under)), side) for _ in range(n)])
            out[i] = np.c_[org[0] + PITCH * ij[:, 0], org[1] + PITCH * ij[:, 1], np.zeros(n)]
            continue
        assert cls == "any" or offset == "origin", (cls, offset)
        ok = ~used & ((ijk[:, "xyz".index(cls[0])] == 0) & (ijk.sum(1) > 0) if cls != "any" else True)
        pick = np.nonzero(ok)[0][:n]
        assert pick.size == n, (cls, n, pick.size)
        used[pick] = True
        out[i] = org + PITCH * ijk[pick].astype(np.float64)
    return out, side


SEEDS = {"generic": 1101, "rank": 1202, "gates": 1303, "refl": 1404, "reflwide": 1505, "dexact": 1606}


@functools.lru_cache(maxsize=None)
def build(case, offset, variant):
    """-> dict(map_xyz (5 nc, 3) f32, map_refl (5 nc,) f32, q_local (n, 3) f32, q_refl (n,) f32, q_map = to_map(q_local), kind (n,) str, cl (n,) cluster of the
    query, centre (nc, 3), exact (nc,) bool, n, nc, side).  The reflectivities are used by livox alone."""
    rng = np.random.default_rng(SEEDS[case] + (7 if offset == "far" else 0) + 100 * VARIANTS.index(variant))
    parts = _parts(case, offset, variant)
    centres, side = _alloc(offset, parts, rng)
    pts, q, kind, exact, mrefl, qrefl, xq, xcl, xkind = [], [], [], [], [], [], [], [], []
    at = 0
    for (k, _, builder, n), c in zip(parts, centres):
        b = builder(rng, c)
        p = b["pts"]
        assert p.shape == (n, 5, 3) and np.linalg.norm(p - c[:, None, :], axis=2).max() <= 0.4 + 1e-6, (k, np.linalg.norm(p - c[:, None, :], axis=2).max())
        qq = b.get("q")
        if qq is None:
            qq = p.mean(1) + np.clip(rng.normal(0, 0.015, (n, 3)), -0.028, 0.028)
        assert np.linalg.norm(qq - c, axis=1).max() <= 0.7, k
        pts.append(p); q.append(qq); kind += [k] * n; exact += [bool(b.get("exact", False))] * n
        d = np.full((n, 5), 2) if b.get("uniform_refl") else rng.integers(1, 4, (n, 5))
        mrefl.append(b["mrefl"] if "mrefl" in b else 100.0 + d * rng.choice([-1, 1], (n, 5)))
        qrefl.append(b["qrefl"] if "qrefl" in b else np.full(n, 100.0))
        if "xq" in b:
            xq.append(b["xq"]); xcl.append(at + b["xcl"]); xkind += b["xkind"]
        at += n
    nc = at
    assert nc <= 1500
    P64, centre = np.concatenate(pts), np.concatenate(centres)
    P32 = P64.astype(np.float32)
    exact = np.array(exact)
    assert np.array_equal(P32[exact].astype(np.float64), P64[exact])                                # what claims to be f32-exact is
    q_abs = np.concatenate(q + xq)
    cl = np.concatenate([np.arange(nc)] + xcl)
    q_local = E._to_local(q_abs)
    mr, qr = np.concatenate(mrefl).astype(np.float32), np.concatenate(qrefl).astype(np.float32)
    out = dict(map_xyz=np.ascontiguousarray(P32.reshape(-1, 3)), map_refl=np.ascontiguousarray(mr.reshape(-1)), q_local=q_local, q_refl=np.ascontiguousarray(qr[cl]),
               q_map=to_map(q_local), kind=np.array(kind + xkind), cl=cl, centre=centre, exact=exact, n=cl.size, nc=nc, side=side, offset=offset)
    assert out["n"] <= 1500
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


def clouds(s, variant):
    """(map, queries) as handed to the device: x y z, and the reflectivity as the auxiliary column for livox"""
    if variant != "livox":
        return s["map_xyz"], s["q_local"]
    return np.ascontiguousarray(np.c_[s["map_xyz"], s["map_refl"]], np.float32), np.ascontiguousarray(np.c_[s["q_local"], s["q_refl"]], np.float32)


@functools.lru_cache(maxsize=None)
def short_map(variant):
    """four map points: fewer than five neighbours, every query is refused"""
    rng = np.random.default_rng(5)
    mp = np.c_[rng.normal(0, 0.1, (4, 3)), 100 + rng.integers(1, 4, 4)].astype(np.float32)
    ql = np.c_[E._to_local(rng.normal(0, 0.05, (50, 3))), np.full(50, 100.0)].astype(np.float32)
    cols = 4 if variant == "livox" else 3
    return dict(map=np.ascontiguousarray(mp[:, :cols]), q=np.ascontiguousarray(ql[:, :cols]), n=50)


@functools.lru_cache(maxsize=None)
def dense_filler(case, offset, variant):
    """The filler of edge_fit_cases.dense_filler for this scene: 40 points within 0.15 m of the centre of every lattice cell, 3.46 m from the nearest nodes,
    appended BEHIND the clusters; (m, 3), or (m, 4) with a reflectivity column for livox."""
    s = build(case, offset, variant)
    side = s["side"]
    ijk = np.stack(np.meshgrid(np.arange(side - 1), np.arange(side - 1), np.arange(side - 1), indexing="ij"), -1).reshape(-1, 3)
    rng = np.random.default_rng(11)
    c = np.asarray(OFFSETS[offset]) + PITCH * (ijk.astype(np.float64) + 0.5)
    f = (c[:, None, :] + rng.uniform(-0.15, 0.15, (c.shape[0], 40, 3))).reshape(-1, 3).astype(np.float32)
    d = np.linalg.norm(f.astype(np.float64)[:, None, :] - s["q_map"].astype(np.float64)[None, ::7, :], axis=2).min()
    assert d > 2.5
    if variant == "livox":
        f = np.ascontiguousarray(np.c_[f, rng.integers(0, 256, f.shape[0])], np.float32)
    f.setflags(write=False)
    return f


# ------------------------------------------------------------------------------------------------
# the model
# ------------------------------------------------------------------------------------------------
def _ints(vals):
    """python floats -> (integers, D): v = integer / D exactly, D a power of two"""
    rats = [float(v).as_integer_ratio() for v in vals]
    D = max(d for _, d in rats)
    return [a * (D // d) for a, d in rats], D


def _cramer(M, r):
    """M x = r for an integer k x k system, k <= 3: (adj(M) r, det M)"""
    k = len(r)
    if k == 1:
        return [r[0]], M[0][0]
    if k == 2:
        return [r[0] * M[1][1] - M[0][1] * r[1], M[0][0] * r[1] - M[1][0] * r[0]], M[0][0] * M[1][1] - M[0][1] * M[1][0]
    det3 = lambda a, b, c: (a[0] * (b[1] * c[2] - b[2] * c[1]) - b[0] * (a[1] * c[2] - a[2] * c[1]) + c[0] * (a[1] * b[2] - a[2] * b[1]))   # noqa: E731  (columns a, b, c)
    col = [[M[i][j] for i in range(3)] for j in range(3)]
    return [det3(r, col[1], col[2]), det3(col[0], r, col[2]), det3(col[0], col[1], r)], det3(*col)


def _ratio(num, den):
    return float(Fraction(num, den))


def _sroot(num, den2, sign=1):
    """sign * |num| / sqrt(den2) for integers, one rounding in the quotient and one in the root"""
    v = math.sqrt(_ratio(num * num, den2))
    return v if (num >= 0) == (sign >= 0) else -v


def _exact_one(p, w, q):
    """p (5, 3), q (3,) f32 values, w (5,) f64 weights -> the exact minimiser of sum w_k^2 (p_k . x + 1)^2 on the non-zero columns, or None if singular"""
    P, Dp = _ints(p.reshape(-1))
    P = [P[3 * k:3 * k + 3] for k in range(5)]
    V, _ = _ints(w)
    V2 = [v * v for v in V]
    cols = [j for j in range(3) if any(P[k][j] != 0 for k in range(5))]
    out = dict(zero_cols=3 - len(cols), rho=0.0)
    if not cols:
        return out, None
    M = [[sum(V2[k] * P[k][i] * P[k][j] for k in range(5)) for j in cols] for i in cols]
    r = [-sum(V2[k] * P[k][i] for k in range(5)) for i in cols]
    a, det = _cramer(M, r)
    if len(cols) == 3:
        sv2, tr, r2 = sum(V2), M[0][0] + M[1][1] + M[2][2], sum(x * x for x in r)
        den = (tr * sv2 - r2) ** 2 * tr                                            # tr S = (tr sum V2 - |r|^2) / sum V2 in the common scale
        out["rho"] = _ratio(det * sv2 * sv2, den) if den else float("nan")
    a2 = sum(x * x for x in a)
    if det == 0 or a2 == 0:
        return out, None
    sgn = 1 if det > 0 else -1
    x = np.zeros(3); nhat = np.zeros(3)
    for i, j in enumerate(cols):
        x[j] = _ratio(Dp * a[i], det)
        nhat[j] = _sroot(a[i], a2, sgn)
    res = [_sroot(sum(a[i] * P[k][j] for i, j in enumerate(cols)) + det, Dp * Dp * a2, sgn) for k in range(5)]
    Q, Dq = _ints(q)
    pd = _sroot(Dp * sum(a[i] * Q[j] for i, j in enumerate(cols)) + det * Dq, Dq * Dq * Dp * Dp * a2, sgn)
    return out, dict(x=x, nhat=nhat, ninv=math.sqrt(_ratio(det * det, Dp * Dp * a2)), res=res, pd=pd)


def weights(map_refl, q_refl, idx, variant):
    """(w (n, 5) f64, sum_w (n,), has a zero difference (n,)) — livox: (1 / |D|) / sum |D|, the difference taken in float; otherwise ones"""
    n = idx.shape[0]
    if variant != "livox":
        return np.ones((n, 5)), np.zeros(n), np.zeros(n, bool)
    ad = np.abs(np.asarray(q_refl, np.float32)[:, None] - np.asarray(map_refl, np.float32)[idx]).astype(np.float64)
    sw = ad[:, 0]
    for k in range(1, 5):
        sw = sw + ad[:, k]
    with np.errstate(divide="ignore", invalid="ignore"):
        return (1.0 / ad) / sw[:, None], sw, (ad == 0).any(1)


def centred_f64(p, w):
    """the centred normal equations in plain numpy f64 without fma, for measuring K_c alone: n = -W adj(S) c / (det S + W c^T adj(S) c); p (n, 5, 3), w (n, 5)"""
    w2 = w * w
    W = w2.sum(1)
    c = (w2[:, :, None] * p).sum(1) / W[:, None]
    e = p - c[:, None, :]
    S = np.einsum("nk,nki,nkj->nij", w2, e, e)
    adj = np.stack([np.cross(S[:, 1], S[:, 2]), np.cross(S[:, 2], S[:, 0]), np.cross(S[:, 0], S[:, 1])], 1)          # rows of adj(S), S symmetric
    u = np.einsum("nij,nj->ni", adj, c)
    det = np.einsum("ni,ni->n", S[:, 0], adj[:, 0])
    denom = det + W * np.einsum("ni,ni->n", c, u)
    return -(W / denom)[:, None] * u


@functools.lru_cache(maxsize=None)
def _core(case, offset, variant):
    """the exact fits of a scene on each query's own cluster rows in the ORDER of the f32 distances (ties by index), shared by every mode"""
    s = build(case, offset, variant)
    T = thresholds(case, offset, variant)
    n = s["n"]
    own = 5 * s["cl"][:, None] + np.arange(5)[None, :]
    d2 = d2_f32(s["q_map"], s["map_xyz"][own])
    order = np.stack([np.lexsort((own[i], d2[i])) for i in range(n)])
    idx = np.take_along_axis(own, order, 1).astype(np.int32)
    d2 = np.take_along_axis(d2, order, 1)
    w, sum_w, zero_diff = weights(s["map_refl"], s["q_refl"], idx, variant)
    p32 = s["map_xyz"][idx]
    p = p32.astype(np.float64)
    c = dict(idx=idx, d2=d2, w=w, sum_w=sum_w, zero_diff=zero_diff, x=np.zeros((n, 3)), nhat=np.full((n, 3), np.nan), ninv=np.full(n, np.nan), res=np.full((n, 5), np.nan),
             pd=np.full(n, np.nan), rho=np.zeros(n), zero_cols=np.zeros(n, np.int64), solved=np.zeros(n, bool), cond=np.full(n, np.inf), sig_ratio=np.zeros(n), theta=np.zeros(n))
    for i in range(n):
        if zero_diff[i]:
            continue
        head, sol = _exact_one(p[i], w[i], s["q_map"][i].astype(np.float64))
        c["rho"][i], c["zero_cols"][i] = head["rho"], head["zero_cols"]
        keep = [j for j in range(3) if (p[i][:, j] != 0).any()]
        if keep:
            sv = np.linalg.svd(w[i][:, None] * p[i][:, keep], compute_uv=False)
            c["sig_ratio"][i] = sv[-1] / sv[0] if sv[0] > 0 else 0.0
            c["cond"][i] = sv[0] / sv[-1] if sv[-1] > 0 else np.inf
        if sol is not None:
            c["solved"][i] = True
            c["x"][i], c["nhat"][i], c["ninv"][i], c["res"][i], c["pd"][i] = sol["x"], sol["nhat"], sol["ninv"], sol["res"], sol["pd"]
            c["theta"][i] = np.linalg.norm(w[i] * c["res"][i]) / sv[0]            # ||r_w|| / (sigma_1 ||x||): r_w = w (p . x + 1) = w res / (1 / |n|), ||x|| = |n|
    full = c["solved"] & (c["zero_cols"] == 0) & (c["sig_ratio"] > RANK_FULL)
    deficient = c["solved"] & (c["zero_cols"] > 0) & (c["sig_ratio"] > RANK_FULL)
    c.update(rank_full=full, rank_deficient=deficient, rank_decided=full | deficient, T=T)
    for v in c.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return c


MODES = {"default": 0, "qr": 16384, "fast": 2048}        # LILI_DEBUG of the run the bound is for


def solution_bound(c, mode="default"):
    """B per query (relative error of x that a correct implementation may show), 1 x the measured constants"""
    k_c = K_C
    with np.errstate(invalid="ignore", over="ignore"):
        B = np.minimum(K_QR * EPS * c["cond"], K_LS * EPS * c["cond"] * (1.0 + c["cond"] * c["theta"]))
    rho = c["rho"]
    with np.errstate(divide="ignore", invalid="ignore"):
        fast = (rho >= 0.99 * RHO_SWITCH) if mode == "default" else (rho > 0) if mode == "fast" else np.zeros(rho.shape, bool)
        B = np.where(fast & (c["zero_cols"] == 0), np.maximum(B, k_c * EPS / rho), B)
    return np.where(c["rank_decided"], B, np.inf)


@functools.lru_cache(maxsize=None)
def model(case, offset, variant, mode="default"):
    s, c = build(case, offset, variant), _core(case, offset, variant)
    T = c["T"]
    n = s["n"]
    B = solution_bound(c, mode)
    Bd = DEVICE_FACTOR * B
    qm = s["q_map"].astype(np.float64)
    qn = np.linalg.norm(qm, axis=1)
    in_radius = c["d2"][:, 4].astype(np.float64) < T["kd_max_radius"]
    refl_ok = ~(c["sum_w"] > T["reflect_thres"]) if variant == "livox" else np.ones(n, bool)
    nan_drop = c["zero_diff"]
    with np.errstate(invalid="ignore", divide="ignore"):
        w_chain = chain_weight(c["pd"], s["q_map"])
        w_exact = 1.0 - 0.9 * np.abs(c["pd"]) / np.sqrt(qn)
        rmax = np.abs(c["res"]).max(1)
        mnorm = np.linalg.norm(s["map_xyz"][c["idx"]].astype(np.float64), axis=2).max(1)
        md = (2.0 * Bd + 8.0 * EPS) * (mnorm + c["ninv"])
        mw = 4.0 * U32 + 0.9 * (2.0 * Bd + 8.0 * EPS) * (qn + c["ninv"]) / np.sqrt(qn)
        plane_ok, weight_ok = ~(rmax > T["surf_dist_thres"]), w_chain.astype(np.float64) > T["surf_weight_min"]
        d_pass, d_refuse = rmax < T["surf_dist_thres"] - md, rmax > T["surf_dist_thres"] + md
        w_pass, w_refuse = w_exact > T["surf_weight_min"] + mw, w_exact < T["surf_weight_min"] - mw
    reach = in_radius & refl_ok & ~nan_drop                                        # the queries that reach the solver with finite weights
    fit_decided = c["rank_decided"] & (d_refuse | w_refuse | (d_pass & w_pass))
    decided = ~reach | fit_decided
    valid = reach & c["solved"] & plane_ok & weight_ok
    und_d, und_w = reach & c["rank_decided"] & ~d_pass & ~d_refuse & ~w_refuse, reach & c["rank_decided"] & d_pass & ~w_pass & ~w_refuse
    wn = w_chain.astype(np.float64)
    m = dict(c, B=B, Bd=Bd, in_radius=in_radius, refl_ok=refl_ok, nan_drop=nan_drop, reach=reach, w_chain=w_chain, w_exact=w_exact, rmax=rmax, md=md, mw=mw,
             plane_ok=plane_ok, weight_ok=weight_ok, valid=valid, decided=decided, und_rank=reach & ~c["rank_decided"], und_d=und_d, und_w=und_w,
             meaningful=c["rank_decided"] & (B <= B_MEANINGLESS), rec_n=wn[:, None] * c["nhat"], rec_d=wn * c["ninv"], fast=(c["rho"] >= RHO_SWITCH) & (c["zero_cols"] == 0))
    for v in m.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return m


def ulp32(x, y):
    """the f32 spacing at the larger magnitude, floor 1e-15 (tests/edge_fit_cases.py)"""
    return np.maximum(np.spacing(np.maximum(np.abs(np.asarray(x, np.float32)), np.abs(np.asarray(y, np.float32)))).astype(np.float64), 1e-15)


def record_excess(rec_n, rec_d, m, sel, factor):
    """err / allowance of the records rec_n (n, 3), rec_d (n,) against the model on the queries sel, the allowance one f32 ulp + factor B w per component
    (and factor B w / |n| for d; 2^-23 + factor B relative for rec.d / ||rec.n|| against 1 / |n|): (worst ratio, its query, ratios (n,))"""
    B = factor * m["B"]
    wn = np.abs(m["w_chain"].astype(np.float64))
    with np.errstate(invalid="ignore", divide="ignore"):
        en = np.abs(rec_n.astype(np.float64) - m["rec_n"]) / (ulp32(rec_n, m["rec_n"]) + (B * wn)[:, None])
        ed = np.abs(rec_d.astype(np.float64) - m["rec_d"]) / (ulp32(rec_d, m["rec_d"]) + B * wn * m["ninv"])
        ratio = rec_d.astype(np.float64) / np.linalg.norm(rec_n.astype(np.float64), axis=1)
        er = np.abs(ratio / m["ninv"] - 1.0) / (2.0 ** -23 + B)
    worst = np.where(sel, np.maximum(np.maximum(en.max(1), ed), er), 0.0)
    worst = np.where(np.isnan(worst), np.inf, worst)
    i = int(np.argmax(worst)) if worst.size else -1
    return (float(worst[i]) if worst.size else 0.0), i, worst


def oracle_excess(rec_n, rec_d, o_n, o_d, m, sel, factor):
    """the same against the oracle's records: two f32 roundings, and (1 + factor) B between two implementations that each keep their own bound"""
    B = (1.0 + factor) * m["B"]
    wn = np.abs(m["w_chain"].astype(np.float64))
    with np.errstate(invalid="ignore", divide="ignore"):
        en = np.abs(rec_n.astype(np.float64) - o_n.astype(np.float64)) / (ulp32(rec_n, o_n) + (B * wn)[:, None])
        ed = np.abs(rec_d.astype(np.float64) - o_d.astype(np.float64)) / (ulp32(rec_d, o_d) + B * wn * m["ninv"])
    worst = np.where(sel, np.maximum(en.max(1), ed), 0.0)
    worst = np.where(np.isnan(worst), np.inf, worst)
    i = int(np.argmax(worst)) if worst.size else -1
    return (float(worst[i]) if worst.size else 0.0), i, worst


@functools.lru_cache(maxsize=None)
def reference(case, offset, variant):
    """(scene, oracle records over ALL queries) — computed once per session and shared, never written to"""
    from oracle import oracle as O
    s = build(case, offset, variant)
    tree = O.KdTree(s["map_xyz"])
    livox = variant == "livox"
    rec = O.associate_surf(tree, s["map_refl"] if livox else None, s["q_local"], s["q_refl"] if livox else None, Q_ASSOC, T_ASSOC, O.params(variant, **overrides(case, offset, variant)))
    for v in rec.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return s, rec


@functools.lru_cache(maxsize=None)
def measure_constants():
    """(K, K_c) over every case, offset and variant: the oracle's lstsq53 and centred_f64 against the exact solution"""
    from oracle import oracle as O
    k_qr = k_ls = k_c = 0.0
    for case, offset, variant in GRID:
        s, c = build(case, offset, variant), _core(case, offset, variant)
        p = s["map_xyz"][c["idx"]].astype(np.float64)
        sel = np.nonzero(c["rank_decided"])[0]
        xn = np.linalg.norm(c["x"], axis=1)
        for i in sel:
            x = O.lstsq53(c["w"][i][:, None] * p[i], -c["w"][i])
            err = np.linalg.norm(x - c["x"][i]) / (xn[i] * EPS * c["cond"][i])
            k_qr, k_ls = max(k_qr, err), max(k_ls, err / (1.0 + c["cond"][i] * c["theta"][i]))
        f = np.nonzero(c["rank_full"] & (c["rho"] > 0))[0]
        with np.errstate(all="ignore"):
            xc = centred_f64(p[f], c["w"][f])
            err = np.linalg.norm(xc - c["x"][f], axis=1) / xn[f]
        err = np.where(np.isfinite(err), np.minimum(err, 1.0), 1.0)              # (an error of 100 % is as wrong as a direction gets)
        k_c = max(k_c, float((err * c["rho"][f] / EPS).max()) if f.size else 0.0)
    return float(k_qr), float(k_ls), float(k_c)


def summary(case, offset, variant, mode="default"):
    """the counts both tests print"""
    s, m = build(case, offset, variant), model(case, offset, variant, mode)
    by = lambda sel: {k: int((sel & (s["kind"] == k)).sum()) for k in sorted(set(s["kind"][sel].tolist()))}   # noqa: E731
    byc = ~np.isin(s["kind"], UNDECIDED_BY_CONSTRUCTION)
    return dict(n=s["n"], clusters=s["nc"], accepted=int((m["decided"] & m["valid"]).sum()), refused=int((m["decided"] & ~m["valid"]).sum()), undecided=int((~m["decided"]).sum()),
                undecided_outside_the_declared_kinds=int((~m["decided"] & byc).sum()), und_rank=by(m["und_rank"]), und_dist=by(m["und_d"]), und_weight=by(m["und_w"]),
                fast_path=int((m["reach"] & m["fast"]).sum()), qr=int((m["reach"] & ~m["fast"]).sum()), meaningless=int((m["reach"] & m["rank_decided"] & ~m["meaningful"]).sum()))
