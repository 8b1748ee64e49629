"""The referee of the global pose graph (tests/pose_graph_model.py) checked against itself and against the library's host functions; no GPU.
  Jacobians    every block of every factor kind against central differences, both sides of the small-angle threshold of Jr^-1 and at a residual rotation of 2 rad;
  solvers      the dense (or natural-order) and the sparse linear solver give the same Gauss-Newton sequence; their largest pose difference per case is D0(case),
               the yardstick of tests/test_pose_graph_gpu.py, printed;
  decisions    every stop decision of every solve case is a factor 10 clear of its threshold, every accepted cost is lower by more than rounding;
  endings      convergence within 10 iterations, apart from the cases built to end otherwise;
  host         lili_loop_measurement and lili_correct_poses against the model's restatements bit for bit, and their refusals;
  layout       lili_pg_options / lili_pg_summary against the header compiled as C."""
import ctypes as C
import os
import subprocess
import time

import numpy as np
import pytest

import lili_om_amd as L
from lili_om_amd import api
from tests import pose_graph_cases as Cs
from tests import pose_graph_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOLVES = Cs.solve_cases()
IDS = [c["name"] for c in SOLVES]


def _numeric(A, B, Z, h=1e-6):
    Ja, Jb = np.zeros((6, 6)), np.zeros((6, 6))
    for k in range(6):
        d = np.zeros(6)
        d[k] = h
        Ja[:, k] = (M.factor_error(M.retract(A, d), B, Z)[0] - M.factor_error(M.retract(A, -d), B, Z)[0]) / (2 * h)
        Jb[:, k] = (M.factor_error(A, M.retract(B, d), Z)[0] - M.factor_error(A, M.retract(B, -d), Z)[0]) / (2 * h)
    return Ja, Jb


@pytest.mark.parametrize("angle", [0.0, 1e-6, 1e-3, 0.0999, 0.1001, 0.5, 2.0, 3.0])
def test_jacobian_blocks_match_central_differences(angle):
    """between-factor (chain and loop are the same factor) and prior (A = the identity, the second node's block), residual rotation `angle`.  Central differences
    with h = 1e-6 carry h^2 |e'''| + eps / h ~ 1e-9 of the entries' size (tens of metres in the [d]x block)."""
    rng = np.random.default_rng(int(angle * 1e6) + 1)
    for trial in range(6):
        A = M.retract(M.IDENTITY, np.concatenate([rng.normal(0, 1.0, 3), rng.normal(0, 10.0, 3)]))
        B = M.retract(A, np.concatenate([rng.normal(0, 1.0, 3), rng.normal(0, 10.0, 3)]))
        axis = rng.normal(size=3)
        axis /= np.linalg.norm(axis)
        for prior in (False, True):
            Ax = M.IDENTITY if prior else A
            Z = M.retract(M.between(Ax, B), np.concatenate([axis * angle, rng.normal(0, 0.3, 3)]))
            e, Ja, Jb = M.factor_jacobians(Ax, B, Z)
            assert abs(np.linalg.norm(e[0:3]) - angle) <= 1e-9
            na, nb = _numeric(Ax, B, Z)
            scale = max(1.0, np.abs(na).max(), np.abs(nb).max())
            assert np.abs(Jb - nb).max() <= 1e-7 * scale
            if not prior:
                assert np.abs(Ja - na).max() <= 1e-7 * scale
            # the blocks the issue lists as zero
            assert not Ja[0:3, 3:6].any() and not Jb[0:3, 3:6].any() and not Jb[3:6, 0:3].any()


def test_jr_inverse_series_meets_the_closed_form_at_the_threshold():
    t = M.SMALL_ANGLE
    lo, hi = M.jr_inv_coefficient(np.array([(t * (1 - 1e-12)) ** 2])), M.jr_inv_coefficient(np.array([(t * (1 + 1e-12)) ** 2]))
    assert abs(lo[0] - hi[0]) <= 1e-13 * hi[0]
    assert abs(M.jr_inv_coefficient(np.array([0.0]))[0] - 1.0 / 12.0) == 0.0


def test_vectorised_evaluate_is_the_jacobian_assembly():
    c = next(c for c in SOLVES if c["name"] == "crossing_and_nested")
    g = Cs.build_model(c)
    cost, grad, D, S, LB = g.evaluate()
    r, J = g.jacobian(g.X)
    H = (J.T @ J).toarray()
    n = g.n
    assert abs(cost - 0.5 * r @ r) <= 1e-14 * cost
    assert np.abs(grad.ravel() - J.T @ r).max() <= 1e-12 * np.abs(grad).max()
    Hb = H.reshape(n, 6, n, 6).transpose(0, 2, 1, 3)
    rest = Hb.copy()
    for i in range(n):
        assert np.abs(Hb[i, i] - D[i]).max() <= 1e-12 * np.abs(D[i]).max()
        rest[i, i] = 0
    for i in range(n - 1):
        rest[i + 1, i] -= S[i]
        rest[i, i + 1] -= S[i].T
    for l, (a, b, _, _) in enumerate(g.loops):
        rest[a, b] -= LB[l]
        rest[b, a] -= LB[l].T
    assert np.abs(rest).max() <= 1e-12 * np.abs(H).max()


def test_evaluate_at_the_cap_is_fast():
    c = Cs.full_size()
    g = Cs.build_model(c)
    g.evaluate()
    t = time.perf_counter()
    g.evaluate()
    dt = time.perf_counter() - t
    print(f"vectorised evaluate at N = {g.n}: {dt:.3f} s")
    assert dt < 1.0


@pytest.mark.parametrize("c", SOLVES, ids=IDS)
def test_solvers_agree_and_decisions_are_clear(c):
    g, X, s, d0 = Cs.reference(c)
    print(f"D0 [{c['name']}] N {g.n} loops {len(g.loops)}: position {d0[0]:.2e} m, angle {d0[1]:.2e} rad; iterations {s['iterations']} termination {s['termination']} "
          f"cost {s['initial_cost']:.6e} -> {s['final_cost']:.6e}")
    assert d0[0] <= 1e-9 and d0[1] <= 1e-9
    if c["expect"] is None:
        assert s["termination"] in M.CONVERGED and s["iterations"] <= 10
    else:
        assert s["termination"] == c["expect"]
    # v = the candidate's cost, thr = the cost before it: an accept decision stands 1e-12 of the cost clear of rounding (a sum of F terms carries ~1e-14)
    assert Cs.decisions_clear(s), s["margins"]


def test_incremental_script_is_clear_too():
    g, out = Cs.run_script_on_model(Cs.incremental_script())
    assert len(out) == 2 and g.n == 300 and len(g.loops) == 2
    for X, s in out:
        assert s["termination"] in M.CONVERGED and s["iterations"] >= 2 and Cs.decisions_clear(s), s["margins"]


def test_cost_increase_case_keeps_the_estimate():
    c = next(c for c in SOLVES if c["name"] == "cost_increases")
    g, X, s, _ = Cs.reference(c)
    assert s["iterations"] == 1 and X.tobytes() == g.X.tobytes() and s["final_cost"] == s["initial_cost"] and s["cost"][0] > 5.0 * s["initial_cost"]


def test_full_size_generator_converges_in_the_model():
    c = Cs.full_size(4096)
    g = Cs.build_model(c)
    X, s = M.gauss_newton(g, **c["options"])
    g0, g1 = np.abs(g.evaluate()[1]).max(), np.abs(g.evaluate(X)[1]).max()
    print(f"full-size generator at N = 4096: iterations {s['iterations']} termination {s['termination']} |g|inf {g0:.2e} -> {g1:.2e} ({g1 / g0:.1e})")
    assert s["termination"] in M.CONVERGED and g1 <= 1e-7 * g0
    costs = [s["initial_cost"]] + s["cost"]
    assert all(b <= a for a, b in zip(costs, costs[1:]))


# ---------------------------------------------------------------- host functions of the library
def _pose(rng, spread=20.0):
    q = rng.normal(size=4)
    return np.concatenate([rng.uniform(-spread, spread, 3), q / np.linalg.norm(q)])


def test_loop_measurement_matches_the_restatement_bit_for_bit():
    rng = np.random.default_rng(5)
    for trial in range(40):
        ang = [0.01, 0.5, 3.1][trial % 3]      # the last one reaches Eigen's matrix-to-quaternion branches with a negative trace
        axis = rng.normal(size=3)
        axis /= np.linalg.norm(axis)
        T = np.eye(4)
        T[:3, :3] = M.qmat(M.qexp(axis * ang))
        T[:3, 3] = rng.normal(0, 0.5, 3)
        T = T.astype(np.float32).astype(np.float64)      # icp.getFinalTransformation().cast<double>()
        a, b = _pose(rng), _pose(rng)
        m = L.loop_measurement(T, a, b)
        assert m.tobytes() == M.loop_measurement(T, a, b).tobytes()
        # and it is between(T o a, b), as far as a float transform is a rigid one (orthonormal to 6e-8; the text rotates with the quaternion as Eigen extracts it)
        q_inc = M.qnormalize(np.array(M._from_matrix(T[:3, :3].tolist())))
        cor = np.concatenate([M.qrot(q_inc, a[0:3]) + T[:3, 3], M.qnormalize(M.qmul(q_inc, a[3:7]))])
        ref = M.between(cor, b)
        assert np.abs(m[0:3] - ref[0:3]).max() <= 1e-6 * 40 and min(np.abs(m[3:7] - ref[3:7]).max(), np.abs(m[3:7] + ref[3:7]).max()) <= 1e-6


def test_loop_measurement_refusals():
    lib = L.load_library()
    T, a, b = np.eye(4).ravel().copy(), np.array([1.0, 2, 3, 1, 0, 0, 0]), np.array([0.0, 0, 0, 1, 0, 0, 0])
    out = np.full(7, 7.5)
    ptr = api._ptr
    assert lib.lili_loop_measurement(None, ptr(a), ptr(b), ptr(out)) == -1 and lib.lili_loop_measurement(ptr(T), ptr(a), ptr(b), None) == -1
    bad = a.copy()
    bad[2] = np.nan
    assert lib.lili_loop_measurement(ptr(T), ptr(bad), ptr(b), ptr(out)) == -1
    zero = b.copy()
    zero[3:7] = 0
    assert lib.lili_loop_measurement(ptr(T), ptr(a), ptr(zero), ptr(out)) == -1
    assert (out == 7.5).all()
    assert lib.lili_loop_measurement(ptr(T), ptr(a), ptr(b), ptr(out)) == 0


def _window_problem(rng, n_kf, width, per_kf=3):
    """a trajectory of n_kf keyframes with per_kf - 1 frames between them; abs_poses has n_kf + 1 rows (row 0: the initial pose), as in the reference"""
    n_frames = (n_kf - 1) * per_kf + 1
    ids = np.arange(n_kf, dtype=np.int32) * per_kf
    sol = np.array([_pose(rng) for _ in range(n_frames)])
    kf = np.array([_pose(rng) for _ in range(n_kf)])
    ab = np.ascontiguousarray(np.array([_pose(rng) for _ in range(n_kf + 1)])[:, [3, 4, 5, 6, 0, 1, 2]])
    return sol, ids, ab, kf


@pytest.mark.parametrize("width", [2, 3])
@pytest.mark.parametrize("f32", [False, True])
def test_correct_poses_matches_the_restatement_bit_for_bit(width, f32):
    """width 2: the window's tail is one keyframe"""
    rng = np.random.default_rng(10 * width + f32)
    for n_kf in (width, width + 1, 9):
        sol, ids, ab, kf = _window_problem(rng, n_kf, width)
        got = L.correct_poses(sol, ids, width, ab, kf, f32_positions=f32)
        ref = M.correct_poses(sol, ids, width, ab, kf, f32_positions=f32)
        for k in ref:
            assert got[k].tobytes() == ref[k].tobytes(), (n_kf, k)
        # what the text does: keyframes outside the tail sit on their solved frames, the tail keeps its relative transforms
        for i in range(n_kf - width + 1):
            assert (got["keyframe_poses"][i, 3:7] == sol[ids[i], 3:7]).all()
            assert (got["abs_poses"][i + 1, 0:4] == sol[ids[i], 3:7]).all()
        for i in range(n_kf + 1 - width, n_kf):
            old = M.between(ab[i][[4, 5, 6, 0, 1, 2, 3]], ab[i + 1][[4, 5, 6, 0, 1, 2, 3]])
            new = M.between(got["abs_poses"][i][[4, 5, 6, 0, 1, 2, 3]], got["abs_poses"][i + 1][[4, 5, 6, 0, 1, 2, 3]])
            assert np.abs(old - new).max() <= 1e-9
        assert (got["last_pose"] == got["abs_poses"][n_kf + 1 - width]).all()
        if f32:
            assert (got["frame_poses"][:, 0:3] == sol[:, 0:3].astype(np.float32).astype(np.float64)).all()


def test_correct_poses_refusals():
    lib = L.load_library()
    rng = np.random.default_rng(3)
    sol, ids, ab, kf = _window_problem(rng, 6, 3)
    ptr = api._ptr

    def call(sol=sol, ids=ids, width=3, ab=ab, kf=kf, n_abs=None, n_kf=None, null=None):
        a, k = ab.copy(), kf.copy()
        frames, last, sel = np.full_like(sol, 7.5), np.full(7, 7.5), np.full(3, 7.5)
        args = [ptr(sol), sol.shape[0], ptr(ids), ids.shape[0] if n_kf is None else n_kf, width, 0, ptr(a), a.shape[0] if n_abs is None else n_abs, ptr(frames), ptr(k), ptr(last), ptr(sel)]
        if null is not None:
            args[null] = None
        rc = lib.lili_correct_poses(*args)
        untouched = a.tobytes() == ab.tobytes() and k.tobytes() == kf.tobytes() and (frames == 7.5).all() and (last == 7.5).all() and (sel == 7.5).all()
        return rc, untouched

    assert call() == (0, False)
    for null in (0, 2, 6, 8, 9, 10, 11):
        assert call(null=null) == (-1, True)
    assert call(width=1) == (-1, True) and call(width=7) == (-1, True)
    assert call(n_abs=4) == (-1, True)           # n_keyframes - width + 2 > n_abs: abs_poses[i + 1] would leave the array
    assert call(n_kf=4) == (-1, True)            # n_abs > n_keyframes + 1: the tail would leave the keyframe arrays
    bad_ids = ids.copy()
    bad_ids[1] = sol.shape[0]
    assert call(ids=bad_ids) == (-1, True)
    bad = sol.copy()
    bad[4, 5] = np.inf
    assert call(sol=bad) == (-1, True)


def test_struct_mirrors_match_the_header(tmp_path):
    """size and the offset of every field of lili_pg_options / lili_pg_summary against the C header compiled as plain C, and the constants"""
    pairs = [("lili_pg_options", api.PgOptions), ("lili_pg_summary", api.PgSummary)]
    lines, expect = [], []
    for cname, T in pairs:
        lines.append(f'printf("%zu\\n", sizeof({cname}));')
        expect.append(C.sizeof(T))
        for fname, _ in T._fields_:
            lines.append(f'printf("%zu\\n", offsetof({cname}, {fname}));')
            expect.append(getattr(T, fname).offset)
    lines.append('printf("%d\\n%d\\n%d\\n%d\\n%d\\n", LILI_PG_MAX_NODES, LILI_PG_MAX_LOOPS, LILI_PG_SEGMENT, LILI_PG_MAX_LOG, LILI_PG_COST_INCREASED);')
    expect += [api.PG_MAX_NODES, api.PG_MAX_LOOPS, api.PG_SEGMENT, api.PG_MAX_LOG, api.PG_COST_INCREASED]
    src = tmp_path / "lay_pg.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "lili_hip.h"\nint main(void){' + "".join(lines) + "return 0;}")
    exe = tmp_path / "lay_pg"
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    assert got == expect, [(i, a, b) for i, (a, b) in enumerate(zip(got, expect)) if a != b]
    assert (Cs.S, Cs.MAX_NODES, Cs.MAX_LOOPS) == (api.PG_SEGMENT, api.PG_MAX_NODES, api.PG_MAX_LOOPS) and M.COST_INCREASED == api.PG_COST_INCREASED
    assert 6 * (api.PG_MAX_NODES // api.PG_SEGMENT + 2 * api.PG_MAX_LOOPS) <= 768
    o = api.PgOptions()
    L.load_library().lili_pg_default_options(C.byref(o))
    assert (o.max_iterations, o.function_tolerance, o.gradient_tolerance, o.parameter_tolerance) == (10, 1e-6, 1e-10, 1e-8)
    assert list(o.prior_var) == list(M.PRIOR_VAR) and list(o.odom_var) == list(M.ODOM_VAR)
