"""The referee of the robust loop factors and of the damped solve (tests/pose_graph_robust_model.py) and the designed graphs (tests/pose_graph_robust_cases.py),
checked on the CPU so that the GPU tests' preconditions hold: the losses' weights are the derivatives of their values, the model's gradient is the gradient of the
model's robust cost, a graph without a loss is the plain model bit for bit, every solve's decisions are clear of their thresholds and independent of the linear
solver, and the losses do on the model what the feature is for.  Also here: the ctypes mirrors of the new structures against the C header."""
import numpy as np
import pytest

from tests import pose_graph_cases as Cs
from tests import pose_graph_model as M
from tests import pose_graph_robust_cases as RC
from tests import pose_graph_robust_model as R

ROBUST = RC.robust_cases()
BRANCH = RC.huber_branch_cases()
LM = RC.lm_cases()
KINDS = [R.HUBER, R.CAUCHY, R.GEMAN_MCCLURE]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("k", [0.7, 1.0, 2.5])
def test_weight_is_the_derivative_of_the_loss(kind, k):
    """w(d) = rho'(d) / d, rho as a function of d, by a central difference; w -> 1 as d -> 0"""
    d = np.array([0.05, 0.3, 0.69, 0.71, 0.99, 1.01, 2.4, 2.6, 7.0, 40.0]) * 1.0
    d = d[np.abs(d - k) > 1e-3]      # (Huber's rho'' jumps at k: the difference must not straddle it)
    h = 1e-6
    rho = lambda x: R.loss_rho(kind, k, x * x)
    num = (rho(d + h) - rho(d - h)) / (2.0 * h) / d
    w = R.loss_weight(kind, k, d * d)
    assert np.abs(num - w).max() <= 1e-8
    assert abs(float(R.loss_weight(kind, k, 1e-24)) - 1.0) <= 1e-15
    assert abs(float(R.loss_rho(kind, k, 1e-8)) / 0.5e-8 - 1.0) <= 1e-7      # and rho -> d^2 / 2


@pytest.mark.parametrize("k", [0.7, 1.0, 2.5])
def test_huber_is_continuous_at_its_scale(k):
    lo, hi = k * (1.0 - 1e-9), k * (1.0 + 1e-9)
    assert abs(float(R.loss_rho(R.HUBER, k, lo * lo)) - float(R.loss_rho(R.HUBER, k, hi * hi))) <= 4e-9 * k * k
    assert float(R.loss_weight(R.HUBER, k, lo * lo)) == 1.0 and abs(float(R.loss_weight(R.HUBER, k, hi * hi)) - 1.0) <= 2e-9
    assert float(R.loss_rho(R.HUBER, k, k * k)) == 0.5 * k * k


@pytest.mark.parametrize("c", ROBUST[0:3], ids=[c["name"] for c in ROBUST[0:3]])
def test_gradient_is_the_gradient_of_the_robust_cost(c):
    """g = J^T W r against a central difference of the model's robust cost along every tangent direction of n40, relative to the largest entry"""
    g = RC.build_model(c)
    grad = g.evaluate()[1]
    num = np.zeros_like(grad)
    h = 1e-6
    for i in range(g.n):
        for k in range(6):
            xi = np.zeros((g.n, 6))
            xi[i, k] = h
            num[i, k] = (g.cost(M.retract(g.X, xi)) - g.cost(M.retract(g.X, -xi))) / (2.0 * h)
    err = np.abs(num - grad).max() / np.abs(grad).max()
    print(f"{c['name']}: gradient vs central difference {err:.2e} of the largest entry")
    assert err <= 1e-6


@pytest.mark.parametrize("name", ["n40", "seg_edges"])
def test_without_a_loss_the_robust_graph_is_the_plain_one(name):
    c = RC.plain_case(name)
    plain = Cs.build_model(c)
    robust = RC.build_model(c)
    assert all(kind == R.NONE for kind, _ in robust.losses) and len(robust.losses) == len(plain.loops)
    for a, b in zip(plain.evaluate(), robust.evaluate()):
        assert np.array_equal(np.asarray(a), np.asarray(b))
    opts = dict(function_tolerance=1e-8, max_iterations=4)
    Xp, sp_ = M.gauss_newton(plain, solver="sparse", **opts)
    Xr, sr = M.gauss_newton(robust, solver="sparse", **opts)
    assert np.array_equal(Xp, Xr)
    assert sp_ == sr
    d2, w = robust.loop_status()
    assert (w == 1.0).all() and d2.shape == (len(plain.loops),)


@pytest.mark.parametrize("c", ROBUST + BRANCH, ids=[c["name"] for c in ROBUST + BRANCH])
def test_robust_solves_are_clear_and_solver_independent(c):
    for kind in ("gn", "lm"):
        g, X, s, d0 = RC.reference(c, kind)      # (asserts that the two linear solvers agree on attempts, pattern and termination)
        assert Cs.decisions_clear(s), (kind, s["margins"])
        assert s["termination"] == (c["expect"] if c["expect"] is not None else s["termination"]) and (c["expect"] is not None or s["termination"] in M.CONVERGED)
        assert s["iterations"] <= 16      # the whole solve fits the device's log
        assert d0[0] <= 1e-9 and d0[1] <= 1e-9
    # on these graphs the damped solve accepts every attempt
    assert all(RC.reference(c, "lm")[2]["accepted"])


def test_huber_branch_cases_sit_on_either_side_of_the_scale():
    below, above = BRANCH
    for c, inside in ((below, True), (above, False)):
        g = RC.build_model(c)
        d2, w = g.loop_status()
        d = float(np.sqrt(d2[0]))
        assert abs(d / c["scale"] - 1.0) <= 2e-3 and abs(d / c["scale"] - 1.0) >= 5e-4      # near the branch, 1e9 roundings clear of it
        assert (d <= c["scale"]) == inside
        assert (w[0] == 1.0) == inside and (inside or abs(w[0] - c["scale"] / d) <= 1e-15)


@pytest.mark.parametrize("c", LM, ids=[c["name"] for c in LM])
def test_damped_solves_are_clear_and_solver_independent(c):
    g, X, s, d0 = RC.reference(c, "lm")
    assert Cs.decisions_clear(s), s["margins"]
    pattern = "".join("A" if a else "r" for a in s["accepted"])
    print(f"{c['name']}: attempts {s['iterations']} pattern {pattern} termination {s['termination']} cost {s['initial_cost']:.6e} -> {s['final_cost']:.6e} lambda {s['lambda'][0]:g} .. {s['final_lambda']:g}")
    assert s["iterations"] == len(s["accepted"]) == len(s["lambda"]) <= 16
    assert s["steps_accepted"] + s["steps_rejected"] == s["iterations"]
    # plain Gauss-Newton gives up on this graph at once
    assert M.gauss_newton(g, solver="sparse")[1]["termination"] == M.COST_INCREASED
    if c["name"] == "lm_lambda_limit":
        assert s["termination"] == R.LAMBDA_LIMIT and not any(s["accepted"]) and np.array_equal(X, g.X) and s["final_cost"] == s["initial_cost"]
        assert s["final_lambda"] > 1e2 >= s["lambda"][-1]
    else:
        assert s["termination"] in M.CONVERGED
        assert pattern.startswith("rrrrrrrrrA" if c["lm"]["diagonal_damping"] == 0 else "rrrArArArA")
        assert s["final_cost"] < 0.03 * s["initial_cost"]      # 5.36e6 -> 1.27e5
    # every lambda is the previous one times or over the factor
    for a, l0, l1 in zip(s["accepted"], s["lambda"], s["lambda"][1:] + [s["final_lambda"]]):
        assert l1 == (max(l0 / 10.0, 1e-10) if a else l0 * 10.0)


@pytest.mark.parametrize("name", ["n40", "seg_edges"])
def test_a_loss_keeps_a_false_loop_from_bending_the_map(name):
    """each loss leaves the solution at most a fifth as far from the clean solve (the same graph without the false loops) as the plain solve of the same graph;
    every false loop ends with a weight <= 0.05; under Huber every true loop of n40 keeps weight 1"""
    clean, s_clean = M.gauss_newton(RC.build_model(RC.plain_case(name, with_false=False)), solver="sparse", **RC.plain_case(name, with_false=False)["options"])
    plain, s_plain = M.gauss_newton(RC.build_model(RC.plain_case(name)), solver="sparse", **RC.plain_case(name)["options"])
    assert Cs.decisions_clear(s_clean) and Cs.decisions_clear(s_plain)
    assert s_clean["termination"] in M.CONVERGED and s_plain["termination"] in M.CONVERGED + (M.MAX_ITERATIONS,)
    d_plain = RC.distance(plain, clean)
    for loss in RC.LOSS_NAMES:
        c = RC.robust_case(name, loss)
        g, X, s, _ = RC.reference(c, "gn")
        d = RC.distance(X, clean)
        _, w = g.loop_status(X)
        print(f"{name} {loss}: {d:.4f} m from the clean solve (plain {d_plain:.4f} m), false loops' weights {np.round(w[c['n_true']:], 4)}, true loops' {np.round(w[:c['n_true']], 4)}")
        assert d <= 0.2 * d_plain
        assert (w[c["n_true"]:] <= 0.05).all()
        if name == "n40" and loss == "huber":
            assert (w[:c["n_true"]] == 1.0).all()


def test_lm_struct_mirrors_match_the_header(tmp_path):
    """size and every field's offset of lili_pg_lm_options / lili_pg_lm_summary (the C header compiled as plain C) against the ctypes mirrors, and the constants"""
    import ctypes as C
    import os
    import subprocess
    from lili_om_amd import api
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    lines, expect = [], []
    for cname, T in (("lili_pg_lm_options", api.PgLmOptions), ("lili_pg_lm_summary", api.PgLmSummary)):
        lines.append(f'printf("%zu\\n", sizeof({cname}));')
        expect.append(C.sizeof(T))
        for fname, _ in T._fields_:
            lines.append(f'printf("%zu\\n", offsetof({cname}, {fname.rstrip("_") if fname == "lambda_" else fname}));')
            expect.append(getattr(T, fname).offset)
    lines.append('printf("%d\\n%d\\n%d\\n%d\\n%d\\n", LILI_PG_LOSS_NONE, LILI_PG_LOSS_HUBER, LILI_PG_LOSS_CAUCHY, LILI_PG_LOSS_GEMAN_MCCLURE, LILI_PG_LAMBDA_LIMIT);')
    expect += [api.PG_LOSS_NONE, api.PG_LOSS_HUBER, api.PG_LOSS_CAUCHY, api.PG_LOSS_GEMAN_MCCLURE, api.PG_LAMBDA_LIMIT]
    src = tmp_path / "lay_lm.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "lili_hip.h"\nint main(void){' + "".join(lines) + "return 0;}")
    exe = tmp_path / "lay_lm"
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(root, "include"), str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    assert got == expect
    assert (R.NONE, R.HUBER, R.CAUCHY, R.GEMAN_MCCLURE, R.LAMBDA_LIMIT) == tuple(expect[-5:])
