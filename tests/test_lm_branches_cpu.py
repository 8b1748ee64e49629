"""Conditions on the inputs of tests/test_lm_branches_gpu.py, on the oracle (oracle/lo_window.py::ceres_lm) alone, no GPU: every case makes the oracle walk
the stated accept / reject pattern to the stated exit, and no decision on the way is within reach of rounding — no rho within a factor of two of the
min_relative_decrease in force, no candidate within 10 % of the function or the parameter tolerance in force, no accepted rho at the switch between the two
radius rules.  These make the device comparison meaningful; they are not measurements."""
import numpy as np
import pytest

import lili_om_amd as L
from tests import lm_branch_cases as B

SOLVERS = ("window",) + B.FLAVOURS


def _run(oracle, case, solver):
    c = B.CASES[case]
    if solver == "window":
        state, sol, info, log = B.oracle_window(oracle, c["window"], c["opts"])
        x0 = B.norm_of(B.values_of(state))
    else:
        t, q, sol, info, log = B.oracle_slot(oracle, solver, c["slot"], c["opts"])
        x0 = B.norm_of(dict(t=t, q=q))
    return sol, info, log, x0


RUNS = [(case, solver) for case in B.CASES for solver in SOLVERS if solver == "window" or B.CASES[case]["slot"] is not None]


@pytest.mark.parametrize("case,solver", RUNS)
def test_the_oracle_walks_the_stated_path(oracle, case, solver):
    sol, info, log, x0 = _run(oracle, case, solver)
    print(f"{case} [{solver}]: {info}  " + " ".join(f"{e['rho']:.4g}@{e['radius']:.6g}" for e in log))
    B.check_conditions(log, info, B.CASES[case]["opts"], B.expect_of(case, solver), x0)


@pytest.mark.parametrize("solver", SOLVERS)
def test_rejection_cases_reject_in_a_row_recover_and_use_both_radius_rules(oracle, solver):
    """case 1: at least two consecutive rejections, a later acceptance, at least one accepted rho below 0.85 (the unclamped radius update); and, over the
    starts of one solver, a rejection after an acceptance that followed rejections (the divisor's restart at 2 shows in the radius after it)"""
    restart = False
    for case in ("rejections", "rejections_again"):
        if solver != "window" and B.CASES[case]["slot"] is None:
            continue
        sol, info, log, _ = _run(oracle, case, solver)
        p = B.pattern_of(log, info, {})
        first = p.index("RR")                                   # the first of at least two rejections in a row
        n_rej = len(p[first:]) - len(p[first:].lstrip("R"))
        recovery = first + n_rej                                # the candidate after them
        assert recovery < len(p) and p[recovery] == "A", p
        assert any(e["rho"] < 0.85 for e, a in zip(log, B.accepts_of(log, info, {})) if a)
        restart = restart or "R" in p[recovery:]
        # each rejection divides the radius of the one before: by 2, then 4, then 8, ...
        for j in range(n_rej):
            assert log[first + j + 1]["radius"] == log[first + j]["radius"] / 2.0 ** (j + 1)
    assert restart


def test_window_rejection_case_has_the_documented_rho_and_radii(oracle):
    """scale 100, seed 2: rejected rho -0.0758 .. -0.0233, accepted rho >= 0.64 with 0.698, 0.644, 0.789 on the unclamped radius update"""
    state, sol, info, log = B.oracle_window(oracle, B.WINDOW_REJECT, {})
    rej = [e["rho"] for e in log[7:13]]
    assert -0.0759 < min(rej) and max(rej) < -0.0233
    acc = [e["rho"] for e in log[:7] + log[13:]]
    assert min(acc) >= 0.64
    assert [round(r, 3) for r in acc if r < 0.85] == [0.698, 0.644, 0.789]
    assert [log[k]["radius"] / log[k + 1]["radius"] for k in range(7, 13)] == [2.0, 4.0, 8.0, 16.0, 32.0, 64.0]


def test_long_case_overflows_the_log_without_touching_a_tolerance(oracle):
    """case 5: rho 1.0001 .. 1.0010 (window), every relative decrease well above the function tolerance, more candidates than LILI_LM_MAX_LOG"""
    state, sol, info, log = B.oracle_window(oracle, None, B.CASES["long"]["opts"])
    assert len(log) == 40 > L.api.LM_MAX_LOG == 32
    assert 1.00005 < min(e["rho"] for e in log) and max(e["rho"] for e in log) < 1.0011
    dec = [(e["cost"] - e["new_cost"]) / e["cost"] for e in log]
    assert 8e-5 < min(dec) and max(dec) < 1e-4


@pytest.mark.parametrize("solver", SOLVERS)
@pytest.mark.parametrize("variant", list(B.NO_CORRESPONDENCE))
def test_the_oracle_on_an_empty_row_block(oracle, solver, variant):
    """case 6: no correspondence = a residual block without rows.  Default options: the gradient is exactly zero, the first iteration ends on the gradient
    tolerance.  gradient_tolerance = -1: the step is exactly zero, the model change exactly 0, five invalid steps end in numerical_failure."""
    v = B.NO_CORRESPONDENCE[variant]
    if solver == "window":
        recs = B.far_window_oracle(oracle)[0]
        assert all((rs["count"], re["count"]) == (0, 0) for rs, re in recs)
        state, sol, info, log = B.oracle_window(oracle, None, v["opts"], far=True)
        start = B.values_of(state)
    else:
        _, n_s, n_e = B.slot_oracle(oracle, solver, True)
        assert (n_s, n_e) == (0, 0)
        t, q, sol, info, log = B.oracle_slot(oracle, solver, None, v["opts"], far=True)
        start = dict(t=t, q=q)
    B.check_conditions(log, info, v["opts"], v["expect"], B.norm_of(start))
    assert info["cost"] == 0.0
    for k in start:
        assert np.array_equal(sol[k], start[k])
