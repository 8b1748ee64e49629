"""Cases that walk the trust-region loops of k_solve_lm / k_solve_lm_window (lili_s2m_lm.hip) and k_window_solve (lili_window.hip) through the branches
the other LM tests never take: rejected candidates (radius / divisor, divisor doubled, reset after the next acceptance, the accepted point surviving the
rejected candidate), the unclamped radius update, the max_radius clamp, the exits on min_radius (and its precedence against max_iterations), on the
gradient and the parameter tolerance, five invalid steps in a row, more candidates than LILI_LM_MAX_LOG, and slots without a single correspondence.

Shared by tests/test_lm_branches_cpu.py (the conditions on the inputs, on the oracle alone) and tests/test_lm_branches_gpu.py (the device against the oracle).
Referee: oracle/lo_window.py::ceres_lm.  Inputs: the window of tests/test_window_solve_gpu.py::test_solve_speed_bias_prior_branch and the room of
tests/test_lm_gpu.py::test_device_lm_takes_the_oracle_lm_decisions, their helpers imported from there."""
import ctypes as C
import functools

import numpy as np

import lili_om_amd as L
from lili_om_amd import synth
from oracle import lo_window as W
from tests import window_harness as H
from tests.test_lm_gpu import _angle, _data, _oracle_problem
from tests.test_window_solve_gpu import build_problem, oracle_side, perturbed, state_of, values_of

MASK = L.MASK_SURF | L.MASK_EDGE
DEFAULTS = dict(max_iterations=15, function_tolerance=1e-6, gradient_tolerance=1e-10, parameter_tolerance=1e-8, initial_radius=1e4, max_radius=1e16,
                min_radius=1e-32, min_relative_decrease=1e-3)          # lili_lm_default_options = Ceres 2.0 with max_num_iterations = 15
ROOM = dict(seed=61, n_surf=3000, n_edge=250)
FLAVOURS = ("livox", "rot")
FAR = np.array([1000.0, 0.0, 0.0], np.float32)                        # case 6: the queries, 1000 m from the map

# ---- starts.  Window: perturbed(state_of(win, 3), seed, scale=scale).  Single slot: synth.perturbed_pose(t0, q0, default_rng(seed), dt, dang_deg) from the
# association pose (t0, q0) of the room.  None = the unperturbed start.  Found by a search on the oracle alone (seeds 0 .. 39, 0 .. 3 m, 150 .. 179 deg: with
# fixed correspondences the oracle rejects nothing below ~170 deg); the oracle's rho per candidate, in order:
#   window 100 / 2    A A A A A A A R R R R R R A A      1.00 1.22 1.52 1.28 1.01 0.964 0.698 | -0.0758 -0.0758 -0.0758 -0.0757 -0.0741 -0.0233 | 0.644 0.789
#   window 300 / 36   A A A A A A A R R R R R A R R      0.89 0.989 1.03 1.43 1.51 0.64 0.735 | -0.24 -0.24 -0.24 -0.238 -0.21 | 0.135 | -0.799 -0.268
#                     (a rejection AFTER an acceptance after rejections: the divisor restarts at 2)
#   livox 0.5 m 179 deg seed 13   A A R R R R A A R R A A A A A      1 0.322 | -0.0767 -0.0766 -0.076 -0.0709 | 0.00554 0.458 | -0.219 -0.115 | 0.239 1.08 1.38 1.42 1.83
#   rot   0 m   178 deg seed 28   A A A A A A A R R R R R R A R      2.44 2.21 2.34 1.97 1.13 1.4 1.3 | -0.0988 -0.0988 -0.0988 -0.0988 -0.0987 -0.0958 | 0.0648 | -1.04
# A start shifted by 1e-13 m moves the oracle's end point by < 1e-13 m (livox, rot) and no decision: the walks are not chaotic.
WINDOW_REJECT = dict(scale=100, seed=2)
WINDOW_REJECT_AGAIN = dict(scale=300, seed=36)
SLOT_REJECT = dict(livox=dict(dt=0.5, dang_deg=179.0, seed=13), rot=dict(dt=0.0, dang_deg=178.0, seed=28))
SLOT_EASY = (dict(dt=0.05, dang_deg=0.5, seed=100), dict(dt=0.05, dang_deg=0.5, seed=102))      # the well-behaved neighbours of lili_s2m_solve_lm_window (test_lm_gpu's)

ALL_REJECTED_RADII = [1e4, 5000.0, 1250.0, 156.25, 9.765625, 0.30517578125, 0.00476837158203125]

# name -> options (the device's names), start of the window, what the oracle must do on the window / on a single slot of either flavour
CASES = {
    "rejections": dict(opts={}, window=WINDOW_REJECT, slot="reject",
                       expect_window=dict(pattern="AAAAAAARRRRRRAA", iterations=15, successful_steps=9, termination="max_iterations"),
                       expect_slot=dict(livox=dict(pattern="AARRRRAARRAAAAA", iterations=15, successful_steps=9, termination="max_iterations"),
                                        rot=dict(pattern="AAAAAAARRRRRRAR", iterations=15, successful_steps=8, termination="max_iterations"))),
    "rejections_again": dict(opts={}, window=WINDOW_REJECT_AGAIN, slot=None,
                             expect_window=dict(pattern="AAAAAAARRRRRARR", iterations=15, successful_steps=8, termination="max_iterations")),
    "all_rejected_min_radius": dict(opts=dict(min_relative_decrease=1e30, min_radius=1e-3, max_iterations=8), window=None, slot="start",
                                    expect=dict(pattern="RRRRRRR", iterations=7, successful_steps=0, termination="min_radius", radii=ALL_REJECTED_RADII)),
    "all_rejected_max_iterations": dict(opts=dict(min_relative_decrease=1e30, min_radius=1e-3, max_iterations=7), window=None, slot="start",
                                        expect=dict(pattern="RRRRRRR", iterations=7, successful_steps=0, termination="max_iterations", radii=ALL_REJECTED_RADII)),
    "gradient_tolerance": dict(opts=dict(gradient_tolerance=1e12), window=None, slot="start",
                               expect=dict(pattern="", iterations=1, successful_steps=0, termination="gradient_tolerance")),
    "parameter_tolerance": dict(opts=dict(parameter_tolerance=0.1), window=None, slot="start",
                                expect=dict(pattern="-", iterations=1, successful_steps=0, termination="parameter_tolerance")),
    "long": dict(opts=dict(initial_radius=1e-3, max_radius=1e-3, max_iterations=40), window=None, slot="start",
                 expect=dict(pattern="A" * 40, iterations=40, successful_steps=40, termination="max_iterations", radii=[1e-3] * 40)),
}
# case 6, on slots without a correspondence
NO_CORRESPONDENCE = {
    "default": dict(opts={}, expect=dict(pattern="", iterations=1, successful_steps=0, termination="gradient_tolerance"), final_radius=1e4, gn_status=0),
    "invalid_steps": dict(opts=dict(gradient_tolerance=-1.0), expect=dict(pattern="", iterations=5, successful_steps=0, termination="numerical_failure"),
                          final_radius=1e4 / 32, gn_status=1),
}


def expect_of(case, solver):
    c = CASES[case]
    if "expect" in c:
        return c["expect"]
    return c["expect_window"] if solver == "window" else c["expect_slot"][solver]


def options_of(opts):
    o = dict(DEFAULTS)
    o.update(opts)
    return o


def oracle_kwargs(opts):
    kw = dict(opts)
    kw["max_num_iterations"] = kw.pop("max_iterations", DEFAULTS["max_iterations"])
    return kw


# ---------------------------------------------------------------- inputs (built once per process, never modified)
@functools.lru_cache(maxsize=None)
def window():
    return H.make_window(n_surf=2500, n_edge=200)


def window_start(start):
    s0 = state_of(window(), 3)
    return s0 if start is None else perturbed(s0, start["seed"], scale=start["scale"])


@functools.lru_cache(maxsize=None)
def window_oracle(oracle):
    """(records, problem) of test_solve_speed_bias_prior_branch: associated once at the initial poses, IMU factors, speed-bias priors at the initial speed-bias"""
    recs, block = oracle_side(oracle, window())
    return recs, H.build_problem(window(), block)


@functools.lru_cache(maxsize=None)
def far_window():
    """the window with every query 1000 m away: no keyframe has a correspondence"""
    win = dict(window())
    win["kfs"] = [dict(kf, q_xyz=kf["q_xyz"] + FAR, eq_xyz=kf["eq_xyz"] + FAR) for kf in win["kfs"]]
    return win


@functools.lru_cache(maxsize=None)
def far_window_oracle(oracle):
    recs, block = oracle_side(oracle, far_window())
    return recs, build_problem(far_window(), block, sb_priors=False, imu=False)


@functools.lru_cache(maxsize=None)
def slot_data(flavour, far=False):
    data = _data(flavour, **ROOM)
    if far:
        data = dict(data, room=dict(data["room"], q_xyz=data["room"]["q_xyz"] + FAR, eq_xyz=data["room"]["eq_xyz"] + FAR))
    return data


@functools.lru_cache(maxsize=None)
def slot_oracle(oracle, flavour, far=False):
    """(problem, n_surf, n_edge): the correspondences of the association pose (t0, q0)"""
    return _oracle_problem(oracle, slot_data(flavour, far), flavour)


def slot_start(flavour, start):
    """start: None / "start" = (t0, q0); "reject" = SLOT_REJECT[flavour]; or a dict(dt, dang_deg, seed)"""
    data = slot_data(flavour)
    if start is None or start == "start":
        return data["t0"].copy(), data["q0"].copy()
    if start == "reject":
        start = SLOT_REJECT[flavour]
    t, q = synth.perturbed_pose(data["t0"], data["q0"], np.random.default_rng(start["seed"]), start["dt"], start["dang_deg"])
    return np.asarray(t, np.float64), np.asarray(q, np.float64)


def run_oracle(pb, values, opts):
    """ceres_lm from `values` (the problem's own parameters stay as they are): (solution, info, log)"""
    keep = pb.params
    pb.params = {k: np.array(v, np.float64) for k, v in values.items()}
    try:
        log = []
        sol, info = W.ceres_lm(pb, log=log, **oracle_kwargs(opts))
    finally:
        pb.params = keep
    return sol, info, log


def oracle_window(oracle, start, opts, far=False):
    pb = (far_window_oracle if far else window_oracle)(oracle)[1]
    state = state_of(far_window(), 3) if far else window_start(start)
    return (state,) + run_oracle(pb, values_of(state), opts)


def oracle_slot(oracle, flavour, start, opts, far=False):
    pb = slot_oracle(oracle, flavour, far)[0]
    t, q = slot_start(flavour, start)
    return (t, q) + run_oracle(pb, dict(t=t, q=q), opts)


# ---------------------------------------------------------------- the oracle's decisions
def by_tolerance(info):
    return info["termination"] in ("function_tolerance", "parameter_tolerance")


def accepts_of(log_o, info_o, opts):
    """what the minimiser does with each evaluated candidate: taken or not (the one that ends the solve on a tolerance is not)"""
    acc = [e["rho"] > options_of(opts)["min_relative_decrease"] for e in log_o]
    if by_tolerance(info_o) and acc:
        acc[-1] = False
    return acc


def pattern_of(log_o, info_o, opts):
    p = ["A" if a else "R" for a in accepts_of(log_o, info_o, opts)]
    if by_tolerance(info_o) and p:
        p[-1] = "-"               # neither accepted nor rejected: the solve returned before the decision
    return "".join(p)


CLAMP_RHO = 0.5 * (1.0 + (2.0 / 3.0) ** (1.0 / 3.0))          # 1 - (2 rho - 1)^3 <= 1/3 from here on: the radius triples (0.93679...)


def check_conditions(log_o, info_o, opts, expect, x0_norm):
    """Conditions on the input, from the oracle alone: the stated walk, and no decision of it that rounding could turn.  x0_norm: |x| of the start — the
    parameter tolerance is relative to |x| of the accepted point, which lies within the summed accepted steps of it."""
    o = options_of(opts)
    assert pattern_of(log_o, info_o, opts) == expect["pattern"], (pattern_of(log_o, info_o, opts), expect["pattern"])
    assert info_o["iterations"] == expect["iterations"] and info_o["successful_steps"] == expect["successful_steps"], info_o
    assert info_o["termination"] == expect["termination"], info_o
    if "radii" in expect:
        assert [e["radius"] for e in log_o] == expect["radii"]
    mrd, ftol, ptol = o["min_relative_decrease"], o["function_tolerance"], o["parameter_tolerance"]
    moved = 0.0
    for e, taken in zip(log_o, accepts_of(log_o, info_o, opts)):
        assert not (0.5 * mrd <= e["rho"] <= 2.0 * mrd), e
        assert not (0.9 * ftol <= abs(e["cost"] - e["new_cost"]) / e["cost"] <= 1.1 * ftol), e
        assert not (0.9 * ptol * (max(x0_norm - moved, 0.0) + ptol) <= e["step"] <= 1.1 * ptol * (x0_norm + moved + ptol)), e
        if taken:
            assert abs(e["rho"] - CLAMP_RHO) > 1e-6 * CLAMP_RHO, e          # which radius rule applies is no coin toss either
            moved += e["step"]


def norm_of(values):
    return float(np.sqrt(sum(float(np.dot(v, v)) for v in values.values())))


# ---------------------------------------------------------------- the device's summary, in a guarded buffer
class GuardedSummaries:
    """n lili_lm_summary inside a larger zeroed buffer.  The kernels write the summary into device memory and the library copies it back at a fixed size, so
    the zero tail guards the host-side copy only; what the kernel itself counted is the raw n_logged field, which dicts() hands over next to the log
    (LmSummary.as_dict cuts the log at the array's 32 entries whatever n_logged says)."""
    PAD = 4096

    def __init__(self, n=1):
        self.size = C.sizeof(L.api.LmSummary) * n
        self.buf = (C.c_ubyte * (self.size + self.PAD))()
        self.s = (L.api.LmSummary * n).from_buffer(self.buf)

    def tail_is_zero(self):
        return not any(bytes(self.buf)[self.size:])

    def dicts(self):
        return [dict(x.as_dict(), n_logged=int(x.n_logged)) for x in self.s]


def _opt(m, opts):
    return m.lm_options(**opts) if opts else None


def solve_slot(m, slot, opts):
    """lili_s2m_solve_lm -> summary dict (with the raw n_logged)"""
    g = GuardedSummaries(1)
    m.solve_lm(slot, MASK, options=_opt(m, opts), summary=g.s[0])
    assert g.tail_is_zero()
    return g.dicts()[0]


def solve_slots(m, slots, opts):
    """lili_s2m_solve_lm_window -> [summary dict]"""
    g = GuardedSummaries(len(slots))
    m.solve_lm_window(list(slots), MASK, options=_opt(m, opts), summary=g.s)
    assert g.tail_is_zero()
    return g.dicts()


def solve_window(ws, state, opts):
    """lili_window_solve -> (final state, summary dict)"""
    g = GuardedSummaries(1)
    final, _ = ws.solve(state, options=_opt(ws.matcher, opts), summary=g.s[0])
    assert g.tail_is_zero()
    return final, g.dicts()[0]


# ---------------------------------------------------------------- device against oracle
def check_decisions(summ, log_o, info_o, opts):
    """Termination, iterations, successful steps, log length, the iteration every candidate belongs to and the accept / reject sequence: equal."""
    assert summ["termination"] == info_o["termination"], (summ["termination"], info_o)
    assert summ["iterations"] == info_o["iterations"] and summ["successful_steps"] == info_o["successful_steps"], (summ["iterations"], summ["successful_steps"], info_o)
    n = min(len(log_o), L.api.LM_MAX_LOG)
    assert summ["n_logged"] == n and len(summ["log"]) == n, (summ["n_logged"], len(summ["log"]), n)      # n_logged: the field as the kernel wrote it
    assert [e["accepted"] for e in summ["log"]] == accepts_of(log_o, info_o, opts)[:n]
    assert [e["it"] for e in summ["log"]] == [e["it"] for e in log_o[:n]]
    mrd = options_of(opts)["min_relative_decrease"]
    for a, b in zip(summ["log"], log_o):
        assert (a["rho"] > mrd) == (b["rho"] > mrd), (a, b)


def radius_after(radius, rho, accepted, rejected_in_a_row, max_radius):
    """Ceres' rule: (next radius, exact).  accepted: min(max_radius, radius / max(1/3, 1 - (2 rho - 1)^3)) — three times the radius or max_radius exactly where
    a clamp is active (as Ceres divides: radius / (1.0 / 3.0)); rejected: radius / 2^(number of rejections in a row, this one included), exactly."""
    if not accepted:
        return radius / 2.0 ** rejected_in_a_row, True
    if rho >= CLAMP_RHO:
        return min(max_radius, radius / (1.0 / 3.0)), True          # Ceres' own expression: within an ulp of 3 x radius, not always on it
    r = radius / (1.0 - (2.0 * rho - 1.0) ** 3)
    return (max_radius, True) if r >= max_radius else (r, False)


def check_radii(summ, log_o, info_o, opts):
    """The device's own radii obey the rule from candidate to candidate — exactly where the rule is exact, else within 1e-9 (tests/test_lm_gpu.py's bound) —
    and they are the oracle's radii within 1e-9; final_radius is the radius after the last logged candidate (all candidates logged only)."""
    o = options_of(opts)
    log, acc = summ["log"], accepts_of(log_o, info_o, opts)
    assert log[0]["radius"] == o["initial_radius"]
    run = 0
    for k, (a, b) in enumerate(zip(log, log_o)):
        assert abs(a["radius"] - b["radius"]) <= 1e-9 * b["radius"], (k, a, b)
        run = 0 if acc[k] else run + 1
        last = k + 1 == len(log_o)
        if last and by_tolerance(info_o):
            nxt, exact = a["radius"], True                  # returned before the radius was touched
        else:
            nxt, exact = radius_after(a["radius"], b["rho"], acc[k], run, o["max_radius"])
        if k + 1 < len(log):
            got = log[k + 1]["radius"]
            assert log[k + 1]["it"] == a["it"] + 1          # no invalid step (unlogged, radius halved) in between
        elif last:
            got = summ["final_radius"]
        else:
            continue
        assert (got == nxt) if exact else (abs(got - nxt) <= 1e-9 * nxt), (k, got, nxt, exact)


def check_log_values(summ, log_o, info_o):
    """_compare's bounds of tests/test_lm_gpu.py: costs 1e-9 relative, steps 1e-6"""
    for a, b in zip(summ["log"], log_o):
        assert abs(a["cost"] - b["cost"]) <= 1e-9 * b["cost"] and abs(a["new_cost"] - b["new_cost"]) <= 1e-9 * b["cost"], (a, b)
        assert abs(a["step"] - b["step"]) <= 1e-6 * max(b["step"], 1e-9), (a, b)
    assert abs(summ["final_cost"] - info_o["cost"]) <= 1e-9 * max(info_o["cost"], 1e-300)
    assert abs(summ["initial_cost"] - (log_o[0]["cost"] if log_o else info_o["cost"])) <= 1e-9 * max(info_o["cost"], 1e-300)


def rejected_candidates_leave_the_accepted_point(summ):
    """`cost` of a candidate is the cost at the accepted point it was proposed from: the same double until a candidate is taken, then that candidate's new_cost"""
    log = summ["log"]
    assert log[0]["cost"] == summ["initial_cost"]
    for a, b in zip(log, log[1:]):
        assert b["cost"] == (a["new_cost"] if a["accepted"] else a["cost"]), (a, b)
    if log and len(log) == summ["iterations"]:
        assert summ["final_cost"] == (log[-1]["new_cost"] if log[-1]["accepted"] else log[-1]["cost"])


def window_distance(final, info, sol_o, info_o):
    """(d_cost relative, d_t m, d_angle rad, d_speed_bias) of a window solve to the oracle's end state"""
    d_cost = abs(info["final_cost"] - info_o["cost"]) / max(info_o["cost"], 1e-300)
    n = final.shape[0]
    dt = max(np.linalg.norm(final[k, 0:3] - sol_o[f"t{k}"]) for k in range(n))
    da = max(_angle(final[k, 3:7], sol_o[f"q{k}"]) for k in range(n))
    dsb = max(np.abs(final[k, 7:16] - sol_o[f"sb{k}"]).max() for k in range(n))
    return d_cost, dt, da, dsb


def slot_distance(t, q, sol_o):
    return np.linalg.norm(t - sol_o["t"]), _angle(q, sol_o["q"])
