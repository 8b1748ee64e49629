"""The states of tests/pose_graph_factor_cases.py and their multi-precision referee (tests/pose_graph_factor_referee.py), without a GPU:
  the referee's analytic Jacobian blocks against central differences of its own error function through its own retract (50 digits, h = 1e-20): 1e-25 of the
  block's largest entry — the referee rests on the header's conventions alone;
  the f64 model (tests/pose_graph_model.py, tests/pose_graph_robust_model.py) against the referee, every output array, which gives D = max |model - referee| / A
  per state and array: D <= 64 eps up to 3.0 rad, D <= eps / delta at pi -/+ delta (the cancellation in 1 + cos t is the closed form's).  D is the
  yardstick of tests/test_pose_graph_factors_gpu.py, so the cap is what keeps that test sharp;
  the yardstick itself: at the generic-frame states A stays within 64 times the largest value of an entry's 3 x 3 quadrant, and D there is of the order of eps;
  the design conditions: |q_e.w| >= 4e-9, the residual angle equals the prescribed one to 1e-15 relative (its distance from pi equals delta to 1e-6), Huber's d
  at least 1e-6 relative away from k, every weight of a loss in (1e-3, 1];
  the one-step cases: the referee's candidate cost <= half the old cost where the step is to be accepted, >= twice where it is to be rejected."""
import mpmath as mp
import pytest

from tests import pose_graph_factor_cases as FC
from tests import pose_graph_factor_referee as R
from tests import pose_graph_model as M
from tests import pose_graph_robust_model as RM

STATES = FC.states()
STEPS = FC.chain_step_cases() + FC.loop_step_cases()


def test_the_set_of_states():
    names = [s["name"] for s in STATES]
    assert len(set(names)) == len(names) and 140 <= len(names) <= 180
    for kind in FC.KINDS:
        assert any(s["kind"] == kind for s in STATES)
    for label, _, _ in FC.THETAS:
        assert sum(s["theta"][0] == label and s["kind"] == "chain" for s in STATES) >= 3 and any(s["theta"][0] == label and s["kind"] == "loop_gt" for s in STATES)
    for s in STATES:
        assert s["twin"] is None or s["twin"] in names


def test_jacobians_against_high_precision_differences():
    worst = 0.0
    with mp.workdps(R.DPS):
        for s in STATES:
            g = FC.referee_graph(s)
            for f in range(g.n + len(g.loops)):
                fac = g.factor(g.X, f)
                Ja, Jb = R.numeric_jacobians(g, f)
                for name, num, ana in (("Ja", Ja, fac["Ja0"]), ("Jb", Jb, fac["Jb0"])):
                    if num is None:
                        continue
                    for blk in ((0, 0), (3, 0), (3, 3), (0, 3)):
                        sub_n = [[num[blk[0] + i][blk[1] + j] for j in range(3)] for i in range(3)]
                        sub_a = [[ana[blk[0] + i][blk[1] + j] for j in range(3)] for i in range(3)]
                        scale = max(abs(x) for row in sub_a for x in row)
                        err = max(abs(sub_n[i][j] - sub_a[i][j]) for i in range(3) for j in range(3))
                        if scale == 0:
                            assert err <= mp.mpf("1e-25"), (s["name"], f, name, blk, err)
                        else:
                            worst = max(worst, float(err / scale))
                            assert err <= mp.mpf("1e-25") * scale, (s["name"], f, name, blk, float(err / scale))
    print(f"analytic blocks against central differences: worst {worst:.2e} of the block's largest entry")


def test_model_against_referee_gives_D_under_its_cap():
    per_theta, bad = {}, []
    for s in STATES:
        _, D = FC.reference(s)
        c = FC.cap(s)
        row = per_theta.setdefault(s["theta"][0], dict.fromkeys(FC.ARRAYS, 0.0))
        for k in FC.ARRAYS:
            row[k] = max(row[k], D[k])
            if not D[k] <= c:
                bad.append((s["name"], k, D[k] / FC.EPS, c / FC.EPS))
    for label, _, _ in FC.THETAS:
        print(f"D [theta {label:>9}] (eps): " + "  ".join(f"{k} {per_theta[label][k] / FC.EPS:.3g}" for k in FC.ARRAYS))
    assert not bad, bad


def test_the_yardstick_is_a_magnitude():
    """A must be the size of an entry's terms, not a compounded bound: max(10 D, 64 eps) A is only as sharp as A is small.  At the generic-frame states with
    coordinates of a few metres: a rotation-matrix entry 1 - 2 (y^2 + z^2) carries at most 3; an absolute-value product of orthonormal rows and columns stays
    within sqrt(3) of that; Jr^-1 up to 3 rad has entries below 2; so an entry of J carries less than 8 times its block's largest, and a Gram entry less than
    8^2 = 64 times its quadrant's largest.  (The states at coordinates near 1e3 m are left out: their lever is the difference of numbers 40 times its size, and A
    says so.)  And D, the f64 model's error in units of A, is then of the order of eps: a median under eps / 4 would mean a yardstick ten times too long."""
    worst, Ds = 0.0, []
    for s in STATES:
        if s["family"] != "S" or s["theta"][1] != "plain" or s["lever"] == "large":
            continue
        ref, D = FC.reference(s)
        Ds.append(D["diag"])
        for k in ("diag", "sub", "loop"):
            for blk in range(ref[k].shape[0]):
                for qi in (0, 3):
                    for qj in (0, 3):
                        v, a = abs(ref[k][blk, qi:qi + 3, qj:qj + 3]), ref["A_" + k][blk, qi:qi + 3, qj:qj + 3]
                        if v.max() > 0:
                            r = float((a[v >= 1e-3 * v.max()] / v.max()).max())
                            worst = max(worst, r)
                            assert r <= 64.0, (s["name"], k, blk, qi, qj, r)
    Ds.sort()
    print(f"A / quadrant's largest value: worst {worst:.3g}; D of the diagonal blocks at {len(Ds)} generic states: median {Ds[len(Ds) // 2] / FC.EPS:.3g} eps")
    assert len(Ds) >= 30 and Ds[len(Ds) // 2] >= 0.25 * FC.EPS


def test_design_conditions():
    with mp.workdps(R.DPS):
        for s in STATES:
            g = FC.referee_graph(s)
            fac = g.factor(g.X, s["factor"])
            label, side, v = s["theta"]
            assert abs(fac["qe"][0]) >= mp.mpf("4e-9"), (s["name"], float(fac["qe"][0]))
            assert (fac["qe"][0] < 0) == ((side == "far") != (s["variant"] == "negated")), s["name"]      # three negated factors: -q_e
            angle = mp.sqrt(sum(x * x for x in fac["e"][0:3]))
            want = FC.expected_angle(s["theta"])
            assert abs(angle - want) <= mp.mpf("1e-15") * want, (s["name"], float((angle - want) / want) if want else float(angle))
            if side != "plain":
                assert abs((mp.pi - angle) - mp.mpf(v)) <= mp.mpf("1e-6") * mp.mpf(v), s["name"]
            if want > 0:
                ax = [mp.mpf(x) for x in FC.AXES[s["axis"]]]
                n = mp.sqrt(sum(x * x for x in ax))
                sign = -1 if side == "far" else 1
                assert max(abs(fac["e"][i] / angle - sign * ax[i] / n) for i in range(3)) <= (mp.mpf("1e-7") if side != "plain" else mp.mpf("1e-14")), s["name"]
            if s["loops"]:
                kind, k = s["loops"][0][4], mp.mpf(s["loops"][0][5])
                if kind == RM.HUBER:
                    assert abs(mp.sqrt(fac["d2"]) - k) >= mp.mpf("1e-6") * k, s["name"]
                    assert (s["loss"] == "huber_below") == (mp.sqrt(fac["d2"]) < k)
                if kind != RM.NONE:
                    assert mp.mpf("1e-3") < fac["w"] <= 1 and (fac["w"] < 1 or s["loss"] == "huber_below"), (s["name"], float(fac["w"]))


@pytest.mark.parametrize("c", STEPS, ids=[c["name"] for c in STEPS])
def test_one_step_cases(c):
    ref, g, X, sm, d1 = FC.step_reference(c)
    print(f"{c['name']}: referee cost {ref['cost']:.6e} -> {ref['new_cost']:.6e}, model {sm['initial_cost']:.6e} -> {sm['cost'][0]:.6e}; the model's miss D1 {d1[0]:.2e} m {d1[1]:.2e} rad")
    if c["expect"] == "accepted":
        assert ref["new_cost"] <= 0.5 * ref["cost"]
        assert sm["termination"] == M.MAX_ITERATIONS and sm["iterations"] == 1
    else:
        assert ref["new_cost"] >= 2.0 * ref["cost"]
        assert sm["termination"] == M.COST_INCREASED
    assert abs(sm["step_inf"][0] - ref["step_inf"]) <= 64 * FC.EPS * ref["step_inf"]
