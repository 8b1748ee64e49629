"""The designed cases of tests/window_factor_cases.py on the CPU: what each case claims to reach holds on the exact model; the model is pinned to the
reference's own ImuFactor.h (tests/golden/ref_imu_cases.npz, recorded from oracle/_ref/libref_imu.so); oracle/lo_window.py is measured against the model,
entry by entry against each entry's own magnitude; and wrong versions of the model are caught by named cases.

Measured here (2^-53 x magnitude = 1):
  model against the reference fixture, 128 factors with covariance = I, worst per block: residual 1.57, d/dPi 2.95, d/dQi 3.03, d/d(speed-bias i) 3.01,
    d/dPj 2.95, d/dQj 2.85, d/d(speed-bias j) 2.95  (asserted at REF_ULPS = 8: Eigen's expression order differs from the model's in at most a few roundings
    per entry — a normalisation, an inverse, two quaternion products and a four-term sum — each at most one unit of the magnitude)
  K = oracle/lo_window.py (imu_factor, Marginalization.factor, speed_bias_prior, Problem.evaluate) against the model, worst over cost, g, H per family:
    attitude 2.58, residual angle 2.14, bias step 1.81, magnitudes 2.66, gravity 1.12, covariance 2.78, covariance scale 2.62, covariance preintegrated 36.5 and covariance
    conditioned 8.69e6 (numpy's f64 inverse and Cholesky of a dense covariance, condition 38 and 1e8: the oracle is not wrong there, it is as exact as f64 LAPACK), covariance
    given 2.33 (those two with the host's sqrt_info given), position 2.77, prior tables 6.24, prior rows 3.53, prior quaternion 4.49, prior x0 norm 2.19, combined 5.73.
    No family shows the oracle wrong.
  numpy's Marginalization against the model's Schur complement of the last-three-columns systems (J0^T J0, J0^T r0; relative to the largest entry), per family:
    window_factor_cases.MARG_NUMPY_WORST; 0 of 75 systems miss the input condition (every eigenvalue of Amm and S >= 1e-3).
  mutations (the smallest ratio among the named catching cases is above 1e12; the device's allowance is at most 50, 293 / 7e7 for `covariance preintegrated` / `conditioned`):
    see MUTATION_CATCHERS."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import lili_om_amd as L
from oracle import lo_window as W
from tests import window_factor_cases as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.path.join(ROOT, "oracle", "_ref", "libref_imu.so")
FIXTURE = os.path.join(ROOT, "tests", "golden", "ref_imu_cases.npz")
REF_ULPS = 8

# mutation of the model -> cases that must notice it (each changes cost, g or H by more than the device's allowance of its family)
MUTATION_CATCHERS = {
    "cq_conjugate": ["bias/dbg0.5_dba0", "position/n2_f0_all", "position/n4_f2_subset"],                  # conjugate instead of inverse() for cq: needs |cq| != 1
    "qleft_sign": ["position/n3_f1_subset", "covariance/preintegrated", "prior_q/w_neg", "attitude/90x"],   # one sign in rows 1..3 of Qleft
    "qright_sign": ["position/n3_f1_subset", "attitude/random0", "bias/dbg0.5_dba0"],                       # one sign in Qright
    "dq_swap": ["attitude/180x-Qj", "position/n4_f1_none", "combined/prior_q/w_zero"],                       # u v^T and v u^T swapped in dq_block (identity attitude: u = 0, blind)
    "rq_unified": ["attitude/identity-Qi", "attitude/180y-Qj", "angle/6:3.641592654", "position/n4_f2_subset"],   # r_q sign-unified: needs r_q.w < 0
    "dw_strict": ["prior_q/w_zero", "combined/prior_q/w_zero"],                                            # >= turned into > at d.w: needs d.w = 0 exactly
    "dq_dbg_transposed": ["position/n3_f0_none", "attitude/identity", "bias/dbg0.01_dba0"],
    "jraw_18": ["position/n4_f0_all", "gravity/tilted", "magnitudes/far_origin"],                            # keyframe j's columns taken from 18 instead of 15
    "prior_T_one_side": ["prior_q/w_zero", "prior_rows/rows1", "combined/prior_rows/rows5"],                 # the prior's T applied on one side of J0^T J0 only
}
# cases that are blind to a mutation by design (the reason the family has more than one member)
MUTATION_BLIND = {"cq_conjugate": ["bias/dbg0_dba0"], "dq_swap": ["attitude/identity"], "rq_unified": ["attitude/90z"], "dw_strict": ["prior_q/w_pos", "prior_q/w_neg"],
                  "prior_T_one_side": ["prior_table/lone_t"], "qright_sign": ["attitude/180z"]}


def _case(name):
    return next(c for c in F.cases() if c["name"] == name)


def test_families_are_complete():
    cs = F.cases()
    assert {c["family"] for c in cs} == set(F.FAMILIES) == set(F.K)
    names = {c["name"] for c in cs}
    for a in ("identity", "90x", "90y", "90z", "180x", "180y", "180z", "random0", "random1", "random2"):
        for sgn in ("", "-Qi", "-Qj", "-Qi-Qj"):
            assert f"attitude/{a}{sgn}" in names
    assert sum(c["family"] == "residual angle" for c in cs) == 7 and sum(c["family"] == "bias step" for c in cs) == 8
    assert {c["imu"][0]["sum_dt"] for c in F.by_family("magnitudes")} == {0.005, 0.2, 2.0, 10.0}
    assert {(c["n_kf"], c["claim"][1]) for c in F.by_family("position")} == {(n, f) for n in (2, 3, 4) for f in range(n - 1)}
    assert {c["prior"]["J0"].shape[1] for c in F.by_family("prior tables")} == {30, 21, 36, 3, 9, 60}
    assert {c["prior"]["J0"].shape[0] for c in F.by_family("prior rows")} == {21, 5, 1, 40, 60}
    assert {(c["n_kf"], c["claim"][1], c["name"].rsplit("_", 1)[1]) for c in F.by_family("position")} == {(n, f, p) for n in (2, 3, 4) for f in range(n - 1) for p in ("all", "none", "subset")}
    full = _case("prior_table/60")
    assert full["n_kf"] == 4 and len(full["prior"]["block_kind"]) == 12 and full["prior"]["J0"].shape == (60, 60)
    for c in cs:          # state quaternions are unit up to rounding
        assert np.abs(np.sum(c["state"][:, 3:7] ** 2, axis=1) - 1.0).max() <= 5e-16, c["name"]
    w0 = _case("attitude/180x")["state"][0, 3:7]
    assert w0[0] == 0.0 and w0[1] == 1.0
    assert np.array_equal(_case("attitude/identity")["state"][0, 3:7], [1.0, 0, 0, 0])
    sb = _case("position/n3_f1_subset")["sb_prior"]
    assert np.isnan(sb[1, 0]) and np.isfinite(sb[1, 1:]).all() and np.isfinite(sb[0]).all()


@pytest.mark.parametrize("family", F.FAMILIES)
def test_claims_hold_on_the_model(family):
    for c in F.by_family(family):
        print(f"{c['name']}: {F.check_claim(c)}")


def _blocks(J):
    out = []
    for b, w in enumerate((3, 4, 9, 3, 4, 9)):
        hi, lo, mg = np.zeros((15, w)), np.zeros((15, w)), np.zeros((15, w))
        for (i, c), v in J[b].items():
            hi[i, c] = float(v.v)
            lo[i, c], mg[i, c] = float(v.v - F.mp.mpf(hi[i, c])), v.m
        out.append([hi, lo, mg])
    return out


def _fixture_factors():
    import importlib.util
    spec = importlib.util.spec_from_file_location("make_ref_golden", os.path.join(ROOT, "tests", "golden", "make_ref_golden.py"))
    G = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(G)
    return G


def test_model_equals_the_reference_fixture():
    G = _fixture_factors()
    facs = G.imu_case_factors()
    fx = np.load(FIXTURE)
    assert [f[0] for f in facs] == list(fx["names"]) and len(facs) >= 90
    worst = np.zeros(7)
    for k, (name, rec, xi, xj) in enumerate(facs):
        r, J, _ = F.imu_factor_global(rec, xi, xj)
        hi = np.array([float(v.v) for v in r])
        ref_r = [hi, np.array([float(v.v - F.mp.mpf(h)) for v, h in zip(r, hi)]), np.array([v.m for v in r])]
        worst[0] = max(worst[0], F.ratios(fx["residual"][k], ref_r).max())
        off = 0
        for b, (w, blk) in enumerate(zip((3, 4, 9, 3, 4, 9), _blocks(J))):
            got = fx["jacobian"][k][off:off + 15 * w].reshape(15, w)
            off += 15 * w
            x = F.ratios(got, blk)
            assert x.max() <= REF_ULPS, (name, b, x.max())
            worst[1 + b] = max(worst[1 + b], x.max())
            assert (got[blk[2] == 0] == 0).all(), (name, b)          # the structural zeros are the reference's
    print("model against the reference fixture, worst per block (residual, six Jacobian blocks), units of 2^-53 magnitude:", np.round(worst, 2))
    assert worst.max() <= REF_ULPS


def test_reference_fixture_regenerates():
    if not os.path.exists(REF):
        pytest.skip("oracle/_ref/libref_imu.so not built (needs the reference sources: oracle/refshim/Makefile)")
    if not hasattr(C.CDLL(REF), "ref_imu_factor_record"):          # nothing is built from a test: a library from before this entry point is as good as none
        pytest.skip("oracle/_ref/libref_imu.so predates ref_imu_factor_record: build oracle/_ref again (make -C oracle/refshim) before the tests")
    G = _fixture_factors()
    now, fx = G.run_imu_cases(), np.load(FIXTURE)
    assert list(now["names"]) == list(fx["names"])
    assert now["residual"].tobytes() == fx["residual"].tobytes() and now["jacobian"].tobytes() == fx["jacobian"].tobytes()
    assert os.path.getsize(FIXTURE) <= os.path.getsize(os.path.join(ROOT, "tests", "golden", "ref_rot_cases.npz"))


@pytest.mark.parametrize("family", F.FAMILIES)
def test_oracle_against_the_model(family):
    k = 0.0
    for c in F.by_family(family):
        m = F.model(c)
        cost, g, H = F.oracle_evaluate(c)
        r = F.worst_ratio(cost, g, H, m)
        assert r < np.inf, c["name"]          # the oracle's structural zeros are exact zeros too
        k = max(k, r)
    print(f"K[{family}] = {k:.3g} (table {F.K[family]:g})")
    assert k <= F.K[family]


@pytest.mark.parametrize("mutation", F.MUTATIONS)
def test_mutations_are_caught(mutation):
    for name in MUTATION_CATCHERS[mutation]:
        c = _case(name)
        base, mm = F.model(c), F.window(c, mut=mutation)
        r = max(F.ratios(mm["H"][0] + mm["H"][1], base["H"]).max(), F.ratios(mm["g"][0] + mm["g"][1], base["g"]).max(), F.ratios(mm["cost"][0] + mm["cost"][1], base["cost"]).max())
        print(f"{mutation}: {name} moves by {r:.3g} units (allowance {F.DEVICE_FACTOR * F.K[c['family']]:g})")
        assert r > 1000 * F.DEVICE_FACTOR * F.K[c["family"]], (mutation, name, r)
    for name in MUTATION_BLIND.get(mutation, []):
        c = _case(name)
        base, mm = F.model(c), F.window(c, mut=mutation)
        assert F.ratios(mm["H"][0] + mm["H"][1], base["H"]).max() <= F.DEVICE_FACTOR * F.K[c["family"]], (mutation, name)


def test_last_three_columns_systems_meet_the_input_condition():
    """every eigenvalue of Amm and of S >= 1e-3 on the model (tests/test_marg_cpu.py's condition); numpy's Marginalization against the model's Schur complement"""
    lc = F.last3_cases()
    assert {c["n_kf"] for c in lc} == {2, 3} and {c["family"] for c in lc} == set(F.IMU_FAMILIES)
    dropped = [c["name"] for c in lc if not F.marg_usable(c)]
    print(f"last-three-columns systems: {len(lc)}, dropped {len(dropped)}: {dropped}")
    assert 4 * len(dropped) <= len(lc)
    worst = {}
    for c in lc:
        if c["name"] in dropped:
            continue
        mm = F.marg_model(c)
        M = W.Marginalization(mm["A"], mm["b"], mm["m"], [])
        d = F.marg_difference(M.linearized_jacobians, M.linearized_residuals, mm)
        worst[c["family"]] = np.maximum(worst.get(c["family"], 0.0), d)
    for fam, d in worst.items():
        print(f"numpy Marginalization against the model [{fam}]: J0^T J0 {d[0]:.3e}  J0^T r0 {d[1]:.3e}")
        assert (d <= np.array(F.MARG_NUMPY_WORST[fam])).all(), (fam, d)


def test_last_three_columns_selection_is_the_documented_one():
    c = F.last3_cases()[0]
    sel, m, kept = F.marg_selection(c)
    assert m == 15 and sel == list(range(30)) and kept == [(0, 1), (1, 1), (2, 1)]
    c3 = next(x for x in F.last3_cases() if x["n_kf"] == 3)
    sel, m, kept = F.marg_selection(c3)
    assert m == 15 and sel == list(range(30)) + list(range(36, 45)) and kept == [(0, 1), (1, 1), (2, 1), (2, 2)]


def test_factor_case_struct_mirrors_match_the_header(tmp_path):
    pairs = [("lili_window_imu", L.api.WindowImu), ("lili_window_prior", L.api.WindowPrior), ("lili_window_problem", L.api.WindowProblem), ("lili_window_prior_storage", L.api.WindowPriorStorage)]
    lines, expect = [], []
    for cname, T in pairs:
        lines.append(f'printf("%zu\\n", sizeof({cname}));')
        expect.append(C.sizeof(T))
        for fname, _ in T._fields_:
            lines.append(f'printf("%zu\\n", offsetof({cname}, {fname}));')
            expect.append(getattr(T, fname).offset)
    src = tmp_path / "lay_factor_cases.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "lili_hip.h"\nint main(void){' + "".join(lines) + "return 0;}")
    exe = tmp_path / "lay_factor_cases"
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    assert got == expect
    assert C.sizeof(L.api.WindowImu) == 470 * 8          # the record the reference shim's ref_imu_factor_record reads is this structure, all doubles
    w = F.window_imu(F.cases()[0]["imu"][0])
    flat = np.frombuffer(bytes(w), np.float64)
    rec = F.cases()[0]["imu"][0]
    assert flat[0] == rec["sum_dt"] and np.array_equal(flat[7:11], rec["delta_q"]) and np.array_equal(flat[14:17], rec["lin_ba"]) and np.array_equal(flat[245:470].reshape(15, 15), rec["covariance"])
