"""The hard sample streams of tests/preint_hard_cases.py, the parts that need no GPU (IMU pre-integration):
  * every case regenerates to the SHA-256 recorded in tests/golden/ref_preint_hard.npz, and that fixture is what the reference's own header gives now
    (oracle/_ref/libref_imu.so, where it is built), bit for bit;
  * every family has the property it was built for; every output is finite and every covariance positive definite; the masks of exactly-zero entries are
    the recorded ones, and the families built for zeros have more of them than the structure of F and V alone gives (138 of the Jacobian, 48 of the covariance);
  * the oracle's numpy restatement (oracle/lo_window.py::Preintegration) against the fixture: state within 1e-13; Jacobian and covariance per 3 x 3 block,
    relative to the block's largest reference entry, within ORACLE_BOUND = 20 x the worst measured over these cases (numpy's `@` sums in another order);
  * the comparison the device is held to (tests/preint_hard_cases.py::compare / equal) notices every fault of MUTANTS — applied to a restatement that,
    unmutated, equals the fixture entry by entry — in at least one hard case; for each it prints whether the earlier measure ("1e-11 of the largest
    entry", on the 33 cases of tests/golden/ref_preint.npz) would have.

Measured here, the oracle against the fixture, worst block-relative difference (Jacobian / covariance) per family; the state is bit-equal in every case:
  rates 9.8e-16 / 1.5e-15    rates_long_dt 1.9e-15 / 1.9e-15    long_dt 7.6e-16 / 1.6e-15    dt_mixed 3.5e-16 / 3.8e-16    tiny_dt 2.0e-16 / 2.5e-16
  bias_large 2.7e-16 / 2.9e-16    acc_big 5.2e-16 / 1.1e-15    still 1.3e-16 / 2.0e-16    gravity_only 2.5e-16 / 1.6e-16    one_axis 2.1e-16 / 2.2e-16
  turns 1.0e-15 / 1.1e-15    max 6.4e-16 / 2.5e-15
Worst 2.54e-15 (covariance, max_4096); ORACLE_BOUND = 20 x that.

Measured here, the mutants (hard cases with n <= 400 that notice, of 20; the earlier measure's worst value over the 33 earlier cases against its bound 1e-11):
  gyr_w_removed 19, earlier 9.77e-12 MISSED     gyr_w_doubled 19, earlier 9.77e-12 MISSED     acc_w_removed 19, earlier 2.5e-10 caught
  rr_normalised 13, earlier 5.0e-07 caught      f012_sixth 15, earlier 8.4e-10 caught         v09_zeroed 14, earlier 1.3e-13 MISSED
  v69_zeroed 14, earlier 1.0e-10 caught         f312_plus_dt 20, earlier 1.9e+00 caught
Which cases do not notice: tiny_dt the three noise mutants and the two V mutants (dt^2 x 1.21e-10, dt^2 x 1e-12 and dt^4-terms vanish against the 1e-4 they are
added to); still, gravity_only and the acc one_axis cases rr_normalised (no rotation: the result quaternion is exactly unit); still and the gyr one_axis cases
f012_sixth, v09_zeroed and v69_zeroed (a_1 = 0, so R_a_1_x = 0 and the changed blocks are zero either way).

Every covariance is positive definite by an exact test (rational elimination of the recorded doubles); eigvalsh's smallest eigenvalue is 3e-10 at n = 4096 and
5.6e-6 for rates_long_dt, where it is within that routine's own error (largest eigenvalue 1.4e11).
"""
import os
from fractions import Fraction

import numpy as np
import pytest

from oracle import lo_window as W
from tests import preint_hard_cases as HC
from tests import preint_model as M

ORACLE_BOUND = 20 * 2.54e-15
STRUCTURAL_ZEROS_J, STRUCTURAL_ZEROS_P = 138, 48      # what every general stream leaves exactly 0


@pytest.fixture(scope="module")
def cases():
    return HC.cases()      # (asserts the names and every case's input hash against the fixture)


def _by_family(cases, family):
    out = [c for c in cases if c["family"] == family]
    assert out, family
    return out


def test_fixture_covers_the_cases(cases):
    assert [c["name"] for c in cases] == list(HC.NAMES) and {c["family"] for c in cases} == set(HC.FAMILIES)
    assert os.path.getsize(HC.GOLDEN) < 200 * 1000
    z = np.load(HC.GOLDEN)
    assert sorted(z.files) == ["covariance", "jacobian", "names", "ns", "sha256", "state", "zero_j", "zero_p"]      # outputs and hashes: no inputs
    assert [int(n) for n in z["ns"]] == [c["n"] for c in cases]
    again = HC.generate()
    for c, g in zip(cases, again):
        assert c["dt"].shape == (c["n"],) and c["acc"].shape == (c["n"], 3) and c["gyr"].shape == (c["n"], 3)
        assert HC.input_bytes(c) == HC.input_bytes(g) and c["sha256"] == g["sha256"] and len(c["sha256"]) == 64
    assert len({c["sha256"] for c in cases}) == len(cases)
    assert {c["n"] for c in cases} >= {1, 2, 65, 129, 4095, 4096}


def test_fixture_equals_the_live_reference(cases):
    lib = M.ref_library()
    if lib is None:
        pytest.skip("oracle/_ref/libref_imu.so not built (needs the reference's sources: oracle/refshim/Makefile)")
    for c in cases:
        state, jac, cov = M.ref_preintegrate(lib, c["dt"], c["acc"], c["gyr"], c["acc0"], c["gyr0"], c["ba"], c["bg"])
        assert state.tobytes() == c["state"].tobytes(), c["name"]
        assert jac.tobytes() == c["jacobian"].tobytes() and cov.tobytes() == c["covariance"].tobytes(), c["name"]


def _exact_pivots(P):
    """the pivots of the elimination of (P + P^T) / 2 without pivoting, in rational arithmetic on the recorded doubles: all 15 positive <=> positive definite.
    (rates_long_dt has eigenvalues from 6e-6 to 1e11: eigvalsh's own error, eps x the largest, is as large as the smallest one and decides nothing there.)"""
    n = P.shape[0]
    A = [[(Fraction(float(P[i, j])) + Fraction(float(P[j, i]))) / 2 for j in range(n)] for i in range(n)]
    out = []
    for k in range(n):
        out.append(A[k][k])
        if A[k][k] <= 0:
            break
        for i in range(k + 1, n):
            f = A[i][k] / A[k][k]
            for j in range(k + 1, n):
                A[i][j] -= f * A[k][j]
    return out


def test_every_output_is_finite_and_every_covariance_positive_definite(cases):
    for c in cases:
        assert np.isfinite(c["state"]).all() and np.isfinite(c["jacobian"]).all() and np.isfinite(c["covariance"]).all(), c["name"]
        P = c["covariance"]
        piv = _exact_pivots(P)
        ev = np.linalg.eigvalsh(0.5 * (P + P.T))
        print(f"{c['name']:>16}: eigenvalues {ev.min():.3e} .. {ev.max():.3e} (eigvalsh), smallest of the 15 exact pivots {float(min(piv)):.3e}, asymmetry {np.abs(P - P.T).max():.1e}")
        assert len(piv) == 15 and min(piv) > 0, (c["name"], len(piv))


def test_every_family_has_its_property(cases):
    off = {}
    for c in cases:
        rq, dq = HC.result_quaternions(c)
        off[c["name"]] = np.abs(np.sqrt((rq * rq).sum(1)) - 1.0).max()
        flips = int((np.sign(dq[1:, 0]) != np.sign(dq[:-1, 0])).sum())
        print(f"{c['name']:>16}: result quaternion up to {off[c['name']]:.3e} off unit, delta_q.w ends at {c['state'][3]:+.3f} after {flips} changes of sign, "
              f"exact zeros {int(c['zero_j'].sum())} / {int(c['zero_p'].sum())}, largest entries {np.abs(c['jacobian']).max():.2e} / {np.abs(c['covariance']).max():.2e}")
        if c["family"] == "rates":
            assert off[c["name"]] >= 0.01 and (c["dt"] == 0.005).all()
        if c["family"] == "turns":
            assert flips >= 2 and (c["dt"] == 0.01).all() and abs(c["state"][10] - 4.0) < 1e-9
        if c["family"] in ("still", "gravity_only"):
            assert c["state"][3:7].tobytes() == np.array([1.0, 0.0, 0.0, 0.0]).tobytes()
    assert sorted(c["n"] for c in _by_family(cases, "rates")) == [1, 65, 200]
    assert _by_family(cases, "rates")[-1]["n"] == 200 and _by_family(cases, "rates")[-1]["state"][3] < 0      # delta_q.w < 0 at the end of the longest
    (c,) = _by_family(cases, "rates_long_dt")
    assert (c["dt"] == 0.02).all() and c["n"] == 100 and np.abs(c["jacobian"]).max() > 1e7 and np.abs(c["covariance"]).max() > 1e10      # large, and finite (above)
    (c,) = _by_family(cases, "long_dt")
    assert (c["dt"] == 0.1).all() and c["n"] == 60
    (c,) = _by_family(cases, "dt_mixed")
    zero = {k for k in range(c["n"]) if c["dt"][k] == 0.0}
    assert c["n"] == 129 and zero == set(range(0, 129, 7)) | {64, 65, 128} and {0, 63, 64, 65, 128} <= zero
    pos = c["dt"][c["dt"] > 0]
    assert 1e-6 <= pos.min() < 1e-5 and 0.1 <= pos.max() <= 0.5
    (c,) = _by_family(cases, "tiny_dt")
    assert (c["dt"] == 1e-6).all() and c["n"] == 65
    (c,) = _by_family(cases, "bias_large")
    assert 1.0 < np.abs(c["ba"]).max() <= 2.0 and 0.25 < np.abs(c["bg"]).max() <= 0.5 and c["n"] == 129
    (c,) = _by_family(cases, "acc_big")
    assert 50.0 < max(np.abs(c["acc"]).max(), np.abs(c["acc0"]).max()) <= 60.0 and (np.abs(c["acc"]) > 18.0).sum() > 100 and c["n"] == 129      # far past keyframe_samples' clamp
    for c in _by_family(cases, "still"):
        assert not c["acc"].any() and not c["gyr"].any() and not c["acc0"].any() and not c["gyr0"].any() and not c["ba"].any() and not c["bg"].any()
        assert int(c["zero_j"].sum()) == 198 and int(c["zero_p"].sum()) == 186
    for c in _by_family(cases, "gravity_only"):
        assert (c["acc"] == [0.0, 0.0, 9.8]).all() and (c["acc0"] == [0.0, 0.0, 9.8]).all() and not c["gyr"].any() and not c["gyr0"].any()
    six = _by_family(cases, "one_axis")
    assert len(six) == 6
    for k, c in enumerate(six):
        rows = np.concatenate([np.concatenate([c["acc0"], c["gyr0"]])[None, :], np.concatenate([c["acc"], c["gyr"]], axis=1)])
        assert c["n"] == 2 and [j for j in range(6) if rows[:, j].any()] == [k] and rows[:, k].all()
        assert int(c["zero_j"].sum()) > STRUCTURAL_ZEROS_J + 40 and int(c["zero_p"].sum()) > STRUCTURAL_ZEROS_P + 100      # many exact zeros beyond the structural ones
    assert sorted(c["n"] for c in _by_family(cases, "max")) == [4095, 4096] and all((c["dt"] == 0.0025).all() for c in _by_family(cases, "max"))
    assert max(off[c["name"]] for c in cases if c["family"] not in ("rates", "rates_long_dt", "dt_mixed", "long_dt")) < 1e-3      # the other families do not share the hazard


def test_zero_masks_are_the_recorded_ones(cases):
    structural_j = structural_p = None
    for c in cases:
        assert np.array_equal(c["zero_j"], c["jacobian"] == 0.0) and np.array_equal(c["zero_p"], c["covariance"] == 0.0), c["name"]
        assert np.array_equal(c["zero_p"], c["zero_p"].T)
        if c["family"] in ("rates_long_dt", "long_dt", "bias_large", "acc_big", "turns", "max"):      # general streams: the structural zeros and no other
            assert int(c["zero_j"].sum()) == STRUCTURAL_ZEROS_J and int(c["zero_p"].sum()) == STRUCTURAL_ZEROS_P, c["name"]
            structural_j = c["zero_j"] if structural_j is None else structural_j
            structural_p = c["zero_p"] if structural_p is None else structural_p
            assert np.array_equal(c["zero_j"], structural_j) and np.array_equal(c["zero_p"], structural_p)
    for c in cases:                                                                                  # every other case has those and more
        assert (c["zero_j"] | ~structural_j).all() and (c["zero_p"] | ~structural_p).all(), c["name"]


def test_oracle_restatement_against_the_fixture(cases):
    worst = {}
    for c in cases:
        pre = W.Preintegration(c["acc0"], c["gyr0"], c["ba"], c["bg"])
        for k in range(c["n"]):
            pre.push_back(c["dt"][k], c["acc"][k], c["gyr"][k])
        mine = np.concatenate([pre.delta_p, pre.delta_q, pre.delta_v, [pre.sum_dt]])
        ds = np.abs(mine - c["state"]).max()
        rel = []
        for got, ref in ((pre.jacobian, c["jacobian"]), (pre.covariance, c["covariance"])):
            d, bm = np.abs(got - ref), HC.block_max(ref)
            assert not d[bm == 0.0].any(), c["name"]                                                # a block the reference leaves all zero is all zero
            rel.append((d[bm > 0] / bm[bm > 0]).max())
        w = worst.setdefault(c["family"], [0.0, 0.0, 0.0])
        worst[c["family"]] = [max(w[0], ds), max(w[1], rel[0]), max(w[2], rel[1])]
        assert ds < 1e-13, (c["name"], ds)
        assert rel[0] <= ORACLE_BOUND and rel[1] <= ORACLE_BOUND, (c["name"], rel)
    for f, w in worst.items():
        print(f"oracle against the fixture, {f:>14}: state {w[0]:.3e}  jacobian {w[1]:.3e}  covariance {w[2]:.3e} of the block's largest entry")
    print(f"worst {max(max(w[1], w[2]) for w in worst.values()):.3e}; bound {ORACLE_BOUND:.3e}")


# ---------------------------------------------------------------- sensitivity of the comparison
@pytest.fixture(scope="module")
def earlier():
    """the 33 earlier cases as (stream case, snapshot counts): a seed's cases are prefixes of one stream, with dt[0] = 0 from n = 40 on"""
    old = M.golden_cases()
    runs = []
    for seed in M.SEEDS:
        mine = {c["n"]: c for c in old if c["seed"] == seed}
        for ns in ([n for n in M.NS if n < 40], [n for n in M.NS if n >= 40]):
            runs.append((mine[max(ns)], [(n, mine[n]) for n in ns]))
    return runs


def _earlier_measure(earlier, mutant):
    worst = 0.0
    for stream, snaps in earlier:
        got = HC.restate(stream, mutant, snapshots=tuple(n for n, _ in snaps))
        for n, ref in snaps:
            st, J, P = got[n]
            if mutant is None:
                assert HC.equal(HC.compare(st, J, P, ref)), (ref["seed"], n)
            worst = max(worst, HC.old_measure(J, P, ref))
    return worst


def test_unmutated_restatement_equals_both_fixtures(cases, earlier):
    """the restatement the mutants are applied to passes the device's comparison on every hard case and every earlier one"""
    for c in cases:
        r = HC.compare(*HC.restate(c), c)
        print(HC.line(c["name"], r))
        assert HC.equal(r), c["name"]
    assert _earlier_measure(earlier, None) == 0.0


@pytest.mark.parametrize("mutant", HC.MUTANTS)
def test_comparison_notices(mutant, cases, earlier):
    caught, missed = [], []
    for c in cases:
        if c["n"] > 400:      # (the two n >= 4095 cases add nothing a shorter stream does not show, and two seconds of Python each)
            continue
        r = HC.compare(*HC.restate(c, mutant), c)
        (missed if HC.equal(r) else caught).append(c["name"])
    old = _earlier_measure(earlier, mutant)
    print(f"{mutant:>14}: noticed by the entry-wise comparison in {len(caught)} of {len(caught) + len(missed)} hard cases (not in {missed}); the earlier measure's worst value on the "
          f"33 earlier cases {old:.3e}: {'caught' if old > 1e-11 else 'MISSED'} by its bound 1e-11")
    assert caught, mutant
