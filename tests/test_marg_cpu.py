"""CPU side of the window's next prior (tests/test_marg_gpu.py holds the device side): the conditions on the inputs of those tests, checked on the oracle alone,
the referee's own assembly on a problem small enough to do by hand, and the ctypes mirror of lili_window_prior_storage against the header.

Input conditions.  MarginalizationInfo's threshold eps = 1e-8 is ABSOLUTE; a comparison between two eigen-solvers means something only where no eigenvalue
lies near it, so that the threshold decides nothing by rounding: on the harness windows every eigenvalue of Amm and of the Schur complement is >= 200
(measured, the reference's factor set at the oracle's 15-iteration solution: Amm 9.98e3 .. 4.73e7 for every n_kf; S 439 .. 4.88e7 (n_kf = 3), 225 .. 4.88e7
(4), 214 .. 4.70e7 (2); second marginalisation of the chain: Amm 1.04e4 .. 2.34e8, S 404 .. 2.42e8), on the synthetic systems every eigenvalue is >= 1e-3 or
<= 1e-12 in magnitude."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import lili_om_amd as L
from oracle import lo_window as W
from tests import marg_harness as MH
from tests import test_window_solve_gpu as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("m,n,special", MH.SCHUR_CASES)
def test_synthetic_systems_keep_clear_of_the_threshold(m, n, special):
    A, b = MH.schur_case(m, n, special)
    rest = A.copy()
    if special == "repeated eigenvalue":                          # the 225 I block the case is about, and O(1) everywhere else
        assert np.allclose(A[m + 12:m + 21, m + 12:m + 21], 225.0 * np.eye(9))
        rest[m + 12:m + 21, m + 12:m + 21] = 0.0
    assert 0.1 < np.abs(rest).max() < 10
    w_mm, w_s = MH.spectra(A, m)
    for w in (w_mm, w_s):
        assert ((w >= 1e-3) | (np.abs(w) <= 1e-12)).all(), (special, w)
    n_zero_mm, n_zero_s = int((np.abs(w_mm) <= 1e-12).sum()), int((np.abs(w_s) <= 1e-12).sum())
    assert n_zero_mm == (1 if special == "singular Amm" else 0)
    assert n_zero_s == (1 if special == "rank-deficient S" else 0)
    if special == "repeated eigenvalue":
        assert int((np.abs(w_s - 225.0) <= 1e-10).sum()) == 9


@pytest.mark.parametrize("n_kf", [3, 4, 2])
def test_harness_windows_keep_clear_of_the_threshold(n_kf):
    _, _, _, sol, pb, M, kept, A, b, m = MH.first_marginalisation(n_kf)
    assert m == 15 and A.shape[0] - m == {2: 15, 3: 21, 4: 36}[n_kf]
    w_mm, w_s = MH.spectra(A, m)
    print(f"n_kf {n_kf}: Amm eigenvalues {w_mm.min():.3g} .. {w_mm.max():.3g}, S eigenvalues {w_s.min():.3g} .. {w_s.max():.3g}")
    assert w_mm.min() >= 200 and w_s.min() >= 200
    # with the reference's set the newest keyframe's speed-bias is touched by nothing (n_kf >= 3)
    assert (f"sb{n_kf - 1}" in kept) == (n_kf == 2)
    # the speed-bias priors sit at their own mean: residual 0, information 225 I (L:1045-1057)
    for fn, names, _ in pb.blocks:
        if names == ["sb0"]:
            r, Js = fn(sol["sb0"])
            assert not r.any() and np.array_equal(Js[0].T @ Js[0], 225.0 * np.eye(9))


def test_second_marginalisation_keeps_clear_of_the_threshold():
    _, _, _, sol2, pb, M, kept, A, b, m = MH.second_marginalisation()
    assert m == 15 and A.shape[0] - m == 21 and kept == ["t1", "q1", "sb1", "t2", "q2"]
    w_mm, w_s = MH.spectra(A, m)
    print(f"second marginalisation: Amm eigenvalues {w_mm.min():.3g} .. {w_mm.max():.3g}, S eigenvalues {w_s.min():.3g} .. {w_s.max():.3g}")
    assert w_mm.min() >= 200 and w_s.min() >= 200


def test_chain_solves_are_decided_clear_of_their_thresholds():
    """DESIGN.md §7h's condition for a comparison of decision sequences, on the oracle's log of both solves of the chain"""
    _, _, _, _, info1, log1 = MH.solved(3)
    S._stable(log1, info1)
    _, info2, log2 = MH.second_solved()
    S._stable(log2, info2)
    for e in log1 + log2:
        assert not (0.9e-3 <= e["rho"] <= 1.1e-3)


def test_referee_factor_set_on_a_hand_made_problem():
    """two residual blocks, done by hand: a block on (t0, q0, t1) and one on (q1); sb0, sb1 and t2 are touched by nothing and are no dimensions;
    quaternion blocks enter by the last three of their four global columns"""
    rng = np.random.default_rng(3)
    Ja, Jq, Jb, Jq1 = rng.normal(size=(4, 3)), rng.normal(size=(4, 4)), rng.normal(size=(4, 3)), rng.normal(size=(2, 4))
    ra, rb = rng.normal(size=4), rng.normal(size=2)
    pb = W.Problem()
    vals = {}
    for k in range(3):
        for nm, v, quat in ((f"t{k}", rng.normal(size=3), False), (f"q{k}", np.array([1.0, 0, 0, 0]), True), (f"sb{k}", rng.normal(size=9), False)):
            pb.add_parameter(nm, v, quat=quat)
            vals[nm] = pb.params[nm]
    pb.add_residual(lambda t0, q0, t1: (ra, [Ja, Jq, Jb]), ["t0", "q0", "t1"])
    pb.add_residual(lambda q1: (rb, [Jq1]), ["q1"])
    M, kept, A, b, m = MH.referee(pb, vals)
    assert kept == ["t1", "q1"] and m == 6 and A.shape == (12, 12)
    Jh = np.zeros((6, 12))
    Jh[:4, 0:3], Jh[:4, 3:6], Jh[:4, 6:9], Jh[4:, 9:12] = Ja, Jq[:, 1:4], Jb, Jq1[:, 1:4]
    rh = np.concatenate([ra, rb])
    assert np.allclose(A, Jh.T @ Jh, rtol=0, atol=1e-14) and np.allclose(b, Jh.T @ rh, rtol=0, atol=1e-14)
    assert MH.shifted(kept) == ["t0", "q0"]
    # and the referee's prior is the marginal of that quadratic: S = Arr - Arm Amm^-1 Amr by a linear solve
    Ss = A[6:, 6:] - A[6:, :6] @ np.linalg.solve(A[:6, :6], A[:6, 6:])
    LJ = M.linearized_jacobians
    assert np.abs(LJ.T @ LJ - Ss).max() <= 1e-12 * np.abs(Ss).max()


def test_prior_storage_mirror_matches_the_header(tmp_path):
    T = L.api.WindowPriorStorage
    lines, expect = ['printf("%zu\\n", sizeof(lili_window_prior_storage));', 'printf("%zu\\n", sizeof(lili_window_prior));'], [C.sizeof(T), C.sizeof(L.api.WindowPrior)]
    for cname, U in (("lili_window_prior_storage", T), ("lili_window_prior", L.api.WindowPrior)):
        for fname, _ in U._fields_:
            lines.append(f'printf("%zu\\n", offsetof({cname}, {fname}));')
            expect.append(getattr(U, fname).offset)
    lines.append('printf("%d %d\\n", 3 * LILI_WINDOW_MAX_KF, 15 * LILI_WINDOW_MAX_KF);')
    src = tmp_path / "lay_marg.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "lili_hip.h"\nint main(void){' + "".join(lines) + "return 0;}")
    exe = tmp_path / "lay_marg"
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    assert got[:-2] == expect, [(i, a, b) for i, (a, b) in enumerate(zip(got, expect)) if a != b]
    assert got[-2] == len(T().block_kind) == len(T().block_keyframe) and got[-1] == len(T().r0) and got[-1] ** 2 == len(T().J0)
    assert {"lili_marg_schur", "lili_window_marginalize"} <= set(L.api.exported_symbols())
