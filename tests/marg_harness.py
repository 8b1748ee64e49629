"""Shared by tests/test_marg_cpu.py and tests/test_marg_gpu.py: the referee of the window's next prior (lili_marg_schur, lili_window_marginalize).

The referee is oracle/lo_window.py::Marginalization (numpy eigh, i.e. LAPACK: independent of the device's Jacobi) on A, b from the last-three-columns
assembly `last3_system` of tests/test_window_solve_gpu.py over an oracle Problem that holds exactly the reference's factor set
(L/src/BackendFusion.cpp:1009-1165): the old prior if there is one, the speed-bias priors, the IMU factor between keyframes 0 and 1 ONLY, the lidar blocks
of every keyframe.  Blocks no factor touches are no dimensions of the system (MarginalizationInfo knows only the blocks its factors name).

J0 and r0 are unique only up to an orthogonal transform of the rows, so everything is compared through J0^T J0, J0^T r0, r0^T r0, the rank, "rows beyond the
rank are exactly zero" and the orthogonality of the rows; differences are relative to the largest entry of the referee's quantity."""
import functools

import numpy as np

from oracle import lo_window as W
from tests import test_window_solve_gpu as S

EPS = W.Marginalization.EPS
SIZES = {"t": 3, "q": 3, "sb": 9}
KINDS = {"t": 0, "q": 1, "sb": 2}


# ---------------------------------------------------------------- synthetic systems for lili_marg_schur
SCHUR_CASES = [(1, 1, None), (3, 3, None), (15, 21, "singular Amm"), (15, 30, "rank-deficient S"), (15, 45, "repeated eigenvalue")]


def schur_case(m, n, special, seed=0):
    """A = J^T J, b = J^T r with J of 3 pos rows, entries N(0, 1 / rows): A is O(1) and its smallest eigenvalue is about (sqrt(3) - 1)^2 / 3 = 0.18.
    singular Amm: a dropped column of J is zero; rank-deficient S: a kept column is zero; repeated eigenvalue: nine kept columns carry a 15 I block and
    nothing else (S then holds a 225 I block)."""
    pos = m + n
    rng = np.random.default_rng(1000 * m + n + seed)
    rows = 3 * pos
    J = rng.normal(0.0, 1.0 / np.sqrt(rows), (rows, pos))
    r = rng.normal(0.0, 1.0, rows)
    if special == "singular Amm":
        J[:, 4] = 0.0
    elif special == "rank-deficient S":
        J[:, m + 7] = 0.0
    elif special == "repeated eigenvalue":
        J[:, m + 12:m + 21] = 0.0
        J = np.vstack([J, np.zeros((9, pos))])
        J[rows:, m + 12:m + 21] = 15.0 * np.eye(9)
        r = np.concatenate([r, rng.normal(0.0, 0.1, 9)])
    return J.T @ J, J.T @ r


def spectra(A, m):
    """numpy's eigenvalues of Amm and of the Schur complement as the referee forms it"""
    A = np.asarray(A, np.float64)
    Amm = 0.5 * (A[:m, :m] + A[:m, :m].T)
    w, V = np.linalg.eigh(Amm)
    inv = V @ np.diag(np.where(w > EPS, 1.0 / np.where(w > EPS, w, 1.0), 0.0)) @ V.T
    return w, np.linalg.eigvalsh(A[m:, m:] - A[m:, :m] @ inv @ A[:m, m:])


# ---------------------------------------------------------------- the compared quantities
def compare_prior(J0, r0, rank, M, bounds, what):
    """device (J0, r0, rank) against the referee M (W.Marginalization); bounds = (J0^T J0, J0^T r0, r0^T r0, row orthogonality), each quantity against its own;
    returns the four relative differences"""
    LJ, LR = M.linearized_jacobians, M.linearized_residuals
    n = LJ.shape[0]
    assert J0.shape == (n, n) and r0.shape == (n,)
    rank_o = int((np.abs(LJ).max(axis=1) > 0).sum())
    So, bo, co = LJ.T @ LJ, LJ.T @ LR, float(LR @ LR)
    d_s = np.abs(J0.T @ J0 - So).max() / np.abs(So).max()
    d_b = np.abs(J0.T @ r0 - bo).max() / max(np.abs(bo).max(), np.finfo(float).tiny)
    d_c = abs(float(r0 @ r0) - co) / max(co, np.finfo(float).tiny)
    G = J0 @ J0.T
    d_o = np.abs(G - np.diag(np.diag(G))).max() / np.diag(G).max()
    zero_rows = int((np.abs(J0).max(axis=1) == 0).sum())
    print(f"prior [{what}]: n {n} rank {rank} (referee {rank_o})  d_JtJ {d_s:.3e}  d_Jtr {d_b:.3e}  d_rtr {d_c:.3e}  row orthogonality {d_o:.3e}")
    assert rank == rank_o, (what, rank, rank_o)
    assert zero_rows == n - rank, (what, zero_rows, n, rank)
    for i in range(n):
        if not J0[i].any():
            assert r0[i] == 0.0, (what, i)
    assert np.isfinite(J0).all() and np.isfinite(r0).all()
    got = (d_s, d_b, d_c, d_o)
    assert all(g <= bd for g, bd in zip(got, bounds)), (what, got, bounds)
    return got


# ---------------------------------------------------------------- the reference's factor set at a state
def marg_problem(win, lidar_block, values, old=None, sb_prior_kfs=()):
    """oracle Problem with the factor set of L:1009-1165 over the window `win`, parameters = `values` (dict t0, q0, sb0, ...):
    old = (Marginalization, names) or None; speed-bias priors on sb_prior_kfs with mean = the value itself (L:1045-1057: residual 0, information 225 I);
    the IMU factor between keyframes 0 and 1; the lidar blocks of every keyframe."""
    n = len(win["kfs"])
    pb = W.Problem()
    for k in range(n):
        pb.add_parameter(f"t{k}", values[f"t{k}"])
        pb.add_parameter(f"q{k}", values[f"q{k}"], quat=True)
        pb.add_parameter(f"sb{k}", values[f"sb{k}"])
    if old is not None:
        pb.add_residual(old[0].factor(), old[1])
    for k in sb_prior_kfs:
        mean = np.array(values[f"sb{k}"], np.float64)
        pb.add_residual(lambda sb, mean=mean: W.speed_bias_prior(mean, sb), [f"sb{k}"])
    pre = win["pres"][0]["pre"]
    pb.add_residual(lambda ti, qi, sbi, tj, qj, sbj, pre=pre: W.imu_factor(pre, ti, qi, sbi, tj, qj, sbj), ["t0", "q0", "sb0", "t1", "q1", "sb1"])
    if lidar_block is not None:
        for k in range(n):
            pb.add_residual(lidar_block(k), [f"t{k}", f"q{k}"])
    return pb


def referee(pb, values):
    """(Marginalization, kept names, A, b, m): keyframe 0's touched blocks dropped, the other touched blocks kept in (keyframe, kind) order"""
    A, b = S.last3_system(pb, values)
    touched = set(nm for _, names, _ in pb.blocks for nm in names)
    sizes = pb.local_sizes()
    offs = dict(zip(pb.order, np.concatenate([[0], np.cumsum(sizes)[:-1]]).astype(int)))
    names = [nm for nm in pb.order if nm in touched]               # pb.order is (keyframe, kind) order, keyframe 0 first
    dropped = [nm for nm in names if nm.endswith("0") and nm[:-1] in SIZES]
    kept = [nm for nm in names if nm not in dropped]
    sel = np.concatenate([np.arange(offs[nm], offs[nm] + (3 if pb.kind[nm] else len(pb.params[nm]))) for nm in dropped + kept])
    m = int(sum(3 if pb.kind[nm] else len(pb.params[nm]) for nm in dropped))
    A, b = A[np.ix_(sel, sel)], b[sel]
    M = W.Marginalization(A, b, m, [(nm, values[nm], bool(pb.kind[nm])) for nm in kept])
    return M, kept, A, b, m


def shifted(names):
    """kept names in the NEXT window's numbering (addr_shift, L:1170-1177)"""
    return [f"{nm.rstrip('0123456789')}{int(nm[len(nm.rstrip('0123456789')):]) - 1}" for nm in names]


def prior_dict(M, kept):
    """the referee's prior in the form WindowSolver.set_problem(prior=...) takes, in the next window's numbering"""
    nm = shifted(kept)
    return dict(block_kind=[KINDS[x.rstrip("0123456789")] for x in nm], block_keyframe=[int(x[len(x.rstrip("0123456789")):]) for x in nm],
                x0=[v for _, v, _ in M.kept], J0=M.linearized_jacobians, r0=M.linearized_residuals)


def check_blocks(prior, kept, state):
    """the device's block list: kinds, shifted keyframes, x0 = the block's bytes in `state`"""
    nm = shifted(kept)
    assert prior["block_kind"] == [KINDS[x.rstrip("0123456789")] for x in nm], (prior["block_kind"], nm)
    assert prior["block_keyframe"] == [int(x[len(x.rstrip("0123456789")):]) for x in nm], (prior["block_keyframe"], nm)
    state = np.asarray(state, np.float64)
    for x, name in zip(prior["x0"], kept):
        kind, k = name.rstrip("0123456789"), int(name[len(name.rstrip("0123456789")):])
        sl = {"t": slice(0, 3), "q": slice(3, 7), "sb": slice(7, 16)}[kind]
        assert np.asarray(x, np.float64).tobytes() == state[k, sl].tobytes(), name


# ---------------------------------------------------------------- the harness windows (oracle only; computed once per session)
@functools.lru_cache(maxsize=None)
def win4():
    return S.make_window_n(4)


@functools.lru_cache(maxsize=None)
def oracle_lib():
    from oracle import oracle as O
    O.build()
    O.lib()
    return O


@functools.lru_cache(maxsize=None)
def solved(n_kf):
    """keyframes 0 .. n_kf - 1 of make_window_n(4), the speed-bias branch, at the oracle's 15-iteration solution:
    (window, oracle records, lidar block, solution values, ceres_lm's info, its log)"""
    win = S.cut(win4(), 0, n_kf)
    recs, block = S.oracle_side(oracle_lib(), win)
    log = []
    sol, info = W.ceres_lm(S.build_problem(win, block), max_num_iterations=15, log=log)
    return win, recs, block, sol, info, log


def first_marginalisation(n_kf):
    """the referee's first prior of a chain: speed-bias priors on keyframes 0 .. n_kf - 2 with mean = the solution (L:1033-1063)"""
    win, recs, block, sol, _, _ = solved(n_kf)
    pb = marg_problem(win, block, sol, sb_prior_kfs=range(n_kf - 1))
    return (win, recs, block, sol, pb) + referee(pb, sol)


@functools.lru_cache(maxsize=None)
def second_window():
    """keyframes 1 .. 3 with the referee's first prior (from keyframes 0 .. 2), keyframes 1 and 2 started a few cm off the linearisation point as
    tests/test_window_solve_gpu.py does: (window, oracle records, lidar block, solve problem, names of the prior's blocks, referee prior, kept names)"""
    _, _, _, sol1, _, M1, kept1, _, _, _ = first_marginalisation(3)
    nxt = S.cut(win4(), 1, 4)
    rng = np.random.default_rng(77)
    for k in (0, 1):
        nxt["init"][k] = dict(t=sol1[f"t{k + 1}"] + rng.normal(0, 0.02, 3), q=W.quat_plus(sol1[f"q{k + 1}"], rng.normal(0, 0.003, 3)),
                              sb=sol1[f"sb{k + 1}"] + np.concatenate([rng.normal(0, 0.02, 3), rng.normal(0, 0.001, 3), rng.normal(0, 0.0002, 3)]))
    recs, block = S.oracle_side(oracle_lib(), nxt)
    names = shifted(kept1)
    pb2 = S.build_problem(nxt, block, marg=(M1, names))
    return nxt, recs, block, pb2, names, M1, kept1


@functools.lru_cache(maxsize=None)
def second_solved():
    nxt, recs, block, pb2, names, M1, kept1 = second_window()
    log = []
    sol2, info2 = W.ceres_lm(pb2, max_num_iterations=15, log=log)
    return sol2, info2, log


def second_marginalisation():
    """the second marginalisation of the chain: the old prior, no speed-bias priors (`marg` is already true), IMU (0, 1), lidar of all three"""
    nxt, recs, block, pb2, names, M1, kept1 = second_window()
    sol2, _, _ = second_solved()
    pb = marg_problem(nxt, block, sol2, old=(M1, names))
    return (nxt, recs, block, sol2, pb) + referee(pb, sol2)
