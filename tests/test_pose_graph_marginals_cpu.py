"""The referee of the pose graph's marginal covariances (tests/pose_graph_marginals_model.py), the host function lili_pose_relative_covariance and the new struct's
layout, without a GPU:
  routes       the model's routes agree on every designed case to 1e-9 of each block's largest entry (D0; measured at the model's solutions: 0 .. 8e-15 at N <= 3,
               8e-13 .. 4e-12 at N = 200 .. 260, 8e-12 .. 4e-11 at N = 511 .. 592 by the three routes, 6e-11 .. 1.2e-10 at chain_1025 and circuit_2048 by the two sparse
               orders on the designed node subset) — the referee is usable;
  chains       a referee with no inverse in it: the forward recursion of the chain's own covariance, diagonal and adjacent cross blocks, within
               max(10 D0, 64 eps) per block (measured 4.1e-12 on chain_511, 3.1e-12 on chain_513, 4e-16 on n2);
  further      the prior alone gives diag(prior_var); on a zero-residual chain the relative covariance of neighbours is diag(odom_var); the host function against
               the model on 50 random pose pairs with random SPD inputs; its argument errors leave the output untouched; the struct mirror against the header."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import lili_om_amd as L
from lili_om_amd import api
from lili_om_amd import pose_graph as PG
from tests import pose_graph_cases as Cs
from tests import pose_graph_marginals_model as MM
from tests import pose_graph_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = [c for c in Cs.solve_cases() if c["expect"] is None]
IDS = [c["name"] for c in CASES]
BY = {c["name"]: c for c in CASES}
INFO, RELATIVE = api.PgMarginalsInfo, PG.relative_covariance      # what this file is about: the binding's mirror of the new struct and the library's host function


def _referee(c):
    """at the model's own solution of the case (pose_graph_cases.reference, shared with the solve tests)"""
    g, X, _, _ = Cs.reference(c)
    nodes, pairs = MM.case_nodes(c), MM.case_pairs(c)
    return (g, X, nodes, pairs) + MM.referee("cpu:" + c["name"], g, X, nodes, pairs)


@pytest.mark.parametrize("c", CASES, ids=IDS)
def test_routes_agree(c):
    g, X, nodes, pairs, cov, cross, d0, routes = _referee(c)
    print(f"marginals model [{c['name']}] N {g.n} loops {len(g.loops)}: {len(nodes)} nodes, {len(pairs)} pairs, routes {routes}, D0 {d0:.2e}")
    assert len(routes) >= 2
    assert np.isfinite(cov).all() and np.isfinite(cross).all()
    assert d0 <= 1e-9


@pytest.mark.parametrize("name", ["n2", "chain_511", "chain_513"])
def test_chain_recursion_agrees(name):
    g, X, nodes, pairs, cov, cross, d0, _ = _referee(BY[name])
    D, Cx = MM.chain_recursion(g, X)
    adj = [(k - 1, k) for k in range(1, g.n)]
    _, cross_adj = MM.marginals(g, X, [], adj, "inv")
    e_d, e_x = MM.block_error(cov, D[nodes]), MM.block_error(cross_adj, Cx)
    print(f"chain recursion [{name}]: diagonal {e_d:.2e} adjacent cross {e_x:.2e} (D0 {d0:.2e}, bound {MM.tolerance(d0):.2e})")
    assert e_d <= MM.tolerance(d0) and e_x <= MM.tolerance(d0)


def test_prior_only_is_the_prior():
    g, X, nodes, pairs, cov, cross, d0, _ = _referee(BY["n1_prior_only"])
    assert cov.shape == (1, 6, 6)
    assert np.abs(cov[0] - np.diag(M.PRIOR_VAR)).max() <= 64 * MM.EPS * M.PRIOR_VAR.max()


def test_relative_covariance_of_neighbours_is_the_odometry_variance():
    _, given = Cs.circuit(40, 5)
    g = M.Graph()
    g.append(None, given)      # estimates = the given poses: every chain residual is zero
    adj = [(k, k + 1) for k in range(g.n - 1)]
    cov, cross = MM.marginals(g, g.X, range(g.n), adj, "inv")
    for k, (i, j) in enumerate(adj):
        for rel in (MM.relative_covariance(g.X[i], g.X[j], cov[i], cov[j], cross[k]), RELATIVE(g.X[i], g.X[j], cov[i], cov[j], cross[k])):
            assert np.abs(rel - np.diag(M.ODOM_VAR)).max() <= 1e-9 * M.ODOM_VAR.max(), (i, rel)


def test_host_relative_covariance_matches_model():
    rng = np.random.default_rng(11)
    worst = 0.0
    for _ in range(50):
        A = M.normalize_poses(np.concatenate([rng.normal(0, 20.0, 3), rng.normal(size=4)]))[0]
        B = M.normalize_poses(np.concatenate([rng.normal(0, 20.0, 3), rng.normal(size=4)]))[0]
        Q = rng.normal(size=(12, 12)) * np.exp(rng.normal(0, 2.0, 12))[:, None]
        Sg = Q @ Q.T
        got = RELATIVE(A, B, Sg[:6, :6], Sg[6:, 6:], Sg[:6, 6:])
        want = MM.relative_covariance(A, B, Sg[:6, :6], Sg[6:, 6:], Sg[:6, 6:])
        worst = max(worst, float(np.abs(got - want).max() / np.abs(want).max()))
    print(f"lili_pose_relative_covariance - model: {worst:.2e} of the block's largest entry")
    assert worst <= 1e-13


def test_host_relative_covariance_argument_errors():
    lib, ptr = L.load_library(), api._ptr
    A, B = M.IDENTITY.copy(), np.array([1.0, 2.0, 3.0, 1.0, 0.0, 0.0, 0.0])
    I6 = np.eye(6)
    out = np.full((6, 6), 7.25)

    def call(a=A, b=B, sii=I6, sjj=I6, sij=I6, o=out):
        return lib.lili_pose_relative_covariance(ptr(a), ptr(b), ptr(sii), ptr(sjj), ptr(sij), ptr(o))

    assert call(a=None) == -1 and call(b=None) == -1 and call(sii=None) == -1 and call(sjj=None) == -1 and call(sij=None) == -1 and call(o=None) == -1
    bad = B.copy(); bad[1] = np.nan
    assert call(b=bad) == -1
    bad = I6.copy(); bad[2, 3] = np.inf
    assert call(sii=bad) == -1 and call(sjj=bad) == -1 and call(sij=bad) == -1
    bad = A.copy(); bad[3] = 1.0 + 1e-5
    assert call(a=bad) == -1
    bad = B.copy(); bad[3:7] = 0.0
    assert call(b=bad) == -1
    assert (out == 7.25).all()
    near = A.copy(); near[3] = 1.0 + 5e-7      # within 1e-6: accepted, normalised
    assert call(a=near) == 0 and np.isfinite(out).all() and not (out == 7.25).any()


def test_marginals_info_mirror_matches_the_header(tmp_path):
    """size and every field offset of lili_pg_marginals_info against the header compiled as plain C"""
    T = INFO
    lines, expect = ['printf("%zu\\n", sizeof(lili_pg_marginals_info));'], [C.sizeof(T)]
    for fname, _ in T._fields_:
        lines.append(f'printf("%zu\\n", offsetof(lili_pg_marginals_info, {fname}));')
        expect.append(getattr(T, fname).offset)
    lines.append('printf("%d\\n", LILI_PG_MAX_PAIRS);')
    expect.append(api.PG_MAX_PAIRS)
    src = tmp_path / "lay_marg.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "lili_hip.h"\nint main(void){' + "".join(lines) + "return 0;}")
    exe = tmp_path / "lay_marg"
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    assert got == expect, (got, expect)
    assert [f for f, _ in T._fields_] == ["status", "n_nodes", "n_loops", "reduced_unknowns", "kernel_ms", "reserved_"]
