"""Referee of the pose graph's marginal covariances (include/lili_hip.h: lili_pose_graph_marginals, lili_pose_relative_covariance; DESIGN.md §7k "Marginal
covariances"), numpy / scipy on top of tests/pose_graph_model.py.

Sigma = H^-1 with H = J^T J from Graph.jacobian at the estimates X.  Routes:
  inv          numpy.linalg.inv of the dense H;
  chol         scipy.linalg.cho_factor / cho_solve of the dense H against the identity;
  lu           scipy.sparse.linalg.splu (COLAMD order), solving only the unit columns of the requested nodes: the only route above DENSE_MAX_NODES nodes;
  lu_mmd       the same in the minimum-degree order of H + H^T: the second elimination order where the dense routes do not fit.  (The natural order, which
               pose_graph_cases.second_solver uses for the solve, fills in forty times as much on the graphs with many loops: 40 s of column solves on loops_200.)
D0(case) = the largest difference between any two available routes over the requested blocks, relative to each block's largest entry: the yardstick of the
device's tolerance, max(10 D0, 64 eps) per block.

The chains have a referee with no inverse in it (chain_recursion).  The pair and node lists of the device tests are built here, and every referee is computed once
per session (referee)."""
import numpy as np
import scipy.linalg as sla
import scipy.sparse as sp
import scipy.sparse.linalg as spla

from tests import pose_graph_model as M

EPS = np.finfo(np.float64).eps
DENSE_MAX_NODES = 700
S = 512      # LILI_PG_SEGMENT


def information(graph, X):
    _, J = graph.jacobian(np.asarray(X, np.float64))
    return (J.T @ J).tocsc()


def _columns(lu, n6, ids, chunk=8):
    """{node: the 6 columns of H^-1 that belong to it (6 N x 6)} through a sparse factorisation, a few nodes at a time"""
    out = {}
    ids = sorted(set(int(i) for i in ids))
    for s in range(0, len(ids), chunk):
        part = ids[s:s + chunk]
        E = np.zeros((n6, 6 * len(part)))
        for k, i in enumerate(part):
            E[6 * i:6 * i + 6, 6 * k:6 * k + 6] = np.eye(6)
        Z = lu.solve(E)
        for k, i in enumerate(part):
            out[i] = Z[:, 6 * k:6 * k + 6].copy()
    return out


def marginals(graph, X, nodes, pairs, route):
    """-> cov (len(nodes), 6, 6): Sigma(i, i); cross (len(pairs), 6, 6): Sigma(i, j), rows: node i"""
    H = information(graph, X)
    nodes = [int(i) for i in nodes]
    pairs = [(int(i), int(j)) for i, j in pairs]
    n6 = H.shape[0]
    if route in ("inv", "chol"):
        Hd = H.toarray()
        Sg = np.linalg.inv(Hd) if route == "inv" else sla.cho_solve(sla.cho_factor(Hd, lower=True), np.eye(n6))
        blk = lambda i, j: Sg[6 * i:6 * i + 6, 6 * j:6 * j + 6]
    elif route in ("lu", "lu_mmd"):
        lu = spla.splu(H, permc_spec="COLAMD" if route == "lu" else "MMD_AT_PLUS_A")
        cols = _columns(lu, n6, nodes + [j for _, j in pairs])
        blk = lambda i, j: cols[j][6 * i:6 * i + 6, :]
    else:
        raise ValueError(route)
    cov = np.array([blk(i, i) for i in nodes]).reshape(-1, 6, 6)
    cross = np.array([blk(i, j) for i, j in pairs]).reshape(-1, 6, 6)
    return cov, cross


def routes_for(n_nodes):
    return ("inv", "chol", "lu") if n_nodes <= DENSE_MAX_NODES else ("lu", "lu_mmd")


def block_error(A, B):
    """largest |A - B| of a block relative to B's largest entry, over the blocks"""
    A, B = np.asarray(A).reshape(-1, 36), np.asarray(B).reshape(-1, 36)
    if A.shape[0] == 0:
        return 0.0
    return float(np.max(np.abs(A - B).max(axis=1) / np.abs(B).max(axis=1)))


def spread(results):
    """D0: the largest pairwise block_error over a list of (cov, cross) results"""
    d = 0.0
    for a in range(len(results)):
        for b in range(len(results)):
            if a != b:
                d = max(d, block_error(results[a][0], results[b][0]), block_error(results[a][1], results[b][1]))
    return d


def tolerance(d0):
    return max(10.0 * d0, 64.0 * EPS)


def relative_covariance(pose_i, pose_j, cov_ii, cov_jj, cov_ij):
    """first-order covariance of between(X_i, X_j) in its own tangent, from the between-factor's Jacobians at Z = between(X_i, X_j)"""
    A, B = M.normalize_poses(pose_i)[0], M.normalize_poses(pose_j)[0]
    _, Ja, Jb = M.factor_jacobians(A, B, M.between(A, B))
    cii, cjj, cij = (np.asarray(v, np.float64).reshape(6, 6) for v in (cov_ii, cov_jj, cov_ij))
    return Ja @ cii @ Ja.T + Ja @ cij @ Jb.T + Jb @ cij.T @ Ja.T + Jb @ cjj @ Jb.T


def chain_recursion(graph, X):
    """A chain's marginals without an inverse of H: Sigma_0 = Jb0^-1 diag(prior_var) Jb0^-T, Sigma_k = A Sigma_(k-1) A^T + Jb^-1 diag(odom_var) Jb^-T with
    A = -Jb^-1 Ja of the unweighted chain factor (k - 1, k).  -> diagonal blocks (N, 6, 6), cross blocks Sigma(k - 1, k) = Sigma_(k-1) A^T (N - 1, 6, 6)"""
    assert not graph.loops
    X = np.asarray(X, np.float64)
    A_, B_, Z_, _, _, _ = graph.factors(X)
    _, Ja, Jb = M.factor_jacobians(A_, B_, Z_)
    n = graph.n
    D, Cx = np.zeros((n, 6, 6)), np.zeros((max(n - 1, 0), 6, 6))
    Jbi = np.linalg.inv(Jb[0])
    D[0] = Jbi @ np.diag(graph.prior_var) @ Jbi.T
    for k in range(1, n):
        Jbi = np.linalg.inv(Jb[k])
        A = -Jbi @ Ja[k]
        Cx[k - 1] = D[k - 1] @ A.T
        D[k] = A @ D[k - 1] @ A.T + Jbi @ np.diag(graph.odom_var) @ Jbi.T
    return D, Cx


# ---- what the device tests ask for --------------------------------------------------------------------------------
def separators(case):
    n = case["poses"].shape[0]
    ids = set(range(0, n, S))
    for a, b, _, _ in case["loops"]:
        ids.add(int(a)); ids.add(int(b))
    return sorted(ids)


def case_nodes(case, seed=7):
    """every node up to DENSE_MAX_NODES nodes; beyond: node 0 and the last, every separator and both its neighbours, the middle node of every segment, 32 seeded
    random nodes"""
    n = case["poses"].shape[0]
    if n <= DENSE_MAX_NODES:
        return list(range(n))
    sep = separators(case)
    ids = {0, n - 1}
    for k, s in enumerate(sep):
        ids.update(v for v in (s - 1, s, s + 1) if 0 <= v < n)
        end = sep[k + 1] if k + 1 < len(sep) else n
        if end - s > 1:
            ids.add((s + end) // 2)
    ids.update(int(v) for v in np.random.default_rng(seed).integers(0, n, 32))
    return sorted(ids)


def case_pairs(case):
    """(0, N - 1); both endpoints of every loop, up to 32; two interior nodes of one segment; two of different segments; an interior node with its bounding
    separator; (i, i); one pair in both orders — as far as the graph has such nodes"""
    n = case["poses"].shape[0]
    sep = separators(case)
    is_sep = set(sep)
    pairs = [(0, n - 1)] if n > 1 else []
    pairs += [(int(a), int(b)) for a, b, _, _ in case["loops"][:32]]
    segs = []      # (left separator, first interior, last interior)
    for k, s in enumerate(sep):
        end = sep[k + 1] if k + 1 < len(sep) else n
        if end - s > 1:
            segs.append((s, s + 1, end - 1))
    wide = [g for g in segs if g[2] - g[1] >= 2]
    if wide:
        s, a, b = max(wide, key=lambda g: g[2] - g[1])
        pairs += [(a, b), (b - 1, a + 1), ((a + b) // 2, b)]
    if len(segs) >= 2:
        pairs += [((segs[0][1] + segs[0][2]) // 2, (segs[-1][1] + segs[-1][2]) // 2), (segs[-1][2], segs[0][1])]
    if segs:
        s, a, b = segs[-1]
        pairs += [(b, s), (s, a)]
        s, a, b = segs[0]
        if b + 1 < n:
            pairs.append(((a + b) // 2, b + 1))      # with the separator on its right
    interior = next((i for i in range(n) if i not in is_sep), 0)
    pairs += [(interior, interior), (sep[-1], sep[-1])]
    if n > 2:
        pairs += [(1, n - 2), (n - 2, 1)]
    elif n == 2:
        pairs += [(0, 1), (1, 0)]
    return pairs


_referee = {}


def referee(name, graph, X, nodes, pairs):
    """the model's marginals of a case at the estimates X, computed once: (cov, cross, D0, routes) of the first route, D0 over every route available at that size"""
    if name not in _referee:
        routes = routes_for(graph.n)
        res = [marginals(graph, X, nodes, pairs, r) for r in routes]
        _referee[name] = (res[0][0], res[0][1], spread(res), routes, np.asarray(X).copy())
    cov, cross, d0, routes, X0 = _referee[name]
    assert np.array_equal(X0, np.asarray(X)), f"{name}: the referee was computed at other estimates"
    return cov, cross, d0, routes
