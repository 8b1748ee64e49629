"""numpy restatement of the loop-closure registration: pcl::IterativeClosestPoint's default pipeline in f64 and the submap assembly of
detectLoopClosure.  The exact 1-NN is the oracle's kd-tree; the source transform is the library's fixed expression, so query points are bit-identical."""
import numpy as np

NOT_CONVERGED, ITERATIONS, TRANSFORM, ABS_MSE, REL_MSE, NO_CORRESPONDENCES = range(6)


def apply(T, src):
    """((r0 x + r1 y) + r2 z) + t in f64, rounded to f32."""
    T = np.asarray(T, np.float64).reshape(4, 4)
    p = np.asarray(src, np.float32)[:, :3].astype(np.float64)
    out = np.empty((p.shape[0], 3), np.float32)
    for r in range(3):
        out[:, r] = (((T[r, 0] * p[:, 0] + T[r, 1] * p[:, 1]) + T[r, 2] * p[:, 2]) + T[r, 3]).astype(np.float32)
    return out


def d2_f32(tgt, q):
    d = np.asarray(tgt, np.float32)[:, :3] - np.asarray(q, np.float32)[:, :3]
    return (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]


def nearest(tree, tgt, q):
    """exact 1-NN (index, f32 d2 of the library's expression)"""
    idx = tree.knn5(q)[0][:, 0].astype(np.int64)
    return idx, d2_f32(tgt[idx], q)


def umeyama_rotation(P, Q):
    """TransformationEstimationSVD without scale: H = sum (p - pm)(q - qm)^T = U S V^T, R = V U^T (V's third column negated if det U det V < 0), t = qm - R pm"""
    P, Q = np.asarray(P, np.float64), np.asarray(Q, np.float64)
    pm, qm = P.mean(0), Q.mean(0)
    H = (P - pm).T @ (Q - qm)
    U, _, Vt = np.linalg.svd(H)
    V = Vt.T
    if np.linalg.det(U) * np.linalg.det(V) < 0:
        V[:, 2] *= -1
    R = V @ U.T
    return R, qm - R @ pm


def convergence_state(iterations, max_iterations, cos_angle, translation_sqr, mse, prev_mse, teps, feps):
    """DefaultConvergenceCriteria::hasConverged with max_iterations_similar_transforms_ = 0, failure_after_max_iter_ = false"""
    if iterations >= max_iterations:
        return ITERATIONS
    if cos_angle >= 1.0 - teps and translation_sqr <= teps:
        return TRANSFORM
    if abs(mse - prev_mse) < 1e-12:
        return ABS_MSE
    if prev_mse != 0 and abs(mse - prev_mse) / prev_mse < feps:
        return REL_MSE
    return NOT_CONVERGED


def replay_states(log, max_iterations, teps=1e-6, feps=1e-6):
    """the states the rule gives a log of (mse, cos_angle, translation_sqr, n_corr) entries"""
    prev, it, out = np.finfo(np.float64).max, 0, []
    for e in log:
        if e["n_corr"] < 3:
            out.append(NO_CORRESPONDENCES)
            break
        it += 1
        s = convergence_state(it, max_iterations, e["cos_angle"], e["translation_sqr"], e["mse"], prev, teps, feps)
        out.append(s)
        prev = e["mse"]
        if s != NOT_CONVERGED:
            break
    return out, it


def step(tree, tgt, src, T, max_corr_dist):
    """one iteration from T: (correspondence index (-1 rejected), d2 (inf rejected), increment 4x4, mse, n_corr)"""
    q = apply(T, src)
    idx, d2 = nearest(tree, tgt, q)
    acc = d2.astype(np.float64) <= max_corr_dist * max_corr_dist
    cidx = np.where(acc, idx, -1).astype(np.int32)
    cd2 = np.where(acc, d2, np.float32(np.inf)).astype(np.float32)
    n = int(acc.sum())
    inc = np.eye(4)
    mse = float(d2[acc].astype(np.float64).sum() / n) if n else 0.0
    if n >= 3:
        R, t = umeyama_rotation(q[acc], np.asarray(tgt, np.float32)[idx[acc], :3])
        inc[:3, :3], inc[:3, 3] = R, t
    return cidx, cd2, inc, mse, n


def align(tree, tgt, src, guess=None, max_corr_dist=30.0, max_iterations=100, teps=1e-6, feps=1e-6):
    T = np.eye(4) if guess is None else np.asarray(guess, np.float64).reshape(4, 4).copy()
    prev, it, log = np.finfo(np.float64).max, 0, []
    while True:
        _, _, inc, mse, n = step(tree, tgt, src, T, max_corr_dist)
        if n < 3:
            log.append(dict(n_corr=n, state=NO_CORRESPONDENCES))
            return dict(transform=T, converged=False, state=NO_CORRESPONDENCES, iterations=it, log=log)
        T = inc @ T
        it += 1
        cos = 0.5 * (np.trace(inc[:3, :3]) - 1.0)
        tr2 = float(inc[:3, 3] @ inc[:3, 3])
        s = convergence_state(it, max_iterations, cos, tr2, mse, prev, teps, feps)
        log.append(dict(mse=mse, cos_angle=cos, translation_sqr=tr2, n_corr=n, state=s))
        prev = mse
        if s != NOT_CONVERGED:
            return dict(transform=T, converged=True, state=s, iterations=it, log=log)


def fitness(tree, tgt, src, T, max_range=np.finfo(np.float64).max):
    """getFitnessScore: mean exact 1-NN d2 of every source point under T (d2 <= max_range)"""
    _, d2 = nearest(tree, tgt, apply(T, src))
    d = d2.astype(np.float64)
    d = d[d <= max_range]
    return (float(d.sum() / d.size) if d.size else np.finfo(np.float64).max), int(d.size)


def assemble(O, clouds, ts, qs, leaf):
    """transformCloud of every cloud (rows x, y, z, aux), concatenated in order, then VoxelGrid(leaf) (the oracle's restatements)"""
    parts = [O.transform_cloud(np.asarray(c, np.float32), q, t) for c, t, q in zip(clouds, ts, qs)]
    raw = np.concatenate(parts, 0) if parts else np.zeros((0, 4), np.float32)
    if leaf <= 0:
        return raw
    return O.voxel_grid(raw, leaf, stable=True)[0]
