"""Global pose graph over every frame (include/lili_hip.h: lili_pose_graph*): the reference's saveKeyFramesAndFactors / performLoopClosure /
correctPoses without GTSAM.  A pose is 7 doubles, p (3) then q (w, x, y, z); the tangent is (omega, v), rotation first.  PoseGraph needs a context (the solve
runs on the GPU, there is no other path); correct_poses and loop_measurement are host functions of the library.

A full loop closure, with a KeyframeArchive `archive`, a FrameTrajectory `traj` whose frames are the graph's nodes and the window's abs_poses:

    found = loop.perform(None, None, select_pose, t_now)                    # LoopClosure(ctx, archive=archive): detect, submaps, ICP
    if found is not None:
        latest, his = found[0], found[1]
        ts, qs, _ = archive.poses()
        graph.add_loop_from_icp(traj.keyframe_id_in_frame[latest], traj.keyframe_id_in_frame[his], loop.last["transform"],
                                np.concatenate([ts[latest], qs[latest]]), np.concatenate([ts[his], qs[his]]), loop.last["fitness"])
        graph.solve(max_iterations=2)                                        # isam->update(graph); isam->update()
        out = correct_poses(graph.poses(), traj.keyframe_id_in_frame, width, abs_poses, np.hstack([ts, qs]))
        traj.rewrite(out["frame_poses"])
        archive.set_poses(0, out["keyframe_poses"][:, 0:3], out["keyframe_poses"][:, 3:7])      # then lili_localmap_repose of the rings

How well the poses are known (gtsam: marginalCovariance / jointMarginalCovariance): graph.marginals() -> the 6 x 6 covariance of every node and of node pairs at the
current estimates, graph.relative_covariance(i, j) -> the covariance of between(X_i, X_j); INTEGRATION.md §1c says what a loop closure can do with them.

A false closure (an ICP that passed lc_icp_thres on a repeated corridor): add_loop / add_loop_from_icp take loss="huber" | "cauchy" | "geman_mcclure" and its scale
(GTSAM's noiseModel::Robust on the loop factor), graph.loop_status() -> every loop's chi2 and the weight its loss leaves it, graph.solve_lm() is the damped
(Levenberg-Marquardt) solve for a graph that starts far from its minimum.
"""
import ctypes as C

import numpy as np

from .api import PG_LOSSES, LiliError, PgLmOptions, PgLmSummary, PgMarginalsInfo, PgOptions, PgSummary, _ptr, load_library


def _f64(a, shape):
    a = np.ascontiguousarray(a, dtype=np.float64)
    if a.size != int(np.prod(shape)):
        raise LiliError(f"expected {int(np.prod(shape))} doubles, got {a.size}")
    return a.reshape(shape)


def loop_measurement(T_icp, pose_latest, pose_closest):
    """The loop factor's measurement (L/src/BackendFusion.cpp:2587-2622): between(T_icp o pose_latest, pose_closest)"""
    T, a, b, m = _f64(T_icp, (16,)), _f64(pose_latest, (7,)), _f64(pose_closest, (7,)), np.zeros(7)
    if load_library().lili_loop_measurement(_ptr(T), _ptr(a), _ptr(b), _ptr(m)) != 0:
        raise LiliError("lili_loop_measurement: bad argument")
    return m


def correct_poses(solution, keyframe_id_in_frame, slide_window_width, abs_poses, keyframe_poses, f32_positions=False):
    """correctPoses (L:2177-2311) on copies of the caller's arrays -> dict(abs_poses (n_abs, 7: q wxyz then p), frame_poses (n_frames, 7), keyframe_poses
    (n_keyframes, 7), last_pose (7, the abs_poses layout), select_pose (3)).  solution: the solved nodes (PoseGraph.poses())."""
    sol = np.ascontiguousarray(solution, np.float64).reshape(-1, 7)
    ids = np.ascontiguousarray(keyframe_id_in_frame, np.int32).reshape(-1)
    ab = np.array(abs_poses, np.float64, order="C").reshape(-1, 7)
    kf = np.array(keyframe_poses, np.float64, order="C").reshape(-1, 7)
    if kf.shape[0] != ids.shape[0]:
        raise LiliError("correct_poses: one keyframe pose per keyframe id")
    frames, last, sel = np.zeros_like(sol), np.zeros(7), np.zeros(3)
    rc = load_library().lili_correct_poses(_ptr(sol), sol.shape[0], _ptr(ids), ids.shape[0], int(slide_window_width), 1 if f32_positions else 0, _ptr(ab), ab.shape[0],
                                           _ptr(frames), _ptr(kf), _ptr(last), _ptr(sel))
    if rc != 0:
        raise LiliError("lili_correct_poses: bad argument")
    return dict(abs_poses=ab, frame_poses=frames, keyframe_poses=kf, last_pose=last, select_pose=sel)


class PoseGraph:
    """The graph of one context: one node per scan, a prior on node 0, chain factors frozen at append time, loop factors.
    max_loops: the context's option "pose_graph_max_loops" (api.PG_MAX_LOOPS .. api.PG_MAX_LOOPS_EXT; None leaves it as it is, api.PG_MAX_LOOPS unless it was set)."""

    def __init__(self, ctx, max_loops=None):
        self.ctx, self.lib = ctx, ctx.lib
        self.last_summary = None
        self.last_marginals = None
        if max_loops is not None:
            self.set_max_loops(max_loops)

    def set_max_loops(self, max_loops):
        """raise (any time) or lower (not below the graph's loop count) the number of loops add_loop accepts"""
        self.ctx.set_option("pose_graph_max_loops", int(max_loops))

    def options(self, **kw):
        o = PgOptions()
        self.lib.lili_pg_default_options(C.byref(o))
        for k, v in kw.items():
            if k in ("prior_var", "odom_var"):
                getattr(o, k)[:] = _f64(v, (6,)).tolist()
            else:
                setattr(o, k, v)
        return o

    def reset(self):
        self.ctx._chk(self.lib.lili_pose_graph_reset(self.ctx.h))

    def info(self):
        """(nodes, loops)"""
        n, l = C.c_int(0), C.c_int(0)
        self.ctx._chk(self.lib.lili_pose_graph_info(self.ctx.h, C.byref(n), C.byref(l)))
        return n.value, l.value

    def append(self, poses, prev=None):
        """new nodes at `poses` (n, 7); prev: None on an empty graph, otherwise the last node's pose in the frame of `poses`.  -> the first new id"""
        p = np.ascontiguousarray(poses, np.float64).reshape(-1, 7)
        pv = None if prev is None else _f64(prev, (7,))
        first = C.c_int(-1)
        self.ctx._chk(self.lib.lili_pose_graph_append(self.ctx.h, _ptr(pv), _ptr(p), p.shape[0], C.byref(first)))
        return first.value

    def add_loop(self, node_from, node_to, meas, var, loss=None, scale=None):
        """loss: None / "none", "huber", "cauchy", "geman_mcclure" (or an api.PG_LOSS_* code); scale: the loss's k in units of the whitened residual (None = 1)"""
        m = _f64(meas, (7,))
        v = np.full(6, float(var)) if np.ndim(var) == 0 else _f64(var, (6,))
        if loss is None and scale is None:
            self.ctx._chk(self.lib.lili_pose_graph_add_loop(self.ctx.h, int(node_from), int(node_to), _ptr(m), _ptr(v)))
            return
        if isinstance(loss, str) and loss not in PG_LOSSES:
            raise LiliError(f"unknown loss {loss!r}: one of {sorted(k for k in PG_LOSSES if k)}")
        kind = PG_LOSSES[loss] if loss is None or isinstance(loss, str) else int(loss)
        self.ctx._chk(self.lib.lili_pose_graph_add_loop_robust(self.ctx.h, int(node_from), int(node_to), _ptr(m), _ptr(v), kind, 1.0 if scale is None else float(scale)))

    def add_loop_from_icp(self, node_from, node_to, T_icp, pose_latest, pose_closest, fitness, loss=None, scale=None):
        """performLoopClosure's factor (L:2587-2625): the measurement from the ICP transform and the two keyframe poses, all six variances = the fitness;
        loss / scale as in add_loop"""
        m = loop_measurement(T_icp, pose_latest, pose_closest)
        self.add_loop(node_from, node_to, m, float(fitness), loss, scale)
        return m

    def loop_status(self, first=0, n=None, options=None):
        """what the loss decided at the current estimates -> chi2 (n,), weight (n,) of loops first .. first + n - 1 in the order they were added (weight 1 without
        a loss); no step is taken"""
        n = self.info()[1] - int(first) if n is None else int(n)
        chi2, weight = np.zeros(max(n, 0)), np.zeros(max(n, 0))
        if n > 0:
            self.ctx._chk(self.lib.lili_pose_graph_loop_status(self.ctx.h, C.byref(options) if options is not None else None, int(first), n, _ptr(chi2), _ptr(weight)))
        return chi2, weight

    def lm_options(self, **kw):
        o = PgLmOptions()
        self.lib.lili_pg_lm_default_options(C.byref(o))
        for k, v in kw.items():
            setattr(o, k, v)
        return o

    def poses(self, first=0, n=None):
        n = self.info()[0] - first if n is None else int(n)
        out = np.zeros((max(n, 0), 7))
        if n > 0:
            self.ctx._chk(self.lib.lili_pose_graph_get(self.ctx.h, int(first), n, _ptr(out)))
        return out

    def set_poses(self, poses, first=0):
        """overwrite estimates; the measurements stay"""
        p = np.ascontiguousarray(poses, np.float64).reshape(-1, 7)
        self.ctx._chk(self.lib.lili_pose_graph_set(self.ctx.h, int(first), p.shape[0], _ptr(p)))

    def evaluate(self, options=None):
        """-> cost, gradient (N, 6), diagonal blocks (N, 6, 6), sub (N - 1, 6, 6): chain block (i + 1, i), loop blocks (L, 6, 6): block (from, to)"""
        n, l = self.info()
        cost, g, D, S, LB = C.c_double(0.0), np.zeros((n, 6)), np.zeros((n, 6, 6)), np.zeros((max(n - 1, 0), 6, 6)), np.zeros((l, 6, 6))
        self.ctx._chk(self.lib.lili_pose_graph_evaluate(self.ctx.h, C.byref(options) if options is not None else None, C.byref(cost), _ptr(g), _ptr(D),
                                                        _ptr(S) if n > 1 else None, _ptr(LB) if l else None))
        return float(cost.value), g, D, S, LB

    def solve(self, options=None, **kw):
        """Gauss-Newton on the device -> summary dict (iterations, termination, costs, step and gradient norms); the estimates are read with poses()"""
        if options is None and kw:
            options = self.options(**kw)
        s = PgSummary()
        self.ctx._chk(self.lib.lili_pose_graph_solve(self.ctx.h, C.byref(options) if options is not None else None, C.byref(s)))
        self.last_summary = s
        return s.as_dict()

    def solve_lm(self, options=None, lm=None, **kw):
        """Levenberg-Marquardt on the device -> summary dict: solve()'s entries per attempt, plus lambda and accepted (one per attempt), steps_accepted,
        steps_rejected, final_lambda.  kw: the fields of either option structure (used where options / lm is None)"""
        lm_names = {f[0] for f in PgLmOptions._fields_}
        if options is None and any(k not in lm_names for k in kw):
            options = self.options(**{k: v for k, v in kw.items() if k not in lm_names})
        if lm is None and any(k in lm_names for k in kw):
            lm = self.lm_options(**{k: v for k, v in kw.items() if k in lm_names})
        s = PgLmSummary()
        self.ctx._chk(self.lib.lili_pose_graph_solve_lm(self.ctx.h, C.byref(options) if options is not None else None, C.byref(lm) if lm is not None else None, C.byref(s)))
        self.last_summary = s
        return s.as_dict()

    def kernel_ms(self):
        ms = C.c_float(0)
        self.ctx._chk(self.lib.lili_pose_graph_kernel_ms(self.ctx.h, C.byref(ms)))
        return float(ms.value)

    def marginals(self, first=0, n=None, pairs=None, options=None):
        """Marginal covariances at the current estimates (no step is taken) -> cov (n, 6, 6): Sigma(i, i) of nodes first .. first + n - 1 (n None: to the last
        node), cross (P, 6, 6): Sigma(i, j) of every pair (i, j), rows: node i — or None without pairs.  Blocks are in the node's tangent (omega, v).  The call's
        info (status, sizes, reduced_unknowns, kernel_ms) is kept in self.last_marginals, also when the call fails on a non-positive pivot."""
        n = self.info()[0] - int(first) if n is None else int(n)
        pr = None if pairs is None else np.ascontiguousarray(pairs, np.int32).reshape(-1, 2)
        n_pairs = 0 if pr is None else pr.shape[0]
        cov = np.zeros((max(n, 0), 6, 6))
        cross = np.zeros((n_pairs, 6, 6)) if n_pairs else None
        info = PgMarginalsInfo()
        rc = self.lib.lili_pose_graph_marginals(self.ctx.h, C.byref(options) if options is not None else None, int(first), n, _ptr(cov) if n > 0 else None,
                                                _ptr(pr) if n_pairs else None, n_pairs, _ptr(cross) if n_pairs else None, C.byref(info))
        self.last_marginals = info.as_dict() if rc in (0, -6) else None
        self.ctx._chk(rc)
        return cov, cross

    def relative_covariance(self, i, j, options=None):
        """first-order covariance (6, 6) of between(X_i, X_j) in its own tangent: one marginals call for the two nodes and the pair, then the host function"""
        i, j = int(i), int(j)
        _, cross = self.marginals(0, 0, [(i, i), (j, j), (i, j)], options)
        return relative_covariance(self.poses(i, 1)[0], self.poses(j, 1)[0], cross[0], cross[1], cross[2])


def relative_covariance(pose_i, pose_j, cov_ii, cov_jj, cov_ij):
    """lili_pose_relative_covariance: J_a S_ii J_a^T + J_a S_ij + S_ij^T J_a^T + S_jj with the between-factor's Jacobian J_a at Z = between(X_i, X_j) (J_b = I)"""
    a, b = _f64(pose_i, (7,)), _f64(pose_j, (7,))
    sii, sjj, sij, out = _f64(cov_ii, (6, 6)), _f64(cov_jj, (6, 6)), _f64(cov_ij, (6, 6)), np.zeros((6, 6))
    if load_library().lili_pose_relative_covariance(_ptr(a), _ptr(b), _ptr(sii), _ptr(sjj), _ptr(sij), _ptr(out)) != 0:
        raise LiliError("lili_pose_relative_covariance: bad argument")
    return out


__all__ = ["PoseGraph", "correct_poses", "loop_measurement", "relative_covariance"]
