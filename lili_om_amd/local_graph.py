"""Per-frame trajectory (include/lili_hip.h: lili_local_graph*): the poses of the scans between two keyframes, from the IMU walk and the
local pose graph of the reference's buildLocalPoseGraph / optimizeLocalGraph, and the bookkeeping of pose_each_frame around them.

A pose is 7 doubles, p (3) then q (w, x, y, z); a measurement is (delta p, delta q).  LocalGraph needs a context (the work runs on the GPU, there is no
other path); FrameTrajectory is host-only numpy."""
import ctypes as C

import numpy as np

from .api import LOCAL_MAX_FRAMES, LiliError, LmOptions, LocalGraphSummary, LocalWalk, _ptr


def _f64(a, shape):
    a = np.ascontiguousarray(a, dtype=np.float64)
    if a.size != int(np.prod(shape)):
        raise LiliError(f"expected {int(np.prod(shape))} doubles, got {a.size}")
    return a.reshape(shape)


class LocalGraph:
    """propagate / evaluate / solve / run on one context.  The walk's arguments: stamps (m), acc / gyr (m, 3) = the raw sample buffer, ii0 = imu_idx_in_kf of the
    left keyframe, T = the n + 2 scan stamps (left keyframe, the n scans, right keyframe), (P0, R0 3 x 3, V0) = the start state, g, left = the left
    anchor's pose; f32_positions: frame positions through pcl::PointXYZI's floats, as the reference stores them."""

    def __init__(self, ctx):
        self.ctx, self.lib = ctx, ctx.lib

    def options(self, **kw):
        o = LmOptions()
        self.lib.lili_lm_default_options(C.byref(o))
        for k, v in kw.items():
            setattr(o, k, v)
        return o

    def _walk(self, stamps, acc, gyr, ii0, T, P0, R0, V0, g, left, f32_positions=False):
        st = np.ascontiguousarray(stamps, np.float64).reshape(-1)
        a, w = _f64(acc, (st.shape[0], 3)), _f64(gyr, (st.shape[0], 3))
        T = np.ascontiguousarray(T, np.float64).reshape(-1)
        n = T.shape[0] - 2
        if n < 0:
            raise LiliError("local graph: at least the two keyframe stamps are needed")
        wk = LocalWalk()
        wk.stamps, wk.acc, wk.gyr, wk.scan_stamps = (x.ctypes.data_as(C.POINTER(C.c_double)) for x in (st, a, w, T))
        wk.n_imu, wk.ii0, wk.f32_positions = st.shape[0], int(ii0), 1 if f32_positions else 0
        for name, v, size in (("P0", P0, 3), ("R0", R0, 9), ("V0", V0, 3), ("g", g, 3), ("left", left, 7)):
            getattr(wk, name)[:] = _f64(v, (size,)).tolist()
        wk._keep = (st, a, w, T)
        return wk, n

    def propagate(self, **walk):
        """-> poses (n, 7), end state (P (3), R (3, 3), V (3)) at the right keyframe's stamp, measurements (n + 1, 7)"""
        wk, n = self._walk(**walk)
        poses, end, meas = np.zeros((n, 7)), np.zeros(15), np.zeros((n + 1, 7))
        self.ctx._chk(self.lib.lili_local_graph_propagate(self.ctx.h, C.byref(wk), n, _ptr(poses) if n else None, _ptr(end), _ptr(meas)))
        return poses, (end[0:3].copy(), end[3:12].reshape(3, 3).copy(), end[12:15].copy()), meas

    def evaluate(self, left, right, meas, poses):
        """-> cost, gradient (6 n), J^T J (6 n, 6 n) of the n + 1 factors at `poses`, local coordinates"""
        meas = np.ascontiguousarray(meas, np.float64).reshape(-1, 7)
        n = meas.shape[0] - 1
        poses = _f64(poses, (n, 7))
        anchors = np.concatenate([_f64(left, (7,)), _f64(right, (7,))])
        cost, grad, jtj = C.c_double(0.0), np.zeros(6 * n), np.zeros((6 * n, 6 * n))
        self.ctx._chk(self.lib.lili_local_graph_evaluate(self.ctx.h, n, _ptr(anchors), _ptr(meas), _ptr(poses) if n else None, C.byref(cost), _ptr(grad) if n else None,
                                                         _ptr(jtj) if n else None))
        return float(cost.value), grad, jtj

    def solve(self, left, right, meas, poses, options=None):
        """-> solved poses (n, 7), summary dict (LmSummary's, with the dogleg case and the reuse flag per logged candidate, and final_mu)"""
        meas = np.ascontiguousarray(meas, np.float64).reshape(-1, 7)
        n = meas.shape[0] - 1
        x = _f64(poses, (n, 7)).copy()
        anchors = np.concatenate([_f64(left, (7,)), _f64(right, (7,))])
        s = LocalGraphSummary()
        self.ctx._chk(self.lib.lili_local_graph_solve(self.ctx.h, n, _ptr(anchors), _ptr(meas), _ptr(x) if n else None, C.byref(options) if options is not None else None, C.byref(s)))
        self.last_summary = s
        return x, s.as_dict()

    def run(self, right, options=None, **walk):
        """propagate and solve in one launch -> solved poses (n, 7), measurements (n + 1, 7), summary dict"""
        wk, n = self._walk(**walk)
        right = _f64(right, (7,))
        poses, meas, s = np.zeros((n, 7)), np.zeros((n + 1, 7)), LocalGraphSummary()
        self.ctx._chk(self.lib.lili_local_graph(self.ctx.h, C.byref(wk), n, _ptr(right), C.byref(options) if options is not None else None, _ptr(poses) if n else None, _ptr(meas),
                                                C.byref(s)))
        self.last_summary = s
        return poses, meas, s.as_dict()

    def kernel_ms(self):
        ms = C.c_float(0)
        self.ctx._chk(self.lib.lili_local_graph_kernel_ms(self.ctx.h, C.byref(ms)))
        return float(ms.value)


class FrameTrajectory:
    """pose_each_frame / keyframe_id_in_frame of the reference (L/src/BackendFusion.cpp:1892-2014, 1370-1383): one pose per scan, keyframes included.
    start(pose) when the window fills (the first keyframe, L:1893-1895); then per keyframe append(frame_poses, keyframe_pose): the n solved poses of the scans
    since the previous keyframe and the right keyframe itself; rewrite(poses) replaces every pose (the caller's correctPoses)."""

    def __init__(self):
        self.poses = np.zeros((0, 7))
        self.keyframe_id_in_frame = []

    def __len__(self):
        return self.poses.shape[0]

    def start(self, keyframe_pose):
        if len(self):
            raise ValueError("FrameTrajectory.start: the trajectory has frames already")
        self.poses = _f64(keyframe_pose, (1, 7)).copy()
        self.keyframe_id_in_frame = [0]

    def append(self, frame_poses, keyframe_pose):
        if not len(self):
            raise ValueError("FrameTrajectory.append: start() first")
        frames = np.ascontiguousarray(frame_poses, np.float64).reshape(-1, 7)
        if frames.shape[0] > LOCAL_MAX_FRAMES:
            raise ValueError(f"FrameTrajectory.append: more than {LOCAL_MAX_FRAMES} frames between two keyframes")
        self.poses = np.vstack([self.poses, frames, _f64(keyframe_pose, (1, 7))])
        self.keyframe_id_in_frame.append(len(self) - 1)
        return self.keyframe_id_in_frame[-1]

    def last_keyframe(self):
        return self.poses[self.keyframe_id_in_frame[-1]].copy()

    def keyframes(self):
        return self.poses[self.keyframe_id_in_frame].copy()

    def rewrite(self, poses):
        self.poses = _f64(poses, self.poses.shape).copy()
