"""Loop closure on the device: performLoopClosure / detectLoopClosure (L/src/BackendFusion.cpp:2423-2642, R/src/BackendFusion.cpp ~2233-2405) up to the
BetweenFactor the reference hands to iSAM2.  The pose graph behind it is lili_om_amd.pose_graph (PoseGraph.add_loop_from_icp, solve, correct_poses).  Nothing here imports oracle/."""
import ctypes as C

import numpy as np

from .api import (Cloud, FeatureOut, IcpParams, IcpResult, MEM_HOST, _f64, _ptr, cloud_from_numpy, keyframe_map_pose)

LOOP_SOURCE, LOOP_TARGET = 0, 1
ICP_NOT_CONVERGED, ICP_ITERATIONS, ICP_TRANSFORM, ICP_ABS_MSE, ICP_REL_MSE, ICP_NO_CORRESPONDENCES = range(6)


def default_icp_params():
    """performLoopClosure's settings (L:2567-2577): max correspondence distance 30, 100 iterations, epsilons 1e-6.  setRANSACIterations(5) has no effect on
    this pipeline (no rejector reads it)."""
    from .api import load_library
    p = IcpParams()
    load_library().lili_icp_default_params(C.byref(p))
    return p


def _qmul(a, b):
    return np.array([a[0] * b[0] - a[1] * b[1] - a[2] * b[2] - a[3] * b[3],
                     a[0] * b[1] + a[1] * b[0] + a[2] * b[3] - a[3] * b[2],
                     a[0] * b[2] + a[2] * b[0] + a[3] * b[1] - a[1] * b[3],
                     a[0] * b[3] + a[3] * b[0] + a[1] * b[2] - a[2] * b[1]])


def _qrot(q, v):
    u = np.asarray(q[1:4], np.float64)
    uv = np.cross(u, v)
    uv = uv + uv
    return (np.asarray(v, np.float64) + uv * q[0]) + np.cross(u, uv)


def quat_from_matrix(R):
    """Eigen::Quaterniond(const Matrix3d&) (w, x, y, z)."""
    R = np.asarray(R, np.float64)
    tr = R[0, 0] + R[1, 1] + R[2, 2]
    if tr > 0:
        t = np.sqrt(tr + 1.0)
        w = 0.5 * t
        t = 0.5 / t
        return np.array([w, (R[2, 1] - R[1, 2]) * t, (R[0, 2] - R[2, 0]) * t, (R[1, 0] - R[0, 1]) * t])
    i = 0
    if R[1, 1] > R[0, 0]:
        i = 1
    if R[2, 2] > R[i, i]:
        i = 2
    j, k = (i + 1) % 3, (i + 2) % 3
    t = np.sqrt(R[i, i] - R[j, j] - R[k, k] + 1.0)
    q = np.zeros(4)
    q[1 + i] = 0.5 * t
    t = 0.5 / t
    q[0] = (R[k, j] - R[j, k]) * t
    q[1 + j] = (R[j, i] + R[i, j]) * t
    q[1 + k] = (R[k, i] + R[i, k]) * t
    return q


def _matrix_from_quat(q):
    w, x, y, z = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


def _result_dict(r):
    n = min(int(r.n_logged), len(r.it))
    return dict(transform=np.array(r.transform[:], np.float64).reshape(4, 4), converged=bool(r.converged), state=int(r.state), iterations=int(r.iterations),
                fitness=float(r.fitness), log=[dict(mse=r.it[k].mse, cos_angle=r.it[k].cos_angle, translation_sqr=r.it[k].translation_sqr, n_corr=int(r.it[k].n_corr),
                                                    state=int(r.it[k].state)) for k in range(n)],
                wall_us=float(r.stage_us[0]), host_syncs=int(r.stage_us[1]), iterations_enqueued=int(r.stage_us[2]))


def _as_cloud(a):
    if isinstance(a, Cloud):
        return a
    a = np.ascontiguousarray(a, np.float32)
    return cloud_from_numpy(a, aux_col=3 if a.shape[1] > 3 else None)


class LoopClosure:
    """The reference's loop-closure thread minus iSAM2.  variant "livox" (LiLi-OM: one source keyframe, two time thresholds) or "rot" (LiLi-OM-ROT: six source
    keyframes, one threshold, no second attempt within 0.2 s of the last loop).  Keyframe clouds (edge_frames[i], surf_frames[i]) are numpy rows (x, y, z[, aux])
    or api.Cloud descriptions of host, page-locked or device memory kept by the caller — or, with `archive` (a KeyframeArchive), the keyframes the archive holds on the
    device: assemble and perform then take keyframe ids only, and detect / perform may read positions (the body translations) and times from the archive."""

    def __init__(self, ctx, variant="livox", lc_search_radius=10.0, lc_map_width=20, lc_icp_thres=0.2, local_lc_time_thres=25.0, global_lc_time_thres=25.0,
                 lc_time_thres=120.0, q_bl=(1.0, 0.0, 0.0, 0.0), t_bl=(0.0, 0.0, 0.0), leaf=0.4, slide_window_width=3, archive=None):
        if variant not in ("livox", "rot"):
            raise ValueError("variant must be 'livox' or 'rot'")
        self.ctx, self.lib, self.variant = ctx, ctx.lib, variant
        self.lc_search_radius, self.lc_map_width, self.lc_icp_thres = float(lc_search_radius), int(lc_map_width), float(lc_icp_thres)
        self.local_lc_time_thres, self.global_lc_time_thres, self.lc_time_thres = float(local_lc_time_thres), float(global_lc_time_thres), float(lc_time_thres)
        self.q_bl, self.t_bl = _f64(q_bl, 4), _f64(t_bl, 3)
        self.leaf, self.slide_window_width = float(leaf), int(slide_window_width)
        self.time_last_loop = 0.0
        self.params = default_icp_params()
        self.last = None
        self.archive = archive      # (its extrinsic is the archive's own: KeyframeArchive(ctx, q_bl, t_bl))

    # ---- detectLoopClosure: candidate selection (L:2431-2473, R:2240-2263) ----
    def detect(self, positions, times, select_pose, t_now):
        """(latest_idx, his_idx) or None.  positions (n, 3) keyframe positions (pose_cloud_frame), times (n,), select_pose the query position, t_now time_new_odom.
        The radius search is kd_tree_his_key_poses->radiusSearch in f32: d2 < radius^2, ascending d2 (ties: smaller index).  With an archive, positions / times
        may be None: the archive's body translations and times."""
        if self.archive is not None and (positions is None or times is None):
            ts, _, tm = self.archive.poses()
            positions = ts if positions is None else positions
            times = tm if times is None else times
        pos = np.asarray(positions, np.float32).reshape(-1, 3)
        times = np.asarray(times, np.float64).reshape(-1)
        if pos.shape[0] == 0:
            return None
        d = pos - np.asarray(select_pose, np.float32).reshape(1, 3)
        d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
        inside = np.nonzero(d2 < np.float32(self.lc_search_radius * self.lc_search_radius))[0]
        order = inside[np.argsort(d2[inside], kind="stable")]
        his = -1
        thr = self.global_lc_time_thres if self.variant == "livox" else self.lc_time_thres
        for idx in order:
            if abs(times[idx] - t_now) > thr:
                his = int(idx)
                break
        if self.variant == "livox":
            if his == -1:
                max_time, max_id = 0.0, -1
                for idx in order:
                    dt = abs(times[idx] - t_now)
                    if self.local_lc_time_thres < dt < self.global_lc_time_thres and dt > max_time:
                        max_time, max_id = dt, int(idx)
                if max_id == -1:
                    return None
                his = max_id
        else:
            if his == -1 or abs(self.time_last_loop - t_now) < 0.2:
                return None
        return pos.shape[0] - self.slide_window_width, his

    def detect_appearance(self, place, t_now=None, *, max_distance):
        """(latest_idx, his_idx, shift, distance) or None: the candidate by APPEARANCE (place: a PlaceRecognition on this closure's archive) — the best
        match of the latest keyframe's descriptor among the keyframes whose time differs from t_now (None: the latest keyframe's) by more than the variant's
        threshold (global_lc_time_thres / lc_time_thres), at every yaw shift, wherever the odometry believes them to be.  latest = n - slide_window_width as
        in detect; ROT: none within 0.2 s of the last loop.  A match counts when distance <= max_distance.  The paper (Kim & Kim, IROS 2018) reports 0.13
        for its data; that is the paper's value, not one measured with this project's sensors: there is no default."""
        if self.archive is None or place.archive is not self.archive:
            raise ValueError("detect_appearance needs the archive the PlaceRecognition describes")
        latest = len(self.archive) - self.slide_window_width
        if latest < 0:
            return None
        place.update()
        t_now = self.archive.pose(latest)[2] if t_now is None else float(t_now)
        if self.variant == "rot" and abs(self.time_last_loop - t_now) < 0.2:
            return None
        thr = self.global_lc_time_thres if self.variant == "livox" else self.lc_time_thres
        found = place.search([latest], k=1, min_time_gap=thr, max_id=latest, times=t_now)[0]
        if not found or not found[0][2] <= max_distance:
            return None
        his, shift, dist = found[0]
        return latest, his, shift, dist

    def source_keyframes(self, latest_idx):
        """L: the latest keyframe; ROT: latest, latest - 1, ..., latest - 5 (in that order, R:2267)."""
        ks = [latest_idx] if self.variant == "livox" else [latest_idx - j for j in range(6)]
        return [k for k in ks if k >= 0]

    def target_keyframes(self, latest_idx, his_idx):
        return [his_idx + j for j in range(-self.lc_map_width, self.lc_map_width + 1) if 0 <= his_idx + j <= latest_idx]

    def _cloud(self, which, keyframes, ts_po, qs_po, edge_frames, surf_frames):
        clouds, ts, qs = [], [], []
        for k in keyframes:
            t, q = keyframe_map_pose(ts_po[k], qs_po[k], self.t_bl, self.q_bl)
            for c in (edge_frames[k], surf_frames[k]):
                clouds.append(_as_cloud(c))
                ts.append(t)
                qs.append(q)
        arr = (Cloud * len(clouds))(*clouds)
        t = np.ascontiguousarray(np.array(ts, np.float64).reshape(-1))
        q = np.ascontiguousarray(np.array(qs, np.float64).reshape(-1))
        a, b = C.c_int64(0), C.c_int64(0)
        self.ctx._chk(self.lib.lili_loop_cloud(self.ctx.h, which, arr, len(clouds), _ptr(t), _ptr(q), float(self.leaf), C.byref(a), C.byref(b)))
        return a.value, b.value

    def _cloud_archive(self, which, keyframes):
        ids = (C.c_int * len(keyframes))(*[int(k) for k in keyframes])
        a, b = C.c_int64(0), C.c_int64(0)
        self.ctx._chk(self.lib.lili_loop_cloud_archive(self.ctx.h, which, ids, len(keyframes), float(self.leaf), C.byref(a), C.byref(b)))
        return a.value, b.value

    def assemble(self, latest_idx, his_idx, ts_po=None, qs_po=None, edge_frames=None, surf_frames=None):
        """Both submaps of detectLoopClosure on the device (L:2475-2548): per keyframe edge then surf, transformCloud at (q_po q_bl, q_po t_bl + t_po),
        VoxelGrid(leaf).  Returns ((n_raw, n_ds) of the source, (n_raw, n_ds) of the target).  With an archive: clouds and poses are the archive's."""
        if self.archive is not None and edge_frames is None:
            return (self._cloud_archive(LOOP_SOURCE, self.source_keyframes(latest_idx)), self._cloud_archive(LOOP_TARGET, self.target_keyframes(latest_idx, his_idx)))
        ts_po = np.asarray(ts_po, np.float64).reshape(-1, 3)
        qs_po = np.asarray(qs_po, np.float64).reshape(-1, 4)
        s = self._cloud(LOOP_SOURCE, self.source_keyframes(latest_idx), ts_po, qs_po, edge_frames, surf_frames)
        t = self._cloud(LOOP_TARGET, self.target_keyframes(latest_idx, his_idx), ts_po, qs_po, edge_frames, surf_frames)
        return s, t

    def align(self, guess=None, params=None):
        """icp.align: a dict with transform (4x4 f64), converged, state, iterations, fitness (getFitnessScore()), log (per iteration), wall_us, host_syncs."""
        r = IcpResult()
        g = None if guess is None else _f64(guess, 16)
        self.ctx._chk(self.lib.lili_icp_align(self.ctx.h, C.byref(params or self.params), _ptr(g), C.byref(r)))
        self.last = _result_dict(r)
        return self.last

    def perform(self, positions, times, select_pose, t_now, ts_po=None, qs_po=None, edge_frames=None, surf_frames=None, detector="position", place=None,
                max_distance=None):
        """performLoopClosure up to the BetweenFactor: None, or (latest_idx, his_idx, pose_from, pose_to, between, noise_score) with poses as (t (3,), q (4,) wxyz):
        pose_from = the latest keyframe's pose corrected by the ICP transform, pose_to = the candidate's, between = pose_from^-1 pose_to; noise_score = the
        fitness (the variances of the reference's Diagonal noise model).  The caller adds BetweenFactor(latest, his, between, noise) and updates iSAM2.
        With an archive: the keyframes' clouds, poses and (where None) positions and times are the archive's.
        detector="appearance" (archive only; place, max_distance as detect_appearance takes them; positions and select_pose are not read): the candidate is
        detect_appearance's, the same submaps are assembled, and the ICP starts from place.guess — the source put on the candidate with the matched yaw —
        instead of the identity."""
        if detector not in ("position", "appearance"):
            raise ValueError("detector must be 'position' or 'appearance'")
        if self.archive is not None and edge_frames is None:
            ts_po, qs_po, a_tm = self.archive.poses()
            positions = ts_po if positions is None else positions
            times = a_tm if times is None else times
        guess = None
        if detector == "appearance":
            if place is None or max_distance is None or edge_frames is not None:
                raise ValueError("detector='appearance' needs an archive, place and max_distance")
            det = self.detect_appearance(place, t_now, max_distance=max_distance)
            if det is None:
                return None
            latest, his = det[:2]
            guess = place.guess(latest, his, det[2])
        else:
            det = self.detect(positions, times, select_pose, t_now)
            if det is None:
                return None
            latest, his = det
        ts_po = np.asarray(ts_po, np.float64).reshape(-1, 3)
        qs_po = np.asarray(qs_po, np.float64).reshape(-1, 4)
        self.assemble(latest, his, ts_po, qs_po, edge_frames, surf_frames)
        res = self.align(guess)
        if not res["converged"] or res["fitness"] > self.lc_icp_thres:
            return None
        T = res["transform"]
        q_inc = quat_from_matrix(T[:3, :3])
        q_from = _qmul(q_inc, qs_po[latest])
        t_from = _qrot(q_inc, ts_po[latest]) + T[:3, 3]
        q_to, t_to = qs_po[his].copy(), ts_po[his].copy()
        R_from = _matrix_from_quat(q_from / np.linalg.norm(q_from))
        R_to = _matrix_from_quat(q_to / np.linalg.norm(q_to))
        between = (R_from.T @ (t_to - t_from), quat_from_matrix(R_from.T @ R_to))
        if self.variant == "rot":
            self.time_last_loop = float(np.asarray(times, np.float64)[latest])
        return latest, his, (t_from, q_from), (t_to, q_to), between, res["fitness"]

    # ---- lower-level access ----
    def set_cloud(self, which, pts):
        self.ctx._chk(self.lib.lili_icp_set_cloud(self.ctx.h, int(which), C.byref(_as_cloud(pts))))

    def get_cloud(self, which, capacity=None):
        fo = FeatureOut(None, 0, 16, MEM_HOST, 0)
        self.ctx._chk(self.lib.lili_icp_get_cloud(self.ctx.h, int(which), C.byref(fo)))
        n = fo.count if capacity is None else min(fo.count, int(capacity))
        out = np.zeros((max(n, 1), 4), np.float32)
        fo = FeatureOut(out.ctypes.data, n, 16, MEM_HOST, 0)
        self.ctx._chk(self.lib.lili_icp_get_cloud(self.ctx.h, int(which), C.byref(fo)))
        return out[:n]

    def fitness(self, T, max_range=np.finfo(np.float64).max):
        f, n = C.c_double(0), C.c_int64(0)
        t = _f64(T, 16)
        self.ctx._chk(self.lib.lili_icp_fitness(self.ctx.h, _ptr(t), float(max_range), C.byref(f), C.byref(n)))
        return f.value, n.value

    def correspondences(self, n):
        idx = np.zeros(max(int(n), 1), np.int32)
        d2 = np.zeros(max(int(n), 1), np.float32)
        self.ctx._chk(self.lib.lili_icp_get_correspondences(self.ctx.h, int(n), _ptr(idx), _ptr(d2)))
        return idx[:n], d2[:n]
