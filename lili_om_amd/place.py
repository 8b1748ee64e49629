"""Place recognition on the device (lili_place_*): a polar descriptor of maximum heights per archived keyframe, in the manner of Scan Context
(Kim & Kim, IROS 2018), and the exact search of a batch of queries over every described keyframe at every circular shift.  Not in the reference, whose
detectLoopClosure searches keyframe positions.  Nothing here imports oracle/."""
import ctypes as C

import numpy as np

from .api import Cloud, PlaceMatch, PlaceParams, PlaceQuery, PlaceSubmap, _f64, _ptr, cloud_from_numpy, keyframe_map_pose, load_library
from .archive import ARCHIVE_FULL

INT32_MAX = 2 ** 31 - 1


def default_place_params():
    p = PlaceParams()
    load_library().lili_place_default_params(C.byref(p))
    return p


def place_layout(params):
    """(ring_r2 (n_ring,), sec_cos (n_sector / 4,), sec_sin (n_sector / 4,)) float32: the boundary tables the kernels decide by (host code, no context)."""
    r, c, s = np.zeros(32, np.float32), np.zeros(16, np.float32), np.zeros(16, np.float32)
    if load_library().lili_place_layout(C.byref(params), _ptr(r), _ptr(c), _ptr(s)) != 0:
        raise ValueError("place_layout: parameters out of range")
    return r[:params.n_ring], c[:params.n_sector // 4], s[:params.n_sector // 4]


def place_guess(pose_src, pose_dst, shift, n_sector):
    """T = M_dst Rz(2 pi shift / n_sector) M_src^-1 (4x4 f64): LoopClosure.align's guess from a match.  Poses are LiDAR map poses, 7 doubles (p, then q w x y z)."""
    a, b, T = _f64(pose_src, 7), _f64(pose_dst, 7), np.zeros(16)
    if load_library().lili_place_guess(_ptr(a), _ptr(b), int(shift), int(n_sector), _ptr(T)) != 0:
        raise ValueError("place_guess: bad argument")
    return T.reshape(4, 4)


def place_frame(pose, level):
    """F of a LiDAR map pose (7 doubles: p, then q w x y z): the pose itself (level false) or its levelled frame — origin p, z the map's z, x the horizontal
    projection of the LiDAR's x axis (host code, no context)."""
    a, f = _f64(pose, 7), np.zeros(7)
    if load_library().lili_place_frame(_ptr(a), int(level), _ptr(f)) != 0:
        raise ValueError("place_frame: bad argument")
    return f


def place_relative(frame, pose):
    """(q_rel (4,), t_rel (3,)) f64: where a member at LiDAR map pose `pose` lies in `frame` — what the device places its rows by (host code, no context)."""
    a, b, q, t = _f64(frame, 7), _f64(pose, 7), np.zeros(4), np.zeros(3)
    if load_library().lili_place_relative(_ptr(a), _ptr(b), _ptr(q), _ptr(t)) != 0:
        raise ValueError("place_relative: bad argument")
    return q, t


def _as_cloud(a):
    if isinstance(a, Cloud):
        return a
    a = np.ascontiguousarray(a, np.float32)
    return cloud_from_numpy(a, aux_col=3 if a.shape[1] > 3 else None)


class PlaceRecognition:
    """Descriptors of a KeyframeArchive's keyframes and their search.  A descriptor is an (n_sector, n_ring) float32 array (a sector's column is a row of it)."""

    def __init__(self, archive, n_ring=None, n_sector=None, max_radius=None, lidar_height=None, kind=ARCHIVE_FULL, back=0, fwd=0, level=False):
        """back / fwd / level: the submap setting (all zero: a keyframe's own rows in the LiDAR frame).  Otherwise keyframe i is described by the rows of keyframes
        i - back .. i + fwd placed in its frame, levelled to the map's z if `level`; a window is counted in keyframes, by index."""
        self.archive, self.ctx, self.lib = archive, archive.ctx, archive.ctx.lib
        self.submap = PlaceSubmap(int(back), int(fwd), int(level), 0)
        p = default_place_params()
        for k, v in (("n_ring", n_ring), ("n_sector", n_sector), ("max_radius", max_radius), ("lidar_height", lidar_height), ("kind", kind)):
            if v is not None:
                setattr(p, k, v)
        self.params = p

    @property
    def shape(self):
        return self.params.n_sector, self.params.n_ring

    def _set(self):
        """this object's submap setting becomes the context's (another one than the context holds drops every descriptor)"""
        self.ctx._chk(self.lib.lili_place_set_submap(self.ctx.h, C.byref(self.submap)))

    def update(self):
        """Describes every archived keyframe that has no descriptor yet and, in a submap setting, every keyframe whose window or relative poses changed; returns
        how many it built."""
        self._set()
        n = C.c_int(0)
        self.ctx._chk(self.lib.lili_place_update(self.ctx.h, C.byref(self.params), C.byref(n)))
        return n.value

    def descriptor(self, kid):
        out = np.zeros(self.shape, np.float32)
        self.ctx._chk(self.lib.lili_place_get(self.ctx.h, int(kid), _ptr(out)))
        return out

    def window(self, kid):
        """(first, last): the keyframes descriptor kid was built from"""
        a, b = C.c_int(0), C.c_int(0)
        self.ctx._chk(self.lib.lili_place_window(self.ctx.h, int(kid), C.byref(a), C.byref(b)))
        return a.value, b.value

    def frame_pose(self, kid):
        """the frame keyframe kid's descriptor is built in, as 7 doubles: its LiDAR map pose, levelled if the setting says so"""
        return place_frame(self.map_pose(kid), self.submap.level)

    def describe_submap(self, clouds, frame=None, poses=None, rel=None):
        """The descriptor of a list of clouds (as describe takes them) whose LiDAR map poses are `poses`, in `frame` (7 doubles each) — or placed by rel[i] =
        (q_rel, t_rel) directly.  A pose or rel entry of None — or neither poses nor rel — reads that cloud untransformed.  The kernel and the bytes of the
        archive path."""
        cs = [_as_cloud(c) for c in clouds]
        arr = (Cloud * max(len(cs), 1))(*cs)
        if rel is None and frame is not None and poses is not None:
            rel = [None if p is None else place_relative(frame, p) for p in poses]
        q = t = None
        if rel is not None:
            q, t = np.zeros((len(cs), 4)), np.zeros((len(cs), 3))
            for i, r in enumerate(rel):
                if r is not None:
                    q[i], t[i] = r
        out = np.zeros(self.shape, np.float32)
        self.ctx._chk(self.lib.lili_place_describe_submap(self.ctx.h, arr, len(cs), _ptr(q), _ptr(t), C.byref(self.params), _ptr(out)))
        return out

    def describe(self, cloud):
        """The descriptor of any cloud: numpy rows (x, y, z[, aux]) or an api.Cloud description of host, page-locked or device memory."""
        c = _as_cloud(cloud)
        out = np.zeros(self.shape, np.float32)
        self.ctx._chk(self.lib.lili_place_describe(self.ctx.h, C.byref(c), C.byref(self.params), _ptr(out)))
        return out

    def info(self):
        """(described keyframes, the parameters they were built with, device bytes of the descriptor store)"""
        n, p, b = C.c_int(0), PlaceParams(), C.c_int64(0)
        self.ctx._chk(self.lib.lili_place_info(self.ctx.h, C.byref(n), C.byref(p), C.byref(b)))
        return n.value, p, b.value

    def search(self, queries, k=1, min_time_gap=0.0, max_id=None, times=None):
        """Per query the up to k best (id, shift, distance), ascending by (distance, id).  A query is an archived keyframe's id or a descriptor array;
        min_time_gap, max_id (None: no bound) and times (None: the archive's time of an archived query) are scalars or one value per query.  A candidate is
        eligible iff id <= max_id, |time - the query's time| > min_time_gap, and it is not the query itself."""
        n_q = len(queries)

        def per_query(v):
            return list(v) if isinstance(v, (list, tuple, np.ndarray)) else [v] * n_q

        gaps, max_ids, tms = per_query(min_time_gap), per_query(max_id), per_query(times)
        arr, keep = (PlaceQuery * max(n_q, 1))(), []
        for i, q in enumerate(queries):
            if isinstance(q, (int, np.integer)):
                arr[i].id, arr[i].desc = int(q), None
                t = self.archive.pose(int(q))[2] if tms[i] is None else tms[i]
            else:
                d = np.ascontiguousarray(q, np.float32)
                if d.shape != self.shape:
                    raise ValueError(f"search: a descriptor is {self.shape}")
                if tms[i] is None:
                    raise ValueError("search: a descriptor query needs its time")
                keep.append(d)
                arr[i].id, arr[i].desc, t = -1, d.ctypes.data, tms[i]
            arr[i].time, arr[i].min_time_gap = float(t), float(gaps[i])
            arr[i].max_id = INT32_MAX if max_ids[i] is None else int(max_ids[i])
        out, found = (PlaceMatch * max(n_q * int(k), 1))(), (C.c_int * max(n_q, 1))()
        self.ctx._chk(self.lib.lili_place_search(self.ctx.h, arr, n_q, int(k), out, found))
        return [[(out[i * int(k) + j].id, out[i * int(k) + j].shift, out[i * int(k) + j].distance) for j in range(found[i])] for i in range(n_q)]

    def map_pose(self, kid):
        """Keyframe kid's LiDAR map pose (q_po q_bl, q_po t_bl + t_po) as 7 doubles (p, then q w x y z)."""
        t_po, q_po, _ = self.archive.pose(kid)
        t, q = keyframe_map_pose(t_po, q_po, self.archive.t_bl, self.archive.q_bl)
        return np.concatenate([t, q])

    def guess(self, src, dst, shift):
        """align's guess for source keyframe `src` matched to candidate `dst` at `shift`; src / dst are keyframe ids or 7-double frame poses (frame_pose: the
        LiDAR map poses unless the descriptors are levelled)."""
        a = self.frame_pose(src) if isinstance(src, (int, np.integer)) else src
        b = self.frame_pose(dst) if isinstance(dst, (int, np.integer)) else dst
        return place_guess(a, b, shift, self.params.n_sector)
