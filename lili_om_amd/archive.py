"""Keyframe archive and global map on the device (lili_archive_* / lili_global_map*): saveKeyFramesAndFactors keeps every keyframe's clouds
(L/src/BackendFusion.cpp:1494-1514), correctPoses gives them new poses (L:2177-2311), publishCompleteMap builds the map (L:2644-2685).  Publishing and PCD writing
stay with the caller."""
import ctypes as C

import numpy as np

from .api import Cloud, FeatureOut, MEM_HOST, _f64, _ptr, cloud_from_numpy

ARCHIVE_EDGE, ARCHIVE_SURF, ARCHIVE_FULL = 0, 1, 2


def _as_cloud(a):
    if a is None or isinstance(a, Cloud):
        return a
    a = np.ascontiguousarray(a, np.float32)
    return cloud_from_numpy(a, aux_col=3 if a.shape[1] > 3 else None)


def _ref(c):
    return None if c is None else C.byref(c)


class KeyframeArchive:
    """Every keyframe's edge / surf / full cloud in device memory (float4 rows in the LiDAR frame, as pushed) with its body pose and time.  Clouds are numpy rows
    (x, y, z[, aux]), api.Cloud descriptions of host, page-locked or device memory, or None (kind absent).  One archive per context."""

    def __init__(self, ctx, q_bl=(1.0, 0.0, 0.0, 0.0), t_bl=(0.0, 0.0, 0.0), max_mb=None, slab_mb=None):
        self.ctx, self.lib = ctx, ctx.lib
        if max_mb is not None:
            ctx.set_option("archive_max_mb", max_mb)
        if slab_mb is not None:
            ctx.set_option("archive_slab_mb", slab_mb)
        self.reset()
        self.set_extrinsic(t_bl, q_bl)

    def reset(self):
        self.ctx._chk(self.lib.lili_archive_reset(self.ctx.h))

    def set_extrinsic(self, t_bl, q_bl):
        t, q = _f64(t_bl, 3), _f64(q_bl, 4)
        self.ctx._chk(self.lib.lili_archive_set_extrinsic(self.ctx.h, _ptr(t), _ptr(q)))
        self.t_bl, self.q_bl = t.copy(), q.copy()

    def push(self, edge, surf, full, time, t_po, q_po):
        """Appends a keyframe; returns its id."""
        e, s, f = _as_cloud(edge), _as_cloud(surf), _as_cloud(full)
        t, q, i = _f64(t_po, 3), _f64(q_po, 4), C.c_int(-1)
        self.ctx._chk(self.lib.lili_archive_push(self.ctx.h, _ref(e), _ref(s), _ref(f), float(time), _ptr(t), _ptr(q), C.byref(i)))
        return i.value

    def push_slot(self, slot, full, time, t_po, q_po):
        """edge / surf = the queries of matcher slot `slot`, device to device."""
        f = _as_cloud(full)
        t, q, i = _f64(t_po, 3), _f64(q_po, 4), C.c_int(-1)
        self.ctx._chk(self.lib.lili_archive_push_slot(self.ctx.h, int(slot), _ref(f), float(time), _ptr(t), _ptr(q), C.byref(i)))
        return i.value

    def set_poses(self, first, ts_po, qs_po):
        t = np.ascontiguousarray(np.asarray(ts_po, np.float64).reshape(-1, 3))
        q = np.ascontiguousarray(np.asarray(qs_po, np.float64).reshape(-1, 4))
        if t.shape[0] != q.shape[0]:
            raise ValueError("set_poses: as many translations as rotations")
        self.ctx._chk(self.lib.lili_archive_set_poses(self.ctx.h, int(first), t.shape[0], _ptr(t), _ptr(q)))

    def info(self):
        """(keyframes, (edge, surf, full) points, bytes of device memory)"""
        n, pts, b = C.c_int(0), (C.c_int64 * 3)(), C.c_int64(0)
        self.ctx._chk(self.lib.lili_archive_info(self.ctx.h, C.byref(n), pts, C.byref(b)))
        return n.value, tuple(int(v) for v in pts), b.value

    def __len__(self):
        return self.info()[0]

    def pose(self, kid):
        """(t_po (3,), q_po (4,) wxyz, time) of keyframe kid"""
        t, q, tm = np.zeros(3), np.zeros(4), C.c_double(0)
        self.ctx._chk(self.lib.lili_archive_pose(self.ctx.h, int(kid), _ptr(t), _ptr(q), C.byref(tm)))
        return t, q, tm.value

    def poses(self):
        """(ts_po (n, 3), qs_po (n, 4), times (n,)) of all keyframes"""
        out = [self.pose(k) for k in range(len(self))]
        return (np.array([o[0] for o in out]).reshape(-1, 3), np.array([o[1] for o in out]).reshape(-1, 4), np.array([o[2] for o in out], np.float64))

    def get(self, kid, kind):
        """(n, 4) float32 rows (x, y, z, aux) of keyframe kid's cloud of `kind`"""
        fo = FeatureOut(None, 0, 16, MEM_HOST, 0)
        self.ctx._chk(self.lib.lili_archive_get(self.ctx.h, int(kid), int(kind), C.byref(fo)))
        out = np.zeros((max(fo.count, 1), 4), np.float32)
        fo = FeatureOut(out.ctypes.data, fo.count, 16, MEM_HOST, 0)
        self.ctx._chk(self.lib.lili_archive_get(self.ctx.h, int(kid), int(kind), C.byref(fo)))
        return out[:fo.count]

    def view(self, kid, kind):
        """api.Cloud device view of the rows (valid until reset / close)"""
        c = Cloud()
        self.ctx._chk(self.lib.lili_archive_view(self.ctx.h, int(kid), int(kind), C.byref(c)))
        return c


class GlobalMap:
    """publishCompleteMap on the archive's keyframes: an accumulating voxel table, bit-identical to one VoxelGrid over everything."""

    def __init__(self, archive, batch_points=None):
        self.archive, self.ctx, self.lib = archive, archive.ctx, archive.ctx.lib
        if batch_points is not None:
            self.ctx.set_option("global_map_batch_points", batch_points)

    def build(self, kind=ARCHIVE_FULL, interval=1, leaf=0.3):
        """(n_raw, n_map): folds what the table does not hold yet, or rebuilds if something it rests on has changed"""
        a, b = C.c_int64(0), C.c_int64(0)
        self.ctx._chk(self.lib.lili_global_map(self.ctx.h, int(kind), int(interval), float(leaf), C.byref(a), C.byref(b)))
        return a.value, b.value

    def get(self):
        """(centroids (m, 4) float32 in voxel-index order, counts (m,) int32)"""
        fo = FeatureOut(None, 0, 16, MEM_HOST, 0)
        self.ctx._chk(self.lib.lili_global_map_get(self.ctx.h, C.byref(fo), None))
        m = fo.count
        out, cnt = np.zeros((max(m, 1), 4), np.float32), np.zeros(max(m, 1), np.int32)
        fo = FeatureOut(out.ctypes.data, m, 16, MEM_HOST, 0)
        self.ctx._chk(self.lib.lili_global_map_get(self.ctx.h, C.byref(fo), _ptr(cnt)))
        return out[:m], cnt[:m]

    def get_device(self, d_ptr, capacity):
        """centroids into a caller's device float4 buffer; returns the number of voxels"""
        fo = FeatureOut(d_ptr, int(capacity), 16, 1, 0)
        self.ctx._chk(self.lib.lili_global_map_get(self.ctx.h, C.byref(fo), None))
        return fo.count

    def crop_into(self, lo, hi, d_ptr, capacity, d_counts=None):
        """lili_global_map_crop into a caller's device buffers (float4 rows; int32 counts, optional): returns the voxels in the box — more than `capacity` means only
        the first `capacity` were written."""
        lo, hi = np.asarray(lo, np.float32).reshape(3), np.asarray(hi, np.float32).reshape(3)
        fo, n = FeatureOut(d_ptr, int(capacity), 16, 1, 0), C.c_int64(0)
        self.ctx._chk(self.lib.lili_global_map_crop(self.ctx.h, _ptr(lo), _ptr(hi), C.byref(fo), d_counts, C.byref(n)))
        return n.value

    def crop(self, lo, hi, device=False):
        """The voxels a point of the closed box [lo, hi] would fall into (+-inf allowed): (centroids (m, 4) float32, counts (m,) int32) in table order —
        numpy arrays, or with device = True torch tensors on the context's device."""
        lo, hi = np.asarray(lo, np.float32).reshape(3), np.asarray(hi, np.float32).reshape(3)
        fo, n = FeatureOut(None, 0, 16, MEM_HOST, 0), C.c_int64(0)
        self.ctx._chk(self.lib.lili_global_map_crop(self.ctx.h, _ptr(lo), _ptr(hi), C.byref(fo), None, C.byref(n)))
        m = n.value
        if device:
            import torch
            out, cnt = torch.empty((max(m, 1), 4), dtype=torch.float32, device="cuda"), torch.empty(max(m, 1), dtype=torch.int32, device="cuda")
            if m:
                self.crop_into(lo, hi, out.data_ptr(), m, cnt.data_ptr())
            return out[:m], cnt[:m]
        out, cnt = np.zeros((max(m, 1), 4), np.float32), np.zeros(max(m, 1), np.int32)
        if m:
            fo = FeatureOut(out.ctypes.data, m, 16, MEM_HOST, 0)
            self.ctx._chk(self.lib.lili_global_map_crop(self.ctx.h, _ptr(lo), _ptr(hi), C.byref(fo), _ptr(cnt), C.byref(n)))
        return out[:m], cnt[:m]

    def export(self):
        """The table itself: dict(keys (m,) uint64 ascending, sums (m, 4) float32, counts (m,) int32, leaf float32, kind int) — what load_table takes."""
        n, leaf, kind = C.c_int64(0), C.c_float(0), C.c_int(0)
        self.ctx._chk(self.lib.lili_global_map_export(self.ctx.h, 0, None, None, None, C.byref(n), C.byref(leaf), C.byref(kind)))
        m = n.value
        keys, sums, cnt = np.zeros(max(m, 1), np.uint64), np.zeros((max(m, 1), 4), np.float32), np.zeros(max(m, 1), np.int32)
        self.ctx._chk(self.lib.lili_global_map_export(self.ctx.h, m, _ptr(keys), _ptr(sums), _ptr(cnt), C.byref(n), C.byref(leaf), C.byref(kind)))
        return dict(keys=keys[:m], sums=sums[:m], counts=cnt[:m], leaf=np.float32(leaf.value), kind=kind.value)

    def load_table(self, keys, sums, counts, leaf, kind):
        """An exported table into this context (lili_global_map_import): it serves get / crop / export / info; the next build() does not extend it but starts from
        an empty table and this context's archive.  Raises LiliError (and leaves no map) if it is not a table."""
        keys, cnt = np.ascontiguousarray(keys, np.uint64).reshape(-1), np.ascontiguousarray(counts, np.int32).reshape(-1)
        sums = np.ascontiguousarray(sums, np.float32).reshape(-1, 4)
        if not keys.shape[0] == sums.shape[0] == cnt.shape[0]:
            raise ValueError("load_table: keys, sums and counts of one length")
        self.ctx._chk(self.lib.lili_global_map_import(self.ctx.h, float(np.float32(leaf)), int(kind), keys.shape[0], _ptr(keys), _ptr(sums), _ptr(cnt)))
        return keys.shape[0]

    FILE_VERSION = 1

    def save(self, path):
        """numpy.savez of export() plus version = 1 (a path without ".npz" gets it appended, as numpy does)"""
        np.savez(path, version=np.int32(self.FILE_VERSION), **self.export())

    def load(self, path):
        """load_table of a file written by save; returns the number of voxels"""
        with np.load(path) as f:
            version = int(f["version"])
            if version != self.FILE_VERSION:
                raise ValueError(f"{path}: map file version {version}, this package reads version {self.FILE_VERSION}")
            return self.load_table(f["keys"], f["sums"], f["counts"], np.float32(f["leaf"]), int(f["kind"]))

    def stats(self):
        """(incremental calls, rebuilds, points folded by the last call)"""
        a, b, c = C.c_int32(0), C.c_int32(0), C.c_int64(0)
        self.ctx._chk(self.lib.lili_global_map_stats(self.ctx.h, C.byref(a), C.byref(b), C.byref(c)))
        return a.value, b.value, c.value

    def info(self):
        """(bytes of the table, bytes of a batch's work buffers)"""
        a, b = C.c_int64(0), C.c_int64(0)
        self.ctx._chk(self.lib.lili_global_map_info(self.ctx.h, C.byref(a), C.byref(b)))
        return a.value, b.value
