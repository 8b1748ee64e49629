"""Localisation in a finished map: a scan is matched against the part of a global map the sensor can reach.  Host-side rule over existing calls —
lili_global_map_crop into a device buffer, lili_map_set on that buffer, the frame call with LILI_FRAME_EXTERNAL_MAP — with no entry point of its own: the host
synchronises for the crop's count, for the index build and for the frame's result (a fused call is the open item of §7n).  Not in the reference."""
import ctypes as C

import numpy as np

from .api import (Cloud, FrontendOdometry, RotFrontendOdometry, LiliError, KIND_SURF, MEM_DEVICE, _f64, make_params)


class MapLocalizer:
    """frame(scan, t_pred, q_pred, q_imu) -> (t, q, info): the pose of a scan in the map of `global_map` (a GlobalMap of this context that holds a table — built, or
    loaded with GlobalMap.load / load_table; kind SURF at the front end's leaf_map is what the surf queries expect).  The matcher sees the crop
    c +- (half_xy, half_xy, half_z) of the table, c = the prediction at the last re-crop; a frame whose prediction has left c by more than `refresh` metres in x or y
    crops again.  variant "livox" / "rot" chooses the frame call (lili_frontend_frame / lili_frontend_frame_rot); `frontend` are further arguments of
    FrontendOdometry / RotFrontendOdometry (extractor thresholds, n_scans, q_lb, ...).  Surf queries only: one table per context, so an edge map stays the caller's."""

    def __init__(self, ctx, global_map, variant="livox", half_xy=60.0, half_z=20.0, refresh=15.0, n_iters=6, leaf_query=0.4, params=None, slot=0, capacity=1 << 16,
                 **frontend):
        if global_map.ctx is not ctx:
            raise ValueError("MapLocalizer: the global map must live in the context the scans are matched in")
        if variant not in ("livox", "rot"):
            raise ValueError("MapLocalizer: variant is 'livox' or 'rot'")
        self.ctx, self.lib, self.gm = ctx, ctx.lib, global_map
        self.params = params if params is not None else make_params("frontend")
        odo = FrontendOdometry if variant == "livox" else RotFrontendOdometry
        self.odo = odo(ctx, self.params, leaf_query=leaf_query, slot=slot, scan_match_cnt=n_iters, external_map=True, **frontend)
        self.half = np.array([half_xy, half_xy, half_z], np.float64)
        self.refresh = float(refresh)
        self.center, self.n_map, self.n_crops = None, 0, 0
        self._buf, self._cap = None, int(capacity)

    def _crop(self, c):
        """the table inside c +- half (the box rounded to f32) into the device buffer, grown by half when short, and the surf index over it"""
        import torch
        lo, hi = (c - self.half).astype(np.float32), (c + self.half).astype(np.float32)
        while True:
            if self._buf is None or self._buf.shape[0] < self._cap:
                self._buf = torch.empty((self._cap, 4), dtype=torch.float32, device="cuda")
            n = self.gm.crop_into(lo, hi, self._buf.data_ptr(), self._cap)
            if n <= self._cap:
                break
            self._cap = max(n, self._cap + self._cap // 2)
        if n == 0:
            raise LiliError(f"MapLocalizer: the map holds nothing within {tuple(self.half)} m of {tuple(c)}")
        cloud = Cloud(self._buf.data_ptr(), n, 16, 12, MEM_DEVICE)
        self.ctx._chk(self.lib.lili_map_set(self.ctx.h, KIND_SURF, C.byref(cloud), float(self.params.kd_max_radius)))
        self.center, self.n_map = c.copy(), n
        self.n_crops += 1

    def frame(self, scan, t_pred, q_pred, q_imu=(1.0, 0, 0, 0)):
        """scan: as the variant's frame call takes it.  info is the frame call's, plus recropped (this frame cropped the map again), n_map (voxels in the crop) and
        crop_center.  Raises LiliError before any frame call if the crop is empty."""
        t_pred = _f64(t_pred, 3)
        recropped = self.center is None or max(abs(t_pred[0] - self.center[0]), abs(t_pred[1] - self.center[1])) > self.refresh
        if recropped:
            self._crop(t_pred)
        t, q, info = self.odo.frame(scan, t_pred, q_pred, q_imu)
        info.update(recropped=recropped, n_map=self.n_map, crop_center=self.center.copy())
        return t, q, info
