"""Exact 5-NN by brute force with FLANN's f32 L2_Simple arithmetic, (dx*dx + dy*dy) + dz*dz, ordered by (d2, map index) — the order the
library's exact selector keys use.  Candidates are cut to the cube of half-edge `reach` around each query first (the map sorted by x once), so
that a 5 M-point map costs milliseconds per query: every point with d2 < reach^2 lies in that cube, so results whose fifth distance is below
reach^2 are exact; a query with fewer than five candidates gets index -1 and d2 = +inf in the empty places."""
import numpy as np


class BruteKnn5:
    def __init__(self, mp):
        self.mp = np.ascontiguousarray(np.asarray(mp, np.float32)[:, :3])
        self.order = np.argsort(self.mp[:, 0], kind="stable")
        self.xs = self.mp[self.order, 0].astype(np.float64)

    def query(self, qw, reach=1.01):
        qw = np.asarray(qw, np.float32)[:, :3]
        idx = np.full((qw.shape[0], 5), -1, np.int32)
        d2 = np.full((qw.shape[0], 5), np.inf, np.float32)
        for i, q in enumerate(qw):
            if not np.isfinite(q).all():
                continue
            lo = int(np.searchsorted(self.xs, float(q[0]) - reach, side="left"))
            hi = int(np.searchsorted(self.xs, float(q[0]) + reach, side="right"))
            cand = self.order[lo:hi]
            c = self.mp[cand]
            keep = (np.abs(c[:, 1].astype(np.float64) - float(q[1])) <= reach) & (np.abs(c[:, 2].astype(np.float64) - float(q[2])) <= reach)
            cand, c = cand[keep], c[keep]
            dx = q[0] - c[:, 0]; dy = q[1] - c[:, 1]; dz = q[2] - c[:, 2]
            d = (dx * dx + dy * dy) + dz * dz
            o = np.lexsort((cand, d))[:5]
            idx[i, :o.size] = cand[o]
            d2[i, :o.size] = d[o]
        return idx, d2
