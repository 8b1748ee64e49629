"""numpy model of the global map's accumulating voxel table: per occupied voxel an ABSOLUTE key — (k, j, i) = floor(f32(p * inv_leaf)) packed
lexicographically —, the running f32 sum and the count, sorted by key.  A batch continues every voxel's left fold from the stored sum (0.0f for a new voxel) over the
batch's members in order.  The claim pinned by tests/test_global_map_model_cpu.py: for any split of a cloud into batches the table equals tests/voxel_model.voxel_grid
of the whole cloud — centroids, counts and order, bit for bit."""
import numpy as np

OFFSET = 1 << 20


def abs_keys(p, leaf):
    """int64 keys of FINITE rows"""
    inv = np.float32(1.0) / np.float32(leaf)
    fl = np.floor(p[:, :3] * inv).astype(np.int64) + OFFSET
    assert (fl >= 0).all() and (fl < 2 * OFFSET).all(), "beyond the key range"
    return (fl[:, 2] << 42) | (fl[:, 1] << 21) | fl[:, 0]


class FoldTable:
    def __init__(self, leaf):
        self.leaf = leaf
        self.keys = np.zeros(0, np.int64)
        self.sums = np.zeros((0, 4), np.float32)
        self.counts = np.zeros(0, np.int64)

    def fold(self, pts):
        p = np.asarray(pts, np.float32).reshape(-1, 4)
        p = p[np.isfinite(p[:, :3]).all(1)]
        if p.shape[0] == 0:
            return
        keys = abs_keys(p, self.leaf)
        order = np.argsort(keys, kind="stable")
        ks, ps = keys[order], p[order]
        head = np.ones(ks.shape[0], bool)
        head[1:] = ks[1:] != ks[:-1]
        start = np.flatnonzero(head)
        counts = np.diff(np.append(start, ks.shape[0]))
        bkeys = ks[start]
        pos = np.searchsorted(self.keys, bkeys)
        found = np.zeros(bkeys.shape[0], bool)
        inside = pos < self.keys.shape[0]
        found[inside] = self.keys[pos[inside]] == bkeys[inside]
        acc = np.zeros((bkeys.shape[0], 4), np.float32)
        acc[found] = self.sums[pos[found]]
        base = np.zeros(bkeys.shape[0], np.int64)
        base[found] = self.counts[pos[found]]
        by_size = np.argsort(-counts, kind="stable")
        sizes = counts[by_size]
        for r in range(int(counts.max())):      # round r adds the r-th member of every voxel that has one: sequential f32 sums in member order
            live = by_size[: np.searchsorted(-sizes, -r, side="left")]
            acc[live] += ps[start[live] + r]
        self.sums[pos[found]] = acc[found]
        self.counts[pos[found]] = base[found] + counts[found]
        new = ~found
        keys_all = np.concatenate([self.keys, bkeys[new]])
        o = np.argsort(keys_all, kind="stable")
        self.keys = keys_all[o]
        self.sums = np.concatenate([self.sums, acc[new]])[o]
        self.counts = np.concatenate([self.counts, counts[new]])[o]

    def result(self):
        return self.sums / self.counts.astype(np.float32)[:, None], self.counts.astype(np.int32)


def qrot(q, v):
    """q * v as Eigen evaluates it (f64), rows of v"""
    u = np.asarray(q[1:4], np.float64)
    uv = np.cross(u, v)
    uv = uv + uv
    return (v + uv * q[0]) + np.cross(u, uv)


def place(cloud, t, q):
    """transformCloud: p' = q * p + t in f64, stored f32; aux carried along (absent: 0)"""
    c = np.asarray(cloud, np.float32)
    out = np.zeros((c.shape[0], 4), np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        out[:, :3] = (qrot(np.asarray(q, np.float64), c[:, :3].astype(np.float64)) + np.asarray(t, np.float64)).astype(np.float32)
    if c.shape[1] > 3:
        out[:, 3] = c[:, 3]
    return out
