"""numpy restatement of pcl::VoxelGrid (PCL >= 1.8, App. B2) with the library's arithmetic: the plain reference the device filter is held to bit for bit.

Non-finite rows are dropped; inv = 1.0f / leaf; the box is floor(f32(coord * inv)) of the extremes; a point's voxel index is int(floor(f32(p * inv)) - f32(min_b)) per axis,
key = i0 + i1 div0 + i2 div0 div1 (refused beyond int32, as PCL does); the points are ordered by a stable sort on the key; a centroid is the f32 sum of its members in
that order, starting at 0.0f, divided by f32(count)."""
import numpy as np


class IndexOverflow(ValueError):
    """PCL's "leaf size is too small for the input dataset": div0 div1 div2 > 2^31 - 1"""


def voxel_keys(pts, leaf):
    """(finite rows (m, 4) f32, keys (m,) int64, div (3,) int64) of an (n, >= 3) cloud"""
    p = np.asarray(pts, np.float32)
    if p.shape[1] < 4:
        p = np.concatenate([p[:, :3], np.zeros((p.shape[0], 1), np.float32)], 1)
    p = p[np.isfinite(p[:, :3]).all(1)][:, :4]
    if p.shape[0] == 0:
        raise ValueError("voxel_grid: cloud holds no finite point")
    inv = np.float32(1.0) / np.float32(leaf)
    fl = np.floor(p[:, :3] * inv)                                  # f32 product, f32 floor
    min_b = fl.min(0).astype(np.int64)                             # floor(min * inv) == min floor(p * inv): the f32 product is monotonic
    max_b = fl.max(0).astype(np.int64)
    div = max_b - min_b + 1
    if int(div[0]) * int(div[1]) * int(div[2]) > 2**31 - 1:
        raise IndexOverflow("voxel_grid: leaf size too small for the cloud extent")
    ijk = (fl - min_b.astype(np.float32)).astype(np.int64)         # f32 subtraction, truncation
    keys = ijk[:, 0] + ijk[:, 1] * div[0] + ijk[:, 2] * (div[0] * div[1])
    return p, keys, div


def voxel_grid(pts, leaf):
    """(centroids (m, 4) f32 — x, y, z, aux —, counts (m,) int32) in voxel-index order"""
    p, keys, _ = voxel_keys(pts, leaf)
    order = np.argsort(keys, kind="stable")
    ks, ps = keys[order], p[order]
    head = np.ones(ks.shape[0], bool)
    head[1:] = ks[1:] != ks[:-1]
    start = np.flatnonzero(head)
    counts = np.diff(np.append(start, ks.shape[0]))
    # sequential f32 sums: round r adds the r-th member of every voxel that has one (np.sum / reduceat would change the order of the additions)
    acc = np.zeros((start.shape[0], 4), np.float32)
    by_size = np.argsort(-counts, kind="stable")                   # voxels by decreasing size: round r works on a prefix of them
    sizes = counts[by_size]
    for r in range(int(counts.max())):
        live = by_size[: np.searchsorted(-sizes, -r, side="left")]  # voxels with more than r members
        acc[live] += ps[start[live] + r]
    return acc / counts.astype(np.float32)[:, None], counts.astype(np.int32)


# ---- clouds at the filter's edges (shared by the CPU and the GPU tests) -------------------------------------------------------------------------------------------------
LEAF = 0.4
SIZES = [1, 2, 63, 64, 65, 8191, 8192, 8193, 262_143, 262_144, 262_145, 1_048_576, 1_048_577, 1_200_000]      # keys: tile sizes, k_voxel_small, 256 tiles
# (extent x, y, z in m, leaf) whose keys need <= 8, 9-16, 17-24 and 25-31 bits: 1 to 4 radix passes of 8-bit digits
BITS = {8: ((2.0, 2.0, 2.0), 0.4), 16: ((20.0, 20.0, 5.0), 0.4), 24: ((100.0, 100.0, 10.0), 0.4), 31: ((200.0, 200.0, 50.0), 0.1)}
OVERFLOW = ((200.0, 200.0, 60.0), 0.1)                                                                   # 2001 x 2001 x 601 voxels > 2^31 - 1
OCCUPANCY = [1, 4, 5, 36, 37, 1024, 1025, 1040, 5000]                                                      # around the member tiers of k_vox_centroid


def sized_cloud(n, seed=0):
    """n finite rows in a 60 m box, a tenth of them exact duplicates (voxels of several points for sure)"""
    rng = np.random.default_rng(seed + n)
    pts = np.concatenate([rng.uniform(-60, 60, (n, 2)), rng.normal(0, 0.5, (n, 1)), rng.uniform(0, 25, (n, 1))], 1).astype(np.float32)
    pts[: n // 10] = pts[n // 10: 2 * (n // 10)][: n // 10]
    return pts


def box_cloud(extent, n, seed=0):
    """n rows filling [0, extent) per axis, both corners included (the box spans the whole key range)"""
    rng = np.random.default_rng(seed)
    pts = np.concatenate([rng.uniform(0, 1, (n, 3)) * np.asarray(extent), rng.uniform(0, 25, (n, 1))], 1).astype(np.float32)
    pts[0, :3] = 0.0
    pts[1, :3] = np.asarray(extent, np.float32) * np.float32(0.9999)
    return pts


def cluster_cloud(leaf=LEAF, seed=0):
    """jittered clusters of OCCUPANCY members, each inside one voxel, among sparse points and non-finite rows, shuffled"""
    rng = np.random.default_rng(seed)
    parts = []
    for k, m in enumerate(OCCUPANCY):
        centre = (np.array([3 * k, 2 * k, k % 5], np.float64) + 0.5) * leaf
        xyz = centre + rng.uniform(-0.4 * leaf, 0.4 * leaf, (m, 3))
        parts.append(np.concatenate([xyz, rng.uniform(0, 100, (m, 1))], 1))
    sparse = np.concatenate([rng.uniform(-30, 30, (20_000, 3)), rng.uniform(0, 100, (20_000, 1))], 1)
    pts = np.concatenate(parts + [sparse]).astype(np.float32)
    bad = np.array([[np.nan, 0, 0, 1], [0, np.inf, 0, 1], [0, 0, -np.inf, 1], [np.nan, np.nan, np.nan, np.nan]], np.float32)
    pts = np.concatenate([pts, np.repeat(bad, 25, 0)])
    return pts[rng.permutation(pts.shape[0])]
