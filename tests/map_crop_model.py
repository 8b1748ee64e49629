"""The crop of the global map's table by a box (lili_global_map_crop) in plain numpy.

A table is its sorted keys, key = k << 42 | j << 21 | i with (i, j, k) = floorf(p * inv_leaf) + 2^20 per axis (x, y, z), inv_leaf = the f32 1.0f / leaf.  The crop
keeps the voxels whose index lies in [face(lo), face(hi)] on every axis, face(x) = floorf(x * inv_leaf) in f32, offset by 2^20 and clipped to [0, 2^21 - 1].

crop_mask is the contract: a brute-force mask over the keys.  crop_runs is the device's route — per (k, j) row of the box one lower and one upper bound over the sorted
keys, k clipped to the table's first and last key — and returns the selected positions in order; tests/test_map_crop_model_cpu.py checks that the two agree."""
import numpy as np

OFFSET, FIELD = 1 << 20, (1 << 21) - 1
MAX_ROWS = 1 << 24


class TooManyRows(ValueError):
    pass


def inv_leaf_of(leaf):
    return np.float32(1.0) / np.float32(leaf)


def face_index(x, leaf):
    """voxel index of a face at coordinate x (f32; +-inf allowed): floorf(x * inv_leaf) + 2^20 clipped to [0, 2^21 - 1]"""
    with np.errstate(over="ignore", invalid="ignore"):
        f = np.floor(np.float32(x) * inv_leaf_of(leaf))
    if f < -float(OFFSET):
        return 0
    if f >= float(OFFSET):
        return FIELD
    return int(f) + OFFSET


def box_indices(lo, hi, leaf):
    """((i0, j0, k0), (i1, j1, k1)) of the box; ValueError for lo > hi on an axis or a NaN"""
    lo, hi = np.asarray(lo, np.float32).reshape(3), np.asarray(hi, np.float32).reshape(3)
    if not (lo <= hi).all():
        raise ValueError("lo > hi on an axis, or a NaN")
    return tuple(face_index(v, leaf) for v in lo), tuple(face_index(v, leaf) for v in hi)


def unpack(keys):
    keys = np.asarray(keys, np.uint64)
    f = np.uint64(FIELD)
    return (keys & f).astype(np.int64), ((keys >> np.uint64(21)) & f).astype(np.int64), (keys >> np.uint64(42)).astype(np.int64)


def pack(i, j, k):
    return (np.asarray(k, np.uint64) << np.uint64(42)) | (np.asarray(j, np.uint64) << np.uint64(21)) | np.asarray(i, np.uint64)


def point_keys(xyz, leaf):
    """abs_voxel_key of finite f32 points within +-2^20 voxels"""
    v = np.floor(np.asarray(xyz, np.float32)[:, :3] * inv_leaf_of(leaf)).astype(np.int64) + OFFSET
    assert ((v >= 0) & (v <= FIELD)).all()
    return pack(v[:, 0], v[:, 1], v[:, 2])


def crop_mask(keys, lo, hi, leaf):
    """positions of the table's voxels inside the box, ascending: the brute-force mask"""
    (i0, j0, k0), (i1, j1, k1) = box_indices(lo, hi, leaf)
    i, j, k = unpack(keys)
    return np.flatnonzero((i >= i0) & (i <= i1) & (j >= j0) & (j <= j1) & (k >= k0) & (k <= k1))


def crop_runs(keys, lo, hi, leaf):
    """the same positions by the run argument: (begin, length) per (k, j) row from two bisections, concatenated in row order"""
    keys = np.asarray(keys, np.uint64)
    (i0, j0, k0), (i1, j1, k1) = box_indices(lo, hi, leaf)
    if keys.shape[0] == 0:
        return np.zeros(0, np.int64)
    k0, k1 = max(k0, int(keys[0] >> np.uint64(42))), min(k1, int(keys[-1] >> np.uint64(42)))
    if k0 > k1:
        return np.zeros(0, np.int64)
    n_rows = (k1 - k0 + 1) * (j1 - j0 + 1)
    if n_rows > MAX_ROWS:
        raise TooManyRows(n_rows)
    kk, jj = np.meshgrid(np.arange(k0, k1 + 1, dtype=np.uint64), np.arange(j0, j1 + 1, dtype=np.uint64), indexing="ij")
    kj = (kk.reshape(-1) << np.uint64(42)) | (jj.reshape(-1) << np.uint64(21))
    begin = np.searchsorted(keys, kj | np.uint64(i0), side="left")
    end = np.searchsorted(keys, kj | np.uint64(i1), side="right")
    live = np.flatnonzero(end > begin)
    if live.shape[0] == 0:
        return np.zeros(0, np.int64)
    return np.concatenate([np.arange(begin[r], end[r], dtype=np.int64) for r in live])
