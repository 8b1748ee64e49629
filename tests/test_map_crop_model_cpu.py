"""The run argument of the global map's crop on the CPU: over a sorted key array, one lower and one upper bound per (k, j) row of the box select exactly
the voxels the brute-force mask selects, in table order.  200 random tables of 0 to 5 000 keys with random boxes: faces on exact multiples of the leaf, negative
coordinates, faces beyond the key range (clipped) and +-inf."""
import numpy as np
import pytest

from tests import map_crop_model as M


def _table(rng, n, leaf, spread):
    if n == 0:
        return np.zeros(0, np.uint64)
    pts = (rng.uniform(-1, 1, (n, 3)) * spread).astype(np.float32)
    return np.unique(M.point_keys(pts, leaf))


def _box(rng, leaf, spread, mode):
    c = rng.uniform(-1, 1, 3) * spread
    h = rng.uniform(0, 1, 3) * spread
    lo, hi = (c - h).astype(np.float32), (c + h).astype(np.float32)
    if mode == 1:      # faces on exact multiples of the leaf (f32 products that land on, or one ulp beside, an integer)
        lo = (np.round(lo / leaf) * np.float32(leaf)).astype(np.float32)
        hi = np.maximum(lo, (np.round(hi / leaf) * np.float32(leaf)).astype(np.float32))
    elif mode == 2:    # a face beyond +-2^20 voxels: clipped (x or z; a clipped y face multiplies the rows as an unbounded one does)
        a = int(rng.choice([0, 2]))
        lo[a], hi[a] = (np.float32(-3e6 * leaf), hi[a]) if rng.integers(0, 2) else (lo[a], np.float32(3e6 * leaf))
    elif mode == 3:    # +-inf on x and z faces (an unbounded y face multiplies the rows: its own test below)
        for a in (0, 2):
            r = int(rng.integers(0, 4))
            if r & 1:
                lo[a] = -np.inf
            if r & 2:
                hi[a] = np.inf
    elif mode == 4:    # a degenerate box: one point
        hi = lo.copy()
    return lo, hi


def test_runs_select_the_mask_in_order():
    rng = np.random.default_rng(2024)
    nonempty = 0
    for t in range(200):
        leaf = float(rng.choice([0.2, 0.3, 0.4, 1.0]))
        spread = float(rng.choice([2.0, 8.0, 30.0]))
        n = int(rng.integers(0, 5001)) if t % 20 else 0
        keys = _table(rng, n, leaf, np.array([spread, spread, spread / 4]))
        assert (np.diff(keys.astype(np.int64)) > 0).all()
        for mode in range(5):
            lo, hi = _box(rng, leaf, spread, mode)
            want = M.crop_mask(keys, lo, hi, leaf)
            got = M.crop_runs(keys, lo, hi, leaf)
            assert np.array_equal(got, want), (t, mode, lo, hi)
            nonempty += want.shape[0] > 0
    assert nonempty > 400


def test_face_index_rule():
    leaf = 0.4
    inv = M.inv_leaf_of(leaf)
    assert M.face_index(0.0, leaf) == M.OFFSET and M.face_index(-0.0, leaf) == M.OFFSET
    assert M.face_index(np.nextafter(np.float32(0), np.float32(-1)), leaf) == M.OFFSET - 1
    assert M.face_index(-np.inf, leaf) == 0 and M.face_index(np.inf, leaf) == M.FIELD
    assert M.face_index(np.float32(-1e9), leaf) == 0 and M.face_index(np.float32(1e9), leaf) == M.FIELD
    # the index of a face is the index abs_voxel_key gives a point on it: f32 product, then floor
    for x in np.random.default_rng(1).uniform(-500, 500, 2000).astype(np.float32):
        assert M.face_index(x, leaf) == int(np.floor(np.float32(x) * inv)) + M.OFFSET
        assert M.point_keys(np.array([[x, x, x]], np.float32), leaf)[0] == M.pack(*[M.face_index(x, leaf)] * 3)
    with pytest.raises(ValueError):
        M.box_indices([0, 1, 0], [1, 0, 1], leaf)
    with pytest.raises(ValueError):
        M.box_indices([0, np.nan, 0], [1, 1, 1], leaf)


def test_unbounded_y_face_and_the_row_limit():
    rng = np.random.default_rng(5)
    leaf = 0.4
    thin = _table(rng, 3000, leaf, np.array([20.0, 20.0, 0.5]))       # k spans a few layers: 2^21 rows each
    lo, hi = np.array([-5, -np.inf, -np.inf], np.float32), np.array([5, np.inf, np.inf], np.float32)
    assert np.array_equal(M.crop_runs(thin, lo, hi, leaf), M.crop_mask(thin, lo, hi, leaf))
    tall = _table(rng, 3000, leaf, np.array([20.0, 20.0, 20.0]))      # ~100 layers x 2^21 rows > 2^24
    with pytest.raises(M.TooManyRows):
        M.crop_runs(tall, lo, hi, leaf)
    lo[1], hi[1] = -3.0, 3.0
    assert np.array_equal(M.crop_runs(tall, lo, hi, leaf), M.crop_mask(tall, lo, hi, leaf))
