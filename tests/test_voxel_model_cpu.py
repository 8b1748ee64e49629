"""The numpy VoxelGrid reference (tests/voxel_model.py) against the oracle's C++ restatement (stable order): the same voxels, order, counts and centroids bit for bit
on the clouds the GPU tests use — sizes around the tile limits, 1 to 4 radix passes, cluster occupancies around the centroid kernel's tiers, non-finite rows —
before any GPU time is spent on them."""
import numpy as np
import pytest

from tests import voxel_model as VM


def _same(pts, leaf, oracle):
    g, gc = VM.voxel_grid(pts, leaf)
    fin = np.isfinite(pts[:, :3]).all(1)
    o, oc = oracle.voxel_grid(np.ascontiguousarray(pts[fin]), leaf, stable=True)
    assert g.shape == o.shape and np.array_equal(gc, oc)
    assert np.array_equal(g.view(np.uint32), o.view(np.uint32))
    assert gc.sum() == fin.sum()
    return gc


@pytest.mark.parametrize("n", VM.SIZES)
def test_model_equals_the_oracle_around_the_tile_limits(oracle, n):
    _same(VM.sized_cloud(n), VM.LEAF, oracle)


@pytest.mark.parametrize("bits", sorted(VM.BITS))
def test_model_equals_the_oracle_for_every_radix_pass_count(oracle, bits):
    extent, leaf = VM.BITS[bits]
    pts = VM.box_cloud(extent, 100_000, seed=bits)
    _, keys, div = VM.voxel_keys(pts, leaf)
    total = int(np.prod(div))
    assert (bits - 8) < int(total).bit_length() <= bits          # the keys need that many bits
    _same(pts, leaf, oracle)


def test_model_refuses_an_index_beyond_int32():
    extent, leaf = VM.OVERFLOW
    with pytest.raises(VM.IndexOverflow):
        VM.voxel_grid(VM.box_cloud(extent, 1000), leaf)
    with pytest.raises(ValueError):
        VM.voxel_grid(np.full((4, 4), np.nan, np.float32), VM.LEAF)


def test_model_equals_the_oracle_on_clusters_and_non_finite_rows(oracle):
    pts = VM.cluster_cloud()
    gc = _same(pts, VM.LEAF, oracle)
    assert set(VM.OCCUPANCY) <= set(gc.tolist())                  # every cluster is one voxel of exactly its size


def test_model_sums_in_member_order():
    """f32 sums in input order: 1e8 + 1 + 1 ... rounds differently from any pairwise order"""
    pts = np.array([[0.1, 0.1, 0.1, 1e8]] + [[0.1, 0.1, 0.1, 4.0]] * 7, np.float32)
    g, c = VM.voxel_grid(pts, 1.0)
    acc = np.float32(0)
    for v in pts[:, 3]:
        acc = np.float32(acc + v)
    assert c.tolist() == [8] and g[0, 3] == acc / np.float32(8)
