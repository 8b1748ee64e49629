"""Every path of the VoxelGrid filter against the plain numpy reference (tests/voxel_model.py), bit for bit: centroids (x, y, z, aux) and counts.

Sizes around the sort's tile-size and tile-count limits and k_voxel_small's, 1 to 4 radix passes, voxels around the member tiers of k_vox_centroid, non-finite rows;
host and device clouds, the measured and the guessed-key-bits filter, the single-workgroup filter on and off, the back-end keyframe's feature filter (whose radix sort
lets its histograms ride on the key and scatter kernels), and each sort option away from its default.  Every test takes a fresh context: the options stay local."""
import numpy as np
import pytest

import lili_om_amd as L
from tests import voxel_model as VM

pytestmark = pytest.mark.gpu

OPTIONS = [None, ("sort_digit_bits", 4), ("sort_fused_scan", 0), ("sort_ride_hist", 0), ("sort_fused_max_tiles", 0), ("sort_fused_max_tiles", 64),
           ("sort_fused_max_tiles", 512), ("voxel_guess_bits", 0), ("voxel_small", 0)]
_ids = ["default"] + [f"{o[0]}={o[1]}" for o in OPTIONS[1:]]

_cache = {}


def _sized(n):
    if n not in _cache:
        pts = VM.sized_cloud(n)
        _cache[n] = (pts, VM.voxel_grid(pts, VM.LEAF))
    return _cache[n]


def _check(got, want, what):
    (g, gc), (m, mc) = got, want
    assert g.shape == m.shape, (what, g.shape, m.shape)
    assert np.array_equal(gc, mc), what
    assert np.array_equal(g.view(np.uint32), m.view(np.uint32)), what


@pytest.mark.parametrize("opt", OPTIONS, ids=_ids)
def test_filter_of_every_size_equals_the_model(opt):
    """each size filtered twice at the same leaf: the first filter measures its box (or runs k_voxel_small), the second guesses its key bits"""
    ctx = L.Context(0)
    try:
        if opt is not None:
            ctx.set_option(*opt)
        for n in VM.SIZES:
            pts, want = _sized(n)
            _check(L.api.voxel_filter(ctx, pts, VM.LEAF), want, ("first", n))
            _check(L.api.voxel_filter(ctx, pts, VM.LEAF), want, ("again", n))
        guesses, misses = L.api.voxel_filter_stats(ctx)
    finally:
        ctx.close()
    small = opt != ("voxel_small", 0)
    n_guessable = sum(2 for n in VM.SIZES if n > 8192 or not small) - 1          # every filter of such a size but the very first one
    if opt == ("voxel_guess_bits", 0):
        assert guesses == 0
    else:
        assert guesses == n_guessable, (guesses, misses, n_guessable)      # (a guess that did not hold is redone the measured way: still counted)


@pytest.mark.parametrize("opt", [None, ("sort_digit_bits", 4), ("sort_fused_scan", 0), ("voxel_guess_bits", 0)], ids=["default", "digits4", "no_fused_scan", "measured"])
def test_filter_for_every_radix_pass_count_equals_the_model(opt):
    """keys of <= 8, 9-16, 17-24 and 25-31 bits (1 to 4 passes of 8-bit digits), each filtered twice; then a cloud whose index would overflow int32 is refused
    on both the measured and the guessed path, and the filter still works afterwards"""
    ctx = L.Context(0)
    try:
        if opt is not None:
            ctx.set_option(*opt)
        for bits, (extent, leaf) in sorted(VM.BITS.items()):
            pts = VM.box_cloud(extent, 300_000, seed=bits)
            want = VM.voxel_grid(pts, leaf)
            _check(L.api.voxel_filter(ctx, pts, leaf), want, ("first", bits))
            _check(L.api.voxel_filter(ctx, pts, leaf), want, ("again", bits))
        extent, leaf = VM.OVERFLOW
        big = VM.box_cloud(extent, 300_000)
        with pytest.raises(VM.IndexOverflow):
            VM.voxel_grid(big, leaf)
        with pytest.raises(L.LiliError):
            L.api.voxel_filter(ctx, big, leaf)                  # leaf 0.1 seen before (31 bits): the guessed path hands it to the measured one, which refuses
        with pytest.raises(L.LiliError):
            L.api.voxel_filter(ctx, big[:5000], leaf)           # k_voxel_small hands it over too
        pts = VM.box_cloud(VM.BITS[31][0], 300_000, seed=31)
        _check(L.api.voxel_filter(ctx, pts, VM.BITS[31][1]), VM.voxel_grid(pts, VM.BITS[31][1]), "after the errors")
    finally:
        ctx.close()


@pytest.mark.parametrize("voxel_small", [1, 0])
def test_filter_of_clusters_around_the_centroid_tiers_equals_the_model(voxel_small):
    """voxels of 1, 4, 5, 36, 37, 1024, 1025, 1040 and 5000 members among sparse points and NaN / Inf rows, whole and cut to <= 8192 rows (k_voxel_small)"""
    pts = VM.cluster_cloud()
    ctx = L.Context(0)
    try:
        ctx.set_option("voxel_small", voxel_small)
        for cloud in (pts, pts[:8192], pts):
            want = VM.voxel_grid(cloud, VM.LEAF)
            _check(L.api.voxel_filter(ctx, cloud, VM.LEAF), want, cloud.shape[0])
        assert set(VM.OCCUPANCY) <= set(want[1].tolist())
    finally:
        ctx.close()


@pytest.mark.parametrize("n", [1, 65, 8192, 8193, 262_145, 1_200_000])
def test_filter_of_device_clouds_equals_the_model(n):
    import torch
    pts, (m, _) = _sized(n)
    d_pts = torch.from_numpy(pts).cuda()
    d_out = torch.zeros((n, 4), dtype=torch.float32, device="cuda")
    ctx = L.Context(0)
    try:
        for _ in range(2):
            oc = L.api.voxel_filter_device(ctx, L.api.cloud_from_device(d_pts.data_ptr(), n, 16, 12), VM.LEAF, d_out.data_ptr(), n)
            ctx.sync()
            got = d_out[: oc.n].cpu().numpy()
            assert got.shape == m.shape and np.array_equal(got.view(np.uint32), m.view(np.uint32)), n
    finally:
        ctx.close()


def _plane_cloud(n, seed):
    """n rows on a 60 x 60 m ground slab (the surf map they make is planar: nearly every down-sampled query finds its plane), a tenth duplicated"""
    rng = np.random.default_rng(seed)
    pts = np.concatenate([rng.uniform(-30, 30, (n, 2)), rng.uniform(0, 0.05, (n, 1)), rng.uniform(0, 1, (n, 1))], 1).astype(np.float32)
    pts[: n // 10] = pts[n // 10: 2 * (n // 10)][: n // 10]
    return pts


@pytest.mark.parametrize("n,opt", [(20_000, None), (262_145, None), (1_048_576, None), (1_200_000, None), (1_200_000, ("sort_fused_max_tiles", 512)),
                                   (1_200_000, ("sort_ride_hist", 0)), (262_145, ("sort_fused_max_tiles", 64))],
                         ids=["20k", "262145", "1048576", "1.2M", "1.2M-max512", "1.2M-noride", "262145-max64"])
def test_backend_keyframe_filter_equals_the_model(n, opt):
    """lili_backend_keyframe_prepare: behind a non-empty ring the new keyframe's surf filter is enqueued behind the commit's index build, whose scratch fill leaves the
    box words zero — from the third call on (a guessed map box, a leaf filtered before) its radix sort lets the histograms ride.  n_query must be the model's voxel count,
    and every query a record holds must be the model's centroid of that index.  With sort_fused_max_tiles 512 a 1.2 M-key sort (293 tiles) must not ride."""
    P = L.make_params("rot")
    surf = _plane_cloud(n, seed=n)
    edge = _plane_cloud(3000, seed=1)
    edge[:, 2] = np.linspace(0, 3, 3000, dtype=np.float32)                # a few vertical lines
    edge[:, 0] = np.repeat(np.arange(10, dtype=np.float32), 300)
    edge[:, 1] = 0.0
    want, want_c = VM.voxel_grid(surf, 0.4)
    ident_t, ident_q = np.zeros(3), np.array([1.0, 0.0, 0.0, 0.0])
    ctx = L.Context(0)
    try:
        if opt is not None:
            ctx.set_option(*opt)
        m = L.ScanToMapMatcher(ctx, P)
        bk = L.BackendKeyframes(ctx, P, leaf_surf=0.4, leaf_edge=0.2, width=4)
        for k in range(4):
            slot = k % 2
            join = None if k == 0 else (1 - slot, ident_t, ident_q)
            counts, info = bk.prepare(join, surf, edge, [slot], [ident_t], [ident_q])
            assert info["n_query"][0] == want.shape[0], (k, info["n_query"], want.shape)
            if k == 0:
                continue
            assert info["associated"]
            rec = m.surf_records(slot, n)
            assert rec["count"] == counts[0][0] and rec["count"] > 0.5 * want.shape[0], (k, rec["count"], want.shape[0])
            qi = rec["query_index"]
            assert np.array_equal(rec["cp"].view(np.uint32), want[qi, :3].view(np.uint32)), k
    finally:
        ctx.close()
