"""Rebuild sequences of dense maps with the default options, as a pipeline rebuilds its map every keyframe (L/src/BackendFusion.cpp:839-840): the guessed box
(hits, misses), the dense hint (the gate-sized index without super-rows), the wrong-hint rebuild, the 8-bit -> 32-bit counter rebuild, per-kind hints,
lili_map_set_begin / _end, the four cloud sources and a fine grid coarsened by max_cells.  After every step the neighbours inside the gate, the records, the
counts and the Gram equal those of ONE build of the same cloud in a fresh context bit for bit, and a sample equals the f32 brute force."""
import numpy as np
import pytest

import lili_om_amd as L
from tests import dense_grid_model as M
from tests.knn_brute import BruteKnn5
from tests.test_dense_map_gpu import _dense_room

pytestmark = pytest.mark.gpu

P = L.make_params("rot")
Q_ID = np.array([1.0, 0, 0, 0])
T0 = np.array([0.2, -0.1, 1.2])


def _queries(mp, seed, n=3000, scale=1.0):
    """queries near the surfaces, some 0.2-0.9 m off them, in the frame of pose (identity, T0 * scale)."""
    rng = np.random.default_rng(seed)
    qw = mp[rng.choice(mp.shape[0], n)].astype(np.float64) + rng.normal(0, 0.01 * scale, (n, 3))
    qw[:200] += rng.uniform(-1, 1, (200, 3)) * rng.uniform(0.2, 0.9, (200, 1))
    return (qw - T0 * scale).astype(np.float32)


def _world(ql, t):
    return (ql.astype(np.float64) + t).astype(np.float32)      # identity rotation: transformPoint is exact up to the f32 rounding of q + t


def _assoc(m, kind, ql, t, slot=0):
    """(count, idx, d2, records, Gram, cost) of one association of `kind` at pose (identity, t)."""
    m.set_queries(slot, kind, ql)
    find = m.find_corresponding_surf_features if kind == L.KIND_SURF else m.find_corresponding_corner_features
    n = find(slot, Q_ID, t)
    idx, d2 = m.neighbors(slot, kind, ql.shape[0])
    if kind == L.KIND_SURF:
        rec = m.surf_records(slot, ql.shape[0])
    else:
        rec = m.edge_records(slot, ql.shape[0])
    G, cost, counts = m.linearize(slot, t, Q_ID, L.MASK_SURF if kind == L.KIND_SURF else L.MASK_EDGE)
    return n, idx, d2, rec, G, cost, tuple(counts)


def _single(cloud, kind, ql, t, **opts):
    """the same association after ONE build of `cloud` in a fresh context."""
    ctx = L.Context(0)
    try:
        for k, v in opts.items():
            ctx.set_option(k, v)
        ctx.set_debug(True)
        m = L.ScanToMapMatcher(ctx, P)
        m.set_input_cloud(kind, cloud)
        return _assoc(m, kind, ql, t), m.map_density(kind)
    finally:
        ctx.close()


def _equal(a, b, tag=""):
    n1, i1, d1, r1, G1, c1, k1 = a
    n2, i2, d2, r2, G2, c2, k2 = b
    inside = d1[:, 4] < 1.0
    assert n1 == n2 and k1 == k2, (tag, n1, n2)
    assert np.array_equal(inside, d2[:, 4] < 1.0), tag
    assert np.array_equal(i1[inside], i2[inside]) and np.array_equal(d1[inside].view(np.uint32), d2[inside].view(np.uint32)), tag
    for k in r1:
        if k != "count":
            assert np.array_equal(r1[k], r2[k]), (tag, k)
    assert np.array_equal(G1, G2) and c1 == c2, tag


def _brute_check(mp, res, ql, t, n=150, tag=""):
    _, idx, d2 = res[:3]
    want_i, want_d = BruteKnn5(mp).query(_world(ql[:n], t))
    inside = want_d[:, 4] < 1.0
    assert inside.sum() > n // 2, tag
    assert np.array_equal(idx[:n][inside], want_i[inside]), (tag, np.nonzero((idx[:n] != want_i).any(1) & inside)[0][:5])
    assert np.array_equal(d2[:n][inside].view(np.uint32), want_d[inside].view(np.uint32)), tag
    assert np.all(~(d2[:n][~inside][:, 4] < 1.0)), tag


@pytest.fixture(scope="module")
def rooms():
    dense = _dense_room(seed=3)                                             # ~150 k points, 0.05 m spacing: a fine index
    sparse = _dense_room(seed=4, step=0.3, size=(72.0, 54.0, 24.0))         # the same room six times larger at six times the spacing: about as many points, none
    assert 0.8 < sparse.shape[0] / dense.shape[0] < 1.25                     # (both within the dense hint's size window)
    small = _dense_room(seed=5, size=(6.0, 5.0, 3.0))                        # ~100 k points, dense
    coarse = _dense_room(seed=6, step=0.3)                                   # the room at 0.3 m: no fine index
    return dict(dense=dense, sparse=sparse, small=small, coarse=coarse)


def test_rebuild_guess_hit_and_miss(rooms):
    mp = rooms["dense"]
    ql = _queries(mp, 1)
    cell = M.gate_cell(1.0)
    shifts = [np.zeros(3), np.array([cell / 3, -cell / 3, cell / 3]), np.array([4.0 * cell, 2.5 * cell, -3.0 * cell])]
    want_stats = [(0, 0), (1, 0), (1, 1)]          # fresh: measured; a third of a cell: the guess holds; several cells: a point outside the guess -> measured again
    ctx = L.Context(0)
    try:
        ctx.set_debug(True)
        m = L.ScanToMapMatcher(ctx, P)
        for k, (s, ws) in enumerate(zip(shifts, want_stats)):
            cloud = np.ascontiguousarray((mp.astype(np.float64) + s).astype(np.float32))
            g0, miss0, _ = m.map_build_stats()
            m.set_input_cloud(L.KIND_SURF, cloud)
            g1, miss1, fb = m.map_build_stats()
            assert (g1 - g0, miss1 - miss0) == ws and fb == 0, (k, g1 - g0, miss1 - miss0)
            assert m.map_density(L.KIND_SURF)[1] > 0, k
            res = _assoc(m, L.KIND_SURF, ql, T0 + s)
            one, _ = _single(cloud, L.KIND_SURF, ql, T0 + s)
            _equal(res, one, f"step {k}")
            _brute_check(cloud, res, ql, T0 + s, tag=f"step {k}")
    finally:
        ctx.close()


def test_rebuild_wrong_dense_hint_then_dense_again(rooms):
    """dense -> a sparse map with about the same point count and the same gate (the dense hint is wrong: the build is repeated with the super-row
    copy of the gate-sized index, which is then the one searched) -> dense again."""
    seq = [("dense", 1.0), ("sparse", 6.0), ("dense", 1.0)]
    ctx = L.Context(0)
    try:
        ctx.set_debug(True)
        m = L.ScanToMapMatcher(ctx, P)
        for k, (name, scale) in enumerate(seq):
            mp = rooms[name]
            ql = _queries(mp, 10 + k, scale=scale)
            t = T0 * scale
            m.set_input_cloud(L.KIND_SURF, mp)
            occ, fcell, fr2 = m.map_density(L.KIND_SURF)
            assert (fcell > 0) == (name == "dense"), (k, occ, fcell)
            res = _assoc(m, L.KIND_SURF, ql, t)
            one, dens = _single(mp, L.KIND_SURF, ql, t)
            assert (dens[1] > 0) == (fcell > 0)
            assert res[0] > 1000, (k, res[0])
            _equal(res, one, f"step {k} ({name})")
            _brute_check(mp, res, ql, t, tag=f"step {k} ({name})")
    finally:
        ctx.close()


def test_rebuild_per_kind_hints_do_not_leak(rooms):
    """The surf kind dense and the edge kind sparse, at about the same sizes, rebuilt in turn (each shifted a little per round)."""
    ctx = L.Context(0)
    try:
        ctx.set_debug(True)
        m = L.ScanToMapMatcher(ctx, P)
        for r in range(3):
            for kind, name, scale in ((L.KIND_SURF, "dense", 1.0), (L.KIND_EDGE, "sparse", 6.0)):
                s = np.array([0.07, -0.05, 0.03]) * r * scale
                mp = np.ascontiguousarray((rooms[name].astype(np.float64) + s).astype(np.float32))
                ql = _queries(rooms[name], 20 + r, n=2000, scale=scale)
                t = T0 * scale + s
                m.set_input_cloud(kind, mp)
                assert (m.map_density(kind)[1] > 0) == (kind == L.KIND_SURF), (r, kind)
                res = _assoc(m, kind, ql, t)
                one, _ = _single(mp, kind, ql, t)
                _equal(res, one, f"round {r} kind {kind}")
            assert m.map_density(L.KIND_SURF)[1] > 0 and m.map_density(L.KIND_EDGE)[1] == 0.0
    finally:
        ctx.close()


def test_rebuild_begin_end_sequence_equals_blocking(rooms):
    """Six maps alternating dense and sparse, the next one built by lili_map_set_begin while the iterations on the current one are in flight, equal
    the blocking lili_map_set sequence bit for bit (poses and the last records)."""
    maps = [rooms["dense"], rooms["coarse"], rooms["small"], rooms["coarse"][::2].copy(), rooms["dense"][::3].copy(), rooms["coarse"]]
    ql = _queries(rooms["dense"], 30, n=4000)
    rng = np.random.default_rng(31)
    t_start = T0 + rng.normal(0, 0.03, 3)
    ang = np.radians(0.4)
    q_start = np.array([np.cos(ang / 2), 0, 0, np.sin(ang / 2)])

    def run(pipelined):
        ctx = L.Context(0)
        try:
            m = L.ScanToMapMatcher(ctx, P)
            m.set_queries(0, L.KIND_SURF, ql)
            m.set_input_cloud(L.KIND_SURF, maps[0])
            poses, dens = [], []
            for k in range(len(maps)):
                dens.append(m.map_density(L.KIND_SURF)[1] > 0)
                m.pose_set(0, t_start, q_start)
                m.iterate(0, 6, L.MASK_SURF)                            # asynchronous
                if k + 1 < len(maps):
                    if pipelined:
                        m.set_input_cloud_begin(L.KIND_SURF, maps[k + 1])
                        t, q, st = m.pose_get(0)
                        m.set_input_cloud_end(L.KIND_SURF)
                    else:
                        t, q, st = m.pose_get(0)
                        m.set_input_cloud(L.KIND_SURF, maps[k + 1])
                else:
                    t, q, st = m.pose_get(0)
                poses.append((t.copy(), q.copy(), st))
            rec = m.surf_records(0, ql.shape[0])
            return poses, dens, rec
        finally:
            ctx.close()

    a, b = run(False), run(True)
    assert a[1] == [True, False, True, False, True, False] == b[1]
    assert len({tuple(np.round(p[0], 9)) for p in a[0]}) > 1
    for (ta, qa, sa), (tb, qb, sb) in zip(a[0], b[0]):
        assert sa == sb and np.array_equal(ta, tb) and np.array_equal(qa, qb)
    for k in ("query_index", "cp", "n", "d", "score"):
        assert np.array_equal(a[2][k], b[2][k]), k


def test_rebuild_every_cloud_source_gives_the_same_index(rooms):
    """One dense map read from host float32 rows, float4 rows with aux, a device cloud and a page-locked cloud: same index, same records."""
    import torch
    mp = rooms["small"]
    ql = _queries(mp, 40)
    want, dens = _single(mp, L.KIND_SURF, ql, T0)
    assert dens[1] > 0
    aux = np.c_[mp, np.arange(mp.shape[0], dtype=np.float32)]
    d_map = torch.from_numpy(np.ascontiguousarray(mp)).cuda()
    pinned = L.api.PinnedArray(mp.shape)
    pinned.array[:] = mp
    sources = {"host f32x3": L.api.cloud_from_numpy(mp), "host f32x4 + aux": L.api.cloud_from_numpy(aux, aux_col=3),
               "device": L.api.cloud_from_device(d_map.data_ptr(), mp.shape[0], 12, -1), "page-locked": L.api.cloud_from_numpy(pinned.array)}
    try:
        for name, cloud in sources.items():
            got, d = _single(cloud, L.KIND_SURF, ql, T0)
            assert d == dens, name
            _equal(got, want, name)
    finally:
        pinned.close()


def test_rebuild_max_cells_coarsens_the_fine_grid_then_the_gate_sized_one(rooms):
    mp = rooms["small"]
    ql = _queries(mp, 50)
    mn, mx = M.box_of(mp)
    gate = M.build_grid(mn, mx, M.gate_cell(1.0))
    ref, dens = _single(mp, L.KIND_SURF, ql, T0, map_guess_box=0)
    occ = dens[0]
    fg, fc, fb = M.fine_index(mn, mx, 1.0, occ)
    assert fg is not None and (dens[1], dens[2]) == (fc, fb)                      # the model, bit for bit
    assert fg.n_cells > 4 * gate.n_cells
    # only the fine grid coarsened
    mc = fg.n_cells // 3
    got, d = _single(mp, L.KIND_SURF, ql, T0, map_guess_box=0, max_cells=mc)
    fg2, fc2, fb2 = M.fine_index(mn, mx, 1.0, d[0], max_cells=mc)
    assert d[0] == occ and d[1] > M.uncoarsened_fine_cell(occ, M.gate_cell(1.0)) and (d[1], d[2]) == (fc2, fb2) and fg2.n_cells <= mc
    _equal(got, ref, "fine grid coarsened")
    _brute_check(mp, got, ql, T0, tag="fine grid coarsened")
    # the gate-sized grid coarsened: no fine index
    got, d = _single(mp, L.KIND_SURF, ql, T0, map_guess_box=0, max_cells=gate.n_cells - 1)
    assert d[1] == 0.0 and d[2] == 0.0 and M.fine_index(mn, mx, 1.0, d[0], max_cells=gate.n_cells - 1)[0] is None
    _equal(got, ref, "gate-sized grid coarsened")
    _brute_check(mp, got, ql, T0, tag="gate-sized grid coarsened")
