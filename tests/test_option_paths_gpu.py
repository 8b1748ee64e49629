"""The launch-structure options no other test turns, each against the default and, where the workload allows, against the oracle's exact kNN: every one of them
promises the same results bit for bit.

* scan_lookback = 0 (the map index's three-kernel cell scan), including a map of more than 1 M cells;
* fine_occupancy 2 / 12 / 10^6 (a dense map's fine index built always, by density, never);
* localmap_super_rows = 1 (ring maps below 400 k points get the super-row copy too);
* frame_extract_stream = 1 and readback_gather = 0 on the Livox frame chain."""
import numpy as np
import pytest

import lili_om_amd as L
from lili_om_amd import synth
from tests.test_dense_map_gpu import _dense_room
from tests.test_frontend_frame_gpu import _circuit, _predict

pytestmark = pytest.mark.gpu

IDENT_Q = np.array([1.0, 0.0, 0.0, 0.0])
ZERO_T = np.zeros(3)


def _knn_scene(seed, n_map, extent, halo=None):
    """n_map points in a box of half-extents `extent` (queries near them); `halo`: (n, half-extents) of sparse points around it that stretch the grid"""
    rng = np.random.default_rng(seed)
    pts = rng.uniform(-1, 1, (n_map, 3)) * np.asarray(extent)
    q = pts[rng.integers(0, n_map, 5000)] + rng.normal(0, 0.2, (5000, 3))
    if halo is not None:
        pts = np.concatenate([pts, rng.uniform(-1, 1, (halo[0], 3)) * np.asarray(halo[1])])
    off = rng.uniform(-300, 300, 3)
    return (pts + off).astype(np.float32), (q + off).astype(np.float32)


@pytest.mark.parametrize("scene", [(0, 40_000, (20.0, 20.0, 5.0), 1.0, None), (1, 60_000, (30.0, 10.0, 0.5), 0.64, None),
                                   (2, 150_000, (5.0, 5.0, 1.0), 0.25, (50_000, (100.0, 100.0, 10.0)))],
                         ids=["room", "flat", "over_1M_cells"])
def test_three_kernel_cell_scan_equals_the_look_back_scan_and_the_kd_tree(oracle, scene):
    seed, n_map, extent, gate, halo = scene
    pts, q = _knn_scene(seed, n_map, extent, halo)
    P = L.make_params("frontend", kd_max_radius=gate)          # identity extrinsic: queries are map-frame points
    res = []
    for lookback in (1, 0):
        ctx = L.Context(0)
        try:
            ctx.set_option("scan_lookback", lookback)
            ctx.set_debug(True)
            m = L.ScanToMapMatcher(ctx, P)
            m.set_input_cloud(L.KIND_SURF, pts)
            m.set_queries(0, L.KIND_SURF, q)
            n = m.find_corresponding_surf_features(0, IDENT_Q, ZERO_T)
            idx, d2 = m.neighbors(0, L.KIND_SURF, q.shape[0])
            rec = m.surf_records(0, q.shape[0])
            res.append((n, idx, d2, rec))
        finally:
            ctx.close()
    (n1, i1, d1, r1), (n0, i0, d0, r0) = res
    assert n1 == n0 and np.array_equal(i1, i0) and np.array_equal(d1.view(np.uint32), d0.view(np.uint32))
    for k in ("query_index", "n", "d", "score"):
        assert np.array_equal(r1[k], r0[k]), k
    bi, bd = oracle.KdTree(pts).knn5(q)
    inside = bd[:, 4] < gate
    assert inside.sum() > 1000
    assert np.array_equal(i0[inside], bi[inside]) and np.array_equal(d0[inside].view(np.uint32), bd[inside].view(np.uint32))
    if halo is not None:
        cell = 0.65 * np.sqrt(gate)                             # reach 2, cell_pct 65: the cell edge of this gate
        assert np.prod(np.ceil((pts.max(0) - pts.min(0)) / cell)) > 1_000_000


def test_fine_index_by_occupancy_threshold_changes_nothing(oracle):
    """fine_occupancy 2 (fine index always), 12 (the default: by density) and 10^6 (never) on the dense room: neighbours, records and Gram identical, and the
    neighbours those of the oracle's kd-tree"""
    mp = _dense_room()
    rng = np.random.default_rng(7)
    qw = (mp[rng.choice(mp.shape[0], 6000)].astype(np.float64) + rng.normal(0, 0.01, (6000, 3)) + rng.uniform(-0.1, 0.1, (6000, 3))).astype(np.float32)
    P = L.make_params("rot")
    res = {}
    for occ in (2, 12, 10**6):
        ctx = L.Context(0)
        try:
            ctx.set_option("fine_occupancy", occ)
            ctx.set_debug(True)
            m = L.ScanToMapMatcher(ctx, P)
            m.set_input_cloud(L.KIND_SURF, mp)
            mean_occ, fcell, _ = m.map_density(L.KIND_SURF)
            m.set_queries(0, L.KIND_SURF, qw)
            n = m.find_corresponding_surf_features(0, IDENT_Q, ZERO_T)
            idx, d2 = m.neighbors(0, L.KIND_SURF, qw.shape[0])
            rec = m.surf_records(0, qw.shape[0])
            tb, qb = L.api.body_pose_from_lidar(ZERO_T, IDENT_Q, P)
            G, cost, counts = m.linearize(0, tb, qb, L.MASK_SURF)
            res[occ] = (n, idx, d2, rec, G, cost, counts, fcell, mean_occ)
        finally:
            ctx.close()
    assert res[2][7] > 0 and res[12][7] > 0 and res[10**6][7] == 0.0          # built always, by density (the room is dense), never
    bi, bd = oracle.KdTree(mp).knn5(qw)
    inside = bd[:, 4] < 1.0
    assert inside.sum() > 5000
    want = res[12]
    assert np.array_equal(want[1][inside], bi[inside]) and np.array_equal(want[2][inside].view(np.uint32), bd[inside].view(np.uint32))
    for occ in (2, 10**6):
        got = res[occ]
        assert got[0] == want[0] and np.array_equal(got[1][inside], want[1][inside]) and np.array_equal(got[2][inside], want[2][inside])
        for k in ("query_index", "n", "d", "score"):
            assert np.array_equal(got[3][k], want[3][k]), (occ, k)
        assert np.array_equal(got[4], want[4]) and got[5] == want[5] and np.array_equal(got[6], want[6])


def test_local_map_super_rows_change_nothing(oracle):
    """LocalMap push (5 keyframes, ring of 4) / commit / associate with the super-row copy of a small ring map (option localmap_super_rows) and without"""
    room = synth.make_room(seed=23, n_query=3000, n_edge_query=50)
    rng = np.random.default_rng(1)
    kfs = []
    for k in range(5):
        sel = rng.choice(room["map_xyz"].shape[0], 6000, replace=False)
        t = np.array([0.3 * k, -0.1 * k, 0.02 * k])
        ang = 0.05 * k
        q = np.array([np.cos(ang / 2), 0.0, 0.0, np.sin(ang / 2)])
        local = synth.quat_rot(q * np.array([1, -1, -1, -1]), room["map_xyz"][sel].astype(np.float64) - t)
        kfs.append((np.concatenate([local, rng.uniform(1, 20, (6000, 1))], 1).astype(np.float32), t, q))
    qw = room["map_xyz"][rng.choice(room["map_xyz"].shape[0], 3000)].astype(np.float32) + rng.normal(0, 0.05, (3000, 3)).astype(np.float32)
    P = L.make_params("frontend")
    res = []
    for opt in (0, 1):
        ctx = L.Context(0)
        try:
            ctx.set_option("localmap_super_rows", opt)
            ctx.set_debug(True)
            lm = L.LocalMap(ctx, L.KIND_SURF, width=4, leaf=0.4, max_sq_radius=1.0)
            for f, t, q in kfs:
                lm.push(f, t, q)
            n_raw, n_map = lm.commit()
            mp = lm.get(n_map)
            m = L.ScanToMapMatcher(ctx, P)
            m.set_queries(0, L.KIND_SURF, qw)
            n = m.find_corresponding_surf_features(0, IDENT_Q, ZERO_T)
            idx, d2 = m.neighbors(0, L.KIND_SURF, qw.shape[0])
            rec = m.surf_records(0, qw.shape[0])
            G, cost, counts = m.linearize(0, ZERO_T, IDENT_Q, L.MASK_SURF)
            res.append((n_raw, n_map, mp, n, idx, d2, rec, G, cost, counts))
        finally:
            ctx.close()
    a, b = res
    assert a[0] == b[0] == 4 * 6000 and a[1] == b[1] and np.array_equal(a[2].view(np.uint32), b[2].view(np.uint32))
    assert a[3] == b[3] > 1000 and np.array_equal(a[4], b[4]) and np.array_equal(a[5], b[5])
    for k in ("query_index", "n", "d", "score"):
        assert np.array_equal(a[6][k], b[6][k]), k
    assert np.array_equal(a[7], b[7]) and a[8] == b[8] and np.array_equal(a[9], b[9])
    bi, bd = oracle.KdTree(np.ascontiguousarray(a[2][:, :3])).knn5(qw)
    inside = bd[:, 4] < 1.0
    assert inside.sum() > 2000
    assert np.array_equal(b[4][inside], bi[inside]) and np.array_equal(b[5][inside].view(np.uint32), bd[inside].view(np.uint32))


def test_frame_chain_with_extraction_stream_and_plain_readbacks_equals_the_default():
    """the 9-frame Livox chain (ring width 5: keyframes pop inside the sequence) with frame_extract_stream = 1 and with readback_gather = 0: poses bit-identical"""
    n_frames = 9
    frames = [synth.make_livox_scan(100 + f, origin=_circuit(f)[0], yaw=_circuit(f)[2], inject_bad=(f == 3)) for f in range(n_frames)]
    P = L.make_params("frontend")

    def run(opt):
        ctx = L.Context(0)
        try:
            if opt is not None:
                ctx.set_option(*opt)
            odo = L.FrontendOdometry(ctx, P, width=5, scan_match_cnt=6, first_match_cnt=12, reference_startup=False)
            odo.reset()
            out = []
            for f in range(n_frames):
                t0, q0 = _circuit(0)[:2] if f == 0 else _predict([(o[0], o[1]) for o in out])
                t, q, info = odo.frame(frames[f], t0, q0)
                assert info["gn_status"] == 0 and info["matched"] == (f > 0)
                out.append((t.copy(), q.copy(), info["n_query"]))
            return out
        finally:
            ctx.close()

    want = run(None)
    assert max(float(np.linalg.norm(p[0] - _circuit(f)[0])) for f, p in enumerate(want)) < 0.15
    for opt in (("frame_extract_stream", 1), ("readback_gather", 0)):
        got = run(opt)
        for f, (a, b) in enumerate(zip(got, want)):
            assert a[2] == b[2] and np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]), (opt, f)
